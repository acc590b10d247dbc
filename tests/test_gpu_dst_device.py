"""Deep Sea Treasure on the device (TaskBatch(device_env=True): pgm_rollout_dst, pgm_eval_dst) against the
host-stepped path on the same device, bit for bit, and against the fp64 reference of tests/cat_ref.py.

Bit equality between the two device paths is a fair demand: both run the same device functions (policy_forward, the
sampling rule, norm_stats, vecnorm_emit) on the same inputs, the env state is integer and both evaluate the env rule
exactly (tests/test_dst_device.py: pgm_dst_transition, the kernels' inline function, equals the host env bit for bit).
Against the reference the bands are those of tests/test_gpu_categorical.py, unwidened."""
import copy
import ctypes as C
import filecmp
import functools
import os

import numpy as np
import pytest
import torch

from pgmorl_amd import _lib
from pgmorl_amd.hostenv import DeepSeaTreasureHostVecEnv
from pgmorl_amd.runtime import TaskBatch

from . import cat_inputs as ci
from . import cat_ref
from .test_gpu_kernels import _close

pytestmark = pytest.mark.gpu

ENV = ci.ENV
SENTINEL = -777.0
VAL, LP = (2e-5, 1e-5), (5e-5, 0.0)
LIMIT = {'max_steps': 12, 'time_limit_is_bad': True}
KWS = pytest.mark.parametrize('kw', [{}, LIMIT], ids=['plain', 'limit12bad'])
STORED = ('obs', 'actions', 'logp', 'values', 'rewards', 'masks', 'bad_masks')
STATE = ('ob_mean', 'ob_var', 'ob_count', 'ret_mean', 'ret_var', 'ret_count', 'obj_mean', 'obj_var', 'obj_count',
         'obj_acc', 'ret', 'obj_valid')


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _load(tb, pols, weights=None):
    for p, pol in enumerate(pols):
        sd = pol if isinstance(pol, dict) else pol.state_dict()
        if weights is None:
            tb.set_task(p, sd)
        else:
            tb.set_task(p, sd, {}, None, weights[p])
    return tb


def _device_batch(pols, N, T, kw=None, weights=None, **tbkw):
    return _load(TaskBatch(ENV, len(pols), num_processes=N, num_steps=T, device_env=True, **(kw or {}), **tbkw), pols,
                 weights)


def _host_batch(pols, N, T, kw=None, weights=None, **tbkw):
    he = DeepSeaTreasureHostVecEnv(ENV, tbkw.get('capacity') or len(pols), N, **(kw or {}))
    return _load(TaskBatch(ENV, len(pols), num_processes=N, num_steps=T, host_env=he, **tbkw), pols, weights)


def _snapshot(tb, names=STORED + STATE):
    return {k: getattr(tb, k).cpu().clone() for k in names}


def _assert_equal(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), f'{k} differs {what}: ' \
            f'{int((a[k] != b[k]).sum())} of {a[k].numel()} elements'


# ------------------------------------------------------------------------------------------------ 4. fused vs host-stepped
@KWS
@pytest.mark.parametrize('P,N', [(1, 1), (2, 4), (3, 3), (2, 8)])
def test_fused_rollout_equals_host_stepped(gpu, P, N, kw):
    """Two batches with the same policies and the same uploaded uniforms, one host-stepped, one fused: R = 2 rollouts
    (the second carried) of T = 48 steps leave every stored field, the bootstrap values, every running statistic and
    count, obj_acc, ret and obj_acc_valid bitwise equal, and the device-side env state is the host env's."""
    T, R = 48, 2
    pols = cat_ref.make_policies(ci.dst_spec(), P, 0)
    uni = torch.rand(R, T, N, generator=torch.Generator().manual_seed(4), dtype=torch.float32)
    th, td = _host_batch(pols, N, T, kw), _device_batch(pols, N, T, kw)
    assert td.device_env and td.host_env is None and not hasattr(td, '_h_act')  # no pinned host staging
    assert td.mode.max_steps == (12 if kw else 50) and td.mode.time_limit_is_bad == bool(kw)
    th.env_reset()
    td.env_reset()
    _assert_equal(_snapshot(th), _snapshot(td), 'after env_reset')
    term = limit = 0
    actions = set()
    for r in range(R):
        th.rollout(r, noise=uni[r], carry=r > 0)
        td.rollout(r, noise=uni[r], carry=r > 0)
        h, d = _snapshot(th), _snapshot(td)
        _assert_equal(h, d, f'(rollout {r})')
        s = td.s.cpu()
        assert torch.equal(s, s.round()) and s.shape == (P, N, 3)
        for j, x in enumerate(th.host_env._st):  # (row, col, step) of the host env, exactly
            np.testing.assert_array_equal(s[..., j].numpy().astype(np.int64), x[:P])
        m, b = h['masks'][:, 1:], h['bad_masks'][:, 1:]
        term += int(((m == 0) & (b == 1)).sum())
        limit += int(((m == 0) & (b == 0)).sum())
        actions |= set(h['actions'].reshape(-1).tolist())
    assert term > 0, 'true terminals (masks 0, bad_masks 1) occur'
    assert (limit > 0) == bool(kw), 'time-limit ends (masks 0, bad_masks 0) occur with max_steps = 12 only'
    assert actions == {0.0, 1.0, 2.0, 3.0}, 'all four actions occur'


# ------------------------------------------------------------------------------------------------ 5. the fp64 reference
@KWS
def test_fused_rollout_against_the_reference(gpu, kw):
    """test_host_rollout_cat's inputs and bands on the fused kernel: it is held to cat_ref on its own."""
    P, N, T, R = 2, 4, 48, 2
    seed, (pols, uni, refs, bad, margins) = ci.first_seed(lambda s: ci.rollout_case(P, N, T, R, s, **kw))
    assert seed == 0 and not bad, (seed, bad)
    tb = _device_batch(pols, N, T, kw)
    tb.env_reset()
    for r in range(R):
        tb.rollout(r, noise=uni[r], carry=r > 0)
        dev = _snapshot(tb, STORED)
        for p in range(P):
            ro = refs[p][0][r]
            what = f' (task {p}, rollout {r})'
            assert torch.equal(dev['actions'][p].double(), ro.actions), 'actions' + what
            np.testing.assert_array_equal(dev['masks'][p].numpy(), ro.masks[..., 0].numpy())
            np.testing.assert_array_equal(dev['bad_masks'][p].numpy(), ro.bad_masks[..., 0].numpy())
            _close(dev['obs'][p], ro.obs, 2e-6, 2e-6, 'obs' + what)
            _close(dev['rewards'][p], ro.rewards, 1e-5, 1e-6, 'rewards' + what)
            _close(dev['values'][p], ro.value_preds, *VAL, 'values (incl. bootstrap)' + what)
            _close(dev['logp'][p], ro.action_log_probs[..., 0], *LP, 'logp' + what)
    for p in range(P):
        vn = refs[p][1]
        _close(tb.obj_var[p].cpu(), vn.obj_rms.var, 0, 1e-9, 'obj_rms.var')
        _close(tb.ob_var[p].cpu(), vn.ob_rms.var, 0, 1e-9, 'ob_rms.var')
        _close(tb.ret_var[p].cpu(), vn.ret_rms.var, 0, 1e-9, 'ret_rms.var')


# ------------------------------------------------------------------------------------------------ 6. nothing else written
def test_rollout_writes_nothing_else(gpu):
    """Capacity P + 1 with P active: returns, adv and task row P of every buffer keep their sentinel."""
    P, N, T = 2, 3, 16
    pols = cat_ref.make_policies(ci.dst_spec(), P, 0)
    tb = _device_batch(pols, N, T, capacity=P + 1)
    tb.env_reset()
    full = dict(tb._full)
    for name, t in full.items():
        t[P].fill_(int(SENTINEL) if t.dtype == torch.int32 else SENTINEL)
    for name in ('returns', 'adv', 'elapsed'):
        full[name].fill_(int(SENTINEL) if full[name].dtype == torch.int32 else SENTINEL)
    tb._state[:, P].fill_(SENTINEL)
    cap = tb.capacity
    for name, off, w, vec in tb._seg:
        tb._stats64[off:off + cap * w].view(cap, w)[P].fill_(SENTINEL)
    tb._eval_ob[:, P].fill_(SENTINEL)
    before = {k: v.cpu().clone() for k, v in full.items()}
    state, stats, evob = tb._state.cpu().clone(), tb._stats64.cpu().clone(), tb._eval_ob.cpu().clone()
    uni = torch.rand(T, N, generator=torch.Generator().manual_seed(1), dtype=torch.float32)
    tb.rollout(0, noise=uni, carry=False)
    tb.rollout(1, noise=None, carry=True)
    torch.cuda.synchronize()
    assert not torch.equal(tb.obs.cpu(), before['obs'][:P]), 'the rollout ran'
    for name, t in full.items():
        assert torch.equal(t[P].cpu(), before[name][P]), f'task row P of {name} was written'
    for name in ('returns', 'adv', 'elapsed'):
        assert torch.equal(full[name].cpu(), before[name]), f'{name} was written'
    assert torch.equal(tb._state.cpu(), state), 'parameters / Adam moments were written'
    assert torch.equal(tb._eval_ob.cpu(), evob)
    for name, off, w, vec in tb._seg:
        assert torch.equal(tb._stats64[off:off + cap * w].view(cap, w)[P].cpu(),
                           stats[off:off + cap * w].view(cap, w)[P]), f'task row P of {name} was written'
        if name == 'weights':
            assert torch.equal(tb._stats64[off:off + cap * w].cpu(), stats[off:off + cap * w])


# ------------------------------------------------------------------------------------------------ 7. in-kernel draws
@KWS
def test_in_kernel_draws_are_the_uniform_stream(gpu, kw):
    """rollout(seed, noise=None) draws element t * N + n of pgm_uniform_noise's stream of `seed` in the kernel: equal,
    in every stored field and statistic over two carried rollouts, to the rollout fed that stream."""
    P, N, T = 2, 3, 40
    pols = cat_ref.make_policies(ci.dst_spec(), P, 0)
    ta, tb = _device_batch(pols, N, T, kw), _device_batch(pols, N, T, kw)
    ta.env_reset()
    tb.env_reset()
    for r, seed in enumerate((7, 1 << 40)):
        ta.rollout(seed, noise=None, carry=r > 0)
        u = torch.full((T, N), SENTINEL, device=gpu)
        _lib.check(_lib.lib().pgm_uniform_noise(T * N, C.c_uint64(seed), _ptr(u), _stream()), 'pgm_uniform_noise')
        tb.rollout(seed + 1, noise=u, carry=r > 0)  # (the seed is not read when a stream is given)
        _assert_equal(_snapshot(ta), _snapshot(tb), f'(rollout {r})')
        assert torch.equal(ta.s, tb.s)
    assert len(set(ta.actions.cpu().reshape(-1).tolist())) == 4


# ------------------------------------------------------------------------------------------------ 8. evaluation
def eval_episode_case(P, use_ob, seed):
    """Policies and frozen statistics whose deterministic episode keeps the top two logits >= MARGIN apart at every
    step, in fp64 and in the reference's fp32 arm (ci.eval_case's rule along the episode)
    -> (pols, rms, per-task fp64 episode objectives at raw = 1, violations, margins)."""
    from oracle.vecenv import RunningMeanStd
    pols = cat_ref.make_policies(ci.dst_spec(), P, seed)
    rng = np.random.RandomState(seed + 7)
    rms, objs, bad, m = [], [], [], {}
    for p in range(P):
        r = RunningMeanStd(shape=(3,))
        r.update(rng.rand(50, 3) * np.array([1.0, 1.0, 0.3]))
        rms.append(r)
        ob = r if use_ob else None
        o64 = cat_ref.ref_evaluate(pols[p], DeepSeaTreasureHostVecEnv(ENV, 1, 1), ob, 1, margins=m)
        o32 = cat_ref.ref_evaluate(copy.deepcopy(pols[p]).float(), DeepSeaTreasureHostVecEnv(ENV, 1, 1), ob, 1)
        if not np.array_equal(o64, o32):
            bad.append(f'task {p}: the fp32 arm plays another episode')
        objs.append(o64)
    if not m['logit'] >= ci.MARGIN:
        bad.append(f'logit margin {m["logit"]:.3g} < {ci.MARGIN}')
    return pols, rms, objs, bad, m


@functools.lru_cache(maxsize=None)
def _eval_case(use_ob):
    return ci.first_seed(lambda s: eval_episode_case(3, use_ob, s))


@pytest.mark.parametrize('use_ob', [0, 1])
@pytest.mark.parametrize('raw', [0, 1])
@pytest.mark.parametrize('E', [1, 3, 8])
def test_eval_dst_equals_host_evaluate(gpu, E, raw, use_ob):
    """pgm_eval_dst against _host_evaluate (pgm_eval_act_cat + the host env) on the same parameters and statistics at
    rel 1e-12, and both against the reference's episode."""
    P, gamma = 3, 0.9
    seed, (pols, rms, _, bad, margins) = _eval_case(use_ob)
    assert not bad, (seed, bad)
    print(f'use_ob {use_ob}: first passing seed {seed}, logit margin {margins["logit"]:.3g}')
    kw = dict(eval_num=E, raw=bool(raw), ob_rms=bool(use_ob), gamma=gamma)
    th, td = _host_batch(pols, 1, 8, **kw), _device_batch(pols, 1, 8, **kw)
    mean = torch.tensor(np.stack([r.mean for r in rms]), device=gpu)
    var = torch.tensor(np.stack([r.var for r in rms]), device=gpu)
    td.objs.fill_(SENTINEL)
    got_h = th.evaluate(mean, var).cpu().numpy().copy()
    got_d = td.evaluate(mean, var).cpu().numpy().copy()
    _close(got_d, got_h, 0, 1e-12, 'pgm_eval_dst vs _host_evaluate')
    for p in range(P):
        want = cat_ref.ref_evaluate(pols[p], DeepSeaTreasureHostVecEnv(ENV, 1, 1), rms[p] if use_ob else None, E,
                                    raw=bool(raw), gamma=gamma)
        _close(got_d[p], want, 0, 1e-12, f'task {p} vs the reference')


def _hand_policy(action=None):
    """A state dict with an all-zero actor head and bias 10 on `action`; action None: the two-step policy -- the one
    live actor unit reads the step feature (z = 100 x_2 - 1: -1 at step 0, +1 at step 1), and the head turns its sign
    into up (h < 0) or down (h > 0); left / right sit at -50."""
    sd = {k: v.clone() for k, v in cat_ref.make_policies(ci.dst_spec(), 1, 0)[0].state_dict().items()}
    sd['dist.linear.weight'].zero_()
    sd['dist.linear.bias'].zero_()
    if action is not None:
        sd['dist.linear.bias'][action] = 10.0
        return sd
    for k in ('base.actor.0.weight', 'base.actor.0.bias', 'base.actor.2.weight', 'base.actor.2.bias'):
        sd[k].zero_()
    sd['base.actor.0.weight'][0, 2] = 100.0
    sd['base.actor.0.bias'][0] = -1.0
    sd['base.actor.2.weight'][0, 0] = 1.0
    sd['dist.linear.weight'][0, 0] = -10.0
    sd['dist.linear.weight'][1, 0] = 10.0
    sd['dist.linear.bias'][2] = sd['dist.linear.bias'][3] = -50.0
    return sd


def test_eval_known_answers(gpu):
    """Hand-set heads: always-down finds the treasure (1, 0) on step 1, (1, 5), with or without discounting;
    always-up and always-right never find one, (0, 0) when the step limit ends the episode; the two-step policy (up,
    blocked, then down) reaches (1, 0) on step 2: (1, 10/3), times gamma when discounted."""
    UP, DOWN, RIGHT = 0, 1, 3
    pols = [_hand_policy(DOWN), _hand_policy(UP), _hand_policy(RIGHT), _hand_policy(None)]
    gamma = 0.5
    for E in (1, 3):
        for raw, g in ((True, 1.0), (False, gamma)):
            for kw in ({}, {'max_steps': 12}, {'max_steps': 2}):
                tb = _device_batch(pols, 1, 8, kw, eval_num=E, raw=raw, ob_rms=False, gamma=gamma)
                tb.objs.fill_(SENTINEL)
                got = tb.evaluate().cpu().numpy()
                want = np.array([[1.0, 5.0], [0.0, 0.0], [0.0, 0.0], [g * 1.0, g * (10.0 / 3.0)]])
                _close(got, want, 0, 1e-12, f'E {E} raw {raw} {kw}')
    # statistics that leave the mode unchanged: the hand-set heads do not read the observation
    tb = _device_batch(pols[:3], 1, 8, eval_num=2, raw=False, ob_rms=True, gamma=gamma)
    mean = torch.full((3, 3), 0.25, dtype=torch.float64, device=gpu)
    var = torch.full((3, 3), 0.04, dtype=torch.float64, device=gpu)
    _close(tb.evaluate(mean, var).cpu().numpy(), np.array([[1.0, 5.0], [0.0, 0.0], [0.0, 0.0]]), 0, 1e-12, 'with ob_rms')
    # max_steps = 1: the one step both finds the treasure and reaches the limit
    tb = _device_batch(pols[:2], 1, 8, {'max_steps': 1}, eval_num=1, raw=True, ob_rms=False)
    _close(tb.evaluate().cpu().numpy(), np.array([[1.0, 5.0], [0.0, 0.0]]), 0, 1e-12, 'max_steps 1')


# ------------------------------------------------------------------------------------------------ 9. MOPG iterations
MOPG_SEED = 1  # test_mopg_iterations_cat's: the first policy seed at which the reference meets the margin rule


def test_mopg_iterations_device_env(gpu):
    """Two MOPG iterations with device_env=True against the reference loop at test_mopg_iterations_cat's tolerances;
    the same on a host-env batch: parameters and Adam moments bitwise equal between the two, objectives at rel 1e-12;
    overlap_eval=True equals the in-order schedule bit for bit."""
    from oracle import ppo as oppo
    c = ci.MOPG
    P, T, N, E, M, iters = (c[k] for k in ('P', 'T', 'N', 'E', 'M', 'iters'))
    args, pols, w, refs, bad, margins = ci.mopg_case(MOPG_SEED)
    assert not bad, bad
    kw = dict(ppo_epoch=E, num_mini_batch=M)
    td, th, to = (_device_batch(pols, N, T, weights=w, **kw), _host_batch(pols, N, T, weights=w, **kw),
                  _device_batch(pols, N, T, weights=w, **kw))
    for tb in (td, th, to):
        tb.env_reset()
    fn = ci.mopg_noise_fn(T, N, E)
    total = int(args.num_env_steps) // T // N
    objs_o = torch.zeros(iters, P, 2, dtype=torch.float64, device=gpu)
    for j in range(iters):
        u, perms = fn(j)
        lr, perms = oppo.linear_lr(j, total, args.lr), torch.stack(perms).numpy()
        for tb in (td, th):
            tb.iteration(j, lr, noise=u, perms=perms, carry=j > 0)
        to.iteration(j, lr, noise=u, perms=perms, carry=j > 0, overlap_eval=True, objs_out=objs_o[j])
        objs, params = td.objs.cpu().numpy().copy(), td.params.cpu().numpy().copy()
        acts, rets = td.actions.cpu(), td.returns.cpu()
        for p in range(P):
            pol, ref_objs, st = refs[p][j]
            assert torch.equal(acts[p].double(), st['actions']), f'task {p} iteration {j}: rollout actions'
            _close(rets[p][:T], st['returns'][:T], 1e-5, 1e-5, f'returns iter {j}')
            _close(params[p], td.layout.flatten(pol.state_dict(), dtype=np.float64), 2e-5, 1e-4, f'params iter {j}')
            _close(objs[p], ref_objs, 0, 1e-12, f'eval objs iter {j}')
        assert torch.equal(td.state, th.state), f'iteration {j}: parameters / Adam moments differ from the host-env batch'
        assert torch.equal(td.adam_step, th.adam_step)
        _assert_equal(_snapshot(td), _snapshot(th), f'(iteration {j}, host-env batch)')
        _close(objs, th.objs.cpu().numpy(), 0, 1e-12, f'objs vs the host-env batch, iteration {j}')
        # the Categorical update resets its own workspace (norm granules + timeout word); pgm_ppo_update_reset clears
        # pgm_ppo_update's larger layout and is never queued for it
        assert not to._reset_pending and to.update_ws.numel() * 8 == _lib.lib().pgm_ppo_update_cat_workspace_bytes(
            C.byref(to.dims))
        to.wait_eval()
        assert torch.equal(to.state, td.state), f'iteration {j}: overlap_eval changes the parameters'
        assert torch.equal(objs_o[j], td.objs), f'iteration {j}: overlap_eval changes the objectives'
        _assert_equal(_snapshot(to), _snapshot(td), f'(iteration {j}, overlap_eval)')
    for tb in (td, th, to):
        tb.check_update()


# ------------------------------------------------------------------------------------------------ 10. the CLI
def _cli(save, rng, extra):
    from pgmorl_amd.run import main
    T, N = 32, 2
    argv = ['--env-name', ENV, '--obj-num', '2', '--num-steps', str(T), '--num-processes', str(N), '--ppo-epoch', '1',
            '--num-mini-batch', '2', '--num-env-steps', str(T * N * 4), '--warmup-iter', '2', '--update-iter', '1',
            '--delta-weight', '0.5', '--selection-method', 'prediction-guided', '--save-dir', str(save),
            '--rl-log-interval', '1', '--rng', rng, '--pbuffer-num', '100'] + extra
    prev = torch.get_default_dtype()
    try:
        main(argv)
    finally:
        torch.set_default_dtype(prev)


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize('rng', ['host', 'device'])
def test_cli_device_env(gpu, tmp_path, capsys, rng):
    """pgmorl_amd.run --device-env at test_cli_dst's tiny budget writes the results tree; with --rng host every file
    but timing.json, log.txt and args.txt equals the tree of --host-env dst --rng host."""
    dev = tmp_path / 'dev'
    _cli(dev, rng, ['--device-env'])
    for it in ('2', '3', '4'):
        for f in ('ep/objs.txt', 'population/objs.txt', 'elites/elites.txt', 'elites/offsprings.txt'):
            assert os.path.exists(dev / it / f), f'{it}/{f}'
    for f in ('args.txt', 'log.txt', 'timing.json', 'final/objs.txt', 'final/EP_policy_0.pt'):
        assert os.path.exists(dev / f), f
    final = np.loadtxt(dev / 'final' / 'objs.txt', delimiter=',', ndmin=2)
    assert final.shape[1] == 2 and np.isfinite(final).all() and (final >= 0).all()
    if rng != 'host':
        capsys.readouterr()
        return
    host = tmp_path / 'host'
    _cli(host, rng, ['--host-env', 'dst'])
    capsys.readouterr()
    files = _tree(dev)
    assert files == _tree(host)
    compared = 0
    for f in files:
        if f in ('timing.json', 'log.txt', 'args.txt'):
            continue
        compared += 1
        if filecmp.cmp(dev / f, host / f, shallow=False):
            continue
        assert f.endswith('.pt'), f'{f} differs between --device-env and --host-env dst'
        a, b = torch.load(dev / f), torch.load(host / f)  # (equal tensors, should the container bytes differ)
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a), f
    assert compared > 12
