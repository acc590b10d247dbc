"""The MO-Dummy envs on the device (pgm_rollout_dummy, pgm_eval_dummy and the dim sets 6/2/2, 6/2/3 of every Gaussian
kernel) against the host-stepped path on the same device, bit for bit, and against the fp64 reference of
tests/dummy_ref.py.

Bit equality between the two device paths is a fair demand: both run the same device functions (policy_forward, the
Gaussian arithmetic of sample_actions, norm_stats, vecnorm_emit) on the same inputs, and both evaluate the env rule
with the same correctly rounded fp64 operations in the same order (tests/test_dummy_device.py: pgm_dummy_transition,
the kernels' inline function, equals the host env bit for bit).  Against the reference the bands are those of
tests/test_gpu_hostenv.py, tests/test_gpu_kernels.py and tests/test_gpu_update_branches.py, unwidened."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import ppo as oppo
from oracle.vecenv import RunningMeanStd
from pgmorl_amd import _lib, envspec
from pgmorl_amd.hostenv import DummyMOHostVecEnv
from pgmorl_amd.runtime import TaskBatch

from . import branch_inputs as bi
from . import dummy_ref as dr
from .helpers import small_args, weights_grid
from .test_gpu_kernels import _close

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
KWS = pytest.mark.parametrize('kw', [{}, dr.SHORT], ids=['defaults', 'limit12'])
KS = pytest.mark.parametrize('K', [2, 3])
STORED = ('obs', 'actions', 'logp', 'values', 'rewards', 'masks', 'bad_masks')
STATE = ('ob_mean', 'ob_var', 'ob_count', 'ret_mean', 'ret_var', 'ret_count', 'obj_mean', 'obj_var', 'obj_count',
         'obj_acc', 'ret', 'obj_valid')
ENVSTATE = ('s', 'elapsed', 'episode')


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


def _device_batch(K, pols, N, T, kw=None, weights=None, **tbkw):
    return _load(TaskBatch(dr.ENVS[K], len(pols), num_processes=N, num_steps=T, **(kw or {}), **tbkw), pols, weights)


def _host_batch(K, pols, N, T, kw=None, weights=None, **tbkw):
    he = DummyMOHostVecEnv(dr.ENVS[K], tbkw.get('capacity') or len(pols), N, seed=tbkw.get('seed', 0), **(kw or {}))
    return _load(TaskBatch(dr.ENVS[K], len(pols), num_processes=N, num_steps=T, host_env=he, **tbkw), pols, weights)


def _snapshot(tb, names=STORED + STATE):
    return {k: getattr(tb, k).cpu().clone() for k in names}


def _assert_equal(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), f'{k} differs {what}: ' \
            f'{int((a[k] != b[k]).sum())} of {a[k].numel()} elements'


def _assert_env_state(td, he, P, what):
    """The device-side env state and episode counters are the host env's."""
    st = he._st
    assert np.array_equal(td.s.cpu().numpy().view(np.int64), st['s'][:P].view(np.int64)), f'env state {what}'
    np.testing.assert_array_equal(td.elapsed.cpu().numpy(), st['step'][:P], err_msg=f'step {what}')
    np.testing.assert_array_equal(td.episode.cpu().numpy(), st['episode'][:P], err_msg=f'episode {what}')


# ------------------------------------------------------------------------------------------------ 1. fused vs host-stepped
@KS
@KWS
@pytest.mark.parametrize('ln,P,N', [(False, 1, 1), (False, 2, 4), (False, 3, 3), (False, 2, 8), (True, 2, 4), (True, 3, 3)])
def test_fused_rollout_equals_host_stepped(gpu, ln, P, N, kw, K):
    """Two batches with the same policies and the same uploaded noise, one host-stepped, one fused: R = 2 rollouts (the
    second carried) of T = 48 steps leave every stored field, the bootstrap values, every running statistic and count,
    obj_acc, ret and obj_acc_valid bitwise equal, and the device-side env state and episode counters are the host
    env's.  Plain towers at the four shapes, LayerNorm towers at two of them."""
    T, R = 48, 2
    pols = bi.make_policies(envspec.make_spec(dr.ENVS[K]), P, 0, layernorm=ln)
    noise = torch.randn(R, T, N, 2, generator=torch.Generator().manual_seed(4), dtype=torch.float32)
    th, td = _host_batch(K, pols, N, T, kw, layernorm=ln), _device_batch(K, pols, N, T, kw, layernorm=ln)
    assert td.dummy_env and td.host_env is None and not hasattr(td, '_h_act') and not th.dummy_env
    th.env_reset()
    td.env_reset()
    _assert_equal(_snapshot(th), _snapshot(td), 'after env_reset')
    _assert_env_state(td, th.host_env, P, 'after env_reset')
    term = limit = 0
    for r in range(R):
        th.rollout(r, noise=noise[r], carry=r > 0)
        td.rollout(r, noise=noise[r], carry=r > 0)
        h, d = _snapshot(th), _snapshot(td)
        _assert_equal(h, d, f'(rollout {r})')
        _assert_env_state(td, th.host_env, P, f'(rollout {r})')
        m, b = h['masks'][:, 1:], h['bad_masks'][:, 1:]
        term += int(((m == 0) & (b == 1)).sum())
        limit += int(((m == 0) & (b == 0)).sum())
    assert term > 0, 'true terminals (masks 0, bad_masks 1) occur'
    assert (limit > 0) == bool(kw), 'time-limit ends (masks 0, bad_masks 0) occur with max_steps = 12 only'
    assert int(td.episode.max()) > 0 and (td.actions.abs() > 1).any() and (td.actions.abs() < 1).any()


def test_reset_table_wraps_on_the_device(gpu):
    """R = 3 at (12, 1.25): the episode counters pass R inside two rollouts and the fused path stays on the host path."""
    K, P, N, T, kw = 3, 2, 4, 48, dict(dr.SHORT, R=3)
    pols = bi.make_policies(envspec.make_spec(dr.ENVS[K]), P, 1)
    noise = torch.randn(2, T, N, 2, generator=torch.Generator().manual_seed(5), dtype=torch.float32)
    th, td = _host_batch(K, pols, N, T, kw), _device_batch(K, pols, N, T, kw)
    th.env_reset()
    td.env_reset()
    for r in range(2):
        th.rollout(r, noise=noise[r], carry=r > 0)
        td.rollout(r, noise=noise[r], carry=r > 0)
        _assert_equal(_snapshot(th), _snapshot(td), f'(rollout {r})')
        _assert_env_state(td, th.host_env, P, f'(rollout {r})')
    assert int(td.episode.min()) > 3


# ------------------------------------------------------------------------------------------------ 2. in-kernel draws
@KWS
@pytest.mark.parametrize('K,ln', [(2, False), (3, True)])
def test_in_kernel_draws_are_the_normal_stream(gpu, K, ln, kw):
    """rollout(seed, noise=None) draws element (t * N + n) * 2 + a of pgm_normal_noise's stream of `seed` in the
    kernel: equal, in every stored field, statistic and env state over two carried rollouts, to the rollout fed that
    stream."""
    P, N, T = 2, 3, 40
    pols = bi.make_policies(envspec.make_spec(dr.ENVS[K]), P, 0, layernorm=ln)
    ta, tb = _device_batch(K, pols, N, T, kw, layernorm=ln), _device_batch(K, pols, N, T, kw, layernorm=ln)
    ta.env_reset()
    tb.env_reset()
    for r, seed in enumerate((7, 1 << 40)):
        ta.rollout(seed, noise=None, carry=r > 0)
        z = torch.full((T, N, 2), SENTINEL, device=gpu)
        _lib.check(_lib.lib().pgm_normal_noise(T * N * 2, C.c_uint64(seed), _ptr(z), _stream()), 'pgm_normal_noise')
        tb.rollout(seed + 1, noise=z, carry=r > 0)  # (the seed is not read when a stream is given)
        _assert_equal(_snapshot(ta, STORED + STATE + ENVSTATE), _snapshot(tb, STORED + STATE + ENVSTATE), f'(rollout {r})')
    assert float(ta.actions.std()) > 0.5


# ------------------------------------------------------------------------------------------------ 3. nothing else written
@KS
def test_rollout_writes_nothing_else(gpu, K):
    """Capacity P + 1 with P active: returns, adv and task row P of every buffer keep their sentinel."""
    P, N, T = 2, 3, 16
    pols = bi.make_policies(envspec.make_spec(dr.ENVS[K]), P, 0)
    tb = _device_batch(K, pols, N, T, dr.SHORT, capacity=P + 1)
    tb.env_reset()
    full = dict(tb._full)
    assert 'episode' in full and 'elapsed' in full and 's' in full
    for name, t in full.items():
        t[P].fill_(int(SENTINEL) if t.dtype == torch.int32 else SENTINEL)
    for name in ('returns', 'adv'):
        full[name].fill_(SENTINEL)
    tb._state[:, P].fill_(SENTINEL)
    cap = tb.capacity
    for name, off, w, vec in tb._seg:
        tb._stats64[off:off + cap * w].view(cap, w)[P].fill_(SENTINEL)
    tb._eval_ob[:, P].fill_(SENTINEL)
    before = {k: v.cpu().clone() for k, v in full.items()}
    state, stats, evob = tb._state.cpu().clone(), tb._stats64.cpu().clone(), tb._eval_ob.cpu().clone()
    tables = tb.mode._dummy_train.cpu().clone(), tb.mode._dummy_eval.cpu().clone()
    noise = torch.randn(T, N, 2, generator=torch.Generator().manual_seed(1), dtype=torch.float32)
    tb.rollout(0, noise=noise, carry=False)
    tb.rollout(1, noise=None, carry=True)
    tb.evaluate()
    torch.cuda.synchronize()
    assert not torch.equal(tb.obs.cpu(), before['obs'][:P]) and int(tb.episode.max()) > 0, 'the rollout ran'
    for name, t in full.items():
        assert torch.equal(t[P].cpu(), before[name][P]), f'task row P of {name} was written'
    for name in ('returns', 'adv'):
        assert torch.equal(full[name].cpu(), before[name]), f'{name} was written'
    assert torch.equal(tb._state.cpu(), state), 'parameters / Adam moments were written'
    assert torch.equal(tb._eval_ob.cpu(), evob)
    assert torch.equal(tb.mode._dummy_train.cpu(), tables[0]) and torch.equal(tb.mode._dummy_eval.cpu(), tables[1])
    for name, off, w, vec in tb._seg:
        assert torch.equal(tb._stats64[off:off + cap * w].view(cap, w)[P].cpu(),
                           stats[off:off + cap * w].view(cap, w)[P]), f'task row P of {name} was written'
        if name == 'weights':
            assert torch.equal(tb._stats64[off:off + cap * w].cpu(), stats[off:off + cap * w])


# ------------------------------------------------------------------------------------------------ 4. the fp64 reference
@KS
@pytest.mark.parametrize('short', [False, True], ids=['defaults', 'limit12'])
def test_fused_rollout_against_the_reference(gpu, K, short):
    """The fused kernel held to the fp64 reference on its own, at the bands of tests/test_gpu_hostenv.py
    (_check_against, test_host_rollout); masks exact.  The inputs come from the reference alone (dummy_ref.rollout_case:
    every landing point >= 1e-4 from the bound, the fp32 arm makes the same episode-end decisions;
    tests/test_dummy_device.py asserts the episode-end counts and that the skipped seeds fail)."""
    P, N, T, R = 2, 4, 48, 2
    seed, (pols, noise, refs, bad, counts), skipped = dr.reference_case(K, short)
    assert not bad, (seed, bad)
    tb = _device_batch(K, pols, N, T, dict(dr.SHORT) if short else {})
    tb.env_reset()
    for r in range(R):
        tb.rollout(r, noise=noise[r], carry=r > 0)
        dev = _snapshot(tb, STORED)
        for p in range(P):
            ro = refs[p][0][r]
            what = f' (task {p}, rollout {r})'
            np.testing.assert_array_equal(dev['masks'][p].numpy(), ro.masks[..., 0].numpy())
            np.testing.assert_array_equal(dev['bad_masks'][p].numpy(), ro.bad_masks[..., 0].numpy())
            for name, g, w in (('obs', dev['obs'][p], ro.obs), ('actions', dev['actions'][p], ro.actions),
                               ('values', dev['values'][p], ro.value_preds), ('rewards', dev['rewards'][p], ro.rewards)):
                print(f'{name}{what}: max abs err {float((g.double() - w).abs().max()):.3e}')
                _close(g, w, 5e-5, 1e-4, name + what)
            _close(dev['logp'][p], ro.action_log_probs[..., 0], 2e-4, 1e-4, 'logp' + what)
    for p in range(P):
        vn = refs[p][1]
        _close(tb.obj_var[p].cpu(), np.broadcast_to(vn.obj_rms.var, (K,)), 0, 1e-6, 'obj_rms.var')
        _close(tb.ob_var[p].cpu(), vn.ob_rms.var, 1e-9, 1e-6, 'ob_rms.var')
        _close(tb.ret_var[p].cpu(), vn.ret_rms.var, 1e-9, 1e-6, 'ret_rms.var')
        env = refs[p][2]
        np.testing.assert_array_equal(tb.episode[p].cpu().numpy(), env._st['episode'][0])
        np.testing.assert_array_equal(tb.elapsed[p].cpu().numpy(), env._st['step'][0])


# ------------------------------------------------------------------------------------------------ 5. evaluation
SAT = 1e-3  # every mean action of a saturated evaluation case is at least this far beyond the clip at +-1


def _saturated_policies(K, P, seed):
    """Perturbed reference-initialised policies whose fc_mean bias is +-4 per component, a different sign pattern per
    task: the mean action depends on the observation but stays beyond the clip."""
    pols = bi.make_policies(envspec.make_spec(dr.ENVS[K]), P, seed)
    signs = [(1, 1), (-1, 1), (1, -1), (-1, -1)]
    for p, pol in enumerate(pols):
        with torch.no_grad():
            pol.dist.fc_mean.bias.copy_(torch.tensor(signs[p % 4], dtype=torch.float64) * 4.0)
    return pols


class _Spy:
    """A policy wrapper recording the smallest |mean action| of every deterministic act."""

    def __init__(self, pol):
        self.pol, self.low = pol, np.inf

    def parameters(self):
        return self.pol.parameters()

    def act(self, x, deterministic=False, noise=None):
        out = self.pol.act(x, deterministic=deterministic, noise=noise)
        self.low = min(self.low, float(out[1].abs().min()))
        return out


@functools.lru_cache(maxsize=None)
def _eval_case(K, use_ob):
    """From the reference alone: the first seed at which, for E = 8 episodes, the fp64 policy and its fp32 arm keep
    every mean action >= SAT beyond the clip (the env then sees exactly +-1 whatever the last bits of the forward, so
    the episode is a function of the fp64 env rule alone and rel 1e-9 bounds only the order of the fp64 sums)."""
    def case(seed):
        P = 3
        pols = _saturated_policies(K, P, seed)
        rng = np.random.RandomState(seed + 7)
        rms, bad = [], []
        for p in range(P):
            r = RunningMeanStd(shape=(6,))
            r.update(rng.randn(50, 6) * np.array([1.0, 1.0, 0.3, 0.3, 2.0, 5.0]))
            rms.append(r)
            for net in (torch.float64, torch.float32):
                spy = _Spy(copy.deepcopy(pols[p]).to(net))
                dr.ref_evaluate(spy, DummyMOHostVecEnv(dr.ENVS[K], 1, 1), r if use_ob else None, 8)
                if not spy.low >= 1.0 + SAT:
                    bad.append(f'task {p} {net}: a mean action of magnitude {spy.low:.6g}')
        return pols, rms, None, bad
    return dr.first_seed(case)


@KS
@pytest.mark.parametrize('use_ob', [0, 1])
@pytest.mark.parametrize('raw', [0, 1])
@pytest.mark.parametrize('E', [1, 3, 8])
def test_eval_dummy_against_the_reference(gpu, E, raw, use_ob, K):
    """pgm_eval_dummy against the reference evaluation (dummy_ref.ref_evaluate, fp64) at rel 1e-9, and against
    _host_evaluate (pgm_eval_act + the host env) on the same parameters and statistics."""
    P, gamma = 3, 0.99
    seed, (pols, rms, _, bad), skipped = _eval_case(K, use_ob)
    assert not bad, (seed, bad)
    kw = dict(eval_num=E, raw=bool(raw), ob_rms=bool(use_ob), gamma=gamma)
    th, td = _host_batch(K, pols, 1, 8, **kw), _device_batch(K, pols, 1, 8, **kw)
    mean = torch.tensor(np.stack([r.mean for r in rms]), device=gpu)
    var = torch.tensor(np.stack([r.var for r in rms]), device=gpu)
    td.objs.fill_(SENTINEL)
    got_h = th.evaluate(mean, var).cpu().numpy().copy()
    got_d = td.evaluate(mean, var).cpu().numpy().copy()
    _close(got_d, got_h, 0, 1e-12, 'pgm_eval_dummy vs _host_evaluate')
    for p in range(P):
        lengths = np.zeros(E, dtype=np.int64)
        want = dr.ref_evaluate(pols[p], DummyMOHostVecEnv(dr.ENVS[K], 1, 1), rms[p] if use_ob else None, E,
                               raw=bool(raw), gamma=gamma, lengths=lengths)
        print(f'task {p}: episode lengths {lengths}, rel err {np.abs(got_d[p] / want - 1).max():.3e}')
        assert lengths.min() >= 5, 'the episodes run several steps before they leave the disc'
        _close(got_d[p], want, 0, 1e-9, f'task {p} vs the reference')


@KS
@pytest.mark.parametrize('use_ob', [0, 1])
def test_eval_dummy_equals_host_evaluate_unsaturated(gpu, use_ob, K):
    """General policies (mean actions inside the clip): the fused evaluation and the host-stepped one run the same fp32
    forward on the same fp64 observations, so their objectives agree at rel 1e-12; E = 8 discounted episodes."""
    P, E = 3, 8
    pols = bi.make_policies(envspec.make_spec(dr.ENVS[K]), P, 2)
    kw = dict(eval_num=E, raw=False, ob_rms=bool(use_ob), gamma=0.995, seed=3)
    th, td = _host_batch(K, pols, 1, 8, **kw), _device_batch(K, pols, 1, 8, **kw)
    rng = np.random.RandomState(3)
    mean = torch.tensor(rng.randn(P, 6) * 0.2, device=gpu)
    var = torch.tensor(rng.rand(P, 6) + 0.5, device=gpu)
    got_h = th.evaluate(mean, var).cpu().numpy().copy()
    got_d = td.evaluate(mean, var).cpu().numpy().copy()
    assert np.isfinite(got_d).all() and (got_d[:, 1] > 0).all()
    _close(got_d, got_h, 0, 1e-12, 'pgm_eval_dummy vs _host_evaluate')


def _hand_policy(K, bias):
    """A state dict whose mean action is the constant `bias` (fc_mean weight zero)."""
    sd = {k: v.clone() for k, v in bi.make_policies(envspec.make_spec(dr.ENVS[K]), 1, 0)[0].state_dict().items()}
    sd['dist.fc_mean.weight'].zero_()
    sd['dist.fc_mean.bias'].copy_(torch.tensor(bias, dtype=torch.float64))
    return sd


def _walk(start, bound, max_steps, gamma):
    """The saturated (1, 0) episode from `start` by the closed form of the damped sum: x_n = x_0 + c (n - q (1 - q^n) /
    (1 - q)), c = 0.1 q / (1 - q), q = 0.95 -> (length, [sum g^n distance_n, sum g^n / 1.1, sum g^n (bound - |pos_n|)])."""
    q, c = 0.95, 0.1 * 0.95 / 0.05
    x = lambda n: start[0] + c * (n - q * (1 - q ** n) / (1 - q))
    acc, g = np.zeros(3), 1.0
    for n in range(1, max_steps + 1):
        r = np.hypot(x(n), start[1])
        acc += g * np.array([x(n) - x(n - 1), 1 / 1.1, bound - r])
        g *= gamma
        assert abs(r - bound) > 1e-6  # (far from the decision: the closed form decides)
        if r > bound:
            break
    return n, acc


@KS
def test_eval_known_answers(gpu, K):
    """Hand-set heads.  A zero mean never moves: (0, 10) per step for max_steps steps (and bound - |start| with three
    objectives).  A saturated (1, 0) walks the closed-form episode from each reset position until it leaves the disc."""
    gamma = 0.9
    pols = [_hand_policy(K, (0.0, 0.0)), _hand_policy(K, (5.0, 0.0))]
    for E in (1, 3):
        starts = envspec.dummy_reset_table(0, E)[:, 0]
        for raw, g in ((True, 1.0), (False, gamma)):
            for kw in ({}, {'max_steps': 12}, {'max_steps': 40, 'bound': 2.0}):
                ms, bound = kw.get('max_steps', 500), kw.get('bound', 5.0)
                tb = _device_batch(K, pols, 1, 8, kw, eval_num=E, raw=raw, ob_rms=False, gamma=gamma)
                tb.objs.fill_(SENTINEL)
                got = tb.evaluate().cpu().numpy()
                geo = sum(g ** n for n in range(ms))
                still = np.mean([[0.0, 10.0 * geo, (bound - np.hypot(*s)) * geo] for s in starts], 0)
                walks = [_walk(s, bound, ms, g) for s in starts]
                if not kw:
                    assert all(n < ms for n, _ in walks), 'the walk leaves the disc before the limit'
                _close(got[0], still[:K], 0, 1e-9, f'zero mean: E {E} raw {raw} {kw}')
                _close(got[1], np.mean([a for _, a in walks], 0)[:K], 0, 1e-9, f'saturated: E {E} raw {raw} {kw}')
                if raw:
                    _close(got[0, :2], [0.0, 10.0 * ms], 0, 1e-12, '(0, 10) * length')


# ------------------------------------------------------------------------------------------------ 6. MOPG iterations
def _noise_fn(T, N, E):
    def fn(j):
        g = torch.Generator().manual_seed(1000 + j)
        return (torch.randn(T, N, 2, generator=g, dtype=torch.float64).float(),
                [torch.randperm(T * N, generator=g) for _ in range(E)])
    return fn


@KS
@pytest.mark.parametrize('ln', [False, True], ids=['plain', 'layernorm'])
def test_mopg_iterations_end_to_end(gpu, K, ln):
    """Two full MOPG iterations (fused rollout, GAE, scalarised PPO, fused evaluation; P 2, T 64, N 4, E 2, M 4)
    against the reference worker (dummy_ref.ref_mopg) at test_mopg_iterations_end_to_end's tolerances; the
    overlap_eval schedule equals the in-order one bit for bit; check_update() is clean."""
    env, P, N, T, E, M, iters = dr.ENVS[K], 2, 4, 64, 2, 4, 2
    args = small_args(env, num_steps=T, num_processes=N, ppo_epoch=E, num_mini_batch=M, num_env_steps=T * N * 10,
                      layernorm=ln)
    spec = envspec.make_spec(env)
    pols = bi.make_policies(spec, P, 0, layernorm=ln)
    w = weights_grid(K, P)
    kw = dict(ppo_epoch=E, num_mini_batch=M, layernorm=ln)
    td, to = _device_batch(K, pols, N, T, weights=w, **kw), _device_batch(K, pols, N, T, weights=w, **kw)
    td.env_reset()
    to.env_reset()
    fn = _noise_fn(T, N, E)
    total = int(args.num_env_steps) // T // N
    objs_o = torch.zeros(iters, P, K, dtype=torch.float64, device=gpu)
    gpu_objs, gpu_params = [], []
    for j in range(iters):
        noise, perms = fn(j)
        lr, perms = oppo.linear_lr(j, total, args.lr), torch.stack(perms).numpy()
        td.iteration(j, lr, noise=noise, perms=perms, carry=j > 0)
        to.iteration(j, lr, noise=noise, perms=perms, carry=j > 0, overlap_eval=True, objs_out=objs_o[j])
        assert to._reset_pending, 'pgm_ppo_update_reset is queued beside the evaluation (these batches use pgm_ppo_update)'
        gpu_objs.append(td.objs.cpu().numpy().copy())
        gpu_params.append(td.params.cpu().numpy().copy())
        to.wait_eval()
        assert torch.equal(to.state, td.state), f'iteration {j}: overlap_eval changes the parameters'
        assert torch.equal(objs_o[j], td.objs), f'iteration {j}: overlap_eval changes the objectives'
        _assert_equal(_snapshot(to, STORED + STATE + ENVSTATE), _snapshot(td, STORED + STATE + ENVSTATE),
                      f'(iteration {j}, overlap_eval)')
    td.check_update()
    to.check_update()
    for p in range(P):
        refs = dr.ref_mopg(args, pols[p], DummyMOHostVecEnv(env, 1, N), w[p], iters, fn)
        for j, (pol, ref_objs, st) in enumerate(refs):
            ref = td.layout.flatten(pol.state_dict(), dtype=np.float64)
            print(f'task {p} iter {j}: params err {np.abs(gpu_params[j][p] - ref).max():.3e}, objs {gpu_objs[j][p]} '
                  f'ref {ref_objs}')
            _close(gpu_params[j][p], ref, 2e-5, 1e-4, f'params iter {j}')
            _close(gpu_objs[j][p], ref_objs, 1e-3, 1e-4, f'eval objs iter {j}')


# ------------------------------------------------------------------------------------------------ 7. the CLI
def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize('rng', ['host', 'device'])
def test_cli_dummy(gpu, tmp_path, capsys, rng):
    """pgmorl_amd.run --env-name MO-Dummy-v0 with no extra flag writes the results tree at a tiny budget."""
    from pgmorl_amd.run import main
    T, N = 32, 2
    argv = ['--env-name', 'MO-Dummy-v0', '--obj-num', '2', '--num-steps', str(T), '--num-processes', str(N),
            '--ppo-epoch', '1', '--num-mini-batch', '2', '--num-env-steps', str(T * N * 4), '--warmup-iter', '2',
            '--update-iter', '1', '--delta-weight', '0.5', '--selection-method', 'prediction-guided', '--save-dir',
            str(tmp_path / 'run'), '--rl-log-interval', '1', '--rng', rng, '--pbuffer-num', '100']
    prev = torch.get_default_dtype()
    try:
        main(argv)
    finally:
        torch.set_default_dtype(prev)
    capsys.readouterr()
    run = tmp_path / 'run'
    for it in ('2', '3', '4'):
        for f in ('ep/objs.txt', 'population/objs.txt', 'elites/elites.txt', 'elites/offsprings.txt'):
            assert os.path.exists(run / it / f), f'{it}/{f}'
    for f in ('args.txt', 'log.txt', 'timing.json', 'final/objs.txt', 'final/EP_policy_0.pt'):
        assert os.path.exists(run / f), f
    final = np.loadtxt(run / 'final' / 'objs.txt', delimiter=',', ndmin=2)
    assert final.shape[1] == 2 and np.isfinite(final).all() and (final[:, 1] > 0).all()


# ------------------------------------------------------------------------------------------------ 8. the update kernels
UPDATE_SHAPE = (2, 64, 4, 2, 2)  # P, T, N, E, M


@functools.lru_cache(maxsize=None)
def _update_case(K, ln):
    """tests/branch_inputs.py's inputs (row a) at the new dims, from the oracle alone: the first seed counting up from
    BASE_SEED at which conditions() and the fp32 arm's decisions hold."""
    shape, hp = (dr.ENVS[K],) + UPDATE_SHAPE, bi.hparams('a')
    env, P, T, N, E, M = shape
    for seed in range(bi.BASE_SEED, bi.BASE_SEED + 40):
        inputs = bi.build_inputs(env, P, T, N, E, M, seed, hp, ln)
        pols, data, perms = inputs[2], inputs[3], inputs[4]
        results, bad = [], []
        for p in range(P):
            r64 = bi.run_oracle(pols[p], hp, data, p, perms, shape)
            r32 = bi.run_oracle(pols[p], hp, data, p, perms, shape, dtype=torch.float32)
            bad += bi.conditions(r64[3], hp)[0] + bi.same_decisions(r64[3], r32[3], hp)
            results.append(r64)
        if not bad:
            return seed, inputs, results
    raise AssertionError(f'no seed meets the input conditions: {bad[:3]}')


@KS
@pytest.mark.parametrize('family', ['auto', 'mfma', 'ln'])
def test_update_kernels_at_the_new_dims(gpu, monkeypatch, family, K):
    """One update per family the launcher can pick at 6/2/K -- automatic (feature-split), PGM_UPDATE_KERNEL=mfma,
    LayerNorm -- against run_oracle at test_gpu_update_branches's bands; check_update() is clean."""
    ln = family == 'ln'
    seed, (args, spec, pols, data, perms), results = _update_case(K, ln)
    hp = bi.hparams('a')
    P, T, N, E, M = UPDATE_SHAPE
    monkeypatch.delenv('PGM_UPDATE_SPLIT', raising=False)
    if family == 'mfma':
        monkeypatch.setenv('PGM_UPDATE_KERNEL', 'mfma')
    else:
        monkeypatch.delenv('PGM_UPDATE_KERNEL', raising=False)
    tb = TaskBatch(dr.ENVS[K], P, num_processes=N, num_steps=T, ppo_epoch=E, num_mini_batch=M, layernorm=ln,
                   clip_param=hp['clip_param'], value_loss_coef=hp['value_loss_coef'], entropy_coef=hp['entropy_coef'],
                   max_grad_norm=hp['max_grad_norm'], use_clipped_value_loss=hp['use_clipped_value_loss'])
    tb.hp.adam_eps, tb.hp.beta1, tb.hp.beta2 = hp['adam_eps'], hp['beta1'], hp['beta2']
    got = tb.update_variant()
    want = {'auto': 'ppo_update_fs_kernel (', 'mfma': 'ppo_update_', 'ln': 'ppo_update_ln_kernel ('}[family]
    print(f'{family} K {K}: seed {seed}, variant {got}')
    assert got.startswith(want) and (family != 'mfma' or 'fs_kernel' not in got), got
    for p, pol in enumerate(pols):
        tb.set_task(p, pol.state_dict())
    obs, actions, logp, values, returns, adv = data
    for dst, src in ((tb.obs, torch.from_numpy(obs)), (tb.actions, actions), (tb.logp, logp), (tb.values, values),
                     (tb.returns, returns), (tb.adv, adv)):
        dst.copy_(src)
    tb.lr.fill_(bi.LR)
    tb.ppo_update(torch.stack(perms).numpy())
    assert int(tb.update_ws[2 * P]) == 0, 'tower exchange timed out'
    tb.check_update()
    params, am, av = tb.params.cpu().numpy(), tb.adam_m.cpu().numpy(), tb.adam_v.cpu().numpy()
    steps, stats = tb.adam_step.cpu(), tb.stats.cpu()
    lay = tb.layout
    for p, (pol, agent, st, _) in enumerate(results):
        ref = lay.flatten(pol.state_dict(), dtype=np.float64)
        m_ref, v_ref, step = lay.adam_from_optimizer_state(agent.optimizer.state_dict()['state'])
        assert int(steps[p]) == step == E * M
        what = f'{family} K {K} task {p}'
        print(f'{what}: params max abs err {np.abs(params[p] - ref).max():.3e}')
        _close(params[p], ref, 2e-6, 1e-5, f'{what}: params')
        _close(am[p], m_ref, 1e-7, 1e-3, f'{what}: exp_avg')
        _close(av[p], v_ref, 1e-10, 1e-3, f'{what}: exp_avg_sq')
        _close(stats[p], st, 1e-5, 1e-4, f'{what}: loss stats')
