"""Discrete-action (Categorical head) policies on the device against the fp64 reference of tests/cat_ref.py:
pgm_act_forward_cat / pgm_rollout_act_cat / pgm_eval_act_cat, the host-stepped rollout on Deep Sea Treasure,
ppo_update_cat_kernel on every loss branch and hyper-parameter, the delayed norm hand-off, pgm_uniform_noise, two MOPG
iterations and the CLI.

Bands are those of the plain towers, unwidened: values 2e-5 + 1e-5 |ref|, log-prob 5e-5, parameters after an update
2e-6 + 1e-5 |ref|, Adam moments rel 1e-3, loss stats 1e-5 + 1e-4 |ref|; actions and masks exact.  The inputs and the
conditions that make exact actions a fair demand (tests/cat_inputs.py: every uniform >= 1e-4 from every cumulative
probability, top-two logits >= 1e-4 apart, the reference's fp32 arm agrees) are asserted from the reference alone
before the device is looked at."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pgmorl_amd import _lib
from pgmorl_amd.hostenv import DeepSeaTreasureHostVecEnv
from pgmorl_amd.layout import STATE_KEYS_CAT
from pgmorl_amd.runtime import TaskBatch

from . import cat_inputs as ci
from .test_gpu_kernels import _close

pytestmark = pytest.mark.gpu

ENV = ci.ENV
SENTINEL = -777.0
VAL, LP = (2e-5, 1e-5), (5e-5, 0.0)
DELAY = 4_000_000  # shader cycles (~2 ms): far beyond one Adam step, far below the 2^26-spin timeout


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _batch(pols, N, T, he=None, **kw):
    P = len(pols)
    tb = TaskBatch(ENV, P, num_processes=N, num_steps=T, host_env=he or DeepSeaTreasureHostVecEnv(ENV, P, N), **kw)
    for p, pol in enumerate(pols):
        tb.set_task(p, pol.state_dict())
    return tb


# ------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize('P,N', [(1, 1), (1, 4), (3, 1), (3, 4)])
def test_rollout_act_cat(gpu, P, N):
    """pgm_rollout_act_cat at t in {0, 2, 4} and the bootstrap value (t = T = 5) on sentinel-filled storage: only
    slot t changes, action_out is the stored action and the reference's exactly; pgm_act_forward_cat on the same rows,
    sampled and deterministic."""
    T = 5
    seed, (pols, obs, uni, refs, bad, margins) = ci.first_seed(lambda s: ci.forward_case(P, N, T, s))
    assert seed == 0 and not bad, (seed, bad)  # the first seed counting up, no case left out
    tb = _batch(pols, N, T)
    assert tb.discrete and tb.actions.shape == (P, T, N, 1) and tb.noise.shape == (T, N)
    tb.obs.copy_(obs)
    tb.noise.copy_(uni)
    out = torch.empty(P, N, dtype=torch.int32, device=gpu)
    for t in (0, 2, 4, 5):
        for x in (tb.values, tb.actions, tb.logp):
            x.fill_(SENTINEL)
        out.fill_(int(SENTINEL))
        last = t == T
        _lib.check(_lib.lib().pgm_rollout_act_cat(C.byref(tb.dims), _ptr(tb.params), C.byref(tb.c_rb), t,
                                                  _ptr(None if last else tb.noise), _ptr(None if last else out),
                                                  _stream()), 'pgm_rollout_act_cat')
        val, act, lp, ao = tb.values.cpu(), tb.actions.cpu(), tb.logp.cpu(), out.cpu()
        assert torch.equal(tb.obs.cpu(), obs), 'observations were written'
        keep = torch.ones(T + 1, dtype=torch.bool)
        keep[t] = False
        assert (val[:, keep] == SENTINEL).all(), f't={t}: values outside slot t changed'
        assert (act[:, keep[:T]] == SENTINEL).all() and (lp[:, keep[:T]] == SENTINEL).all(), \
            f't={t}: actions / logp outside slot t changed'
        if last:
            assert (ao == int(SENTINEL)).all()
        else:
            assert torch.equal(ao.float(), act[:, t, :, 0]), 'action_out is not the stored action'
        for p in range(P):
            _close(val[p, t], refs[p]['values'][t], *VAL, f'value t={t}')
            if not last:
                assert torch.equal(ao[p].long(), refs[p]['actions'][t]), f'task {p} t={t}: actions'
                _close(lp[p, t], refs[p]['logp'][t], *LP, f'log_prob t={t}')
    for t in (1, 3):
        v, a, lp = (x.cpu() for x in tb.act(obs[:, t].to(gpu), uni[t].to(gpu)))
        _, am, lpm = (x.cpu() for x in tb.act(obs[:, t].to(gpu), deterministic=True))
        assert a.dtype == torch.int32 and a.shape == (P, N)
        for p in range(P):
            _close(v[p], refs[p]['values'][t], *VAL, 'act: value')
            assert torch.equal(a[p].long(), refs[p]['actions'][t]) and torch.equal(am[p].long(), refs[p]['mode'][t])
            _close(lp[p], refs[p]['logp'][t], *LP, 'act: log_prob')
            with torch.no_grad():
                _, _, rl = pols[p].act(obs[p, t].double(), deterministic=True)
            _close(lpm[p], rl[:, 0], *LP, 'act: log_prob of the mode')


@pytest.mark.parametrize('E', [1, 3, 8])
def test_eval_act_cat(gpu, E):
    """The deterministic action on fp64 raw observations normalised with frozen statistics (mopg.py:36-39)."""
    P = 3
    seed, (pols, raw, rms, want, bad, margins) = ci.first_seed(lambda s: ci.eval_case(P, E, s))
    assert seed == 0 and not bad, (seed, bad)
    tb = _batch(pols, 4, 8)
    mean = torch.tensor(np.stack([r.mean for r in rms]), device=gpu)
    var = torch.tensor(np.stack([r.var for r in rms]), device=gpu)
    d_raw = torch.tensor(raw, device=gpu)
    out = torch.full((P, E), int(SENTINEL), dtype=torch.int32, device=gpu)
    d = _lib.Dims(P, 99, -3, 3, 4, 2, 64, 0)  # N and T are ignored
    _lib.check(_lib.lib().pgm_eval_act_cat(C.byref(d), _ptr(tb.params), _ptr(mean), _ptr(var), 1, _ptr(d_raw), E,
                                           _ptr(out), _stream()), 'pgm_eval_act_cat')
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    for p in range(P):
        ob = (raw[p] - rms[p].mean) / np.sqrt(rms[p].var + 1e-8)
        assert (np.abs(ob) > 10.0).any(), 'the clip is exercised'


# ------------------------------------------------------------------------------------------------ 2. host rollout
@pytest.mark.parametrize('kw', [{}, {'max_steps': 12, 'time_limit_is_bad': True}], ids=['plain', 'limit12bad'])
def test_host_rollout_cat(gpu, kw):
    """TaskBatch(host_env=DeepSeaTreasureHostVecEnv).rollout with uploaded uniforms against the reference rollout,
    two rollouts with the after_update carry.  max_steps = 12 with time_limit_is_bad: both true terminals (masks 0,
    bad_masks 1) and time-limit ends (masks 0, bad_masks 0) occur.  The env state is discrete: equal actions give
    bitwise-equal raw observations, so nothing is chaotic and actions / masks are exact."""
    P, N, T, R = 2, 4, 48, 2
    seed, (pols, uni, refs, bad, margins) = ci.first_seed(lambda s: ci.rollout_case(P, N, T, R, s, **kw))
    assert seed == 0 and not bad, (seed, bad)
    for snaps, _ in refs:
        for ro in snaps:
            m, b = ro.masks[1:, :, 0], ro.bad_masks[1:, :, 0]
            assert int(((m == 0) & (b == 1)).sum()) > 0, 'true terminals in the reference'
            if kw:
                assert int(((m == 0) & (b == 0)).sum()) > 0, 'time-limit ends in the reference'
            assert len(set(ro.actions.reshape(-1).tolist())) == 4, 'all four actions occur'
    tb = _batch(pols, N, T, he=DeepSeaTreasureHostVecEnv(ENV, P, N, **kw))
    tb.env_reset()
    for r in range(R):
        tb.rollout(r, noise=uni[r], carry=r > 0)
        dev = {k: getattr(tb, k).cpu().clone() for k in ('obs', 'actions', 'logp', 'values', 'rewards', 'masks',
                                                         'bad_masks')}
        for p in range(P):
            ro = refs[p][0][r]
            what = f' (task {p}, rollout {r})'
            assert torch.equal(dev['actions'][p].double(), ro.actions), 'actions' + what
            np.testing.assert_array_equal(dev['masks'][p].numpy(), ro.masks[..., 0].numpy())
            np.testing.assert_array_equal(dev['bad_masks'][p].numpy(), ro.bad_masks[..., 0].numpy())
            _close(dev['obs'][p], ro.obs, 2e-6, 2e-6, 'obs' + what)          # bands of test_env_ingest
            _close(dev['rewards'][p], ro.rewards, 1e-5, 1e-6, 'rewards' + what)
            _close(dev['values'][p], ro.value_preds, *VAL, 'values (incl. bootstrap)' + what)
            _close(dev['logp'][p], ro.action_log_probs[..., 0], *LP, 'logp' + what)
    for p in range(P):
        vn = refs[p][1]
        _close(tb.obj_var[p].cpu(), vn.obj_rms.var, 0, 1e-9, 'obj_rms.var')
        _close(tb.ob_var[p].cpu(), vn.ob_rms.var, 0, 1e-9, 'ob_rms.var')
        _close(tb.ret_var[p].cpu(), vn.ret_rms.var, 0, 1e-9, 'ret_rms.var')


# ------------------------------------------------------------------------------------------------ 3. the update
def _load_update(tb, data, pols):
    for p, pol in enumerate(pols):
        tb.set_task(p, pol.state_dict())
    obs, actions, logp, values, returns, adv = data
    for dst, src in ((tb.obs, torch.from_numpy(obs)), (tb.actions, actions), (tb.logp, logp), (tb.values, values),
                     (tb.returns, returns), (tb.adv, adv)):
        dst.copy_(src)
    tb.lr.fill_(ci.LR)


def _update_batch(shape, row):
    hp = ci.hparams(row)
    env, P, T, N, E, M = ci.SHAPES[shape]
    tb = TaskBatch(env, P, num_processes=N, num_steps=T, ppo_epoch=E, num_mini_batch=M,
                   host_env=DeepSeaTreasureHostVecEnv(env, P, N), clip_param=hp['clip_param'],
                   value_loss_coef=hp['value_loss_coef'], entropy_coef=hp['entropy_coef'],
                   max_grad_norm=hp['max_grad_norm'], use_clipped_value_loss=hp['use_clipped_value_loss'])
    tb.hp.adam_eps, tb.hp.beta1, tb.hp.beta2 = hp['adam_eps'], hp['beta1'], hp['beta2']
    return tb


def _check_update(tb, results, what, E, M):
    params, am, av = tb.params.cpu().numpy(), tb.adam_m.cpu().numpy(), tb.adam_v.cpu().numpy()
    steps, stats = tb.adam_step.cpu(), tb.stats.cpu()
    lay = tb.layout
    for p, (pol, agent, st, _) in enumerate(results):
        ref = lay.flatten(pol.state_dict(), dtype=np.float64)
        m_ref, v_ref, step = lay.adam_from_optimizer_state(agent.optimizer.state_dict()['state'])
        for name, g, r, atol, rtol in (('params', params[p], ref, 2e-6, 1e-5), ('exp_avg', am[p], m_ref, 1e-7, 1e-3),
                                       ('exp_avg_sq', av[p], v_ref, 1e-10, 1e-3),
                                       ('loss stats', stats[p].numpy(), st, 1e-5, 1e-4)):
            err = np.abs(np.asarray(g, np.float64) - r)
            print(f'{what} task {p}: {name} max abs err {err.max():.3e}, '
                  f'{(err / (atol + rtol * np.abs(r))).max():.3f} of the band')
        assert int(steps[p]) == step == E * M
        _close(params[p], ref, 2e-6, 1e-5, f'{what} task {p}: params')
        _close(am[p], m_ref, 1e-7, 1e-3, f'{what} task {p}: exp_avg')
        _close(av[p], v_ref, 1e-10, 1e-3, f'{what} task {p}: exp_avg_sq')
        _close(stats[p], st, 1e-5, 1e-4, f'{what} task {p}: loss stats')


@pytest.mark.parametrize('shape,row', ci.CASES)
def test_update_branches_cat(gpu, shape, row):
    """ppo_update_cat_kernel on branch_inputs' mixtures with actions drawn from the policy's own distribution:
    hyper-parameter rows a-f at (P 2, T 64, N 4, E 2, M 2), row a at the ragged shape, at P = 9 (a partial second
    group of eight tasks, single-tile minibatches) and over 64 Adam steps.  Row f: the entropy gradient reaches every
    actor parameter, and the reference without the term is > 10 bands away (asserted by oracle_case)."""
    (args, spec, pols, data, perms), results, worst = ci.oracle_case(shape, row)
    env, P, T, N, E, M = ci.SHAPES[shape]
    tb = _update_batch(shape, row)
    assert tb.update_variant().startswith('ppo_update_cat_kernel')
    _load_update(tb, data, pols)
    tb.ppo_update(torch.stack(perms).numpy())
    assert int(tb.update_ws[2 * P]) == 0, 'tower exchange timed out'
    tb.check_update()
    _check_update(tb, results, f'cat {shape} row {row}', E, M)
    if row == 'f':  # the entropy term's own gradient moves the head: its exp_avg differs from row a's reference
        assert worst['entropy term, x band'] > 10.0


def _cat_block(task, tower):
    """blockIdx.x of (task, tower 0 = critic / 1 = actor) in ppo_update_cat_kernel: groups of 16 blocks per 8 tasks."""
    return 16 * (task // 8) + 8 * tower + (task & 7)


@pytest.mark.parametrize('tower,step', [(0, 1), (1, 1), (0, 3), (1, 3)])
def test_norm_handoff_under_delay_cat(gpu, tower, step, monkeypatch):
    """One workgroup of task 0 stalls a bounded 2 ms between its norm-granule store and its poll at Adam step 1 or at
    the last step (3): the step-parity double buffering keeps the hand-off intact, check_update() stays clean and the
    parameters stay in band.  Runs through the test build (libpgm_test.so), as tests/test_gpu_layernorm.py does."""
    shape, row = 'dst2', 'a'
    (args, spec, pols, data, perms), results, _ = ci.oracle_case(shape, row)
    env, P, T, N, E, M = ci.SHAPES[shape]
    assert E * M == 4
    monkeypatch.setenv('PGM_TEST_DELAY', f'{step}:{_cat_block(0, tower)}:2:{DELAY}')
    tb = _update_batch(shape, row)
    _load_update(tb, data, pols)
    with _lib.test_build():
        tb.ppo_update(torch.stack(perms).numpy())
    tb.check_update()
    _check_update(tb, results, f'cat delayed {"actor" if tower else "critic"} step {step}', E, M)


# ------------------------------------------------------------------------------------------------ 4. uniform stream
def test_uniform_noise(gpu):
    """Two calls with one seed are bitwise equal, another seed differs; all values in [0, 1) on the 2^-24 grid; over
    2^20 draws each of 64 equal bins is within 6 sigma of 2^14, sigma = sqrt(2^20 (1/64)(63/64)) ~ 127."""
    n = 1 << 20
    a, b, c = (torch.full((n,), SENTINEL, device=gpu) for _ in range(3))
    for buf, seed in ((a, 5), (b, 5), (c, 6)):
        _lib.check(_lib.lib().pgm_uniform_noise(n, C.c_uint64(seed), _ptr(buf), _stream()), 'pgm_uniform_noise')
    assert torch.equal(a, b) and not torch.equal(a, c)
    x = a.cpu().numpy().astype(np.float64)
    assert x.min() >= 0.0 and x.max() < 1.0
    assert np.array_equal(x * (1 << 24), np.round(x * (1 << 24)))
    counts = np.bincount((x * 64).astype(np.int64), minlength=64)
    sigma = np.sqrt(n * (1 / 64) * (63 / 64))
    assert np.abs(counts - (1 << 14)).max() <= 6 * sigma, counts
    short = torch.full((1000,), SENTINEL, device=gpu)  # element i is keyed by (seed, i): a prefix of the long stream
    _lib.check(_lib.lib().pgm_uniform_noise(999, C.c_uint64(5), _ptr(short), _stream()), 'pgm_uniform_noise')
    assert torch.equal(short[:999], a[:999]) and float(short[999]) == SENTINEL


# ------------------------------------------------------------------------------------------------ 5. MOPG iterations
MOPG_SEED = 1  # the first policy seed, counting up from 0, at which the reference meets the margin rule (seed 0: no)


def test_mopg_iterations_cat(gpu):
    """Two host-stepped MOPG iterations on Deep Sea Treasure (rollout, GAE, advantages, update, evaluation) against
    the reference loop.  Rollout actions are exact; evaluation actions are equal under the logit-margin rule, so the
    objectives are exact up to the fp64 sum."""
    c = ci.MOPG
    P, T, N, E, M, iters = (c[k] for k in ('P', 'T', 'N', 'E', 'M', 'iters'))
    assert ci.mopg_case(0)[4], 'seed 0 meets the conditions: MOPG_SEED is not the first'
    args, pols, w, refs, bad, margins = ci.mopg_case(MOPG_SEED)
    assert not bad, bad
    tb = TaskBatch(ENV, P, num_processes=N, num_steps=T, ppo_epoch=E, num_mini_batch=M,
                   host_env=DeepSeaTreasureHostVecEnv(ENV, P, N))
    for p, pol in enumerate(pols):
        tb.set_task(p, pol.state_dict(), {}, None, w[p])
    tb.env_reset()
    fn = ci.mopg_noise_fn(T, N, E)
    total = int(args.num_env_steps) // T // N
    from oracle import ppo as oppo
    for j in range(iters):
        u, perms = fn(j)
        tb.iteration(j, oppo.linear_lr(j, total, args.lr), noise=u, perms=torch.stack(perms).numpy(), carry=j > 0)
        objs, params = tb.objs.cpu().numpy().copy(), tb.params.cpu().numpy().copy()
        acts, rets = tb.actions.cpu(), tb.returns.cpu()
        for p in range(P):
            pol, ref_objs, st = refs[p][j]
            assert torch.equal(acts[p].double(), st['actions']), f'task {p} iteration {j}: rollout actions'
            _close(rets[p][:T], st['returns'][:T], 1e-5, 1e-5, f'returns iter {j}')  # band of test_gae
            _close(params[p], tb.layout.flatten(pol.state_dict(), dtype=np.float64), 2e-5, 1e-4,
                   f'params iter {j}')  # band of test_host_mopg_iterations_end_to_end
            _close(objs[p], ref_objs, 0, 1e-12, f'eval objs iter {j}')
    tb.check_update()


# ------------------------------------------------------------------------------------------------ 6. the CLI
@pytest.mark.parametrize('rng', ['host', 'device'])
def test_cli_dst(gpu, tmp_path, capsys, rng):
    """pgmorl_amd.run --env-name MO-DeepSeaTreasure-v0 --host-env dst at a tiny budget: the results tree is written
    and final/EP_policy_*.pt holds the 12 reference keys of a Discrete-space Policy."""
    from pgmorl_amd.run import main
    T, N = 32, 2
    argv = ['--env-name', ENV, '--obj-num', '2', '--num-steps', str(T), '--num-processes', str(N), '--ppo-epoch', '1',
            '--num-mini-batch', '2', '--num-env-steps', str(T * N * 4), '--warmup-iter', '2', '--update-iter', '1',
            '--delta-weight', '0.5', '--selection-method', 'prediction-guided', '--save-dir', str(tmp_path),
            '--rl-log-interval', '1', '--rng', rng, '--pbuffer-num', '100', '--host-env', 'dst']
    prev = torch.get_default_dtype()
    try:
        main(argv)
    finally:
        torch.set_default_dtype(prev)
    capsys.readouterr()
    for it in ('2', '3', '4'):
        for f in ('ep/objs.txt', 'population/objs.txt', 'elites/elites.txt', 'elites/offsprings.txt'):
            assert os.path.exists(tmp_path / it / f), f'{it}/{f}'
    for f in ('args.txt', 'log.txt', 'timing.json', 'final/objs.txt', 'final/EP_policy_0.pt'):
        assert os.path.exists(tmp_path / f), f
    final = np.loadtxt(tmp_path / 'final' / 'objs.txt', delimiter=',', ndmin=2)
    assert final.shape[1] == 2 and np.isfinite(final).all() and (final >= 0).all()
    sd = torch.load(tmp_path / 'final' / 'EP_policy_0.pt')
    assert list(sd.keys()) == [k for k, _, _ in STATE_KEYS_CAT] and len(sd) == 12
    assert sd['dist.linear.weight'].shape == (4, 64) and sd['dist.linear.bias'].shape == (4,)
    from .cat_ref import make_cat_policy
    make_cat_policy(3, 4, 2).load_state_dict(sd)  # loads into the reference-shaped Policy of a Discrete space
