"""The runtime-dim kernel family (the *_any entry points) on the device.

1. On dim sets that compiled kernels exist for, pgm_rollout_act_any / pgm_eval_act_any / pgm_env_ingest_any write what
   pgm_rollout_act(_cat) / pgm_eval_act(_cat) / pgm_env_ingest write, bit for bit (torch.equal).
2. At dims no kernel is compiled for, against the fp64 reference (tests/anydims_ref.py), in the bands of
   tests/test_gpu_hostenv.py (Gaussian) and tests/test_gpu_categorical.py (Categorical), unwidened.
3. pgm_ppo_update_any against oracle.ppo on branch_inputs' / cat_inputs' constructions: parameters 2e-6 + 1e-5 |ref|,
   Adam moments rel 1e-3, loss statistics 1e-5 + 1e-4 |ref|.
4. Two host-stepped MOPG iterations on the tiny envs of tests/anydims_envs.py, and the CLI on them.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import ppo as oppo
from pgmorl_amd import _lib, envspec
from pgmorl_amd._lib import Dims
from pgmorl_amd.hostenv import DeepSeaTreasureHostVecEnv, SynthHostVecEnv
from pgmorl_amd.runtime import TaskBatch

from . import anydims_envs as envs
from . import anydims_ref as ar
from . import cat_inputs as ci
from . import cat_ref
from .test_gpu_kernels import _close

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
# bands of test_gpu_hostenv (PLAIN) and test_gpu_categorical (LP)
VAL, ACT, LP_G, LP_C = (2e-5, 1e-5), (2e-5, 1e-5), (5e-5, 1e-5), (5e-5, 0.0)
DST = 'MO-DeepSeaTreasure-v0'
# (env, N): the compiled dim sets of the issue, 17/6/2 N 4, 8/2/2 N 3, 11/3/3 N 8 and (Categorical) 3/4/2 N 4
COMPILED = [('MO-Walker2d-v2', 4), ('MO-Swimmer-v2', 3), ('MO-Hopper-v3', 8), (DST, 4)]


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _compiled_batch(env, P, N, T, seed=3, **kw):
    """A batch of an env with compiled kernels (whose buffers both kernel families are launched on) + its policies."""
    spec = envspec.make_spec(env)
    disc = bool(spec.get('discrete'))
    he = DeepSeaTreasureHostVecEnv(env, P, N) if disc else None
    tb = TaskBatch(env, P, num_processes=N, num_steps=T, host_env=he, **kw)
    pols = ar.make_policies(spec, P, seed)
    for p, pol in enumerate(pols):
        tb.set_task(p, pol.state_dict())
    return spec, disc, tb, pols


def _any_batch(dims, disc, P, N, T, pols=None, **kw):
    tb = TaskBatch(ar.env_of(dims, disc), P, num_processes=N, num_steps=T, host_env=ar.StubHostEnv(dims, disc, P, N),
                   **kw)
    assert tb.any_dims and tb.update_variant() == 'ppo_update_any_kernel'
    for p, pol in enumerate(pols or []):
        tb.set_task(p, pol.state_dict())
    return tb


def _rollout_act(tb, any_, disc, t, out):
    L, last = _lib.lib(), t == tb.T
    rnd, ao = _ptr(None if last else tb.noise), _ptr(None if last else out)
    if any_:
        rc, what = L.pgm_rollout_act_any(C.byref(tb.dims), int(disc), _ptr(tb.params), C.byref(tb.c_rb), t, rnd, ao,
                                         _stream()), 'pgm_rollout_act_any'
    else:
        fn = L.pgm_rollout_act_cat if disc else L.pgm_rollout_act
        rc, what = fn(C.byref(tb.dims), _ptr(tb.params), C.byref(tb.c_rb), t, rnd, ao, _stream()), 'pgm_rollout_act'
    _lib.check(rc, what)


def _act_out(tb, disc, gpu):
    return (torch.empty(tb.P, tb.N, dtype=torch.int32, device=gpu) if disc
            else torch.empty(tb.P, tb.N, tb.A, device=gpu))


def _sentinel_step(tb, any_, disc, t, out):
    """One act launch on sentinel-filled storage -> (values, actions, logp, action_out) on the host, after checking
    that only slot t changed and that action_out is the stored action."""
    T = tb.T
    for x in (tb.values, tb.actions, tb.logp):
        x.fill_(SENTINEL)
    out.fill_(int(SENTINEL))
    obs0 = tb.obs.cpu().clone()
    _rollout_act(tb, any_, disc, t, out)
    val, act, lp, ao = tb.values.cpu(), tb.actions.cpu(), tb.logp.cpu(), out.cpu()
    assert torch.equal(tb.obs.cpu(), obs0), 'observations were written'
    keep = torch.ones(T + 1, dtype=torch.bool)
    keep[t] = False
    assert (val[:, keep] == SENTINEL).all(), f't={t}: values outside slot t changed'
    assert (act[:, keep[:T]] == SENTINEL).all() and (lp[:, keep[:T]] == SENTINEL).all(), \
        f't={t}: actions / logp outside slot t changed'
    if t == T:
        assert (ao == int(SENTINEL)).all() and (act == SENTINEL).all() and (lp == SENTINEL).all()
    else:
        assert torch.equal(ao.float().reshape(act[:, t].shape), act[:, t]), 'action_out is not the stored action'
        assert (val[:, t] != SENTINEL).all() and (lp[:, t] != SENTINEL).all()
    return val, act, lp, ao


# ------------------------------------------------------------------------------------------------ 1. equal to compiled
@pytest.mark.parametrize('env,N', COMPILED)
def test_rollout_act_any_equals_compiled(gpu, env, N):
    """t = 0, an inner t and t = T on sentinel-filled storage: the two families write the same bits."""
    P, T = 3, 5
    spec, disc, tb, _ = _compiled_batch(env, P, N, T)
    g = torch.Generator().manual_seed(11)
    tb.obs.copy_(torch.randn(P, T + 1, N, spec['obs_dim'], generator=g))
    tb.noise.copy_(torch.rand(T, N, generator=g) if disc else torch.randn(T, N, spec['act_dim'], generator=g))
    out = _act_out(tb, disc, gpu)
    for t in (0, 3, T):
        ref = _sentinel_step(tb, False, disc, t, out)
        got = _sentinel_step(tb, True, disc, t, out)
        for name, a, b in zip(('values', 'actions', 'logp', 'action_out'), got, ref):
            assert torch.equal(a, b), f'{env} t={t}: {name} differ from the compiled kernel'


@pytest.mark.parametrize('use_ob', [0, 1])
@pytest.mark.parametrize('E', [1, 8])
@pytest.mark.parametrize('env,N', COMPILED)
def test_eval_act_any_equals_compiled(gpu, env, N, E, use_ob):
    P = 3
    spec, disc, tb, _ = _compiled_batch(env, P, N, 4, seed=5)
    O, A, K = spec['obs_dim'], spec['act_dim'], spec['obj_num']
    rng = np.random.RandomState(7 + E)
    mean = torch.tensor(rng.randn(P, O) * 0.1, device=gpu)
    var = torch.tensor(rng.rand(P, O) * 0.2 + 0.05, device=gpu)
    raw = rng.randn(P, E, O) * 0.3 + 0.1
    raw[:, :, 1] = 9.0  # normalises far beyond the clip at 10
    d_raw = torch.tensor(raw, device=gpu)
    shape, dt = ((P, E), torch.int32) if disc else ((P, E, A), torch.float32)
    ref, got = (torch.full(shape, int(SENTINEL), dtype=dt, device=gpu) for _ in range(2))
    d = Dims(P, 99, -3, O, A, K, 64, 0)  # N and T are ignored
    L = _lib.lib()
    m, v = _ptr(mean if use_ob else None), _ptr(var if use_ob else None)
    _lib.check((L.pgm_eval_act_cat if disc else L.pgm_eval_act)(C.byref(d), _ptr(tb.params), m, v, use_ob, _ptr(d_raw),
                                                               E, _ptr(ref), _stream()), 'pgm_eval_act')
    _lib.check(L.pgm_eval_act_any(C.byref(d), int(disc), _ptr(tb.params), m, v, use_ob, _ptr(d_raw), E, _ptr(got),
                                  _stream()), 'pgm_eval_act_any')
    assert (ref != int(SENTINEL)).all() and torch.equal(got, ref)


def _script(T, P, N):
    """test_env_ingest's flags: a done without bad, a done with bad, two dones in one step, a done in the last step."""
    done = np.zeros((T, P, N), dtype=bool)
    bad = np.zeros((T, P, N), dtype=bool)
    done[3, :, 0] = True
    done[5, :, N - 1] = bad[5, :, N - 1] = True
    done[7, :, :2] = True
    bad[7, 0, 0] = True
    done[T - 1, 1, N // 2] = bad[T - 1, 1, N // 2] = True
    return done, bad


def _ingest(tb, any_, t, obs, obj=None, rew=None, done=None, bad=None):
    d = [None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dt).to(tb.dev)
         for x, dt in ((obs, torch.float64), (obj, torch.float64), (rew, torch.float64), (done, torch.int32),
                       (bad, torch.int32))]
    fn, what = ((_lib.lib().pgm_env_ingest_any, 'pgm_env_ingest_any') if any_
                else (_lib.lib().pgm_env_ingest, 'pgm_env_ingest'))
    _lib.check(fn(C.byref(tb.dims), C.byref(tb.c_state), C.byref(tb.c_norm), C.byref(tb.c_rb), t,
                  *(_ptr(x) for x in d), _stream()), what)


INGEST_STATE = ('obs', 'rewards', 'masks', 'bad_masks', 'ret', 'obj_acc', 'obj_valid', 'ob_mean', 'ob_var', 'ob_count',
                'ret_mean', 'ret_var', 'ret_count', 'obj_mean', 'obj_var', 'obj_count')


def _ingest_prepare(tb):
    for name in ('obs', 'rewards', 'masks', 'bad_masks'):
        getattr(tb, name).fill_(SENTINEL)
    tb.ret.fill_(3.0)  # a reset must clear these
    tb.obj_valid.fill_(1)


@pytest.mark.parametrize('use_ob,use_obj', [(1, 1), (0, 0)])
@pytest.mark.parametrize('env,N', COMPILED)
def test_env_ingest_any_equals_compiled(gpu, env, N, use_ob, use_obj):
    """A reset and 12 scripted transitions through both kernels on two batches: every buffer and every running
    statistic bitwise equal after every step."""
    P, T = 2, 12
    kw = dict(gamma=0.995, ob_rms=bool(use_ob), obj_rms=bool(use_obj))
    spec, disc, ta, _ = _compiled_batch(env, P, N, T, **kw)
    _, _, tc, _ = _compiled_batch(env, P, N, T, **kw)
    O, K = spec['obs_dim'], spec['obj_num']
    rng = np.random.RandomState(100 * O + 10 * N + 2 * use_ob + use_obj)
    done, bad = _script(T, P, N)
    _ingest_prepare(ta)
    _ingest_prepare(tc)

    def same(what):
        for k in INGEST_STATE:
            assert torch.equal(getattr(ta, k), getattr(tc, k)), f'{what}: {k} differs from the compiled kernel'
    raw = rng.randn(P, N, O) * 0.4 + 0.2
    _ingest(ta, True, -1, raw)
    _ingest(tc, False, -1, raw)
    same('reset')
    for t in range(T):
        raw = rng.randn(P, N, O) * 0.4 + 0.2
        if t == 6:
            raw[:, :, 0] = 40.0  # far outside: the clip at +-clipob
        robj, rew = rng.randn(P, N, K) * 2.0 + 1.0, rng.randn(P, N) * 1.5 + 0.5
        _ingest(ta, True, t, raw, robj, rew, done[t], bad[t])
        _ingest(tc, False, t, raw, robj, rew, done[t], bad[t])
        same(f'step {t}')
    assert (ta.obs != SENTINEL).all() and (ta.rewards != SENTINEL).all()


# ------------------------------------------------------------------------------------------------ 2. fp64 reference
NEW_DIMS = [(d, False) for d in ar.GAUSS_DIMS] + [(d, True) for d in ar.CAT_DIMS]


@pytest.mark.parametrize('N', [1, 3, 8])
@pytest.mark.parametrize('dims,disc', NEW_DIMS)
def test_rollout_act_any(gpu, dims, disc, N):
    P, T = 3, 5
    seed, (pols, obs, rnd, refs, bad, margins) = ci.first_seed(lambda s: ar.forward_case(dims, disc, P, N, T, s))
    assert seed == ar.FORWARD_SEEDS.get((dims, disc, N), 0) and not bad, (seed, bad)  # the first seed counting up
    tb = _any_batch(dims, disc, P, N, T, pols)
    assert tb.actions.shape == (P, T, N, 1 if disc else dims[1])
    tb.obs.copy_(obs)
    tb.noise.copy_(rnd)
    out = _act_out(tb, disc, gpu)
    for t in (0, 2, 4, 5):
        val, act, lp, ao = _sentinel_step(tb, True, disc, t, out)
        for p in range(P):
            _close(val[p, t], refs[p]['values'][t], *VAL, f'value t={t}')
            if t == T:
                continue
            if disc:
                assert torch.equal(ao[p].long(), refs[p]['actions'][t]), f'task {p} t={t}: actions'
                _close(lp[p, t], refs[p]['logp'][t], *LP_C, f'log_prob t={t}')
            else:
                _close(act[p, t], refs[p]['actions'][t], *ACT, f'action t={t}')
                _close(lp[p, t], refs[p]['logp'][t], *LP_G, f'log_prob t={t}')


@pytest.mark.parametrize('E', [1, 8])
@pytest.mark.parametrize('dims,disc', NEW_DIMS)
def test_eval_act_any(gpu, dims, disc, E):
    P = 3
    seed, (pols, raw, rms, want, bad, margins) = ci.first_seed(lambda s: ar.eval_case(dims, disc, P, E, s))
    assert seed == 0 and not bad, (seed, bad)
    tb = _any_batch(dims, disc, P, 4, 8, pols)
    mean = torch.tensor(np.stack([r.mean for r in rms]), device=gpu)
    var = torch.tensor(np.stack([r.var for r in rms]), device=gpu)
    shape, dt = ((P, E), torch.int32) if disc else ((P, E, dims[1]), torch.float32)
    out = torch.full(shape, int(SENTINEL), dtype=dt, device=gpu)
    d = Dims(P, 99, -3, *dims, 64, 0)  # N and T are ignored
    _lib.check(_lib.lib().pgm_eval_act_any(C.byref(d), int(disc), _ptr(tb.params), _ptr(mean), _ptr(var), 1,
                                           _ptr(torch.tensor(raw, device=gpu)), E, _ptr(out), _stream()),
               'pgm_eval_act_any')
    if disc:
        np.testing.assert_array_equal(out.cpu().numpy(), want)
    else:
        _close(out.cpu(), want, *ACT, 'deterministic action')
    assert (np.abs((raw[0] - rms[0].mean) / np.sqrt(rms[0].var + 1e-8)) > 10.0).any(), 'the clip is exercised'


@pytest.mark.parametrize('N', [1, 3, 8])
@pytest.mark.parametrize('dims,disc', NEW_DIMS)
def test_env_ingest_any(gpu, dims, disc, N):
    """test_env_ingest's reset + 12 scripted transitions against the fp64 VecNormalize, in its bands, at every new dim
    set crossed with every N (the kernel's thread roles depend on N k, its loop bounds on o)."""
    P, T, gamma = 3, 12, 0.995
    O, _, K = dims
    tb = _any_batch(dims, disc, P, N, T, gamma=gamma)
    ref = [cat_ref.RefVecNormalize(N, O, gamma) for _ in range(P)]
    rng = np.random.RandomState(100 * O + 10 * N)
    done, bad = _script(T, P, N)
    _ingest_prepare(tb)
    raw = rng.randn(P, N, O) * 0.4 + 0.2
    _ingest(tb, True, -1, raw)
    for p in range(P):
        _close(tb.obs[p, 0].cpu(), ref[p].reset(raw[p]), 2e-6, 2e-6, 'reset obs')
    assert (tb.masks[:, 0] == 1).all() and (tb.bad_masks[:, 0] == 1).all() and (tb.obs[:, 1:] == SENTINEL).all()
    assert not tb.ret.cpu().numpy().any() and not tb.obj_valid.cpu().numpy().any()
    for t in range(T):
        raw = rng.randn(P, N, O) * 0.4 + 0.2
        if t == 6:
            raw[:, :, 0] = 40.0
        robj, rew = rng.randn(P, N, K) * 2.0 + 1.0, rng.randn(P, N) * 1.5 + 0.5
        _ingest(tb, True, t, raw, robj, rew, done[t], bad[t])
        assert (tb.obs[:, t + 2:] == SENTINEL).all() and (tb.rewards[:, t + 1:] == SENTINEL).all()
        for p in range(P):
            o, r = ref[p].step(raw[p], rew[p], done[t, p], robj[p])
            _close(tb.obs[p, t + 1].cpu(), o, 2e-6, 2e-6, f'obs step {t}')
            _close(tb.rewards[p, t].cpu(), r, 1e-5, 1e-6, f'rewards step {t}')
            np.testing.assert_array_equal(tb.masks[p, t + 1].cpu().numpy(), np.where(done[t, p], 0.0, 1.0))
            np.testing.assert_array_equal(tb.bad_masks[p, t + 1].cpu().numpy(), np.where(bad[t, p], 0.0, 1.0))
            _close(tb.ret[p].cpu(), ref[p].ret, 0, 1e-9, f'ret step {t}')
            _close(tb.obj_acc[p].cpu(), ref[p].obj, 0, 1e-9, f'obj accumulator step {t}')
    for p in range(P):
        for got, want, what in ((tb.ob_mean, ref[p].ob_rms.mean, 'ob_rms.mean'),
                                (tb.ob_var, ref[p].ob_rms.var, 'ob_rms.var'),
                                (tb.obj_mean, ref[p].obj_rms.mean, 'obj_rms.mean'),
                                (tb.obj_var, ref[p].obj_rms.var, 'obj_rms.var'),
                                (tb.ret_mean, ref[p].ret_rms.mean, 'ret_rms.mean'),
                                (tb.ret_var, ref[p].ret_rms.var, 'ret_rms.var')):
            _close(got[p].cpu(), want, 0, 1e-9, what)
        assert float(tb.ob_count[p]) == ref[p].ob_rms.count and float(tb.obj_count[p]) == ref[p].obj_rms.count


# ------------------------------------------------------------------------------------------------ 3. the update
def _update_batch(dims, disc, shape, row, any_dims=True):
    hp = ar.hparams(row)
    P, T, N, E, M = ar.SHAPES[shape]
    env = ar.case_env(dims, disc)
    if env in ar.COMPILED_ENVS.values():
        he = DeepSeaTreasureHostVecEnv(env, P, N) if disc else SynthHostVecEnv(env, P, N)
    else:
        he = ar.StubHostEnv(dims, disc, P, N)
    tb = TaskBatch(env, P, num_processes=N, num_steps=T, ppo_epoch=E, num_mini_batch=M, host_env=he,
                   clip_param=hp['clip_param'], value_loss_coef=hp['value_loss_coef'], entropy_coef=hp['entropy_coef'],
                   max_grad_norm=hp['max_grad_norm'], use_clipped_value_loss=hp['use_clipped_value_loss'],
                   any_dims=any_dims)
    tb.hp.adam_eps, tb.hp.beta1, tb.hp.beta2 = hp['adam_eps'], hp['beta1'], hp['beta2']
    return tb


def _load_update(tb, data, pols):
    for p, pol in enumerate(pols):
        tb.set_task(p, pol.state_dict())
    obs, actions, logp, values, returns, adv = data
    for dst, src in ((tb.obs, torch.from_numpy(obs)), (tb.actions, actions), (tb.logp, logp), (tb.values, values),
                     (tb.returns, returns), (tb.adv, adv)):
        dst.copy_(src)
    tb.lr.fill_(ar.bi.LR)


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


def _run_update(tb, case):
    (args, spec, pols, data, perms), results, worst = ar.update_case(*case)
    P, T, N, E, M = ar.SHAPES[case[2]]
    _load_update(tb, data, pols)
    tb.ppo_update(torch.stack(perms).numpy())
    assert int(tb.update_ws[2 * P]) == 0, 'tower exchange timed out'
    tb.check_update()
    _check_update(tb, results, f'{case}', E, M)
    return worst


@pytest.mark.parametrize('dims,disc,shape,row', ar.UPDATE_CASES)
def test_update_any(gpu, dims, disc, shape, row):
    """ppo_update_any_kernel at dims no kernel is compiled for: hyper-parameter rows a-f at (P 2, T 64, N 4, E 2, M 2),
    row a at the ragged shape and at P = 9.  Categorical row f: the reference without the entropy term is > 10 bands
    away (asserted by update_case)."""
    tb = _update_batch(dims, disc, shape, row)
    assert tb.update_variant() == 'ppo_update_any_kernel'
    worst = _run_update(tb, (dims, disc, shape, row))
    if row == 'f' and disc:
        assert worst['entropy term, x band'] > 10.0


@pytest.mark.parametrize('dims,disc,shape,row', ar.COMPILED_CASES)
def test_update_any_beside_the_compiled_kernel(gpu, dims, disc, shape, row):
    """17/6/2 and 3/4/2: the kernel TaskBatch picks there today and ppo_update_any_kernel on the same inputs, each
    inside the same bands of the same reference."""
    tc = _update_batch(dims, disc, shape, row, any_dims=False)
    assert 'any' not in tc.update_variant()
    _run_update(tc, (dims, disc, shape, row))
    ta = _update_batch(dims, disc, shape, row, any_dims=True)
    assert ta.update_variant() == 'ppo_update_any_kernel'
    _run_update(ta, (dims, disc, shape, row))


# ------------------------------------------------------------------------------------------------ 4. MOPG iterations
@pytest.mark.parametrize('disc', [False, True], ids=['Tiny-v0', 'TinyDiscrete-v0'])
def test_mopg_iterations_any(gpu, disc):
    """Two host-stepped MOPG iterations through TaskBatch on the tiny envs behind GymHostVecEnv against the reference
    worker, at test_mopg_iterations_end_to_end's tolerances; the storage shows true terminals."""
    c = ar.MOPG
    P, T, N, E, M, iters = (c[k] for k in ('P', 'T', 'N', 'E', 'M', 'iters'))
    seed = ar.MOPG_SEEDS[disc]
    for earlier in range(seed):
        assert ar.mopg_case(disc, earlier)[5], 'an earlier seed meets the conditions'
    name, args, pols, w, refs, bad, margins = ar.mopg_case(disc, seed)
    assert not bad, bad
    tb = TaskBatch(name, P, num_processes=N, num_steps=T, ppo_epoch=E, num_mini_batch=M,
                   host_env=ar.host_env(name, P, N))
    assert tb.any_dims and tb.discrete == disc
    for p, pol in enumerate(pols):
        tb.set_task(p, pol.state_dict(), {}, None, w[p])
    tb.env_reset()
    fn = ci.mopg_noise_fn(T, N, E) if disc else ar.gauss_noise_fn(T, N, tb.A, E)
    total = int(args.num_env_steps) // T // N
    for j in range(iters):
        rnd, perms = fn(j)
        tb.iteration(j, oppo.linear_lr(j, total, args.lr), noise=rnd, perms=torch.stack(perms).numpy(), carry=j > 0)
        objs, params = tb.objs.cpu().numpy().copy(), tb.params.cpu().numpy().copy()
        acts, rets = tb.actions.cpu(), tb.returns.cpu()
        masks, bads = tb.masks.cpu(), tb.bad_masks.cpu()
        if j == 0:
            assert int(((masks == 0) & (bads == 1)).sum()) > 0, 'a true terminal (masks 0, bad_masks 1) in the storage'
        for p in range(P):
            pol, ref_objs, st = refs[p][j]
            # (the storage of iteration j was snapshotted before after_update)
            if disc:
                assert torch.equal(acts[p].double(), st['actions']), f'task {p} iteration {j}: rollout actions'
            else:
                _close(acts[p], st['actions'], 5e-5, 1e-4, f'actions iter {j}')  # band of test_rollout
            _close(rets[p][:T], st['returns'][:T], 1e-5, 1e-5, f'returns iter {j}')  # band of test_gae
            _close(params[p], tb.layout.flatten(pol.state_dict(), dtype=np.float64), 2e-5, 1e-4, f'params iter {j}')
            _close(objs[p], ref_objs, *ar.OBJ_BAND, f'eval objs iter {j}')
    tb.check_update()
    tb.host_env.close()


# ------------------------------------------------------------------------------------------------ 5. the CLI
@pytest.mark.parametrize('rng', ['host', 'device'])
def test_cli_tiny(gpu, tmp_path, capsys, rng):
    """pgmorl_amd.run --env-name Tiny-v0 --host-env tests.anydims_envs:make_env at a tiny budget: the unknown env
    name is registered from one probe env, the results tree is written and final/objs.txt is finite."""
    from pgmorl_amd.run import main
    T, N = 32, 2
    argv = ['--env-name', envs.CONT, '--obj-num', '2', '--num-steps', str(T), '--num-processes', str(N),
            '--ppo-epoch', '1', '--num-mini-batch', '2', '--num-env-steps', str(T * N * 4), '--warmup-iter', '2',
            '--update-iter', '1', '--delta-weight', '0.5', '--selection-method', 'prediction-guided', '--save-dir',
            str(tmp_path), '--rl-log-interval', '1', '--rng', rng, '--pbuffer-num', '100', '--host-env',
            'tests.anydims_envs:make_env']
    prev = torch.get_default_dtype()
    try:
        main(argv)
    finally:
        torch.set_default_dtype(prev)
    capsys.readouterr()
    assert envs.CONT in envspec.user_env_names()
    for it in ('2', '3', '4'):
        for f in ('ep/objs.txt', 'population/objs.txt', 'elites/elites.txt', 'elites/offsprings.txt'):
            assert os.path.exists(tmp_path / it / f), f'{it}/{f}'
    for f in ('args.txt', 'log.txt', 'final/objs.txt', 'final/EP_policy_0.pt'):
        assert os.path.exists(tmp_path / f), f
    final = np.loadtxt(tmp_path / 'final' / 'objs.txt', delimiter=',', ndmin=2)
    assert final.shape[1] == 2 and np.isfinite(final).all()
    sd = torch.load(tmp_path / 'final' / 'EP_policy_0.pt')
    assert sd['base.actor.0.weight'].shape == (64, 5) and sd['dist.fc_mean.weight'].shape == (1, 64)


def test_capacity_slots_stay_untouched(gpu):
    """A batch of capacity P + 1 running P tasks: one iteration writes nothing in the spare slot."""
    P, T, N = 2, 32, 2
    envspec.register_env(envs.CONT, 5, 1, 2)
    tb = TaskBatch(envs.CONT, P, num_processes=N, num_steps=T, ppo_epoch=1, num_mini_batch=2, capacity=P + 1,
                   host_env=ar.host_env(envs.CONT, P + 1, N))
    pols = ar.make_policies(tb.spec, P, 0)
    for p, pol in enumerate(pols):
        tb.set_task(p, pol.state_dict(), {}, None, np.array([0.5, 0.5]))
    names = ('obs', 'actions', 'logp', 'values', 'returns', 'rewards', 'adv', 'masks', 'bad_masks', 'stats', 'objs',
             'ret', 'obj_acc', 'adam_step')
    for k in names:
        tb._full[k][P].fill_(int(SENTINEL))
    tb._state[:, P].fill_(SENTINEL)
    spare64 = tb._stats64.clone()
    tb.env_reset()
    tb.iteration(0, 3e-4)
    tb.check_update()
    for k in names:
        assert (tb._full[k][P] == int(SENTINEL)).all(), f'{k}: the slot past the active tasks was written'
    assert (tb._state[:, P] == SENTINEL).all(), 'parameters / Adam moments past the active tasks were written'
    live = tb.stat_views(tb._stats64.cpu().numpy(), P + 1)
    before = tb.stat_views(spare64.cpu().numpy(), P + 1)
    for k in live:
        assert np.array_equal(live[k][P], before[k][P]), f'{k}: the statistics slot past the active tasks was written'
    assert np.isfinite(tb.objs.cpu().numpy()).all()
    tb.host_env.close()
