"""Pareto-set re-evaluation on the device (pgm_eval_episodes, pgmorl_amd.evaluate) against pgm_eval's block kernel
(bit for bit, episode by episode), the CPU oracle (tests/eval_ref.py, the bands of tests/test_gpu_kernels.py; Humanoid
the 1e-3 + 2e-4 |ref| of tests/test_gpu_runs.py R4) and a finished tiny run.

Shapes: M = 3 policies, the episode limit cut to 20 steps through the spec (5 for the many-policy case), E in
{1, 8, 9, 17} (one row, a full chunk of 8, the chunk edge, a ragged third chunk).  The oracle runs once per family for
17 starts: the tables of smaller E are its prefixes (start e is the reset state of env seed eval_seed + e)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle.policy import make_policy
from oracle.vecenv import RunningMeanStd
from pgmorl_amd import _lib, envspec, evaluate
from pgmorl_amd.layout import ParamLayout
from pgmorl_amd.runtime import TaskBatch

from .eval_ref import episodes_ref
from .helpers import perturb

pytestmark = pytest.mark.gpu

STEPS, M, EMAX, SEED = 20, 3, 17, 41
# (env, layernorm, raw): dims 17/6/2, 11/3/3, LayerNorm 11/3/2 and 376/17/2
FAMILIES = [('MO-Walker2d-v2', False, True), ('MO-Hopper-v3', False, False), ('MO-Hopper-v2', True, False),
            ('MO-Humanoid-v2', False, True)]
GAMMA = 0.995


def _band(spec):
    return (1e-3, 2e-4) if spec['obs_dim'] > 48 else (1e-4, 1e-5)


def _close(a, b, band, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err = np.abs(a - b)
    bad = err > band[0] + band[1] * np.abs(b)
    print(f'{what}: max abs err {err.max():.3e} (band {band[0]:g} + {band[1]:g} |ref|)')
    assert not bad.any(), f'{what}: {bad.sum()}/{bad.size} off, max abs err {err.max():.3e}'


@functools.lru_cache(maxsize=None)
def _case(env, ln, logstd_shift=0.0):
    """The family's spec (20-step episodes), M fp32-rounded perturbed policies with their flat parameters, and
    per-policy observation statistics."""
    spec = dict(envspec.make_spec(env), max_episode_steps=STEPS)
    O, A, K = spec['obs_dim'], spec['act_dim'], spec['obj_num']
    torch.manual_seed(3)
    gen = torch.Generator().manual_seed(103)
    rng = np.random.RandomState(2)
    lay = ParamLayout(O, A, K, layernorm=ln)
    pols, stats = [], []
    for _ in range(M):
        pol = make_policy(O, A, K, layernorm=ln)
        with torch.no_grad():
            for prm in pol.parameters():
                prm.copy_(prm.float().double())
        pol = perturb(pol, 0.05, gen)
        with torch.no_grad():
            b = pol.dist.logstd._bias
            b.copy_((b + logstd_shift).float().double())
        pols.append(pol)
        r = RunningMeanStd(shape=(O,))
        r.update(rng.randn(50, O) * 0.3 + 0.1)
        stats.append(r)
    params = torch.from_numpy(np.stack([lay.flatten(p.state_dict()) for p in pols]))
    mean = torch.from_numpy(np.stack([r.mean for r in stats]))
    var = torch.from_numpy(np.stack([r.var for r in stats]))
    return spec, pols, stats, params, mean, var


@functools.lru_cache(maxsize=None)
def _oracle(env, ln, raw):
    """[M][EMAX][K] deterministic per-episode sums of the oracle, computed once per family."""
    spec, pols, stats, *_ = _case(env, ln)
    starts = envspec.reset_table(spec['obs_dim'], SEED, EMAX)
    ref = np.stack([episodes_ref(spec, starts, pols[m], stats[m], raw=raw, gamma=GAMMA) for m in range(M)])
    ref.setflags(write=False)
    return ref


def _run(env, ln, raw, E, params, mean, var, **kw):
    return evaluate.evaluate_policies(env, params, mean, var, E, SEED, gamma=GAMMA, raw=raw, layernorm=ln,
                                      max_episode_steps=kw.pop('steps', STEPS), return_objs=True, **kw)


def _in_order_mean(ep):
    acc = np.zeros((ep.shape[0], ep.shape[2]))
    for e in range(ep.shape[1]):
        acc = acc + ep[:, e]
    return acc / ep.shape[1]


# ------------------------------------------------------------------------------------------------ 1. pgm_eval, bitwise
@pytest.mark.parametrize('env,ln,raw', FAMILIES)
def test_episodes_equal_pgm_eval_block_kernel(gpu, monkeypatch, env, ln, raw):
    """episodes_out[m][e] is what pgm_eval's block kernel returns for eval_num = 1 from start row e: the two kernels run
    the same device functions row by row (no field needs a band)."""
    monkeypatch.setenv('PGM_EVAL_KERNEL', 'block')
    E = 9
    spec, pols, stats, *_ = _case(env, ln)
    tb = TaskBatch(env, M, num_processes=1, num_steps=8, eval_num=1, layernorm=ln, raw=raw, gamma=GAMMA)
    tb.c_spec.max_episode_steps = STEPS
    for p in range(M):
        tb.set_task(p, pols[p].state_dict())
        tb.set_env_params(p, {'ob_rms': stats[p]})
    ep, _ = _run(env, ln, raw, E, tb.params.clone().cpu(), tb.ob_mean.clone().cpu(), tb.ob_var.clone().cpu())
    starts = torch.tensor(envspec.reset_table(spec['obs_dim'], SEED, E), dtype=torch.float64, device=gpu)
    for e in range(E):
        tb.s0_eval.copy_(starts[e:e + 1])
        want = tb.evaluate().cpu()
        assert torch.equal(torch.from_numpy(ep[:, e]), want), f'episode {e}: {ep[:, e]} vs {want}'


# ------------------------------------------------------------------------------------------------ 2. the oracle
@pytest.mark.parametrize('E', [1, 8, 9, 17])
@pytest.mark.parametrize('env,ln,raw', FAMILIES)
def test_episodes_against_the_oracle(gpu, env, ln, raw, E):
    spec, _, _, params, mean, var = _case(env, ln)
    ep, objs = _run(env, ln, raw, E, params, mean, var)
    assert ep.shape == (M, E, spec['obj_num']) and objs.shape == (M, spec['obj_num'])
    _close(ep, _oracle(env, ln, raw)[:, :E], _band(spec), f'{env} ln={ln} E={E} episodes')
    np.testing.assert_array_equal(objs, _in_order_mean(ep))


def test_chunked_upload_equals_one_launch(gpu):
    env, ln, raw = FAMILIES[0]
    _, _, _, params, mean, var = _case(env, ln)
    one = _run(env, ln, raw, 9, params, mean, var)
    for chunk in (1, 2):
        got = _run(env, ln, raw, 9, params, mean, var, chunk=chunk)
        np.testing.assert_array_equal(got[0], one[0])
        np.testing.assert_array_equal(got[1], one[1])


def test_without_ob_rms(gpu):
    env, ln, raw = FAMILIES[1]
    spec, pols, _, params, _, _ = _case(env, ln)
    ep, _ = _run(env, ln, raw, 9, params, None, None, use_ob_rms=False)
    starts = envspec.reset_table(spec['obs_dim'], SEED, 9)
    ref = np.stack([episodes_ref(spec, starts, pols[m], None, raw=raw, gamma=GAMMA) for m in range(M)])
    _close(ep, ref, _band(spec), 'no ob_rms')


# ------------------------------------------------------------------------------------------------ 3. stochastic
@functools.lru_cache(maxsize=None)
def _stochastic_oracle(env, ln, raw, E):
    """The first noise seed, counting up from 0, at which no unclipped oracle action of any policy sits within 1e-4 of
    a clip bound (there the fp32 device action may clip where the fp64 one does not), and the oracle's episodes."""
    spec, pols, stats, *_ = _case(env, ln, -3.0)
    starts = envspec.reset_table(spec['obs_dim'], SEED, E)
    for seed in range(16):
        res = [episodes_ref(spec, starts, pols[m], stats[m], raw=raw, gamma=GAMMA, noise_seed=seed) for m in range(M)]
        if min(r[1] for r in res) >= 1e-4:
            return seed, np.stack([r[0] for r in res])
    raise AssertionError('no noise seed below 16 keeps every oracle action 1e-4 away from the clip bounds')


@pytest.mark.parametrize('env,ln,raw', [FAMILIES[0], FAMILIES[2]])
def test_stochastic_against_the_restated_stream(gpu, env, ln, raw):
    E = 9
    spec, _, _, params, mean, var = _case(env, ln, -3.0)  # exp(logstd) ~ 0.05
    seed, ref = _stochastic_oracle(env, ln, raw, E)
    ep, objs = _run(env, ln, raw, E, params, mean, var, stochastic=True, noise_seed=seed)
    _close(ep, ref, _band(spec), f'{env} ln={ln} stochastic (noise seed {seed})')
    np.testing.assert_array_equal(objs, _in_order_mean(ep))
    det, _ = _run(env, ln, raw, E, params, mean, var, noise_seed=seed)
    other, _ = _run(env, ln, raw, E, params, mean, var, stochastic=True, noise_seed=seed + 1)
    assert not np.array_equal(det, ep) and not np.array_equal(other, ep)
    # common random numbers: policies 0 and 2 with identical parameters and statistics see identical draws
    idx = [0, 1, 0]
    twin, _ = _run(env, ln, raw, E, params[idx], mean[idx], var[idx], stochastic=True, noise_seed=seed)
    np.testing.assert_array_equal(twin[0], twin[2])
    np.testing.assert_array_equal(twin[:2], ep[:2])
    # the deterministic policy does not read the noise seed
    det2, _ = _run(env, ln, raw, E, params, mean, var, noise_seed=seed + 12345)
    np.testing.assert_array_equal(det, det2)


# ------------------------------------------------------------------------------------------------ 4. many policies
def test_more_policies_than_twice_the_cus(gpu):
    """M = 600 workgroups of one row each (MI355X: 256 CUs): no co-residency is needed; policies 0, 299 and 599 are
    what single-policy launches give, bit for bit."""
    env, ln, raw = FAMILIES[0]
    _, _, _, params, mean, var = _case(env, ln)
    Mbig = 600
    assert Mbig > 2 * torch.cuda.get_device_properties(gpu).multi_processor_count
    g = torch.Generator().manual_seed(9)
    idx = torch.arange(Mbig) % M
    big = params[idx] + 0.01 * torch.randn(Mbig, params.shape[1], generator=g)
    bmean = mean[idx] + 0.01 * torch.randn(Mbig, mean.shape[1], generator=g, dtype=torch.float64)
    bvar = var[idx]
    ep, objs = _run(env, ln, raw, 1, big, bmean, bvar, steps=5)
    assert np.isfinite(ep).all() and len(np.unique(ep[:, 0, 0])) > Mbig // 2
    for m in (0, 299, 599):
        solo, solo_objs = _run(env, ln, raw, 1, big[m:m + 1], bmean[m:m + 1], bvar[m:m + 1], steps=5)
        np.testing.assert_array_equal(solo[0], ep[m])
        np.testing.assert_array_equal(solo_objs[0], objs[m])


# ------------------------------------------------------------------------------------------------ 5. sentinels
@pytest.mark.parametrize('E', [8, 9])
def test_spare_rows_keep_their_sentinel_and_objs_out_is_optional(gpu, E):
    env, ln, raw = FAMILIES[1]
    spec, _, _, params, mean, var = _case(env, ln)
    O, A, K = spec['obs_dim'], spec['act_dim'], spec['obj_num']
    f64 = dict(dtype=torch.float64, device=gpu)
    st = {k: torch.tensor(np.ascontiguousarray(spec[k]), **f64) for k in evaluate.SPEC_KEYS}
    c_spec = _lib.EnvSpec(*(C.c_void_p(st[k].data_ptr()) for k in evaluate.SPEC_KEYS), STEPS, 0)
    starts = torch.tensor(envspec.reset_table(O, SEED, E), **f64)
    prm, mu, vr = params.to(gpu), mean.to(gpu), var.to(gpu)
    d = _lib.Dims(M, 1, 0, O, A, K, 64, int(ln))

    def call(ep, objs):
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        _lib.check(_lib.lib().pgm_eval_episodes(C.byref(d), p(prm), C.byref(c_spec), p(mu), p(vr), p(starts), E, 1,
                                                int(raw), GAMMA, 0, 0, p(ep), p(objs),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'pgm_eval_episodes')
        torch.cuda.synchronize()

    ep = torch.full((M + 1, E, K), -123.0, **f64)
    objs = torch.full((M + 1, K), -123.0, **f64)
    call(ep, objs)
    assert (ep[M] == -123.0).all() and (objs[M] == -123.0).all(), 'the spare row was written'
    assert (ep[:M] != -123.0).all() and (objs[:M] != -123.0).all()
    want, want_objs = _run(env, ln, raw, E, params, mean, var)
    assert np.array_equal(ep[:M].cpu().numpy(), want) and np.array_equal(objs[:M].cpu().numpy(), want_objs)
    ep2 = torch.full((M + 1, E, K), -123.0, **f64)
    call(ep2, None)
    assert torch.equal(ep2, ep)


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_command_reproduces_the_stored_front(gpu, tmp_path, capsys):
    """A tiny finished run (Hopper-v2, T 32, N 2, --rng host, --eval-num 2), then the command with its defaults: E =
    eval_num episodes from the run's own seed are the episodes the run's evaluation (the wave kernel) measured, so
    eval/objs.txt reproduces final/objs.txt within the evaluation band (both files carry the '{:5f}' rounding, 5e-7)."""
    from pgmorl_amd.run import main
    T, N, eval_num = 32, 2, 2
    run = tmp_path / 'run'
    argv = ['--env-name', 'MO-Hopper-v2', '--obj-num', '2', '--num-steps', str(T), '--num-processes', str(N),
            '--ppo-epoch', '1', '--num-mini-batch', '2', '--num-env-steps', str(T * N * 4), '--warmup-iter', '2',
            '--update-iter', '1', '--delta-weight', '0.5', '--selection-method', 'prediction-guided', '--save-dir',
            str(run), '--rl-log-interval', '1', '--rng', 'host', '--pbuffer-num', '100', '--seed', '3', '--eval-num',
            str(eval_num)]
    prev = torch.get_default_dtype()
    try:
        main(argv)
    finally:
        torch.set_default_dtype(prev)
    stored = np.loadtxt(run / 'final' / 'objs.txt', delimiter=',', ndmin=2)
    summary = evaluate.main([str(run), '--episodes', str(eval_num)])
    capsys.readouterr()
    out = run / 'eval'
    got = np.loadtxt(out / 'objs.txt', delimiter=',', ndmin=2)
    assert got.shape == stored.shape and len(stored) >= 1
    _close(got, stored, (1e-4, 1e-5), 'eval/objs.txt vs final/objs.txt')
    # summary.json and objs.txt restate episodes.npy
    ep = np.load(out / 'episodes.npy')
    assert ep.shape == (len(stored), eval_num, 2) and ep.dtype == np.float64
    assert json.load(open(out / 'summary.json')) == summary
    assert (summary['M'], summary['E'], summary['eval_seed'], summary['stochastic']) == (len(stored), eval_num, 3, False)
    assert summary == evaluate.summarise(ep, stored, 3, 0, False)
    assert 1 <= summary['non_dominated'] <= len(stored)
    np.testing.assert_allclose(summary['mean_std_per_objective'], ep.std(axis=1).mean(axis=0), rtol=1e-12)
    fmt = '{:5f},{:5f}\n'
    assert (out / 'objs.txt').read_text() == ''.join(fmt.format(*o) for o in _in_order_mean(ep))
    # other start states: another front
    other = tmp_path / 'other'
    evaluate.main([str(run), '--episodes', str(eval_num), '--eval-seed', '4', '--out', str(other)])
    capsys.readouterr()
    assert (other / 'objs.txt').read_text() != (out / 'objs.txt').read_text()
    assert json.load(open(other / 'summary.json'))['eval_seed'] == 4
    assert sorted(os.listdir(other)) == ['episodes.npy', 'objs.txt', 'summary.json']
