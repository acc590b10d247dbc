"""The perf-mode random streams on the device against their numpy restatement (oracle/streams.py): pgm_uniform_noise
(bitwise), pgm_normal_noise (derived tolerance below), pgm_randperm (exact, at every size class of the LDS sort), the
counter draws inside every rollout kernel (bitwise against the same rollout fed pgm_normal_noise's stream, and the
stored actions teacher-forced against the restated stream's element [t][n][a]), and two perf-mode iterations against the oracle MOPG worker fed the restated streams.

Normal tolerance, derived and not measured: u1 and u2 are exact fp32 values on both sides.  The library is built
without any fast-math flag, so logf, sqrtf and cospif are the correctly-rounded-to-a-few-ulp OCML functions and the
two multiplies round once each: under about 8 ulp ~ 5e-7 relative on |z| <= 5.9, plus an absolute floor for the zeros
of the cosine.  Asserted: |dev - ref| <= 1e-6 + 2e-6 |ref| (the repository's bar is 1e-5)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ppo as oppo
from oracle import streams
from oracle.mopg import initial_sample, mopg_worker
from pgmorl_amd import _lib, envspec
from pgmorl_amd.runtime import TaskBatch

from .helpers import small_args, weights_grid
from .test_gpu_kernels import _batch_with_policies, _close
from .test_gpu_layernorm import _ln_batch

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
ISENT = -7
PAD = 8
SEEDS = (5, 0xC0FFEE1234567895)  # a small seed and one whose key product wraps 2^64
NOISE_N = (1, 999, (1 << 20) + 3)  # 2^20 + 3 > 4096 * 256 grid threads: the grid-stride loop wraps
NORMAL_ATOL, NORMAL_RTOL = 1e-6, 2e-6


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _draw(name, n, seed, gpu):
    """n draws of the named ABI stream into a sentinel-filled buffer; returns the draws after checking the tail."""
    buf = torch.full((n + PAD,), SENTINEL, device=gpu)
    _lib.check(getattr(_lib.lib(), name)(n, C.c_uint64(seed), _ptr(buf), _stream()), name)
    out = buf.cpu().numpy()
    assert (out[n:] == SENTINEL).all(), f'{name} wrote past n = {n}'
    return out[:n]


# ------------------------------------------------------------------------------------------------ 1. uniform stream
@pytest.mark.parametrize('seed', SEEDS)
def test_uniform_noise_is_the_restated_stream(gpu, seed):
    for n in NOISE_N:
        got = _draw('pgm_uniform_noise', n, seed, gpu)
        np.testing.assert_array_equal(got, streams.uniform(seed, n), err_msg=f'n = {n}')


# ------------------------------------------------------------------------------------------------ 2. normal stream
@pytest.fixture(scope='module')
def normal_ref():
    n = max(NOISE_N)
    return {seed: streams.normal(seed, n) for seed in SEEDS}


@pytest.mark.parametrize('seed', SEEDS)
def test_normal_noise_is_the_restated_stream(gpu, seed, normal_ref):
    """See the module docstring for the tolerance; the test prints the measured maximum next to it.  Measured on an
    MI355X over 2^20 + 3 draws: max |dev - ref| 5.4e-7 and 5.5e-7 at the two seeds, at most 0.09 of the bound; 42 % of
    the draws differ from the fp32 rounding of the restatement (so an oracle fed the stream takes the device's)."""
    ref = normal_ref[seed]
    got = {n: _draw('pgm_normal_noise', n, seed, gpu) for n in NOISE_N}
    for n in NOISE_N:
        dev = got[n].astype(np.float64)
        err = np.abs(dev - ref[:n])
        tol = NORMAL_ATOL + NORMAL_RTOL * np.abs(ref[:n])
        ulp_off = np.count_nonzero(got[n] != ref[:n].astype(np.float32))
        print(f'pgm_normal_noise seed {seed:#x} n {n}: max |dev - ref| {err.max():.3e}, '
              f'max err / tol {np.max(err / tol):.3f}, {ulp_off} of {n} differ from fp32(ref)')
        assert np.isfinite(dev).all()
        assert (err <= tol).all(), f'n = {n}: {np.count_nonzero(err > tol)} off, max abs err {err.max():.3e}'
    big = got[max(NOISE_N)]
    for n in NOISE_N:  # element i is keyed by (seed, i) alone: a shorter call is a prefix of a longer one
        np.testing.assert_array_equal(got[n], big[:n])


# ------------------------------------------------------------------------------------------------ 3. permutations
def _randperm(n, count, seed, gpu, size=None):
    buf = torch.full((count * n + PAD if size is None else size,), ISENT, dtype=torch.int32, device=gpu)
    rc = _lib.lib().pgm_randperm(n, count, C.c_uint64(seed), _ptr(buf), _stream())
    return rc, buf.cpu().numpy()


# minimum sizes; non-power-of-two (padding keys); exactly one workgroup pass and just past it; a power of two; the
# most padding; the LDS limit (128 KB of keys)
@pytest.mark.parametrize('n', [1, 2, 3, 150, 1024, 1025, 8192, 10000, 16384])
def test_randperm_is_the_restated_sort(gpu, n):
    for seed in SEEDS:
        for count in (1, 5) + ((64,) if n == 150 else ()):
            rc, out = _randperm(n, count, seed, gpu)
            _lib.check(rc, 'pgm_randperm')
            assert (out[count * n:] == ISENT).all(), f'n = {n} count = {count}: wrote past the last row'
            np.testing.assert_array_equal(out[:count * n].reshape(count, n), streams.randperms(seed, count, n),
                                          err_msg=f'n = {n} count = {count} seed = {seed:#x}')


def test_randperm_refusals_launch_nothing(gpu):
    L = _lib.lib()
    rc, out = _randperm(16385, 1, 5, gpu)
    assert rc == _lib.PGM_E_UNSUPPORTED and b'16385' in L.pgm_last_error()
    assert (out == ISENT).all()
    for n, count in ((0, 1), (1, 0), (-3, 1), (4, -1)):
        rc, out = _randperm(n, count, 5, gpu, size=64)
        assert rc == _lib.PGM_E_INVALID_ARG and L.pgm_last_error(), (n, count)
        assert (out == ISENT).all()


# ------------------------------------------------------------------------------------------------ 4. in-kernel draws
ENV_STATE = ('s', 'elapsed', 'obj_acc', 'obj_valid', 'ret')
RUNNING = ('ob_mean', 'ob_var', 'ob_count', 'obj_mean', 'obj_var', 'obj_count', 'ret_mean', 'ret_var', 'ret_count')
STORAGE = ('obs', 'actions', 'logp', 'values', 'rewards', 'masks', 'bad_masks')


def _counter_vs_explicit(tb, spec, pols, gpu, seed, carry):
    """rollout(seed, noise=None) and, from the same state, rollout(seed, noise=pgm_normal_noise(seed)): the same bits
    in every stored field, in the environment state and in the running statistics.  Both runs index the stream with
    the same code, so the stored actions are also checked teacher-forced against the restatement: the fp64 policy on
    the device's observation of step t with element [t][n][a] of streams.normal(seed), at test_rollout's band."""
    snap = {k: getattr(tb, k).clone() for k in ENV_STATE + RUNNING + STORAGE}
    tb.rollout(seed, noise=None, carry=carry)
    first = {k: getattr(tb, k).clone() for k in ENV_STATE + RUNNING + STORAGE}
    for k, v in snap.items():
        getattr(tb, k).copy_(v)
    nz = torch.full((tb.T * tb.N * spec['act_dim'] + PAD,), SENTINEL, device=gpu)
    _lib.check(_lib.lib().pgm_normal_noise(nz.numel() - PAD, C.c_uint64(seed), _ptr(nz), _stream()), 'noise')
    tb.rollout(seed, noise=nz[:-PAD].view(tb.T, tb.N, spec['act_dim']), carry=carry)
    for k in STORAGE + RUNNING + ENV_STATE:
        assert torch.equal(first[k], getattr(tb, k)), f'{k} differs between the counter draw and the explicit stream'
    assert not torch.equal(first['actions'], snap['actions']), 'the rollout stored no actions'
    T, N, O, A = tb.T, tb.N, spec['obs_dim'], spec['act_dim']
    eps = torch.from_numpy(streams.normal(seed, T * N * A).reshape(T * N, A))
    for p, pol in enumerate(pols):
        with torch.no_grad():
            _, action, _ = pol.act(first['obs'][p, :T].cpu().double().reshape(T * N, O), noise=eps)
        _close(first['actions'][p].cpu().reshape(T * N, A), action, 5e-5, 1e-4, f'actions of task {p} vs streams.normal')
    return first


# lanes: T < 32; a ragged last chunk; two chunk boundaries exactly; NE = 2 with a ragged third chunk; CR = 4 (A = 8);
# block: the workgroup-per-step kernel, also at the N the lane kernel does not take; wide: the Humanoid kernel with
# three chunks, two chunks and T < 32; ln: the LayerNorm towers (block kernel family)
@pytest.mark.parametrize('kernel,env,N,T', [
    ('lanes', 'MO-Walker2d-v2', 1, 33), ('lanes', 'MO-Walker2d-v2', 2, 70), ('lanes', 'MO-Walker2d-v2', 4, 64),
    ('lanes', 'MO-Walker2d-v2', 8, 95), ('lanes', 'MO-Ant-v2', 4, 40), ('lanes', 'MO-Hopper-v3', 8, 3),
    ('block', 'MO-Walker2d-v2', 4, 33), ('block', 'MO-Hopper-v3', 6, 40),
    ('wide', 'MO-Humanoid-v2', 8, 70), ('wide', 'MO-Humanoid-v2', 2, 33), ('wide', 'MO-Humanoid-v2', 1, 20),
    ('ln', 'MO-Walker2d-v2', 4, 70)])
def test_rollout_counter_draws_equal_explicit_stream(gpu, kernel, env, N, T, monkeypatch):
    monkeypatch.setenv('PGM_ROLLOUT_KERNEL', 'block' if kernel == 'block' else 'lanes')
    spec, tb, pols = (_ln_batch if kernel == 'ln' else _batch_with_policies)(env, 2, N, T)
    assert (spec['obs_dim'] > 48) == (kernel == 'wide')
    tb.env_reset()
    _counter_vs_explicit(tb, spec, pols, gpu, 77, carry=False)


@pytest.mark.parametrize('env,N,T', [('MO-Walker2d-v2', 4, 70), ('MO-Humanoid-v2', 4, 40)])
def test_rollout_counter_draws_carried(gpu, env, N, T, monkeypatch):
    """A second rollout with the after_update carry, keyed by the next seed (lane kernel and wide kernel)."""
    monkeypatch.setenv('PGM_ROLLOUT_KERNEL', 'lanes')
    spec, tb, pols = _batch_with_policies(env, 2, N, T)
    tb.env_reset()
    a0 = _counter_vs_explicit(tb, spec, pols, gpu, 3, carry=False)
    a1 = _counter_vs_explicit(tb, spec, pols, gpu, 4, carry=True)
    assert torch.equal(a1['obs'][:, 0], a0['obs'][:, T]) and not torch.equal(a0['actions'], a1['actions'])


# ------------------------------------------------------------------------------------------------ 5. perf-mode iteration
def test_perf_mode_iterations_against_the_oracle(gpu):
    """Two perf-mode iterations (tb.iteration(j, lr): no noise, no perms) against the oracle worker fed the restated
    streams.  This fixes the seed convention: iteration j keys both streams, permutation row c is PPO epoch c, and
    the noise is laid out [T][N][A].  The oracle consumes the device's own fp32 normals (they may differ from the
    rounded restatement by an ulp), after they are checked against the restatement at the derived tolerance."""
    env, P, N, T, E, M, iters = 'MO-Hopper-v2', 2, 4, 64, 2, 4, 2
    args = small_args(env, num_steps=T, num_processes=N, ppo_epoch=E, num_mini_batch=M, num_env_steps=T * N * 10)
    spec = envspec.make_spec(env)
    A, B = spec['act_dim'], T * N
    tb = TaskBatch(env, P, num_processes=N, num_steps=T, ppo_epoch=E, num_mini_batch=M)
    w = weights_grid(spec['obj_num'], P)
    torch.manual_seed(0)
    samples = [initial_sample(args, spec) for _ in range(P)]
    for s in samples:
        with torch.no_grad():
            for prm in s.actor_critic.parameters():
                prm.copy_(prm.float().double())
    for p, s in enumerate(samples):
        tb.set_task(p, s.actor_critic.state_dict(), {}, s.env_params, w[p])
    tb.env_reset()
    total = int(args.num_env_steps) // T // N
    gpu_objs, gpu_params, draws = [], [], {}
    for j in range(iters):
        tb.iteration(j, oppo.linear_lr(j, total, args.lr), carry=j > 0)
        gpu_objs.append(tb.objs.cpu().numpy().copy())
        gpu_params.append(tb.params.cpu().numpy().copy())
        dev_noise = tb.noise.cpu().numpy().astype(np.float64)
        ref_noise = streams.normal(j, T * N * A).reshape(T, N, A)
        err = np.abs(dev_noise - ref_noise)
        assert (err <= NORMAL_ATOL + NORMAL_RTOL * np.abs(ref_noise)).all(), f'noise of iteration {j}: {err.max():.3e}'
        ref_perms = streams.randperms(j, E, B)
        np.testing.assert_array_equal(tb.perms.cpu().numpy(), ref_perms, err_msg=f'perms of iteration {j}')
        draws[j] = (torch.from_numpy(dev_noise), [torch.from_numpy(r.astype(np.int64)) for r in ref_perms])
    s0_train = envspec.reset_table(spec['obs_dim'], 0, N)
    s0_eval = envspec.reset_table(spec['obs_dim'], 0, 1)
    for p in range(P):
        offs = mopg_worker(args, spec, s0_train, s0_eval, samples[p], w[p], 0, iters, noise_fn=draws.__getitem__)
        for j, off in enumerate(offs):
            ref = tb.layout.flatten(off.actor_critic.state_dict(), dtype=np.float64)
            _close(gpu_params[j][p], ref, 2e-5, 1e-4, f'params iter {j}')
            _close(gpu_objs[j][p], off.objs, 1e-3, 1e-4, f'eval objs iter {j}')
