"""Edges of the return sweep (pgm_gae) and of the advantage scalarisation + normalisation (pgm_adv_normalize) against
the fp64 oracle (oracle/ppo.py), called through the C ABI directly with hand-built pgm_dims / pgm_rollout_buf so that
every lane count is reachable.  Tolerance 1e-5 + 1e-5 |ref| as tests/test_gpu_kernels.py: both kernels accumulate
in fp64 from fp32 inputs and round once on the way out."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ppo as oppo
from pgmorl_amd import _lib
from pgmorl_amd._lib import Dims, RolloutBuf

from .helpers import weights_grid
from .test_gpu_kernels import _close, _random_storage

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
PAD = 8
GAMMA, LAM = 0.99, 0.95
FLAGS = [(True, True), (True, False), (False, True), (False, False)]


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(x, gpu, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=gpu, dtype=dtype)


def _gae(gpu, rew, val, masks, bad, use_gae, proper):
    """pgm_gae on [P][T][N][K] storage; returns (rc, returns [P][T+1][N][K] pre-filled with the sentinel, the
    sentinel words allocated behind it)."""
    P, T, N, K = rew.shape
    flat = torch.full((P * (T + 1) * N * K + PAD,), SENTINEL, device=gpu)
    t = [_dev(x, gpu) for x in (rew, val, masks, bad)]
    rb = RolloutBuf(values=_ptr(t[1]), rewards=_ptr(t[0]), masks=_ptr(t[2]), bad_masks=_ptr(t[3]),
                    returns=_ptr(flat))
    d = Dims(P, N, T, 11, 3, K, 64, 0)
    rc = _lib.lib().pgm_gae(C.byref(d), C.byref(rb), GAMMA, LAM, int(use_gae), int(proper), _stream())
    out = flat.cpu().numpy()
    return rc, out[:-PAD].reshape(P, T + 1, N, K), out[-PAD:]


def _gae_ref(rew, val, masks, bad, use_gae, proper):
    P, T, N, K = rew.shape
    out = np.zeros((P, T + 1, N, K))
    for p in range(P):
        r, v = torch.from_numpy(rew[p]).double(), torch.from_numpy(val[p]).double()
        m = torch.from_numpy(masks[p]).double().unsqueeze(-1)
        b = torch.from_numpy(bad[p]).double().unsqueeze(-1)
        ret = torch.zeros(T + 1, N, K, dtype=torch.float64)
        oppo.compute_returns_inplace(r, v.clone(), m, b, ret, v[-1], use_gae, GAMMA, LAM, proper)
        out[p] = ret.numpy()
    return out


def _check_gae(gpu, storage, use_gae, proper, what):
    rew, val, masks, bad = storage
    T = rew.shape[1]
    rc, got, tail = _gae(gpu, rew, val, masks, bad, use_gae, proper)
    _lib.check(rc, 'pgm_gae')
    ref = _gae_ref(rew, val, masks, bad, use_gae, proper)
    _close(got[:, :T], ref[:, :T], 1e-5, 1e-5, f'returns {what}')
    if use_gae:  # compute_returns leaves returns[T] alone under GAE (storage.py:83-98)
        assert (got[:, T] == SENTINEL).all(), 'GAE wrote returns[T]'
    else:        # returns[-1] = next_value (storage.py:100)
        np.testing.assert_array_equal(got[:, T], val[:, T])
    assert (tail == SENTINEL).all(), 'pgm_gae wrote past the returns'


# T = 1; Hopper-v3 production lanes (12 lanes: 85 chunks of 25 steps, the last one short, 4 threads idle); 3 lanes
# (341 chunks of 7 steps, one thread idle); N*K = 64 (16 chunks of 3 steps, the last two empty); N*K = 63 (16 chunks
# of 2 steps, 16 threads idle)
@pytest.mark.parametrize('use_gae,proper', FLAGS)
@pytest.mark.parametrize('N,K,T', [(4, 2, 1), (4, 3, 2048), (1, 3, 2048), (32, 2, 40), (21, 3, 17)])
def test_gae_lane_and_chunk_edges(gpu, use_gae, proper, N, K, T):
    _check_gae(gpu, _random_storage(3, T, N, K, seed=T + N), use_gae, proper, f'N={N} K={K} T={T}')


@pytest.mark.parametrize('use_gae,proper', FLAGS)
def test_gae_mask_patterns(gpu, use_gae, proper):
    """Masks the random 5 % does not give, at Hopper-v3's production lanes (chunks of 25 steps): env 0 done at every
    step; env 1 a time-limit cut (bad = 0) at steps 1 and T; env 2 done exactly on chunk boundaries, once together
    with bad = 0, and on both sides of one; env 3 the random pattern."""
    P, N, K, T = 2, 4, 3, 2048
    rew, val, masks, bad = _random_storage(P, T, N, K, seed=21)
    chunk = -(-T // (1024 // (N * K)))
    assert chunk == 25
    masks[:, :, 0] = 0.0
    bad[:, :, 0] = 1.0
    masks[:, :, 1], bad[:, :, 1] = 1.0, 1.0
    bad[:, [1, T], 1] = 0.0
    masks[:, 1, 1] = 0.0
    masks[:, :, 2], bad[:, :, 2] = 1.0, 1.0
    masks[:, [chunk, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1, 40 * chunk, 81 * chunk, T - 1], 2] = 0.0
    bad[:, 40 * chunk, 2] = 0.0
    _check_gae(gpu, (rew, val, masks, bad), use_gae, proper, 'mask patterns')


def test_gae_refuses_more_than_64_lanes(gpu):
    rew, val, masks, bad = _random_storage(1, 4, 33, 2, seed=1)
    rc, got, tail = _gae(gpu, rew, val, masks, bad, True, True)
    assert rc == _lib.PGM_E_SHAPE and b'N*K <= 64' in _lib.lib().pgm_last_error()
    assert (got == SENTINEL).all() and (tail == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ advantages
def _adv(gpu, R, V, w, var):
    """pgm_adv_normalize on [P][T+1][N][K] returns / values; (rc, adv [P][T][N] pre-filled, sentinel tail)."""
    P, T1, N, K = R.shape
    T = T1 - 1
    flat = torch.full((P * T * N + PAD,), SENTINEL, device=gpu)
    r, v = _dev(R, gpu), _dev(V, gpu)
    wd = _dev(w, gpu, torch.float64)
    vd = None if var is None else _dev(var, gpu, torch.float64)
    rb = RolloutBuf(values=_ptr(v), returns=_ptr(r), adv=_ptr(flat))
    d = Dims(P, N, T, 11, 3, K, 64, 0)
    rc = _lib.lib().pgm_adv_normalize(C.byref(d), C.byref(rb), _ptr(wd), _ptr(vd), _stream())
    out = flat.cpu().numpy()
    return rc, out[:-PAD].reshape(P, T, N), out[-PAD:]


def _check_adv(gpu, R, V, use_obj_rms, what):
    P, _, _, K = R.shape
    w = weights_grid(K, P)  # P distinct weight vectors
    var = np.random.RandomState(5).rand(P, K) * 4 + 0.1 if use_obj_rms else None
    rc, got, tail = _adv(gpu, R, V, w, var)
    _lib.check(rc, 'pgm_adv_normalize')
    for p in range(P):
        ref = oppo.scalarized_normalized_advantages(torch.from_numpy(R[p]).double(), torch.from_numpy(V[p]).double(),
                                                    w[p], None if var is None else var[p])
        _close(got[p], ref.numpy(), 1e-5, 1e-5, f'advantages {what} task {p}')
    assert (tail == SENTINEL).all(), 'pgm_adv_normalize wrote past the advantages'
    return got


def _rv(P, T, N, K, seed=5):
    rng = np.random.RandomState(seed)
    R = (rng.randn(P, T + 1, N, K) * 3 + 1).astype(np.float32)
    V = (rng.randn(P, T + 1, N, K) * 2).astype(np.float32)
    return R, V


# B = T*N against the kernel's 1024 threads: the minimum 2; 1023; 1025; 150 (Hopper-v3, K = 3); 8192
@pytest.mark.parametrize('use_obj_rms', [True, False])
@pytest.mark.parametrize('T,N,K', [(1, 2, 2), (341, 3, 3), (205, 5, 2), (50, 3, 3), (2048, 4, 2)])
def test_adv_normalize_batch_edges(gpu, use_obj_rms, T, N, K):
    R, V = _rv(3, T, N, K)
    got = _check_adv(gpu, R, V, use_obj_rms, f'T={T} N={N} K={K}')
    if T * N == 2:  # two samples normalise to -+ 1/sqrt(2) (up to the 1e-5 in the denominator)
        np.testing.assert_allclose(np.abs(got).reshape(3, 2), 2 ** -0.5, rtol=1e-4)


@pytest.mark.parametrize('use_obj_rms', [True, False])
def test_adv_normalize_large_common_offset(gpu, use_obj_rms):
    """returns and values both near +1000 with unit spread: the mean is removed in fp64, not in fp32."""
    rng = np.random.RandomState(6)
    R = (1000 + rng.randn(3, 513, 4, 2)).astype(np.float32)
    V = (1000 + rng.randn(3, 513, 4, 2)).astype(np.float32)
    _check_adv(gpu, R, V, use_obj_rms, 'offset 1000')


@pytest.mark.parametrize('use_obj_rms', [True, False])
def test_adv_normalize_near_constant_batch(gpu, use_obj_rms):
    """returns - values equal across the batch to within 1e-6: std is far below the 1e-5 added to it, which then
    sets the scale of the output."""
    rng = np.random.RandomState(7)
    V = rng.randn(3, 513, 4, 2).astype(np.float32)
    R = (V + np.float32(0.5)).astype(np.float32)  # fp32 rounding of the sum leaves ~1e-7 of spread
    x = R.astype(np.float64) - V.astype(np.float64)
    spread = x.max(axis=(1, 2)) - x.min(axis=(1, 2))
    assert (spread <= 1e-6).all() and (spread > 0).all(), spread
    got = _check_adv(gpu, R, V, use_obj_rms, 'near-constant')
    assert np.abs(got).max() < 0.2  # ~ spread / 1e-5: nowhere near unit variance


def test_adv_normalize_refuses_one_sample(gpu):
    R, V = _rv(1, 1, 1, 2)
    rc, got, tail = _adv(gpu, R, V, weights_grid(2, 1), None)
    assert rc == _lib.PGM_E_SHAPE and _lib.lib().pgm_last_error()
    assert (got == SENTINEL).all() and (tail == SENTINEL).all()
