"""oracle/streams.py on its own (CPU): the numpy restatement of the perf-mode counter streams is a sound normal
stream and an unbiased permutation stream.  Every condition is a fixed-seed, deterministic statement; the bounds are
5-6 standard errors of the statistic under the exact distribution, never fitted to a device."""
import itertools
import math
from statistics import NormalDist

import numpy as np
import pytest

from oracle import streams

M64 = (1 << 64) - 1
N_NORMAL = 1 << 20


def _py_splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def test_splitmix64_known_answers_and_wraparound():
    # the first outputs of the published splitmix64 generator seeded with 0 (state += golden, then the finaliser)
    assert int(streams.splitmix64(0)) == 0xE220A8397B1DCDAF
    assert int(streams.splitmix64(0x9E3779B97F4A7C15)) == 0x6E789E6AA1B965F4
    xs = [0, 1, 77, 2**63, M64, 0xDEADBEEFCAFEF00D]
    got = streams.splitmix64(np.array(xs, dtype=np.uint64))
    assert [int(g) for g in got] == [_py_splitmix64(x) for x in xs]


@pytest.mark.parametrize('seed', [0, 1, 9, 77, 2**40 + 3, M64])
def test_hash_matches_python_integers(seed):
    key = _py_splitmix64((seed * 0xD1B54A32D192ED03 + 0x632BE59BD9B4E019) & M64)
    assert int(streams.stream_key(seed)) == key
    idx = [0, 1, 2, 12345, 2**32 + 5]
    got = streams.hash_at(seed, np.array(idx, dtype=np.uint64))
    assert [int(g) for g in got] == [_py_splitmix64(key ^ i) for i in idx]
    h = [_py_splitmix64(key ^ i) for i in range(8)]
    np.testing.assert_array_equal(streams.uniform(seed, 8), np.array([(x >> 40) / 2.0**24 for x in h], np.float32))
    np.testing.assert_array_equal(streams.uniform(seed, 5, start=3), streams.uniform(seed, 8)[3:])
    np.testing.assert_array_equal(streams.normal(seed, 5, start=3), streams.normal(seed, 8)[3:])


def test_uniform_range_and_moments():
    u = streams.uniform(3, N_NORMAL)
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    u = u.astype(np.float64)
    assert abs(u.mean() - 0.5) <= 5 * math.sqrt(1 / 12 / u.size)
    assert abs(u.var() - 1 / 12) <= 5 * math.sqrt(1 / 180 / u.size)


def test_normal_u1_is_formed_in_fp32():
    """(top24 + 0.5f) rounds to nearest even in fp32 once top24 >= 2^23: u1 is in (0, 1], and reaches 1 only through
    that rounding (z = 0, harmless); log(0) cannot happen."""
    top = np.array([0, 1, 2**23 - 1, 2**23, 2**23 + 1, 2**24 - 2, 2**24 - 1], dtype=np.uint64)
    u1 = (top.astype(np.float32) + np.float32(0.5)) * np.float32(2.0**-24)
    assert u1.dtype == np.float32
    exact = (top.astype(np.float64) + 0.5) * 2.0**-24
    np.testing.assert_array_equal(u1[:3], exact[:3].astype(np.float32))   # below 2^23 the half is representable
    assert u1[3] == np.float32(2.0**23 * 2.0**-24)                         # 2^23 + 0.5 -> 2^23 (tie to even)
    assert u1[4] == np.float32((2.0**23 + 2) * 2.0**-24)                   # 2^23 + 1.5 -> 2^23 + 2
    assert u1[-1] == np.float32(1.0) and u1.min() > 0
    a, b = streams.normal_uniforms(9, 1 << 16)
    assert a.dtype == np.float32 and b.dtype == np.float32
    assert a.min() > 0 and a.max() <= 1 and b.min() >= 0 and b.max() < 1


@pytest.fixture(scope='module')
def normals():
    return {s: streams.normal(s, N_NORMAL) for s in (0, 1, 9, 10)}


@pytest.mark.parametrize('seed', [0, 1, 9])
def test_normal_stream_statistics(normals, seed):
    z = normals[seed]
    n = z.size
    assert z.dtype == np.float64 and np.isfinite(z).all()
    assert np.abs(z).max() <= math.sqrt(-2.0 * math.log(2.0**-25))  # the smallest u1 is 2^-25
    mean, std = z.mean(), z.std(ddof=1)
    skew, kurt = np.mean(z**3), np.mean(z**4)
    lag1 = np.corrcoef(z[:-1], z[1:])[0, 1]
    print(f'seed {seed}: mean {mean:.3e} std {std:.6f} Ez3 {skew:.3e} Ez4 {kurt:.5f} lag1 {lag1:.3e}')
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(std - 1) <= 5 / math.sqrt(2 * n)
    assert abs(skew) <= 5 * math.sqrt(15 / n)
    assert abs(kurt - 3) <= 5 * math.sqrt(96 / n)
    assert abs(lag1) <= 5 / math.sqrt(n)
    edges = np.array([NormalDist().inv_cdf(k / 64) for k in range(1, 64)])
    counts = np.bincount(np.searchsorted(edges, z), minlength=64)
    sigma = math.sqrt(n * (1 / 64) * (63 / 64))
    dev = np.abs(counts - n / 64).max() / sigma
    print(f'seed {seed}: worst of 64 equiprobable bins {dev:.2f} sigma')
    assert counts.sum() == n and dev <= 6


def test_normal_streams_of_neighbouring_seeds_are_uncorrelated(normals):
    r = np.corrcoef(normals[9], normals[10])[0, 1]
    print(f'seed 9 / seed 10 correlation {r:.3e}')
    assert abs(r) <= 5 / math.sqrt(N_NORMAL)


@pytest.mark.parametrize('seed', [0, 5])
def test_permutations_of_six_are_uniform(seed):
    rows = streams.randperms(seed, 72000, 6)
    assert rows.shape == (72000, 6) and rows.dtype == np.int32
    code = np.zeros(rows.shape[0], dtype=np.int64)
    for col in range(6):
        code = code * 6 + rows[:, col]
    valid = {sum(v * 6**(5 - k) for k, v in enumerate(p)) for p in itertools.permutations(range(6))}
    vals, counts = np.unique(code, return_counts=True)
    assert set(vals.tolist()) == valid, 'every row is a permutation and all 720 occur'
    chi2 = float(((counts - 100.0)**2 / 100.0).sum())
    print(f'seed {seed}: chi2 {chi2:.1f} over 719 degrees of freedom')
    assert chi2 <= 719 + 6 * math.sqrt(2 * 719)


@pytest.mark.parametrize('n,rows', [(150, 4096), (1000, 1024)])
def test_permutation_positions_are_unbiased(n, rows):
    perms = streams.randperms(0, rows, n)
    np.testing.assert_array_equal(np.sort(perms, axis=1), np.broadcast_to(np.arange(n), (rows, n)))
    sigma = math.sqrt((n * n - 1) / 12 / rows)
    dev = np.abs(perms.mean(axis=0) - (n - 1) / 2).max() / sigma
    print(f'n {n}: worst position mean {dev:.2f} sigma')
    assert dev <= 6


def test_randperm_rows_and_single_row_agree():
    many = streams.randperms(5, 4, 37)
    for c in range(4):
        np.testing.assert_array_equal(streams.randperm(5, c, 37), many[c])
    assert len({r.tobytes() for r in many}) == 4
    np.testing.assert_array_equal(streams.randperm(5, 0, 1), [0])
