"""numpy restatement of the perf-mode counter streams -- TEST INFRASTRUCTURE ONLY.

The device draws its perf-mode randomness from stateless counter streams (pgmorl_amd/csrc/pgm_common.hpp
``counter_normal``, pgm_hostenv.hip ``counter_uniform``, pgm_misc.hip ``randperm_kernel``): element ``i`` of stream
``seed`` is a function of ``(seed, i)`` alone.  This module states those functions once more, independently, in
uint64 arithmetic with wrap-around:

    splitmix64(x)            the 64-bit finaliser (Steele, Lea, Flood 2014)
    stream_key(seed)       = splitmix64(seed * 0xD1B54A32D192ED03 + 0x632BE59BD9B4E019)
    hash_at(seed, i)       = splitmix64(stream_key(seed) ^ i)
    uniform(seed, n)         float32(h >> 40) * 2^-24                           exact in fp32: the device matches bitwise
    normal(seed, n)          sqrt(-2 ln u1) cos(2 pi u2), u1, u2 formed in fp32  fp64 result: the device matches to ulps
    randperm(seed, c, n)     argsort of (splitmix64(s ^ i) & ~0xFFFFFFFF) | i    exact: a sort of distinct keys

Seed convention of an iteration (pgmorl_amd.runtime.TaskBatch.iteration): iteration ``j`` keys both streams, the
noise is laid out ``[T][N][A]`` and permutation row ``c`` is PPO epoch ``c``.
"""
import numpy as np

U64 = np.uint64
_GOLDEN = U64(0x9E3779B97F4A7C15)
_KEY_MUL = U64(0xD1B54A32D192ED03)
_KEY_ADD = U64(0x632BE59BD9B4E019)
_INV24 = np.float32(1.0 / 16777216.0)


def splitmix64(x):
    """splitmix64 of a uint64 scalar or array (wraps modulo 2^64)."""
    x = np.asarray(x, dtype=U64)
    with np.errstate(over='ignore'):
        x = x + _GOLDEN
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def _u64(v):
    return np.asarray(int(v) & 0xFFFFFFFFFFFFFFFF, dtype=U64)


def stream_key(seed):
    with np.errstate(over='ignore'):
        return splitmix64(_u64(seed) * _KEY_MUL + _KEY_ADD)


def hash_at(seed, i):
    """The 64-bit hash of element(s) ``i`` of stream ``seed``."""
    return splitmix64(stream_key(seed) ^ np.asarray(i, dtype=U64))


def uniform(seed, n, start=0):
    """fp32 uniforms in [0, 1) with 24 random bits: elements start .. start + n - 1 of stream ``seed``."""
    h = hash_at(seed, np.arange(start, start + n, dtype=U64))
    return (h >> U64(40)).astype(np.float32) * _INV24


def normal_uniforms(seed, n, start=0):
    """(u1, u2) of the Box-Muller draw, formed in fp32 as the device forms them.  The top 24 bits plus one half are
    rounded to fp32 (round to nearest even) before the scaling, so for h >> 40 >= 2^23 the half rounds away and
    u1 lies in (0, 1]: u1 = 1 gives z = 0.  u2 lies in [0, 1)."""
    h = hash_at(seed, np.arange(start, start + n, dtype=U64))
    u1 = ((h >> U64(40)).astype(np.float32) + np.float32(0.5)) * _INV24
    u2 = (h & U64(0xFFFFFF)).astype(np.float32) * _INV24
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    return u1, u2


def normal(seed, n, start=0):
    """fp64 standard normals: Box-Muller's cosine branch on the fp32 uniforms of ``normal_uniforms``."""
    u1, u2 = normal_uniforms(seed, n, start)
    u1, u2 = u1.astype(np.float64), u2.astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def randperm_keys(seed, c, n):
    """The n distinct 64-bit sort keys of permutation row(s) ``c``: a 32-bit hash above the element's index.
    ``c`` may be an array of rows; the keys then have shape c.shape + (n,)."""
    c = np.asarray(c, dtype=U64)
    with np.errstate(over='ignore'):
        s = splitmix64(_u64(seed) * _GOLDEN + c * _KEY_MUL + U64(1))
    i = np.arange(n, dtype=U64)
    return (splitmix64(s[..., None] ^ i) & U64(0xFFFFFFFF00000000)) | i


def randperm(seed, c, n):
    """Row(s) ``c`` of the permutations of 0..n-1 keyed by ``seed``: the low words of the sorted keys."""
    keys = np.sort(randperm_keys(seed, c, n), axis=-1)
    return (keys & U64(0xFFFFFFFF)).astype(np.int32)


def randperms(seed, count, n):
    """Rows 0 .. count-1 as one [count, n] int32 array."""
    return randperm(seed, np.arange(count), n)
