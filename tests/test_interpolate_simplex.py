"""CPU-side checks of the simplex blends of the dense-front tool (pgmorl_amd.interpolate --simplex / pgm_eval_blend3):
the entry point's argument refusals (before any device work, in pgm_eval_blend's order), the unchanged version pair and
feature values, blend3's definition and its three exact consequences, the neighbour triangles, the simplex candidate
table, the table check, the analysis on constructed means, and the command's refusals and files with a constructed
evaluator -- with and without --simplex.  No kernel is launched here: every ABI call below stops at a refusal."""
import ctypes as C
import io
import json
import os

import numpy as np
import pytest
import torch

from pgmorl_amd import _lib, evaluate, interpolate
from pgmorl_amd._lib import PGM_E_INVALID_ARG, PGM_E_SHAPE, PGM_E_UNSUPPORTED, PGMError
from pgmorl_amd.layout import ParamLayout
from pgmorl_amd.pareto import compute_hypervolume, compute_sparsity, get_ep_indices

from .test_interpolate import _refused, _write_run

ONE = C.c_void_p(1)  # a non-NULL pointer nothing dereferences: every call below is refused before device work
NAME = 'pgm_eval_blend3'


def _err():
    return _lib.lib().pgm_last_error().decode()


# ------------------------------------------------------------------------------------------------ ABI
def test_symbol_is_present_and_the_abi_values_are_unchanged():
    L = _lib.lib()
    assert _lib.has_eval_blend3() and all(hasattr(L, s) for s in _lib.EVAL_BLEND3_SYMBOLS)
    _lib.require_eval_blend3()
    assert NAME in _lib.EXPORTS and _lib.has_eval_blend() and _lib.has_eval_episodes()
    assert (L.pgm_abi_version(), L.pgm_abi_minor()) == (5, 1)
    assert L.pgm_abi_features() == 7 and L.pgm_abi_feature_mask() == 15


def _call(dims=None, params=ONE, M=3, ob_mean=ONE, ob_var=ONE, src=ONE, w=ONE, spec_null=False, spec_steps=20,
          spec_ptr=True, starts=ONE, E=9, use_ob=1, out=ONE, objs=ONE, dims_ptr=True):
    d = dict(P=7, N=4, T=64, O=17, A=6, K=2, H=64, LN=0)
    d.update(dims or {})
    spec = _lib.EnvSpec(*([None if spec_null else ONE] * 8), spec_steps, 0)
    dd = _lib.Dims(*(d[k] for k in ('P', 'N', 'T', 'O', 'A', 'K', 'H', 'LN')))
    return _lib.lib().pgm_eval_blend3(C.byref(dd) if dims_ptr else None, params, M, ob_mean, ob_var, src, w,
                                      C.byref(spec) if spec_ptr else None, starts, E, use_ob, 1, 0.995, out, objs, None)


MATERIALISE = 'materialise the candidates and use pgm_eval_episodes'
# pgm_eval_blend's order: (what is wrong, variants, status, a piece of the message); every entry is tried with every
# later entry wrong as well (where two entries change the same field, the earlier entry's value stays)
ORDER = [
    ('null', [dict(params=None), dict(src=None), dict(w=None), dict(starts=None), dict(out=None),
              dict(ob_mean=None), dict(ob_var=None), dict(spec_ptr=False), dict(dims_ptr=False)],
     PGM_E_INVALID_ARG, 'null pointer'),
    ('dims', [dict(dims=dict(P=0)), dict(dims=dict(K=0))], PGM_E_SHAPE, 'non-positive dims'),
    ('dims H', [dict(dims=dict(H=32))], PGM_E_UNSUPPORTED, 'hidden size'),
    ('LN', [dict(dims=dict(LN=2))], PGM_E_INVALID_ARG, 'pgm_dims.LN'),
    ('LN Humanoid', [dict(dims=dict(O=376, A=17, LN=1))], PGM_E_UNSUPPORTED, 'LayerNorm towers are built'),
    ('LN = 1', [dict(dims=dict(LN=1)), dict(dims=dict(O=11, A=3, K=3, LN=1))], PGM_E_UNSUPPORTED, MATERIALISE),
    ('spec', [dict(spec_null=True), dict(spec_steps=0)], PGM_E_INVALID_ARG, 'env spec'),
    ('M', [dict(M=0), dict(M=-2)], PGM_E_SHAPE, 'members outside'),
    ('E', [dict(E=0), dict(E=65537), dict(E=-3)], PGM_E_SHAPE, 'episodes per candidate outside [1, 65536]'),
    ('Q * E', [dict(dims=dict(P=1 << 20), E=65536)], PGM_E_SHAPE, 'waves of one call'),
    ('dim set', [dict(dims=dict(O=19)), dict(dims=dict(O=376, A=17))], PGM_E_UNSUPPORTED, None),
]
DIM_SET_TEXT = {19: 'unsupported dims O=19 A=6 K=2', 376: MATERIALISE}


def _merge(a, b):
    out = dict(a)
    for k, v in b.items():
        out[k] = dict(v, **out[k]) if k == 'dims' and k in out else out.get(k, v)  # the earlier entry's fields win
    return out


def test_refusals_in_the_documented_order():
    for i, (what, variants, rc, text) in enumerate(ORDER):
        for kw in variants:
            want = DIM_SET_TEXT[kw['dims']['O']] if text is None else text
            assert _call(**kw) == rc and want in _err() and _err().startswith(NAME + ':'), (what, kw, _err())
            later = dict(kw)
            for _, later_variants, _, _ in ORDER[i + 1:]:
                later = _merge(later, later_variants[0])
            got = _call(**later)
            assert got == rc and want in _err() and _err().startswith(NAME + ':'), (what, later, got, _err())


def test_a_call_that_passes_every_argument_check_stops_at_the_dim_set():
    """What the entry point accepts, as far as a host can tell without device work: the call passes every argument
    check and is stopped by the last one (a dim set no kernel is compiled for)."""
    last = dict(dims=dict(O=19))
    assert _call(**last) == PGM_E_UNSUPPORTED and 'unsupported dims' in _err()
    assert _call(use_ob=0, ob_mean=None, ob_var=None, objs=None, **last) == PGM_E_UNSUPPORTED
    assert 'unsupported dims' in _err()
    assert _call(use_ob=1, ob_var=None, **last) == PGM_E_INVALID_ARG
    assert _call(dims=dict(N=9, T=-1, O=19)) == PGM_E_UNSUPPORTED and 'unsupported dims' in _err()
    assert _call(dims=dict(P=256, O=19), E=65536) == PGM_E_UNSUPPORTED and 'unsupported dims' in _err()
    assert _call(dims=dict(O=376, A=17)) == PGM_E_UNSUPPORTED and MATERIALISE in _err()
    assert _err().startswith(NAME + ':')


# ------------------------------------------------------------------------------------------------ blend3
def _members(M=4, L=37, O=5, seed=0):
    rng = np.random.RandomState(seed)
    return (rng.randn(M, L).astype(np.float32), rng.randn(M, O), rng.rand(M, O) + 0.5)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


def test_blend3_members_pairs_swap_and_definition():
    prm, mean, var = _members()
    alphas = [0.0, 1.0, 0.5, 0.3, 1 / 3, 0.7, 5 / 16]
    rows = [(i, i, i, 1.0, 0.0, 0.0) for i in range(4)]                         # 0..3: the members
    rows += [(0, 1, 1, 1.0 - al, al, 0.0) for al in alphas]                     # 4..10: pairs as triples
    rows += [(0, 1, 2, 0.5, 0.25, 0.25), (1, 0, 2, 0.25, 0.5, 0.25),            # 11, 12: the first two slots swapped
             (2, 3, 1, 0.2, 0.3, 0.5), (3, 2, 1, 0.3, 0.2, 0.5),                # 13, 14
             (0, 1, 2, 1 / 3, 1 / 3, 1 / 3), (3, 3, 2, 0.5, 0.5, 0.0), (1, 2, 3, 1 / 6, 2 / 6, 3 / 6)]
    table = interpolate.make_table3(rows)
    assert table[0].dtype == np.int32 and table[0].shape == (len(rows), 3)
    assert table[1].dtype == np.float64 and table[1].shape == (len(rows), 3)
    bp, bm, bv = interpolate.blend3(prm, mean, var, table)
    assert bp.dtype == np.float32 and bm.dtype == bv.dtype == np.float64
    assert bp.shape == (len(rows), prm.shape[1]) and bm.shape == bv.shape == (len(rows), mean.shape[1])
    for got, x in ((bp, prm), (bm, mean), (bv, var)):
        # member rows are the members, bit for bit
        np.testing.assert_array_equal(_bits(got[:4]), _bits(x))
        # the swap of the first two (index, weight) slots changes no bit
        np.testing.assert_array_equal(_bits(got[11]), _bits(got[12]))
        np.testing.assert_array_equal(_bits(got[13]), _bits(got[14]))
    # pair rows == blend's
    pp, pm, pv = interpolate.blend(prm, mean, var, interpolate.make_table([(0, 1, al) for al in alphas]))
    assert (bp[4:11] == pp).all() and (bm[4:11] == pm).all() and (bv[4:11] == pv).all()
    # the documented expression, written out
    src, w = table
    wa, wb, wc = (w[:, i, None] for i in range(3))
    f64 = np.float64
    A, B, Cc = (prm[src[:, i]].astype(f64) for i in range(3))
    np.testing.assert_array_equal(_bits(bp), _bits(((wa * A + wb * B) + wc * Cc).astype(np.float32)))
    for got, x in ((bm, mean), (bv, var)):
        np.testing.assert_array_equal(_bits(got), _bits((wa * x[src[:, 0]] + wb * x[src[:, 1]]) + wc * x[src[:, 2]]))
    # torch in, torch out, the same values; statistics are optional
    tp, tm, tv = interpolate.blend3(torch.from_numpy(prm), torch.from_numpy(mean), torch.from_numpy(var), table)
    assert isinstance(tp, torch.Tensor) and tp.dtype == torch.float32 and tm.dtype == tv.dtype == torch.float64
    assert np.array_equal(tp.numpy(), bp) and np.array_equal(tm.numpy(), bm) and np.array_equal(tv.numpy(), bv)
    only = interpolate.blend3(prm, None, None, table)
    assert np.array_equal(only[0], bp) and only[1] is None and only[2] is None
    with pytest.raises(PGMError, match=r'blend3: candidate 1 names members \(0, 1, 4\)'):
        interpolate.blend3(prm, mean, var, interpolate.make_table3([(0, 1, 2, 0.5, 0.25, 0.25), (0, 1, 4, 1, 0, 0)]))


# ------------------------------------------------------------------------------------------------ the table check
def test_check_table3_names_the_candidate_it_rejects():
    good = interpolate.make_table3([(0, 0, 0, 1.0, 0.0, 0.0), (0, 1, 2, 0.5, 0.25, 0.25)])
    src, w = interpolate._check_table3(good, 3, 'x')
    assert np.array_equal(src, good[0]) and np.array_equal(w, good[1])
    interpolate._check_table3(interpolate.make_table3([(0, 1, 2, 1 / 3, 1 / 3, 1 / 3 + 5e-10)]), 3, 'x')  # inside 1e-9

    def refused(text, table, M=3):
        with pytest.raises(PGMError, match=text):
            interpolate._check_table3(table, M, 'where')

    mk = interpolate.make_table3
    refused('where: table must be the pair', (good[0],))
    refused('where: table must be the pair', 7)
    refused(r'table src must be int32 \[Q\]\[3\]', (good[0].astype(np.int64), good[1]))
    refused(r'table src must be int32 \[Q\]\[3\]', (good[0][:, :2], good[1]))
    refused(r'table src must be int32 \[Q\]\[3\]', (good[0].tolist(), good[1]))
    refused(r'table w must be fp64 \[2\]\[3\]', (good[0], good[1].astype(np.float32)))
    refused(r'table w must be fp64 \[2\]\[3\]', (good[0], good[1][:1]))
    refused(r'table w must be fp64 \[2\]\[3\]', (good[0], good[1][:, :2]))
    refused('no candidates', (good[0][:0], good[1][:0]))
    refused(r'candidate 1 names members \(0, 1, 3\) outside \[0, 3\)', mk([(0, 1, 2, 1, 0, 0), (0, 1, 3, 1, 0, 0)]))
    refused(r'candidate 0 names members \(-1, 1, 2\)', mk([(-1, 1, 2, 1, 0, 0)]))
    refused(r'candidate 0 names members \(0, 2, 1\) outside \[0, 2\)', mk([(0, 2, 1, 1, 0, 0)]), M=2)
    refused(r'candidate 2 has weights \(1.5, 0.0, -0.5\) outside \[0, 1\]',
            mk([(0, 1, 2, 1, 0, 0), (0, 1, 2, 0, 1, 0), (0, 1, 2, 1.5, 0.0, -0.5)]))
    refused(r'candidate 0 has weights \(0.5, nan, 0.5\)', mk([(0, 1, 2, 0.5, float('nan'), 0.5)]))
    refused(r'candidate 1 has weights \(0.5, 0.5, -0.0001\)', mk([(0, 1, 2, 1, 0, 0), (0, 1, 2, 0.5, 0.5, -1e-4)]))
    refused(r'candidate 1 has weights summing to 0.75', mk([(0, 1, 2, 1, 0, 0), (0, 1, 2, 0.25, 0.25, 0.25)]))
    refused(r'candidate 0 has weights summing to 1.0000000\d+, not to 1 within 1e-09', mk([(0, 1, 2, 0.5, 0.25, 0.25 + 3e-9)]))
    refused(r'candidate 0 has weights summing to 1.5', mk([(0, 1, 2, 0.5, 0.5, 0.5)]))


def test_evaluate_candidates3_refuses_bad_arguments_before_the_library(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(interpolate, 'lib', no_library)
    monkeypatch.setattr(interpolate, 'require_eval_blend3', no_library)
    monkeypatch.setattr(interpolate, 'evaluate_policies', no_library)
    lay = ParamLayout(11, 3, 3)
    prm, st = torch.zeros(2, lay.total), torch.ones(2, 11, dtype=torch.float64)
    table = interpolate.make_table3([(0, 0, 0, 1, 0, 0), (0, 1, 1, 0.5, 0.5, 0)])

    def refused(text, tbl=table, p=prm, mean=st, var=st, env='MO-Hopper-v3', **kw):
        with pytest.raises(PGMError, match=text):
            interpolate.evaluate_candidates3(env, p, mean, var, tbl, **dict(dict(episodes=4, eval_seed=0, device='cpu'), **kw))

    refused(r'evaluate_candidates3: candidate 1 names members \(0, 1, 2\) outside \[0, 2\)',
            interpolate.make_table3([(0, 1, 1, 1, 0, 0), (0, 1, 2, 1, 0, 0)]))
    refused('candidate 0 has weights summing to 0.5', interpolate.make_table3([(0, 1, 1, 0.25, 0.25, 0)]))
    refused(r'table src must be int32 \[Q\]\[3\]', interpolate.make_table([(0, 1, 0.5)]))  # a pair table
    refused('episodes=0', episodes=0)
    refused('chunk=0', chunk=0)
    refused('max_episode_steps=0', max_episode_steps=0)
    refused('evaluate_candidates3: params must be fp32', p=prm[:, :-1])
    refused('ob_mean is required', mean=None)
    refused('covers the SynthMO device envs', env='MO-Dummy3-v0')


# ------------------------------------------------------------------------------------------------ neighbour triangles
def _plane(uv):
    """Points (u, v, 20 - u - v): mutually non-dominated."""
    return np.array([[u, v, 20.0 - u - v] for u, v in uv])


def test_neighbour_triangles_known_answers():
    # two clusters of three, far apart.  Scaled: u and v by 6, the third objective (20 .. 9) by 11.
    six = _plane([(0, 0), (1, 0), (0, 1), (5, 5), (6, 5), (5, 6)])
    # neighbours = 2: every member pairs with its two cluster mates
    assert interpolate.neighbour_pairs(six, 2) == [(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5)]
    assert interpolate.neighbour_triangles(six, 2) == [(0, 1, 2), (3, 4, 5)]
    assert interpolate.neighbour_triangles(six) == [(0, 1, 2), (3, 4, 5)]
    # neighbours = 1: the nearest mate only (0-1, 1-0, 2-0, 3-4, 4-3, 5-3): no three mutual edges
    assert interpolate.neighbour_pairs(six, 1) == [(0, 1), (0, 2), (3, 4), (3, 5)]
    assert interpolate.neighbour_triangles(six, 1) == []
    # neighbours = 3: each member adds its nearest member of the other cluster -- 0, 1, 2 -> 3 (5, 5); 3 -> 1 (a tie
    # with 2, the lower index; both edges exist anyway); 4 (6, 5) -> 1 (1, 0); 5 (5, 6) -> 2 (0, 1)
    assert interpolate.neighbour_pairs(six, 3) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (1, 4), (2, 3), (2, 5),
                                                   (3, 4), (3, 5), (4, 5)]
    assert interpolate.neighbour_triangles(six, 3) == [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3), (1, 3, 4), (2, 3, 5),
                                                       (3, 4, 5)]
    # every pair -> every triple
    assert interpolate.neighbour_triangles(six, 5) == [(a, b, c) for a in range(6) for b in range(a + 1, 6)
                                                       for c in range(b + 1, 6)]
    # the middle objective constant (it scales to 0): test_interpolate's four points, scaled (0, 1), (.25, .33),
    # (1, 0), (.5, .17); neighbours = 2 gives the pairs (0,1) (0,3) (1,2) (1,3) (2,3)
    pts = np.array([[0, 5, 7], [1, 5, 3], [4, 5, 1], [2, 5, 2]], dtype=np.float64)
    assert interpolate.neighbour_triangles(pts, 1) == []
    assert interpolate.neighbour_pairs(pts, 2) == [(0, 1), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert interpolate.neighbour_triangles(pts, 2) == [(0, 1, 3), (1, 2, 3)]
    assert interpolate.neighbour_triangles(pts, 3) == [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]
    # M = 1, M = 2: none; M = 3 with neighbours = 2: one
    assert interpolate.neighbour_triangles(six[:1], 2) == [] and interpolate.neighbour_triangles(six[:2], 2) == []
    assert interpolate.neighbour_triangles(six[:3], 2) == [(0, 1, 2)]
    assert interpolate.neighbour_triangles(six[:3], 1) == []
    with pytest.raises(PGMError, match='neighbours=0'):
        interpolate.neighbour_triangles(six, 0)


# ------------------------------------------------------------------------------------------------ candidate table
def test_candidate_table3_rows_lattice_and_weights():
    pairs, triangles = [(0, 2), (1, 2)], [(0, 1, 2), (1, 2, 3)]
    for points in (2, 3, 4, 5, 15):
        src, w = interpolate.candidate_table3(4, pairs, triangles, points)
        per = points * (points - 1) // 2
        Q = 4 + 2 * points + 2 * per
        assert src.dtype == np.int32 and w.dtype == np.float64 and src.shape == w.shape == (Q, 3)
        assert np.abs((w[:, 0] + w[:, 1]) + w[:, 2] - 1.0).max() <= 1e-12 and (w >= 0).all() and (w <= 1).all()
        interpolate._check_table3((src, w), 4, 'x')
        # members
        assert src[:4].tolist() == [[i, i, i] for i in range(4)] and w[:4].tolist() == [[1.0, 0.0, 0.0]] * 4
        # pairs: (a, b, b, 1 - alpha_j, alpha_j, 0) with candidate_table's alphas and the fp64 subtraction 1 - alpha
        s2, alpha = interpolate.candidate_table(4, pairs, points)
        n2 = 4 + 2 * points
        assert src[4:n2, :2].tolist() == s2[4:].tolist() and src[4:n2, 2].tolist() == s2[4:, 1].tolist()
        assert w[4:n2, 1].tolist() == alpha[4:].tolist() and w[4:n2, 0].tolist() == (1.0 - alpha[4:]).tolist()
        assert (w[4:n2, 2] == 0.0).all()
        # triangles: i ascending, then j ascending, in Python floats
        n = points + 1
        lattice = [(i, j, n - i - j) for i in range(1, n) for j in range(1, n) if n - i - j >= 1]
        assert len(lattice) == per and lattice == sorted(lattice)
        for t, tri in enumerate(triangles):
            rows = slice(n2 + t * per, n2 + (t + 1) * per)
            assert src[rows].tolist() == [list(tri)] * per
            assert w[rows].tolist() == [[i / n, j / n, k / n] for i, j, k in lattice]
    src, w = interpolate.candidate_table3(4, pairs, triangles, 3)
    assert w[4 + 6:4 + 6 + 3].tolist() == [[0.25, 0.25, 0.5], [0.25, 0.5, 0.25], [0.5, 0.25, 0.25]]
    # points = 1: a triangle has no interior lattice point; no triangles: the pair table as triples
    assert len(interpolate.candidate_table3(4, pairs, triangles, 1)[0]) == 4 + 2
    src, w = interpolate.candidate_table3(1, [], [], 7)
    assert src.tolist() == [[0, 0, 0]] and w.tolist() == [[1.0, 0.0, 0.0]]


# ------------------------------------------------------------------------------------------------ analyse3
def _constructed3():
    """4 members, pairs (0,1) and (1,2), triangles (0,1,2) and (0,1,3), 3 points: 3 rows per pair and per triangle."""
    members = [[4.0, 1.0, 1.0], [1.0, 4.0, 1.0], [1.0, 1.0, 4.0], [3.0, 3.0, 0.5]]
    pair_rows = [[3.5, 2.0, 1.0], [2.8, 2.8, 1.0], [2.0, 3.5, 1.0],    # (0,1): none dominated
                 [1.0, 3.5, 2.0], [0.9, 2.5, 2.5], [1.0, 2.0, 3.5]]    # (1,2)
    tri_rows = [[2.5, 2.5, 2.5], [2.0, 3.0, 2.0], [3.0, 2.0, 2.0],     # (0,1,2): none dominated
                [3.2, 2.9, 0.6], [2.9, 2.9, 0.4], [2.9, 3.2, 0.6]]     # (0,1,3): the second is dominated by member 3
    table = interpolate.candidate_table3(4, [(0, 1), (1, 2)], [(0, 1, 2), (0, 1, 3)], 3)
    return table, np.array(members + pair_rows + tri_rows)


def test_analyse3_on_constructed_means():
    table, means = _constructed3()
    an = interpolate.analyse3(table, means, 4, 3, 2, 2)
    assert an['triangles'] == [(0, 1, 2), (0, 1, 3)] and an['filled'] == [True, False]
    assert (an['num_triangles'], an['num_filled']) == (2, 1)
    # the pair results are analyse's on the member and pair rows
    t2 = interpolate.candidate_table(4, [(0, 1), (1, 2)], 3)
    an2 = interpolate.analyse(t2, means[:10], 4, 3)
    for k in ('pairs', 'connected', 'family', 'families', 'M', 'points', 'num_pairs', 'num_connected', 'num_families',
              'family_sizes', 'members'):
        assert an[k] == an2[k], k
    assert an['pairs'] == [(0, 1), (1, 2)] and an['connected'] == [True, True] and an['families'] == [[0, 1, 2], [3]]
    # the dense front is over all Q rows
    assert an['Q'] == 16 and an['front'] == get_ep_indices(means) and 14 not in an['front'] and 10 in an['front']
    assert an['dense'] == {'hypervolume': compute_hypervolume(means[an['front']]),
                           'sparsity': compute_sparsity(means[an['front']])}
    assert (an['dense_front_size'], an['dense_front_interpolants']) == (len(an['front']), sum(i >= 4 for i in an['front']))
    assert set(an) == set(an2) | {'triangles', 'filled', 'num_triangles', 'num_filled'}
    # an interior point EQUAL to a member's mean is not dominated by it; one that loses in one objective and ties the
    # others is
    eq = means.copy()
    eq[14] = [3.0, 3.0, 0.5]
    assert interpolate.analyse3(table, eq, 4, 3, 2, 2)['filled'] == [True, True]
    eq[14] = [3.0, 3.0, 0.49]
    assert interpolate.analyse3(table, eq, 4, 3, 2, 2)['filled'] == [True, False]
    # a dominated pair row breaks the pair and leaves the triangles alone, and the reverse
    m2 = means.copy()
    m2[8] = [0.9, 2.5, 0.9]  # (1,2)'s middle row, dominated by member 1
    an3 = interpolate.analyse3(table, m2, 4, 3, 2, 2)
    assert an3['connected'] == [True, False] and an3['filled'] == [True, False] and an3['families'] == [[0, 1], [2], [3]]
    m2 = means.copy()
    m2[10] = [0.5, 0.5, 3.9]  # (0,1,2)'s first row, dominated by member 2
    an3 = interpolate.analyse3(table, m2, 4, 3, 2, 2)
    assert an3['connected'] == [True, True] and an3['filled'] == [False, False] and an3['num_filled'] == 0
    # no triangles: analyse on the pair rows, the front included
    an0 = interpolate.analyse3((table[0][:10], table[1][:10]), means[:10], 4, 3, 2, 0)
    assert an0['triangles'] == [] and an0['filled'] == [] and an0['front'] == an2['front'] and an0['dense'] == an2['dense']
    with pytest.raises(PGMError, match='are not 4 members, 2 pairs of 3 points and 1 triangles of 3 points'):
        interpolate.analyse3(table, means, 4, 3, 2, 1)
    with pytest.raises(PGMError, match='are not pair rows'):
        interpolate.analyse3(table, means, 4, 3, 3, 1)
    src = table[0].copy()
    src[6] = [1, 2, 2]
    with pytest.raises(PGMError, match=r'analyse3: rows 4..6 of the table are not one pair'):
        interpolate.analyse3((src, table[1]), means, 4, 3, 2, 2)
    src = table[0].copy()
    src[11] = [0, 1, 3]
    with pytest.raises(PGMError, match=r'analyse3: rows 10..12 of the table are not one triangle'):
        interpolate.analyse3((src, table[1]), means, 4, 3, 2, 2)
    src = table[0].copy()
    src[1] = [0, 0, 0]
    with pytest.raises(PGMError, match='the first M rows of the table are not the members'):
        interpolate.analyse3((src, table[1]), means, 4, 3, 2, 2)
    with pytest.raises(PGMError, match='means must be'):
        interpolate.analyse3(table, means[:-1], 4, 3, 2, 2)


# ------------------------------------------------------------------------------------------------ the command
def _write_run3(save_dir, **kw):
    _write_run(save_dir, env='MO-Hopper-v3', O=11, A=3, K=3, **kw)


def test_cli_refusals_leave_no_out_dir(tmp_path, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('a refused call reached the evaluator')
    monkeypatch.setattr(interpolate, 'evaluate_candidates', no_device)
    monkeypatch.setattr(interpolate, 'evaluate_candidates3', no_device)
    out = tmp_path / 'elsewhere'
    two, three = tmp_path / 'two', tmp_path / 'three'
    _write_run(two)
    _write_run3(three)
    # a two-objective run
    _refused([two, '--simplex'], r'--simplex: the run has --obj-num 2', two / 'continuous')
    _refused([two, '--simplex', '--out', out, '--save-policies'], r'--simplex: the run has --obj-num 2', out,
             two / 'continuous')
    # no interior lattice points
    for run in (two, three):
        _refused([run, '--simplex', '--points', '1'], r'--simplex with --points 1', run / 'continuous')
        _refused([run, '--simplex', '--points', '1', '--out', out], r'--simplex with --points 1', out, run / 'continuous')
    # the refusals the command already had stay in front
    _refused([three, '--simplex', '--points', '0'], r'--points 0: outside \[1, 1024\]', three / 'continuous')
    _refused([three, '--simplex', '--episodes', '0', '--out', out], '--episodes', out, three / 'continuous')
    _refused([tmp_path / 'nothing', '--simplex'], 'no args.txt', tmp_path / 'nothing' / 'continuous')


def _in_order_mean(ep):
    acc = np.zeros((ep.shape[0], ep.shape[2]))
    for e in range(ep.shape[1]):
        acc = acc + ep[:, e]
    return acc / ep.shape[1]


def _fake_evaluator3(stored, calls):
    """evaluate_candidates3 with constructed numbers: candidate (a, b, c, wa, wb, wc) measures the blend of the stored
    objectives plus a bulge of (wa wb + wb wc + wc wa) / 5, so no interpolant is dominated by a member; episode e adds
    e / 8."""
    def fake(env_name, params, ob_mean, ob_var, table, episodes, eval_seed, **kw):
        calls.append(dict(kw, env_name=env_name, episodes=episodes, eval_seed=eval_seed))
        src, w = table
        assert src.shape[1] == 3 and w.shape == src.shape
        wa, wb, wc = (w[:, i, None] for i in range(3))
        base = wa * stored[src[:, 0]] + wb * stored[src[:, 1]] + wc * stored[src[:, 2]]
        base = base + 0.2 * (wa * wb + wb * wc + wc * wa)
        ep = base[:, None, :] + np.arange(episodes)[None, :, None] / 8.0
        return ep, _in_order_mean(ep)
    return fake


@pytest.mark.parametrize('save', [False, True])
def test_simplex_command_files_with_a_constructed_evaluator(tmp_path, monkeypatch, capsys, save):
    run = tmp_path / 'run'
    _write_run3(run)
    args, params, ob_mean, ob_var, stored = evaluate.load_pareto_set(str(run))
    assert stored.shape == (4, 3)
    calls = []
    monkeypatch.setattr(interpolate, 'evaluate_candidates3', _fake_evaluator3(stored, calls))

    def not_this_one(*a, **k):
        raise AssertionError('--simplex reached evaluate_candidates')
    monkeypatch.setattr(interpolate, 'evaluate_candidates', not_this_one)
    points, E, M = 3, 2, 4
    out = run / 'continuous' if not save else tmp_path / 'dense'
    argv = [str(run), '--simplex', '--points', str(points), '--episodes', str(E)]
    summary = interpolate.main(argv + (['--out', str(out), '--save-policies'] if save else []))
    assert 'of 2 triangles filled' in capsys.readouterr().out
    assert len(calls) == 1 and calls[0]['eval_seed'] == 5 and calls[0]['episodes'] == E
    assert (calls[0]['gamma'], calls[0]['raw'], calls[0]['use_ob_rms'], calls[0]['layernorm']) == (0.995, True, True, False)
    pairs = interpolate.neighbour_pairs(stored, 2)
    triangles = interpolate.neighbour_triangles(stored, 2)
    assert pairs == [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)] and triangles == [(0, 1, 2), (1, 2, 3)]
    table = interpolate.candidate_table3(M, pairs, triangles, points)
    Q = M + len(pairs) * points + len(triangles) * 3
    want = sorted(['candidates.txt', 'objs.txt', 'episodes.npy', 'segments.txt', 'triangles.txt', 'front.txt',
                   'summary.json'] + (['args.txt', 'final'] if save else []))
    assert sorted(os.listdir(out)) == want
    # candidates.txt: a,b,c,repr(wa),repr(wb),repr(wc)
    lines = (out / 'candidates.txt').read_text().splitlines()
    assert lines == [f'{a},{b},{c},{float(wa)!r},{float(wb)!r},{float(wc)!r}'
                     for (a, b, c), (wa, wb, wc) in zip(table[0], table[1])]
    assert lines[:M] == [f'{i},{i},{i},1.0,0.0,0.0' for i in range(M)] and lines[M] == '0,1,1,0.75,0.25,0.0'
    assert lines[M + 15] == '0,1,2,0.25,0.25,0.5' and len(lines) == Q
    # episodes.npy, objs.txt
    ep = np.load(out / 'episodes.npy')
    assert ep.shape == (Q, E, 3) and ep.dtype == np.float64
    means = _in_order_mean(ep)
    assert (out / 'objs.txt').read_text() == ''.join('{:5f},{:5f},{:5f}\n'.format(*o) for o in means)
    # segments.txt, triangles.txt, front.txt and summary.json restate analyse3
    an = interpolate.analyse3(table, means, M, points, len(pairs), len(triangles))
    assert an['connected'] == [True] * 5 and an['filled'] == [True, True] and M < len(an['front']) <= Q
    assert (out / 'segments.txt').read_text().splitlines() == [f'{a},{b},1,0' for a, b in pairs]
    assert (out / 'triangles.txt').read_text().splitlines() == ['0,1,2,1', '1,2,3,1']
    assert [int(x) for x in (out / 'front.txt').read_text().split()] == an['front']
    assert any(i >= M + len(pairs) * points for i in an['front']), 'no triangle candidate on the dense front'
    assert json.load(open(out / 'summary.json')) == summary
    base = interpolate.summarise(an, stored, 2, E, 5, 5)
    assert summary == dict(base, simplex=True, num_triangles=2, num_filled=2)
    assert (summary['M'], summary['Q'], summary['points'], summary['num_pairs']) == (M, Q, points, 5)
    assert summary['dense']['hypervolume'] == compute_hypervolume(means[an['front']])
    if not save:
        return
    # --save-policies: --out is a save dir holding the dense front's policies in front.txt order, through blend3
    assert (out / 'args.txt').read_text() == (run / 'args.txt').read_text()
    args2, params2, mean2, var2, stored2 = evaluate.load_pareto_set(str(out))
    assert (args2.env_name, args2.seed, args2.obj_num) == (args.env_name, args.seed, 3) and len(stored2) == len(an['front'])
    front = np.asarray(an['front'])
    bp, bm, bv = interpolate.blend3(params, ob_mean, ob_var, (table[0][front], table[1][front]))
    assert torch.equal(params2, bp) and torch.equal(mean2, bm) and torch.equal(var2, bv)
    for j, i in enumerate(an['front']):
        if i < M:  # a member is the member
            assert torch.equal(params2[j], params[i]) and torch.equal(mean2[j], ob_mean[i])
    np.testing.assert_array_equal(stored2, np.array([[float('{:5f}'.format(x)) for x in means[i]] for i in an['front']]))


def test_without_simplex_the_command_writes_what_it_wrote(tmp_path, monkeypatch, capsys):
    """No --simplex, on a two- and on a three-objective run: every file is, byte for byte, what the functions the
    module had before the flag give (candidate_table, analyse, summarise, blend), and no simplex name appears."""
    from .test_interpolate import _fake_evaluator

    def not_this_one(*a, **k):
        raise AssertionError('the command reached evaluate_candidates3 without --simplex')
    monkeypatch.setattr(interpolate, 'evaluate_candidates3', not_this_one)
    for name, write, K in (('two', _write_run, 2), ('three', _write_run3, 3)):
        run = tmp_path / name
        write(run)
        args, params, ob_mean, ob_var, stored = evaluate.load_pareto_set(str(run))
        calls = []
        monkeypatch.setattr(interpolate, 'evaluate_candidates', _fake_evaluator(stored, calls))
        points, E, M = 4, 3, 4
        summary = interpolate.main([str(run), '--points', str(points), '--episodes', str(E), '--save-policies'])
        text = capsys.readouterr().out
        assert 'triangles' not in text and len(calls) == 1
        out = run / 'continuous'
        assert sorted(os.listdir(out)) == ['args.txt', 'candidates.txt', 'episodes.npy', 'final', 'front.txt',
                                           'objs.txt', 'segments.txt', 'summary.json']
        pairs = interpolate.neighbour_pairs(stored, 2)
        table = interpolate.candidate_table(M, pairs, points)
        ep, means = _fake_evaluator(stored, [])(args.env_name, params, ob_mean, ob_var, table, E, 5)
        an = interpolate.analyse(table, means, M, points)
        want_summary = interpolate.summarise(an, stored, 2, E, 5, 5)
        assert summary == want_summary and not {'simplex', 'num_triangles', 'num_filled'} & set(summary)
        fmt = '{:5f}' + (K - 1) * ',{:5f}' + '\n'
        npy = io.BytesIO()
        np.save(npy, ep)
        want = {
            'candidates.txt': ''.join(f'{a},{b},{float(al)!r}\n' for (a, b), al in zip(*table)).encode(),
            'objs.txt': ''.join(fmt.format(*o) for o in means).encode(),
            'episodes.npy': npy.getvalue(),
            'segments.txt': ''.join(f'{a},{b},{int(ok)},{an["family"][a]}\n'
                                    for (a, b), ok in zip(an['pairs'], an['connected'])).encode(),
            'front.txt': ''.join(f'{i}\n' for i in an['front']).encode(),
            'summary.json': json.dumps(want_summary, indent=1).encode(),
            'args.txt': (run / 'args.txt').read_bytes(),
            'final/objs.txt': ''.join(fmt.format(*means[i]) for i in an['front']).encode(),
        }
        for f, data in want.items():
            assert (out / f).read_bytes() == data, f
        front = np.asarray(an['front'])
        bp, bm, bv = interpolate.blend(params, ob_mean, ob_var, (table[0][front], table[1][front]))
        _, params2, mean2, var2, _ = evaluate.load_pareto_set(str(out))
        assert torch.equal(params2, bp) and torch.equal(mean2, bm) and torch.equal(var2, bv)
