"""CPU-side checks of the dense-front tool (pgmorl_amd.interpolate / pgm_eval_blend): the entry point's argument
refusals (before any device work, in the order include/pgm_abi.h documents), the unchanged version pair and feature
values, the blend's definition, the neighbour pairs, the candidate table, the Pareto analysis on constructed means, and
the command's refusals and files with a constructed evaluator.  No kernel is launched here: every ABI call below stops
at a refusal."""
import argparse
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from pgmorl_amd import _lib, evaluate, interpolate
from pgmorl_amd._lib import PGM_E_INVALID_ARG, PGM_E_SHAPE, PGM_E_UNSUPPORTED, PGMError
from pgmorl_amd.layout import ParamLayout
from pgmorl_amd.pareto import compute_hypervolume, compute_sparsity, get_ep_indices
from pgmorl_amd.run import merge_argv

ONE = C.c_void_p(1)  # a non-NULL pointer nothing dereferences: every call below is refused before device work
NAME = 'pgm_eval_blend'


def _err():
    return _lib.lib().pgm_last_error().decode()


# ------------------------------------------------------------------------------------------------ ABI
def test_symbol_is_present_and_the_abi_values_are_unchanged():
    L = _lib.lib()
    assert _lib.has_eval_blend() and all(hasattr(L, s) for s in _lib.EVAL_BLEND_SYMBOLS)
    _lib.require_eval_blend()
    assert _lib.has_eval_episodes()
    assert (L.pgm_abi_version(), L.pgm_abi_minor()) == (5, 1)
    assert L.pgm_abi_features() == 7 and L.pgm_abi_feature_mask() == 15


def _call(dims=None, params=ONE, M=3, ob_mean=ONE, ob_var=ONE, src=ONE, alpha=ONE, spec_null=False, spec_steps=20,
          spec_ptr=True, starts=ONE, E=9, use_ob=1, out=ONE, objs=ONE, dims_ptr=True):
    d = dict(P=7, N=4, T=64, O=17, A=6, K=2, H=64, LN=0)
    d.update(dims or {})
    spec = _lib.EnvSpec(*([None if spec_null else ONE] * 8), spec_steps, 0)
    dd = _lib.Dims(*(d[k] for k in ('P', 'N', 'T', 'O', 'A', 'K', 'H', 'LN')))
    return _lib.lib().pgm_eval_blend(C.byref(dd) if dims_ptr else None, params, M, ob_mean, ob_var, src, alpha,
                                     C.byref(spec) if spec_ptr else None, starts, E, use_ob, 1, 0.995, out, objs, None)


MATERIALISE = 'materialise the candidates and use pgm_eval_episodes'
# the documented order: (what is wrong, variants, status, a piece of the message); every entry is tried with every
# later entry wrong as well (where two entries change the same field, the earlier entry's value stays)
ORDER = [
    ('null', [dict(params=None), dict(src=None), dict(alpha=None), dict(starts=None), dict(out=None),
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


def test_optional_pointers_and_ignored_dims():
    """What the entry point accepts, as far as a host can tell without device work: the call passes every argument
    check and is stopped by the last one (a dim set no kernel is compiled for)."""
    last = dict(dims=dict(O=19))
    assert _call(**last) == PGM_E_UNSUPPORTED and 'unsupported dims' in _err()
    # ob_mean / ob_var are read with use_ob_rms only, and objs_out may be NULL
    assert _call(use_ob=0, ob_mean=None, ob_var=None, objs=None, **last) == PGM_E_UNSUPPORTED
    assert 'unsupported dims' in _err()
    assert _call(use_ob=1, ob_mean=None, **last) == PGM_E_INVALID_ARG
    # d->N and d->T are not this call's
    assert _call(dims=dict(N=9, T=-1, O=19)) == PGM_E_UNSUPPORTED and 'unsupported dims' in _err()
    # the largest E and a grid the call can hold
    assert _call(dims=dict(P=256, O=19), E=65536) == PGM_E_UNSUPPORTED and 'unsupported dims' in _err()
    # Humanoid (plain towers) is outside the wave form: the message says what to do instead
    assert _call(dims=dict(O=376, A=17)) == PGM_E_UNSUPPORTED and MATERIALISE in _err()


# ------------------------------------------------------------------------------------------------ blend
def _members(M=3, L=37, O=5, seed=0):
    rng = np.random.RandomState(seed)
    return (rng.randn(M, L).astype(np.float32), rng.randn(M, O), rng.rand(M, O) + 0.5)


def test_blend_endpoints_symmetry_and_definition():
    prm, mean, var = _members()
    rows = [(0, 1, 0.0), (0, 1, 1.0), (2, 2, 0.7), (0, 1, 0.5), (1, 0, 0.5), (1, 2, 0.3), (2, 1, 0.7), (0, 2, 1 / 3)]
    table = interpolate.make_table(rows)
    bp, bm, bv = interpolate.blend(prm, mean, var, table)
    assert bp.dtype == np.float32 and bm.dtype == bv.dtype == np.float64
    assert bp.shape == (len(rows), prm.shape[1]) and bm.shape == bv.shape == (len(rows), mean.shape[1])
    # alpha 0 and 1 are the members, bit for bit
    for got, x in ((bp, prm), (bm, mean), (bv, var)):
        np.testing.assert_array_equal(got[0], x[0])
        np.testing.assert_array_equal(got[1], x[1])
        np.testing.assert_array_equal(got[3], got[4])  # (a, b, 0.5) and (b, a, 0.5)
    # the documented expression
    src, alpha = table
    al = alpha[:, None]
    A, B = prm[src[:, 0]], prm[src[:, 1]]
    np.testing.assert_array_equal(bp, ((1 - al) * A.astype(np.float64) + al * B.astype(np.float64)).astype(np.float32))
    np.testing.assert_array_equal(bm, (1 - al) * mean[src[:, 0]] + al * mean[src[:, 1]])
    np.testing.assert_array_equal(bv, (1 - al) * var[src[:, 0]] + al * var[src[:, 1]])
    # torch in, torch out, the same values; statistics are optional
    tp, tm, tv = interpolate.blend(torch.from_numpy(prm), torch.from_numpy(mean), torch.from_numpy(var), table)
    assert isinstance(tp, torch.Tensor) and tp.dtype == torch.float32 and tm.dtype == tv.dtype == torch.float64
    assert np.array_equal(tp.numpy(), bp) and np.array_equal(tm.numpy(), bm) and np.array_equal(tv.numpy(), bv)
    only = interpolate.blend(prm, None, None, table)
    assert np.array_equal(only[0], bp) and only[1] is None and only[2] is None
    with pytest.raises(PGMError, match=r'candidate 1 names members \(0, 3\)'):
        interpolate.blend(prm, mean, var, interpolate.make_table([(0, 1, 0.5), (0, 3, 0.5)]))


# ------------------------------------------------------------------------------------------------ neighbour pairs
def test_neighbour_pairs_known_answers():
    # five points on the line y = 4 - x at x = 0, 1, 3, 4, 2: member 4 (x = 2) is as far from member 1 as from member
    # 2, member 1 as far from 0 as from 4, member 2 as far from 3 as from 4: the lower index wins each tie
    front = np.array([[0, 4], [1, 3], [3, 1], [4, 0], [2, 2]], dtype=np.float64)
    assert interpolate.neighbour_pairs(front, 1) == [(0, 1), (1, 4), (2, 3)]
    assert interpolate.neighbour_pairs(front, 2) == [(0, 1), (0, 4), (1, 4), (2, 3), (2, 4), (3, 4)]
    assert interpolate.neighbour_pairs(front) == interpolate.neighbour_pairs(front, 2)
    # scaling: stretching one objective changes nothing
    assert interpolate.neighbour_pairs(front * np.array([1000.0, 0.001]), 1) == [(0, 1), (1, 4), (2, 3)]
    # three objectives, the middle one constant (it scales to 0, not to NaN)
    pts = np.array([[0, 5, 7], [1, 5, 3], [4, 5, 1], [2, 5, 2]], dtype=np.float64)
    assert interpolate.neighbour_pairs(pts, 1) == [(0, 1), (1, 3), (2, 3)]
    every = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert interpolate.neighbour_pairs(pts, 3) == every and interpolate.neighbour_pairs(pts, 5) == every
    assert interpolate.neighbour_pairs(front[:1], 2) == []
    assert interpolate.neighbour_pairs(front[:2], 2) == [(0, 1)]
    assert interpolate.neighbour_pairs(np.array([[1.0, 1.0], [1.0, 1.0]]), 1) == [(0, 1)]  # every objective constant
    with pytest.raises(PGMError, match='neighbours=0'):
        interpolate.neighbour_pairs(front, 0)


# ------------------------------------------------------------------------------------------------ candidate table
def test_candidate_table_rows_and_alphas():
    pairs = [(0, 2), (1, 2)]
    src, alpha = interpolate.candidate_table(3, pairs, 4)
    assert src.dtype == np.int32 and alpha.dtype == np.float64 and src.shape == (3 + 2 * 4, 2) and alpha.shape == (11,)
    assert src[:3].tolist() == [[0, 0], [1, 1], [2, 2]] and alpha[:3].tolist() == [0.0, 0.0, 0.0]
    assert src[3:7].tolist() == [[0, 2]] * 4 and src[7:].tolist() == [[1, 2]] * 4
    assert alpha[3:7].tolist() == alpha[7:].tolist() == [1 / 5, 2 / 5, 3 / 5, 4 / 5]
    assert interpolate.candidate_table(3, pairs, 15)[1][3:18].tolist() == [j / 16 for j in range(1, 16)]
    src, alpha = interpolate.candidate_table(1, [], 7)
    assert src.tolist() == [[0, 0]] and alpha.tolist() == [0.0]


# ------------------------------------------------------------------------------------------------ analyse
def _constructed():
    """4 members on a line, pairs (0,1), (1,2), (2,3), 2 points each: the interpolants of (0,1) and (2,3) lie beyond the
    members' line, one interior point of (1,2) is dominated by member 2."""
    members = [[1.0, 4.0], [2.0, 3.0], [3.0, 2.0], [4.0, 1.0]]
    inter = [[1.4, 3.9], [1.8, 3.5],   # (0,1): both non-dominated
             [2.2, 2.9], [2.5, 1.9],   # (1,2): the second is dominated by member 2 (3, 2)
             [3.4, 1.8], [3.8, 1.4]]   # (2,3)
    table = interpolate.candidate_table(4, [(0, 1), (1, 2), (2, 3)], 2)
    return table, np.array(members + inter)


def test_analyse_on_constructed_means():
    table, means = _constructed()
    an = interpolate.analyse(table, means, 4, 2)
    assert an['pairs'] == [(0, 1), (1, 2), (2, 3)] and an['connected'] == [True, False, True]
    assert an['family'] == [0, 0, 2, 2] and an['families'] == [[0, 1], [2, 3]]
    assert (an['num_pairs'], an['num_connected'], an['num_families'], an['family_sizes']) == (3, 2, 2, [2, 2])
    # every row but the dominated one, by the first objective
    assert an['front'] == [0, 4, 5, 1, 6, 2, 8, 9, 3] == get_ep_indices(means)
    assert (an['dense_front_size'], an['dense_front_interpolants'], an['M'], an['Q'], an['points']) == (9, 5, 4, 10, 2)
    assert an['members'] == {'hypervolume': compute_hypervolume(means[:4]), 'sparsity': compute_sparsity(means[:4])}
    assert an['dense'] == {'hypervolume': compute_hypervolume(means[an['front']]),
                           'sparsity': compute_sparsity(means[an['front']])}
    assert an['members']['hypervolume'] == 10.0 and an['dense']['hypervolume'] > an['members']['hypervolume']
    # a point EQUAL to a member's mean is not dominated by it; one that loses in one objective and ties the other is
    eq = means.copy()
    eq[7] = [3.0, 2.0]
    assert interpolate.analyse(table, eq, 4, 2)['connected'] == [True, True, True]
    assert interpolate.analyse(table, eq, 4, 2)['families'] == [[0, 1, 2, 3]]
    eq[7] = [3.0, 1.99]
    assert interpolate.analyse(table, eq, 4, 2)['connected'] == [True, False, True]
    # union-find labels: connecting (0,1) and (1,2) but not (2,3)
    m2 = means.copy()
    m2[7] = [2.6, 2.5]
    m2[8] = [3.4, 0.9]  # dominated by member 3 (4, 1)
    an2 = interpolate.analyse(table, m2, 4, 2)
    assert an2['connected'] == [True, True, False] and an2['family'] == [0, 0, 0, 3]
    assert an2['families'] == [[0, 1, 2], [3]]
    with pytest.raises(PGMError, match='not 4 members and 4 points per pair'):
        interpolate.analyse(table, means, 4, 4)
    with pytest.raises(PGMError, match=r'rows 4..6 of the table are not one pair'):
        interpolate.analyse(table, means, 4, 3)
    with pytest.raises(PGMError, match='means must be'):
        interpolate.analyse(table, means[:-1], 4, 2)


# ------------------------------------------------------------------------------------------------ host refusals
def test_evaluate_candidates_refuses_bad_arguments_before_the_library(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(interpolate, 'lib', no_library)
    monkeypatch.setattr(interpolate, 'require_eval_blend', no_library)
    monkeypatch.setattr(interpolate, 'evaluate_policies', no_library)
    lay = ParamLayout(11, 3, 2)
    prm, st = torch.zeros(2, lay.total), torch.ones(2, 11, dtype=torch.float64)
    ok = dict(episodes=4, eval_seed=0, device='cpu')
    table = interpolate.make_table([(0, 0, 0.0), (1, 1, 0.0), (0, 1, 0.5)])

    def refused(text, tbl=table, p=prm, mean=st, var=st, env='MO-Hopper-v2', **kw):
        with pytest.raises(PGMError, match=text):
            interpolate.evaluate_candidates(env, p, mean, var, tbl, **dict(ok, **kw))

    refused(r'candidate 1 names members \(0, 2\) outside \[0, 2\)', interpolate.make_table([(0, 1, 0.5), (0, 2, 0.5)]))
    refused(r'candidate 0 names members \(-1, 1\)', interpolate.make_table([(-1, 1, 0.5)]))
    refused(r'candidate 2 has alpha=1.5 outside \[0, 1\]', interpolate.make_table([(0, 1, 0.5), (0, 1, 1.0), (0, 1, 1.5)]))
    refused('alpha=nan', interpolate.make_table([(0, 1, float('nan'))]))
    refused('alpha=-0.25', interpolate.make_table([(0, 1, -0.25)]))
    refused('table alpha must be fp64', (table[0], table[1].astype(np.float32)))
    refused('table src must be int32', (table[0].astype(np.int64), table[1]))
    refused('table src must be int32', (table[0][:, :1], table[1]))
    refused(r'table alpha must be fp64 \[3\]', (table[0], table[1][:2]))
    refused('table must be the pair', table[0])
    refused('no candidates', (table[0][:0], table[1][:0]))
    refused('episodes=0', episodes=0)
    refused('episodes=65537', episodes=65537)
    refused('chunk=0', chunk=0)
    refused('max_episode_steps=0', max_episode_steps=0)
    refused('params must be fp32', p=prm[:, :-1])
    refused('params must be fp32', p=prm.double())
    refused('params must be fp32', layernorm=True)
    refused('ob_var must be fp64', var=st.float())
    refused('ob_mean is required', mean=None)
    refused('covers the SynthMO device envs', env='MO-Dummy-v0')


def test_wave_form_is_every_synthmo_env_but_humanoid():
    from pgmorl_amd import envspec
    for env, want in [('MO-Walker2d-v2', True), ('MO-HalfCheetah-v2', True), ('MO-Hopper-v2', True),
                      ('MO-Hopper-v3', True), ('MO-Ant-v2', True), ('MO-Swimmer-v2', True), ('MO-Humanoid-v2', False)]:
        sp = envspec.make_spec(env)
        assert interpolate.wave_form(sp['obs_dim'], sp['obj_num']) is want, env
        assert interpolate.wave_form(sp['obs_dim'], sp['obj_num'], layernorm=True) is False


# ------------------------------------------------------------------------------------------------ the command
def _write_run(save_dir, env='MO-Hopper-v2', O=11, A=3, K=2, layernorm=False, M=4, extra=(), seed=5):
    """args.txt as pgmorl_amd.run writes it and a final/ tree from morl.write_final."""
    from pgmorl_amd.morl import write_final
    from pgmorl_amd.pareto import EP
    from pgmorl_amd.sample import DeviceSnapshot, RunningMeanStd, Sample
    lay = ParamLayout(O, A, K, layernorm=layernorm)
    rng = np.random.RandomState(7)
    samples = []
    for k in range(M):
        z = torch.zeros(lay.total)
        snap = DeviceSnapshot(lay, torch.from_numpy(rng.randn(lay.total).astype(np.float32)), z, z, 10 * k)
        ob = RunningMeanStd(shape=(O,))
        ob.mean, ob.var = rng.randn(O), rng.rand(O) + 0.5
        obj = RunningMeanStd(shape=())
        obj.mean, obj.var = rng.randn(K), rng.rand(K) + 0.5
        objs = np.array([k + 1.25, M - k + 0.5] + [1.0] * (K - 2))  # a strict front: every sample stays a member
        samples.append(Sample.from_snapshot(snap, {'ob_rms': ob, 'ret_rms': RunningMeanStd(shape=()), 'obj_rms': obj},
                                            objs=objs))
    ep = EP()
    ep.update(samples)
    assert len(ep.sample_batch) == M
    os.makedirs(save_dir, exist_ok=True)
    argv = ['--env-name', env, '--obj-num', str(K), '--seed', str(seed), '--save-dir', str(save_dir),
            *(['--layernorm'] if layernorm else []), *extra]
    with open(os.path.join(save_dir, 'args.txt'), 'w') as fp:
        fp.write(str(merge_argv(argv)))
    write_final(argparse.Namespace(obj_num=K, obj_rms=True, save_dir=str(save_dir)), ep)


def _refused(argv, text, *dirs):
    with pytest.raises(PGMError, match=text):
        interpolate.main([str(a) for a in argv])
    for d in dirs:
        assert not os.path.exists(d), f'{d} was created by a refused call'


def test_cli_refusals_leave_no_out_dir(tmp_path, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('a refused call reached the evaluator')
    monkeypatch.setattr(interpolate, 'evaluate_candidates', no_device)
    out = tmp_path / 'elsewhere'

    def both(run, text):
        _refused([run], text, run / 'continuous')
        _refused([run, '--out', out, '--save-policies'], text, out, run / 'continuous')

    both(tmp_path / 'nothing', 'no args.txt')
    run = tmp_path / 'a'
    _write_run(run)
    for flag, bad in [('--points', '0'), ('--points', '1025'), ('--points', '-1'), ('--neighbours', '0'),
                      ('--neighbours', '-2'), ('--episodes', '0'), ('--episodes', '65537'), ('--chunk', '0')]:
        _refused([run, flag, bad], flag, run / 'continuous')
        _refused([run, flag, bad, '--out', out], flag, out, run / 'continuous')
    # load_pareto_set's refusals, with their texts
    r = tmp_path / 'shape0'  # Hopper-shaped (11/3/2) dicts under args that name Walker2d
    _write_run(r, env='MO-Walker2d-v2')
    both(r, 'does not fit the plain layout of MO-Walker2d-v2')
    r = tmp_path / 'count'
    _write_run(r)
    os.remove(r / 'final' / 'EP_policy_3.pt')
    both(r, 'the same number of each')
    r = tmp_path / 'nofinal'
    _write_run(r)
    os.rename(r / 'final', r / 'final_moved')
    both(r, 'no final/')
    scope = 'covers the SynthMO device envs'
    for i, (kw, flag) in enumerate([(dict(extra=['--host-env', 'synth']), '--host-env'),
                                    (dict(extra=['--device-env']), '--device-env'),
                                    (dict(extra=['--env-plugin', 'some/env.hpp']), '--env-plugin'),
                                    (dict(env='MO-Dummy-v0'), 'MO-Dummy-v0'),
                                    (dict(env='MO-DeepSeaTreasure-v0'), 'MO-DeepSeaTreasure-v0')]):
        r = tmp_path / f'scope{i}'
        _write_run(r, **kw)
        with pytest.raises(PGMError, match=scope) as ei:
            interpolate.main([str(r)])
        assert flag in str(ei.value)
        both(r, scope)


def _fake_evaluator(stored, calls):
    """evaluate_candidates with constructed numbers: candidate (a, b, alpha) measures the blend of the stored objectives
    plus a bulge of alpha (1 - alpha) / 5, so no interpolant is dominated by a member; episode e adds e / 8."""
    def fake(env_name, params, ob_mean, ob_var, table, episodes, eval_seed, **kw):
        calls.append(dict(kw, env_name=env_name, episodes=episodes, eval_seed=eval_seed))
        src, alpha = table
        al = alpha[:, None]
        base = (1 - al) * stored[src[:, 0]] + al * stored[src[:, 1]] + 0.2 * al * (1 - al)
        ep = base[:, None, :] + np.arange(episodes)[None, :, None] / 8.0
        acc = np.zeros_like(base)
        for e in range(episodes):
            acc = acc + ep[:, e]
        return ep, acc / episodes
    return fake


@pytest.mark.parametrize('save', [False, True])
def test_command_files_with_a_constructed_evaluator(tmp_path, monkeypatch, capsys, save):
    run = tmp_path / 'run'
    _write_run(run)
    args, params, ob_mean, ob_var, stored = evaluate.load_pareto_set(str(run))
    calls = []
    monkeypatch.setattr(interpolate, 'evaluate_candidates', _fake_evaluator(stored, calls))
    points, E = 3, 2
    out = run / 'continuous' if not save else tmp_path / 'dense'
    argv = [str(run), '--points', str(points), '--episodes', str(E)]
    summary = interpolate.main(argv + (['--out', str(out), '--save-policies'] if save else []))
    capsys.readouterr()
    assert len(calls) == 1 and calls[0]['eval_seed'] == 5 and calls[0]['episodes'] == E  # the run's --seed
    assert (calls[0]['gamma'], calls[0]['raw'], calls[0]['use_ob_rms'], calls[0]['layernorm']) == (0.995, True, True, False)
    M = 4
    pairs = interpolate.neighbour_pairs(stored, 2)
    assert pairs == [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]
    table = interpolate.candidate_table(M, pairs, points)
    Q = M + len(pairs) * points
    want = sorted(['candidates.txt', 'objs.txt', 'episodes.npy', 'segments.txt', 'front.txt', 'summary.json'] +
                  (['args.txt', 'final'] if save else []))
    assert sorted(os.listdir(out)) == want
    # candidates.txt: a,b,repr(alpha)
    lines = (out / 'candidates.txt').read_text().splitlines()
    assert lines == [f'{a},{b},{float(al)!r}' for (a, b), al in zip(table[0], table[1])]
    assert lines[:M] == [f'{i},{i},0.0' for i in range(M)] and lines[M] == '0,1,0.25' and len(lines) == Q
    # episodes.npy, objs.txt
    ep = np.load(out / 'episodes.npy')
    assert ep.shape == (Q, E, 2) and ep.dtype == np.float64
    means = (ep[:, 0] + ep[:, 1]) / 2
    assert (out / 'objs.txt').read_text() == ''.join('{:5f},{:5f}\n'.format(*o) for o in means)
    # segments.txt, front.txt and summary.json restate analyse
    an = interpolate.analyse(table, means, M, points)
    assert an['connected'] == [True] * 5 and an['families'] == [[0, 1, 2, 3]] and M < len(an['front']) <= Q
    assert (out / 'segments.txt').read_text().splitlines() == [f'{a},{b},1,0' for a, b in pairs]
    assert [int(x) for x in (out / 'front.txt').read_text().split()] == an['front']
    assert json.load(open(out / 'summary.json')) == summary
    assert summary == interpolate.summarise(an, stored, 2, E, 5, 5)
    assert (summary['M'], summary['Q'], summary['points'], summary['neighbours'], summary['E']) == (M, Q, points, 2, E)
    assert (summary['eval_seed'], summary['run_seed']) == (5, 5)
    assert (summary['num_pairs'], summary['num_connected'], summary['num_families'], summary['family_sizes']) == \
        (5, 5, 1, [4])
    assert summary['stored'] == {'hypervolume': compute_hypervolume(stored), 'sparsity': compute_sparsity(stored)}
    assert summary['members'] == {'hypervolume': compute_hypervolume(means[:M]), 'sparsity': compute_sparsity(means[:M])}
    assert summary['dense']['hypervolume'] == compute_hypervolume(means[an['front']])
    assert summary['dense']['hypervolume'] > summary['members']['hypervolume']
    assert (summary['dense_front_size'], summary['dense_front_interpolants']) == \
        (len(an['front']), sum(i >= M for i in an['front']))
    if not save:
        # --eval-seed overrides the run's seed
        interpolate.main([str(run), '--points', '1', '--eval-seed', '9', '--out', str(tmp_path / 'other')])
        capsys.readouterr()
        assert calls[-1]['eval_seed'] == 9 and calls[-1]['episodes'] == 1
        assert json.load(open(tmp_path / 'other' / 'summary.json'))['eval_seed'] == 9
        return
    # --save-policies: --out is a save dir holding the dense front's policies in front.txt order
    assert (out / 'args.txt').read_text() == (run / 'args.txt').read_text()
    args2, params2, mean2, var2, stored2 = evaluate.load_pareto_set(str(out))
    assert (args2.env_name, args2.seed) == (args.env_name, args.seed) and len(stored2) == len(an['front'])
    front = np.asarray(an['front'])
    bp, bm, bv = interpolate.blend(params, ob_mean, ob_var, (table[0][front], table[1][front]))
    assert torch.equal(params2, bp) and torch.equal(mean2, bm) and torch.equal(var2, bv)
    for j, i in enumerate(an['front']):
        if i < M:  # a member is the member
            assert torch.equal(params2[j], params[i]) and torch.equal(mean2[j], ob_mean[i])
    np.testing.assert_array_equal(stored2, np.array([[float('{:5f}'.format(x)) for x in means[i]] for i in an['front']]))
    import pickle
    with open(out / 'final' / 'EP_env_params_0.pkl', 'rb') as fp:
        with open(run / 'final' / 'EP_env_params_0.pkl', 'rb') as fp0:
            assert type(pickle.load(fp)['ob_rms']) is type(pickle.load(fp0)['ob_rms'])
