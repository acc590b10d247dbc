"""Blended-policy evaluation on the device (pgm_eval_blend, pgmorl_amd.interpolate) against the CPU oracle on the
materialised blend (tests/eval_ref.py; the band of tests/test_gpu_kernels.py::test_eval, 1e-4 + 1e-5 |ref|), against
the existing kernels on materialised candidates (pgm_eval's wave kernel bit for bit, pgm_eval_episodes' block kernel in
the band), its endpoints and symmetry, the materialising fallback (LayerNorm towers, MO-Humanoid) and a finished tiny
run.

Shapes: M = 3 members, the episode limit cut to 20 steps through the spec (5 for the many-candidate case), 7
candidates, E in {1, 4, 5, 9}: with 4 waves per workgroup that is 7, 28, 35 and 63 work items -- a ragged second
workgroup, full workgroups only, one wave past a full workgroup, and many workgroups with a ragged tail.  The oracle
runs once per family for 9 starts: the tables of smaller E are its prefixes."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle.policy import make_policy
from oracle.vecenv import RunningMeanStd
from pgmorl_amd import _lib, envspec, evaluate, interpolate
from pgmorl_amd.layout import ParamLayout

from .eval_ref import episodes_ref
from .helpers import perturb

pytestmark = pytest.mark.gpu

STEPS, M, EMAX, SEED, GAMMA = 20, 3, 9, 41, 0.995
BAND = (1e-4, 1e-5)
ROWS = [(0, 0, 0.0), (1, 1, 0.0), (2, 2, 0.0), (0, 1, 0.5), (1, 0, 0.25), (0, 2, 1.0), (2, 2, 0.7)]
# (family, raw): dims 17/6/2, 11/3/3 discounted, 27/8/2 and 6/2/2 (a SynthMO spec of the MO-Dummy dims)
FAMILIES = [('MO-Walker2d-v2', True), ('MO-Hopper-v3', False), ('MO-Ant-v2', True), ('synth-6-2-2', True)]


def _spec(name):
    if name != 'synth-6-2-2':
        return dict(envspec.make_spec(name), max_episode_steps=STEPS)
    O, A, K = 6, 2, 2
    rng = np.random.RandomState(5)
    return {'name': name, 'obs_dim': O, 'act_dim': A, 'obj_num': K, 'max_episode_steps': STEPS,
            'd': rng.uniform(-0.9, 0.9, O), 'U': rng.uniform(-1, 1, (O, A)) / np.sqrt(A), 'c': rng.uniform(-0.1, 0.1, O),
            'V': rng.uniform(-1, 1, (K, O)), 'ebase': np.array([1.0, 2.0]), 'ecoef': np.array([0.0, 0.5]),
            'act_lo': np.full(A, -1.0), 'act_hi': np.full(A, 1.0)}


def _close(a, b, band, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err = np.abs(a - b)
    bad = err > band[0] + band[1] * np.abs(b)
    print(f'{what}: max abs err {err.max():.3e} (band {band[0]:g} + {band[1]:g} |ref|)')
    assert not bad.any(), f'{what}: {bad.sum()}/{bad.size} off, max abs err {err.max():.3e}'


@functools.lru_cache(maxsize=None)
def _case(name, ln=False):
    """The family's spec (20-step episodes) and M fp32-rounded perturbed members: flat parameters and statistics."""
    spec = _spec(name)
    O, A, K = spec['obs_dim'], spec['act_dim'], spec['obj_num']
    torch.manual_seed(3)
    gen = torch.Generator().manual_seed(103)
    rng = np.random.RandomState(2)
    lay = ParamLayout(O, A, K, layernorm=ln)
    rows, means, vars_ = [], [], []
    for _ in range(M):
        pol = make_policy(O, A, K, layernorm=ln)
        with torch.no_grad():
            for prm in pol.parameters():
                prm.copy_(prm.float().double())
        pol = perturb(pol, 0.05, gen)
        rows.append(lay.flatten(pol.state_dict()))
        r = RunningMeanStd(shape=(O,))
        r.update(rng.randn(50, O) * 0.3 + 0.1)
        means.append(r.mean)
        vars_.append(r.var)
    params, mean, var = torch.from_numpy(np.stack(rows)), torch.from_numpy(np.stack(means)), torch.from_numpy(np.stack(vars_))
    return spec, lay, params, mean, var


def _blended_policies(name, ln, table, use_ob=True):
    """The oracle's view of the candidates: policies built from blend() through ParamLayout.unflatten, with the
    blended statistics."""
    spec, lay, params, mean, var = _case(name, ln)
    bp, bm, bv = interpolate.blend(params, mean, var, table)
    out = []
    for q in range(len(bp)):
        pol = make_policy(spec['obs_dim'], spec['act_dim'], spec['obj_num'], layernorm=ln)
        pol.load_state_dict(lay.unflatten(bp[q]))
        rms = None
        if use_ob:
            rms = RunningMeanStd(shape=(spec['obs_dim'],))
            rms.mean, rms.var = bm[q].numpy(), bv[q].numpy()
        out.append((pol, rms))
    return out


@functools.lru_cache(maxsize=None)
def _oracle(name, raw, use_ob=True):
    """[7][EMAX][K] per-episode sums of the oracle on the blended policies, computed once per family."""
    spec = _case(name)[0]
    starts = envspec.reset_table(spec['obs_dim'], SEED, EMAX)
    ref = np.stack([episodes_ref(spec, starts, pol, rms, raw=raw, gamma=GAMMA)
                    for pol, rms in _blended_policies(name, False, interpolate.make_table(ROWS), use_ob)])
    ref.setflags(write=False)
    return ref


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _spec_on(spec, gpu, steps):
    st = {k: torch.tensor(np.ascontiguousarray(spec[k]), dtype=torch.float64, device=gpu) for k in evaluate.SPEC_KEYS}
    return st, _lib.EnvSpec(*(_p(st[k]) for k in evaluate.SPEC_KEYS), steps, 0)


def _launch(gpu, name, table, E, raw=True, use_ob=True, steps=STEPS, spare=0, objs=True, fill=-123.0):
    """pgm_eval_blend through the ABI: (episodes [Q + spare][E][K], objs [Q + spare][K] or None), on the host."""
    spec, _, params, mean, var = _case(name)
    O, A, K = spec['obs_dim'], spec['act_dim'], spec['obj_num']
    f64 = dict(dtype=torch.float64, device=gpu)
    keep, c_spec = _spec_on(spec, gpu, steps)
    starts = torch.tensor(envspec.reset_table(O, SEED, E), **f64)
    prm, mu, vr = params.to(gpu), mean.to(gpu), var.to(gpu)
    src, alpha = (torch.from_numpy(t).to(gpu) for t in table)
    Q = len(table[0])
    ep = torch.full((Q + spare, E, K), fill, **f64)
    ob = torch.full((Q + spare, K), fill, **f64) if objs else None
    d = _lib.Dims(Q, 1, 0, O, A, K, 64, 0)
    _lib.check(_lib.lib().pgm_eval_blend(C.byref(d), _p(prm), M, _p(mu) if use_ob else None, _p(vr) if use_ob else None,
                                         _p(src), _p(alpha), C.byref(c_spec), _p(starts), E, int(use_ob), int(raw), GAMMA,
                                         _p(ep), _p(ob), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               'pgm_eval_blend')
    torch.cuda.synchronize()
    return ep.cpu().numpy(), None if ob is None else ob.cpu().numpy()


def _in_order_mean(ep):
    acc = np.zeros((ep.shape[0], ep.shape[2]))
    for e in range(ep.shape[1]):
        acc = acc + ep[:, e]
    return acc / ep.shape[1]


# ------------------------------------------------------------------------------------------------ G1. the oracle
@pytest.mark.parametrize('E', [1, 4, 5, 9])
@pytest.mark.parametrize('name,raw', FAMILIES)
def test_blend_against_the_oracle(gpu, name, raw, E):
    spec = _case(name)[0]
    ep, objs = _launch(gpu, name, interpolate.make_table(ROWS), E, raw=raw)
    assert ep.shape == (len(ROWS), E, spec['obj_num'])
    _close(ep, _oracle(name, raw)[:, :E], BAND, f'{name} E={E} episodes')
    np.testing.assert_array_equal(objs, _in_order_mean(ep))


def test_blend_without_ob_rms(gpu):
    name, raw = FAMILIES[1]
    ep, objs = _launch(gpu, name, interpolate.make_table(ROWS), 5, raw=raw, use_ob=False)
    _close(ep, _oracle(name, raw, False)[:, :5], BAND, 'no ob_rms')
    np.testing.assert_array_equal(objs, _in_order_mean(ep))
    with_ob, _ = _launch(gpu, name, interpolate.make_table(ROWS), 5, raw=raw)
    assert not np.array_equal(with_ob, ep)


# ------------------------------------------------------------------------------------------------ G2. endpoints
@pytest.mark.parametrize('name,raw', FAMILIES[:2])
def test_endpoints_and_symmetry(gpu, name, raw):
    rows = []
    pairs = [(0, 1), (1, 2), (2, 0)]
    for i, j in pairs:
        rows += [(i, i, 0.0), (i, j, 0.0), (j, i, 1.0)]
    rows += [(0, 1, 0.5), (1, 0, 0.5), (1, 1, 0.5)]
    ep, objs = _launch(gpu, name, interpolate.make_table(rows), 5, raw=raw)
    ep, objs = torch.from_numpy(ep), torch.from_numpy(objs)
    for n in range(len(pairs)):
        a, b, c = ep[3 * n], ep[3 * n + 1], ep[3 * n + 2]
        assert torch.equal(a, b) and torch.equal(a, c), pairs[n]
        assert torch.equal(objs[3 * n], objs[3 * n + 1]) and torch.equal(objs[3 * n], objs[3 * n + 2])
    assert torch.equal(ep[9], ep[10]) and torch.equal(objs[9], objs[10])
    assert torch.equal(ep[11], ep[3])  # (1, 1, 0.5): x / 2 + x / 2 is x
    assert not torch.equal(ep[0], ep[3]) and not torch.equal(ep[9], ep[0]) and not torch.equal(ep[9], ep[3])


# ------------------------------------------------------------------------------------------------ G3. existing kernels
@pytest.mark.parametrize('name,raw', FAMILIES[:3])
def test_equals_the_existing_kernels_on_materialised_candidates(gpu, name, raw):
    """The same table with blend() on the host: pgm_eval (eval_num = 1 from start row e: the wave kernel at these dims)
    runs the same ActorLane::forward_reg / EnvLane::step on the same fp32 weights, and returns the same bits;
    pgm_eval_episodes' block kernel agrees within the band."""
    E = 5
    spec, _, params, mean, var = _case(name)
    O, A, K = spec['obs_dim'], spec['act_dim'], spec['obj_num']
    table = interpolate.make_table(ROWS)
    Q = len(ROWS)
    ep, _ = _launch(gpu, name, table, E, raw=raw)
    bp, bm, bv = interpolate.blend(params, mean, var, table)
    f64 = dict(dtype=torch.float64, device=gpu)
    keep, c_spec = _spec_on(spec, gpu, STEPS)
    prm, mu, vr = bp.to(gpu), bm.to(gpu), bv.to(gpu)
    starts = torch.tensor(envspec.reset_table(O, SEED, E), **f64)
    d = _lib.Dims(Q, 1, 8, O, A, K, 64, 0)
    opts = _lib.launch_opts({})
    worst = 0.0
    for e in range(E):
        out = torch.zeros(Q, K, **f64)
        _lib.check(_lib.lib().pgm_eval(C.byref(d), _p(prm), C.byref(c_spec), _p(mu), _p(vr), _p(starts[e:e + 1]), 1, 1,
                                       int(raw), GAMMA, _p(out), C.byref(opts),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'pgm_eval')
        torch.cuda.synchronize()
        worst = max(worst, float(np.abs(out.cpu().numpy() - ep[:, e]).max()))
        assert torch.equal(out.cpu(), torch.from_numpy(ep[:, e])), f'episode {e}: max abs diff {worst:.3e}'
    print(f'{name}: pgm_eval_blend vs pgm_eval on materialised candidates: max abs diff {worst:.3e}')
    block = evaluate.evaluate_policies(name, bp, bm, bv, E, SEED, gamma=GAMMA, raw=raw, max_episode_steps=STEPS)
    _close(ep, block, BAND, f'{name} vs pgm_eval_episodes (block kernel)')
    # the Python entry point is the same launch
    got, objs = interpolate.evaluate_candidates(name, params, mean, var, table, E, SEED, gamma=GAMMA, raw=raw,
                                                max_episode_steps=STEPS, return_objs=True)
    np.testing.assert_array_equal(got, ep)
    np.testing.assert_array_equal(objs, _in_order_mean(ep))


# ------------------------------------------------------------------------------------------------ G4. fallback
@pytest.mark.parametrize('name,ln,band', [('MO-Hopper-v2', True, BAND), ('MO-Humanoid-v2', False, (1e-3, 2e-4))])
def test_fallback_materialises_and_matches_the_oracle(gpu, monkeypatch, name, ln, band):
    def no_blend_kernel():
        raise AssertionError('the fallback reached pgm_eval_blend')
    monkeypatch.setattr(interpolate, 'require_eval_blend', no_blend_kernel)
    spec, _, params, mean, var = _case(name, ln)
    table = interpolate.make_table(ROWS[3:])
    E = 2
    ep, objs = interpolate.evaluate_candidates(name, params, mean, var, table, E, SEED, gamma=GAMMA, raw=True,
                                               layernorm=ln, max_episode_steps=STEPS, chunk=3, return_objs=True)
    assert ep.shape == (4, E, spec['obj_num'])
    starts = envspec.reset_table(spec['obs_dim'], SEED, E)
    ref = np.stack([episodes_ref(spec, starts, pol, rms, raw=True, gamma=GAMMA)
                    for pol, rms in _blended_policies(name, ln, table)])
    _close(ep, ref, band, f'{name} ln={ln} fallback')
    np.testing.assert_array_equal(objs, _in_order_mean(ep))


# ------------------------------------------------------------------------------------------------ G5. many candidates
def test_many_candidates_and_chunks(gpu):
    """Q = 2,000 candidates of one episode each, 500 workgroups (MI355X: 256 CUs): waves never wait for each other, so
    candidates 0, 999 and 1,999 are what launches holding only that candidate give, and slices of 1 and of 7
    candidates give what one launch gives, bit for bit."""
    name, raw = FAMILIES[0]
    _, _, params, mean, var = _case(name)
    Q = 2000
    assert Q // 4 > torch.cuda.get_device_properties(gpu).multi_processor_count
    rng = np.random.RandomState(11)
    src = rng.randint(0, M, size=(Q, 2)).astype(np.int32)
    alpha = rng.rand(Q)
    ep, objs = _launch(gpu, name, (src, alpha), 1, raw=raw, steps=5)
    assert np.isfinite(ep).all() and len(np.unique(ep[:, 0, 0])) > Q // 3
    for q in (0, 999, 1999):
        solo, solo_objs = _launch(gpu, name, (src[q:q + 1], alpha[q:q + 1]), 1, raw=raw, steps=5)
        np.testing.assert_array_equal(solo[0], ep[q])
        np.testing.assert_array_equal(solo_objs[0], objs[q])
    sub = slice(0, 40)
    for chunk in (65536, 7, 1):
        got, gobjs = interpolate.evaluate_candidates(name, params, mean, var, (src[sub], alpha[sub]), 1, SEED,
                                                     gamma=GAMMA, raw=raw, max_episode_steps=5, chunk=chunk,
                                                     return_objs=True)
        np.testing.assert_array_equal(got, ep[sub])
        np.testing.assert_array_equal(gobjs, objs[sub])


# ------------------------------------------------------------------------------------------------ G6. sentinels
@pytest.mark.parametrize('E', [4, 5])
def test_spare_rows_keep_their_sentinel_and_objs_out_is_optional(gpu, E):
    name, raw = FAMILIES[1]
    table = interpolate.make_table(ROWS)
    Q = len(ROWS)
    ep, objs = _launch(gpu, name, table, E, raw=raw, spare=1)
    assert (ep[Q] == -123.0).all() and (objs[Q] == -123.0).all(), 'the spare row was written'
    assert (ep[:Q] != -123.0).all() and (objs[:Q] != -123.0).all()
    want, want_objs = _launch(gpu, name, table, E, raw=raw)
    assert np.array_equal(ep[:Q], want) and np.array_equal(objs[:Q], want_objs)
    ep2, none = _launch(gpu, name, table, E, raw=raw, spare=1, objs=False)
    assert none is None and np.array_equal(ep2, ep)


# ------------------------------------------------------------------------------------------------ G7. end to end
def test_command_on_a_finished_run(gpu, tmp_path, capsys):
    """A tiny finished run (Hopper-v2, T 32, N 2, --rng host), then the command with --save-policies: the files restate
    each other, the member rows are what pgmorl_amd.evaluate measures, and the written dense-front set evaluates to
    its own rows of objs.txt."""
    from pgmorl_amd.run import main
    T, N, E, points = 32, 2, 2, 3
    run = tmp_path / 'run'
    argv = ['--env-name', 'MO-Hopper-v2', '--obj-num', '2', '--num-steps', str(T), '--num-processes', str(N),
            '--ppo-epoch', '1', '--num-mini-batch', '2', '--num-env-steps', str(T * N * 4), '--warmup-iter', '2',
            '--update-iter', '1', '--delta-weight', '0.5', '--selection-method', 'prediction-guided', '--save-dir',
            str(run), '--rl-log-interval', '1', '--rng', 'host', '--pbuffer-num', '100', '--seed', '3', '--eval-num', '2']
    prev = torch.get_default_dtype()
    try:
        main(argv)
    finally:
        torch.set_default_dtype(prev)
    stored = np.loadtxt(run / 'final' / 'objs.txt', delimiter=',', ndmin=2)
    Mr = len(stored)
    summary = interpolate.main([str(run), '--points', str(points), '--episodes', str(E), '--save-policies'])
    capsys.readouterr()
    out = run / 'continuous'
    assert sorted(os.listdir(out)) == ['args.txt', 'candidates.txt', 'episodes.npy', 'final', 'front.txt', 'objs.txt',
                                       'segments.txt', 'summary.json']
    pairs = interpolate.neighbour_pairs(stored, 2)
    table = interpolate.candidate_table(Mr, pairs, points)
    Q = Mr + len(pairs) * points
    ep = np.load(out / 'episodes.npy')
    assert ep.shape == (Q, E, 2) and ep.dtype == np.float64 and np.isfinite(ep).all()
    means = _in_order_mean(ep)
    assert (out / 'objs.txt').read_text() == ''.join('{:5f},{:5f}\n'.format(*o) for o in means)
    assert (out / 'candidates.txt').read_text().splitlines() == \
        [f'{a},{b},{float(al)!r}' for (a, b), al in zip(table[0], table[1])]
    # front.txt, segments.txt and summary.json are analyse() of the tool's own means
    an = interpolate.analyse(table, means, Mr, points)
    assert [int(x) for x in (out / 'front.txt').read_text().split()] == an['front']
    assert (out / 'segments.txt').read_text().splitlines() == \
        [f'{a},{b},{int(ok)},{an["family"][a]}' for (a, b), ok in zip(an['pairs'], an['connected'])]
    assert json.load(open(out / 'summary.json')) == summary == interpolate.summarise(an, stored, 2, E, 3, 3)
    assert (summary['M'], summary['Q'], summary['E'], summary['eval_seed']) == (Mr, Q, E, 3)
    # the member rows are the re-evaluation's
    evaluate.main([str(run), '--episodes', str(E)])
    capsys.readouterr()
    members = np.loadtxt(run / 'eval' / 'objs.txt', delimiter=',', ndmin=2)
    got = np.loadtxt(out / 'objs.txt', delimiter=',', ndmin=2)
    _close(got[:Mr], members, BAND, 'member rows vs pgmorl_amd.evaluate')
    # the written dense-front set is a save dir: evaluating it reproduces its rows of objs.txt
    evaluate.main([str(out), '--episodes', str(E)])
    capsys.readouterr()
    dense = np.loadtxt(out / 'eval' / 'objs.txt', delimiter=',', ndmin=2)
    assert len(dense) == len(an['front']) >= 1
    _close(dense, got[an['front']], BAND, 'evaluate on the dense-front set vs objs.txt')
    np.testing.assert_array_equal(np.loadtxt(out / 'final' / 'objs.txt', delimiter=',', ndmin=2), got[an['front']])
