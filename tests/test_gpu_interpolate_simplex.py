"""Three-member blended evaluation on the device (pgm_eval_blend3, pgmorl_amd.interpolate --simplex) against the CPU
oracle on the materialised blend (tests/eval_ref.py on policies built with blend3; the band of
tests/test_gpu_interpolate.py, 1e-4 + 1e-5 |ref|), bit for bit against the existing kernels (pgm_eval's wave kernel on
the members and on blend3's rows, pgm_eval_blend on a pair written as a triple), the materialising fallback (LayerNorm
towers, MO-Humanoid), many candidates, untouched spare rows, and a finished tiny three-objective run.

Shapes: M = 4 members, the episode limit cut to 20 steps through the spec (5 for the many-candidate case), 9
candidates, E in {1, 4, 5, 9}: with 4 waves per workgroup that is 9, 36, 45 and 81 work items -- a ragged workgroup,
full workgroups only, one wave past a full workgroup, and many workgroups with a ragged tail.  The oracle runs once per
family for 9 starts: the tables of smaller E are its prefixes.

No dominance, connectedness or filledness decision is asserted here on device numbers: those are tested on the CPU on
constructed values (tests/test_interpolate_simplex.py)."""
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
from .test_gpu_interpolate import BAND, _close, _in_order_mean, _p, _spec, _spec_on

pytestmark = pytest.mark.gpu

STEPS, M, EMAX, SEED, GAMMA = 20, 4, 9, 41, 0.995
ROWS = [(0, 0, 0, 1.0, 0.0, 0.0), (1, 1, 1, 1.0, 0.0, 0.0), (2, 2, 2, 1.0, 0.0, 0.0), (3, 3, 3, 1.0, 0.0, 0.0),
        (0, 1, 1, 0.75, 0.25, 0.0),             # 4: a pair as a triple
        (0, 1, 2, 1 / 3, 1 / 3, 1 / 3),         # 5
        (0, 1, 2, 0.5, 0.25, 0.25),             # 6
        (1, 0, 2, 0.25, 0.5, 0.25),             # 7: row 6 with its first two slots swapped
        (3, 3, 2, 0.5, 0.5, 0.0)]               # 8
# (family, raw): dims 11/3/3 discounted and raw, 17/6/2, 27/8/2 and 6/2/2 (a SynthMO spec of the MO-Dummy dims)
FAMILIES = [('MO-Hopper-v3', False), ('MO-Hopper-v3', True), ('MO-Walker2d-v2', True), ('MO-Ant-v2', True),
            ('synth-6-2-2', True)]


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
    """The oracle's view of the candidates: policies built from blend3() through ParamLayout.unflatten, with the
    blended statistics."""
    spec, lay, params, mean, var = _case(name, ln)
    bp, bm, bv = interpolate.blend3(params, mean, var, table)
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
    """[9][EMAX][K] per-episode sums of the oracle on the blended policies, computed once per (family, raw)."""
    spec = _case(name)[0]
    starts = envspec.reset_table(spec['obs_dim'], SEED, EMAX)
    ref = np.stack([episodes_ref(spec, starts, pol, rms, raw=raw, gamma=GAMMA)
                    for pol, rms in _blended_policies(name, False, interpolate.make_table3(ROWS), use_ob)])
    ref.setflags(write=False)
    return ref


def _launch(gpu, name, table, E, raw=True, use_ob=True, steps=STEPS, spare=0, objs=True, fill=-123.0, entry='pgm_eval_blend3'):
    """pgm_eval_blend3 (or pgm_eval_blend on a pair table) through the ABI: (episodes [Q + spare][E][K],
    objs [Q + spare][K] or None), on the host."""
    spec, _, params, mean, var = _case(name)
    O, A, K = spec['obs_dim'], spec['act_dim'], spec['obj_num']
    f64 = dict(dtype=torch.float64, device=gpu)
    keep, c_spec = _spec_on(spec, gpu, steps)
    starts = torch.tensor(envspec.reset_table(O, SEED, E), **f64)
    prm, mu, vr = params.to(gpu), mean.to(gpu), var.to(gpu)
    src, wts = (torch.from_numpy(np.ascontiguousarray(t)).to(gpu) for t in table)
    Q = len(table[0])
    ep = torch.full((Q + spare, E, K), fill, **f64)
    ob = torch.full((Q + spare, K), fill, **f64) if objs else None
    d = _lib.Dims(Q, 1, 0, O, A, K, 64, 0)
    _lib.check(getattr(_lib.lib(), entry)(C.byref(d), _p(prm), M, _p(mu) if use_ob else None, _p(vr) if use_ob else None,
                                          _p(src), _p(wts), C.byref(c_spec), _p(starts), E, int(use_ob), int(raw), GAMMA,
                                          _p(ep), _p(ob), C.c_void_p(torch.cuda.current_stream().cuda_stream)), entry)
    torch.cuda.synchronize()
    return ep.cpu().numpy(), None if ob is None else ob.cpu().numpy()


def _pgm_eval(gpu, name, prm, mu, vr, E, raw):
    """pgm_eval (eval_num = 1, s0_eval = start row e: the wave kernel at these dims) of the policies prm [Q][L] with
    statistics mu / vr [Q][O]: [Q][E][K] on the host."""
    spec = _case(name)[0]
    O, A, K = spec['obs_dim'], spec['act_dim'], spec['obj_num']
    f64 = dict(dtype=torch.float64, device=gpu)
    keep, c_spec = _spec_on(spec, gpu, STEPS)
    prm, mu, vr = prm.to(gpu), mu.to(gpu), vr.to(gpu)
    starts = torch.tensor(envspec.reset_table(O, SEED, E), **f64)
    Q = len(prm)
    d = _lib.Dims(Q, 1, 8, O, A, K, 64, 0)
    opts = _lib.launch_opts({})
    got = torch.zeros(Q, E, K, dtype=torch.float64)
    for e in range(E):
        out = torch.zeros(Q, K, **f64)
        _lib.check(_lib.lib().pgm_eval(C.byref(d), _p(prm), C.byref(c_spec), _p(mu), _p(vr), _p(starts[e:e + 1]), 1, 1,
                                       int(raw), GAMMA, _p(out), C.byref(opts),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'pgm_eval')
        torch.cuda.synchronize()
        got[:, e] = out.cpu()
    return got


# ------------------------------------------------------------------------------------------------ G1. the oracle
@pytest.mark.parametrize('E', [1, 4, 5, 9])
@pytest.mark.parametrize('name,raw', FAMILIES)
def test_blend3_against_the_oracle(gpu, name, raw, E):
    spec = _case(name)[0]
    ep, objs = _launch(gpu, name, interpolate.make_table3(ROWS), E, raw=raw)
    assert ep.shape == (len(ROWS), E, spec['obj_num'])
    _close(ep, _oracle(name, raw)[:, :E], BAND, f'{name} raw={raw} E={E} episodes')
    np.testing.assert_array_equal(objs, _in_order_mean(ep))


def test_blend3_without_ob_rms(gpu):
    name, raw = FAMILIES[0]
    ep, objs = _launch(gpu, name, interpolate.make_table3(ROWS), 5, raw=raw, use_ob=False)
    _close(ep, _oracle(name, raw, False)[:, :5], BAND, 'no ob_rms')
    np.testing.assert_array_equal(objs, _in_order_mean(ep))
    with_ob, _ = _launch(gpu, name, interpolate.make_table3(ROWS), 5, raw=raw)
    assert not np.array_equal(with_ob, ep)


# ------------------------------------------------------------------------------------------------ G2. bit equalities
@pytest.mark.parametrize('name,raw', [FAMILIES[0], FAMILIES[2], FAMILIES[3]])
def test_bit_equalities(gpu, name, raw):
    """Member rows are pgm_eval on the member; every row is pgm_eval (the wave kernel: the same ActorLane::forward_reg /
    EnvLane::step on the same fp32 weights) on blend3's materialised rows; the pair written as a triple is
    pgm_eval_blend's pair; the first-two-slot swap changes nothing."""
    E = 5
    _, _, params, mean, var = _case(name)
    table = interpolate.make_table3(ROWS)
    ep, objs = _launch(gpu, name, table, E, raw=raw)
    ep, objs = torch.from_numpy(ep), torch.from_numpy(objs)
    members = _pgm_eval(gpu, name, params, mean, var, E, raw)
    assert torch.equal(ep[:M], members), f'member rows: max abs diff {(ep[:M] - members).abs().max():.3e}'
    bp, bm, bv = interpolate.blend3(params, mean, var, table)
    rows = _pgm_eval(gpu, name, bp, bm, bv, E, raw)
    print(f'{name}: pgm_eval_blend3 vs pgm_eval on materialised candidates: max abs diff {(ep - rows).abs().max():.3e}')
    assert torch.equal(ep, rows)
    pair, pair_objs = _launch(gpu, name, interpolate.make_table([(0, 1, 0.25)]), E, raw=raw, entry='pgm_eval_blend')
    assert torch.equal(ep[4], torch.from_numpy(pair[0])) and torch.equal(objs[4], torch.from_numpy(pair_objs[0]))
    assert torch.equal(ep[6], ep[7]) and torch.equal(objs[6], objs[7])
    assert torch.equal(ep[8], ep[3])  # (3, 3, 2, 0.5, 0.5, 0): x / 2 + x / 2 + 0 y is x
    # the other rows are different policies
    assert len({ep[q].numpy().tobytes() for q in (0, 1, 2, 3, 4, 5, 6)}) == 7
    # the Python entry point is the same launch
    got, gobjs = interpolate.evaluate_candidates3(name, params, mean, var, table, E, SEED, gamma=GAMMA, raw=raw,
                                                  max_episode_steps=STEPS, return_objs=True)
    np.testing.assert_array_equal(got, ep.numpy())
    np.testing.assert_array_equal(gobjs, objs.numpy())


# ------------------------------------------------------------------------------------------------ G3. fallback
@pytest.mark.parametrize('name,ln,band', [('MO-Hopper-v2', True, BAND), ('MO-Humanoid-v2', False, (1e-3, 2e-4))])
def test_fallback_materialises_and_matches_the_oracle(gpu, monkeypatch, name, ln, band):
    def no_blend_kernel():
        raise AssertionError('the fallback reached pgm_eval_blend3')
    monkeypatch.setattr(interpolate, 'require_eval_blend3', no_blend_kernel)
    spec, _, params, mean, var = _case(name, ln)
    table = interpolate.make_table3(ROWS[4:8])
    E = 2
    ep, objs = interpolate.evaluate_candidates3(name, params, mean, var, table, E, SEED, gamma=GAMMA, raw=True,
                                                layernorm=ln, max_episode_steps=STEPS, chunk=3, return_objs=True)
    assert ep.shape == (4, E, spec['obj_num'])
    starts = envspec.reset_table(spec['obs_dim'], SEED, E)
    ref = np.stack([episodes_ref(spec, starts, pol, rms, raw=True, gamma=GAMMA)
                    for pol, rms in _blended_policies(name, ln, table)])
    _close(ep, ref, band, f'{name} ln={ln} fallback')
    np.testing.assert_array_equal(objs, _in_order_mean(ep))


# ------------------------------------------------------------------------------------------------ G4. many candidates
def test_many_candidates_and_chunks(gpu):
    """Q = 2,000 candidates of one episode each, 500 workgroups (MI355X: 256 CUs): waves never wait for each other, so
    candidates 0, 999 and 1,999 are what launches holding only that candidate give, and slices of 1 and of 7
    candidates give what one launch gives, bit for bit."""
    name, raw = FAMILIES[1]
    _, _, params, mean, var = _case(name)
    Q = 2000
    assert Q // 4 > torch.cuda.get_device_properties(gpu).multi_processor_count
    rng = np.random.RandomState(11)
    src = rng.randint(0, M, size=(Q, 3)).astype(np.int32)
    w = rng.rand(Q, 3)
    w = w / w.sum(axis=1, keepdims=True)
    interpolate._check_table3((src, w), M, 'the test table')
    ep, objs = _launch(gpu, name, (src, w), 1, raw=raw, steps=5)
    assert np.isfinite(ep).all() and len(np.unique(ep[:, 0, 0])) > Q // 3
    for q in (0, 999, 1999):
        solo, solo_objs = _launch(gpu, name, (src[q:q + 1], w[q:q + 1]), 1, raw=raw, steps=5)
        np.testing.assert_array_equal(solo[0], ep[q])
        np.testing.assert_array_equal(solo_objs[0], objs[q])
    sub = slice(0, 40)
    for chunk in (65536, 7, 1):
        got, gobjs = interpolate.evaluate_candidates3(name, params, mean, var, (src[sub], w[sub]), 1, SEED,
                                                      gamma=GAMMA, raw=raw, max_episode_steps=5, chunk=chunk,
                                                      return_objs=True)
        np.testing.assert_array_equal(got, ep[sub])
        np.testing.assert_array_equal(gobjs, objs[sub])


# ------------------------------------------------------------------------------------------------ G5. sentinels
@pytest.mark.parametrize('E', [4, 5])
def test_spare_rows_keep_their_sentinel_and_objs_out_is_optional(gpu, E):
    name, raw = FAMILIES[0]
    table = interpolate.make_table3(ROWS)
    Q = len(ROWS)
    ep, objs = _launch(gpu, name, table, E, raw=raw, spare=1)
    assert (ep[Q] == -123.0).all() and (objs[Q] == -123.0).all(), 'the spare row was written'
    assert (ep[:Q] != -123.0).all() and (objs[:Q] != -123.0).all()
    want, want_objs = _launch(gpu, name, table, E, raw=raw)
    assert np.array_equal(ep[:Q], want) and np.array_equal(objs[:Q], want_objs)
    ep2, none = _launch(gpu, name, table, E, raw=raw, spare=1, objs=False)
    assert none is None and np.array_equal(ep2, ep)


# ------------------------------------------------------------------------------------------------ G6. end to end
NEIGHBOURS = 4  # the tiny run's archive has triangles at the issue's --neighbours 4


def test_simplex_command_on_a_finished_run(gpu, tmp_path, capsys):
    """A tiny finished three-objective run (Hopper-v3, T 32, N 2, --rng host), then the command with --simplex and
    --save-policies: the files restate each other and the written dense-front set evaluates to its own rows of
    objs.txt."""
    from pgmorl_amd.run import main
    T, N, E, points = 32, 2, 2, 3
    run = tmp_path / 'run'
    argv = ['--env-name', 'MO-Hopper-v3', '--obj-num', '3', '--num-steps', str(T), '--num-processes', str(N),
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
    pairs = interpolate.neighbour_pairs(stored, NEIGHBOURS)
    triangles = interpolate.neighbour_triangles(stored, NEIGHBOURS)
    print(f'the tiny run: {Mr} members, {len(pairs)} pairs and {len(triangles)} triangles at --neighbours {NEIGHBOURS}')
    assert stored.shape[1] == 3 and len(triangles) >= 1, (Mr, pairs)
    summary = interpolate.main([str(run), '--simplex', '--neighbours', str(NEIGHBOURS), '--points', str(points),
                                '--episodes', str(E), '--save-policies'])
    capsys.readouterr()
    out = run / 'continuous'
    assert sorted(os.listdir(out)) == ['args.txt', 'candidates.txt', 'episodes.npy', 'final', 'front.txt', 'objs.txt',
                                       'segments.txt', 'summary.json', 'triangles.txt']
    table = interpolate.candidate_table3(Mr, pairs, triangles, points)
    Q = Mr + len(pairs) * points + len(triangles) * points * (points - 1) // 2
    ep = np.load(out / 'episodes.npy')
    assert ep.shape == (Q, E, 3) and ep.dtype == np.float64 and np.isfinite(ep).all()
    means = _in_order_mean(ep)
    assert (out / 'objs.txt').read_text() == ''.join('{:5f},{:5f},{:5f}\n'.format(*o) for o in means)
    assert (out / 'candidates.txt').read_text().splitlines() == \
        [f'{a},{b},{c},{float(wa)!r},{float(wb)!r},{float(wc)!r}' for (a, b, c), (wa, wb, wc) in zip(table[0], table[1])]
    # triangles.txt, segments.txt, front.txt and summary.json are analyse3() of the tool's own means
    an = interpolate.analyse3(table, means, Mr, points, len(pairs), len(triangles))
    assert an['triangles'] == triangles
    assert (out / 'triangles.txt').read_text().splitlines() == \
        [f'{a},{b},{c},{int(ok)}' for (a, b, c), ok in zip(an['triangles'], an['filled'])]
    assert [int(x) for x in (out / 'front.txt').read_text().split()] == an['front']
    assert (out / 'segments.txt').read_text().splitlines() == \
        [f'{a},{b},{int(ok)},{an["family"][a]}' for (a, b), ok in zip(an['pairs'], an['connected'])]
    want = dict(interpolate.summarise(an, stored, NEIGHBOURS, E, 3, 3), simplex=True, num_triangles=len(triangles),
                num_filled=an['num_filled'])
    assert json.load(open(out / 'summary.json')) == summary == want
    assert (summary['M'], summary['Q'], summary['E'], summary['eval_seed']) == (Mr, Q, E, 3)
    # the written dense-front set is a save dir: evaluating it reproduces its rows of objs.txt
    got = np.loadtxt(out / 'objs.txt', delimiter=',', ndmin=2)
    evaluate.main([str(out), '--episodes', str(E)])
    capsys.readouterr()
    dense = np.loadtxt(out / 'eval' / 'objs.txt', delimiter=',', ndmin=2)
    assert len(dense) == len(an['front']) >= 1
    _close(dense, got[an['front']], BAND, 'evaluate on the dense-front set vs objs.txt')
    np.testing.assert_array_equal(np.loadtxt(out / 'final' / 'objs.txt', delimiter=',', ndmin=2), got[an['front']])
