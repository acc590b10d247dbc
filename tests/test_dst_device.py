"""The device Deep Sea Treasure without a device: the env rule (pgm_dst_transition, the inline function the kernels
call) against DeepSeaTreasureHostVecEnv on every (state, action), the argument checks of the new entry points, the
feature bit, and the constructor / CLI refusals."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

from pgmorl_amd import _lib
from pgmorl_amd._lib import Dims, DstSpec, EnvState, NormState, PGMError, RolloutBuf
from pgmorl_amd.hostenv import DeepSeaTreasureHostVecEnv

from . import cat_inputs as ci
from .test_categorical import SHORTEST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ci.ENV
ONE = C.c_void_p(1)  # a non-NULL pointer that no validated-away call dereferences
SPECS = [(ms, tlb) for ms in (50, 12) for tlb in (0, 1)]


def _p(a):
    return C.c_void_p(a.ctypes.data)


def transition(ms, tlb, row, col, step, action):
    """pgm_dst_transition on int32 arrays -> (row, col, step, obs [n, 3], obj [n, 2], reward, done, bad)."""
    row, col, step, action = (np.ascontiguousarray(x, dtype=np.int32) for x in (row, col, step, action))
    n = len(row)
    ro, co, so, done, bad = (np.full(n, -9, dtype=np.int32) for _ in range(5))
    obs, obj, rew = np.full((n, 3), np.nan), np.full((n, 2), np.nan), np.full(n, np.nan)
    rc = _lib.lib().pgm_dst_transition(C.byref(DstSpec(ms, tlb)), n, _p(row), _p(col), _p(step), _p(action), _p(ro),
                                       _p(co), _p(so), _p(obs), _p(obj), _p(rew), _p(done), _p(bad))
    _lib.check(rc, 'pgm_dst_transition')
    return ro, co, so, obs, obj, rew, done, bad


def exhaustive(ms):
    """Every open cell x action 0..3 x step in {0, 1, max_steps - 2, max_steps - 1} -> int32 (row, col, step, action)."""
    he = DeepSeaTreasureHostVecEnv(ENV, 1, 1)
    cells = [(r, c) for r in range(11) for c in range(11) if he.open[r, c]]
    assert len(cells) == 11 + sum(11 - r for r in range(1, 11)) + 4  # row 0, the r <= c triangle, four treasures
    cases = [(r, c, st, a) for (r, c), a, st in itertools.product(cells, range(4), (0, 1, ms - 2, ms - 1))]
    return tuple(np.array(x, dtype=np.int32) for x in zip(*cases))


def host_step(ms, tlb, row, col, step, action):
    """The same (state, action) pairs through DeepSeaTreasureHostVecEnv, its state arrays set directly."""
    n = len(row)
    he = DeepSeaTreasureHostVecEnv(ENV, 1, n, max_steps=ms, time_limit_is_bad=bool(tlb))
    he.reset()
    he._st = tuple(np.array(x, dtype=np.int64)[None].copy() for x in (row, col, step))
    obs, rew, done, bad, obj = he.step(np.asarray(action, dtype=np.int32)[None])
    return he._st[0][0], he._st[1][0], he._st[2][0], obs[0], obj[0], rew[0], done[0], bad[0]


# ------------------------------------------------------------------------------------------------ 1. the env rule
@pytest.mark.parametrize('ms,tlb', SPECS)
def test_transition_matches_the_host_env_exhaustively(ms, tlb):
    """Every output exactly, the fp64 ones bit for bit; the kinds of transition that must occur among the cases do."""
    row, col, step, action = exhaustive(ms)
    got = transition(ms, tlb, row, col, step, action)
    want = host_step(ms, tlb, row, col, step, action)
    for name, g, w in zip(('row', 'col', 'step', 'raw obs', 'obj', 'reward', 'done', 'bad'), got, want):
        if g.dtype == np.float64:
            assert w.dtype == np.float64 and np.array_equal(g.view(np.int64), w.view(np.int64)), name
        else:
            np.testing.assert_array_equal(g.astype(np.int64), np.asarray(w).astype(np.int64), err_msg=name)
    ro, co, so, obs, obj, rew, done, bad = got
    for value in (1.0, 3.0, 8.0, 20.0):
        assert ((rew == value) & (done == 1)).any(), f'a treasure end at the treasure worth {value}'
    assert ((done == 1) & (rew == 0)).any(), 'a step-limit end'
    assert (bad == 1).any() == bool(tlb) and not (bad & ~done).any()
    nr = row + np.array([-1, 1, 0, 0])[action]
    nc = col + np.array([0, 0, -1, 1])[action]
    off = (nr < 0) | (nr > 10) | (nc < 0) | (nc > 10)
    live = done == 0
    stay = live & (ro == row) & (co == col)
    assert (stay & off).any(), 'an off-grid move'
    assert (stay & ~off).any(), 'a blocked move'
    assert (so[live] == step[live] + 1).all() and not (ro[done == 1] | co[done == 1] | so[done == 1]).any()
    assert np.array_equal(obs, np.stack([ro / 10, co / 10, so / ms], -1).astype(np.float32).astype(np.float64))


def test_shortest_paths_give_the_reference_front():
    """The four shortest paths replayed through pgm_dst_transition: (1, 5), (3, 2.5), (8, 1.25), (20, 10/14), the
    lines of the reference run's own final front."""
    want = {(1, 0): (1, 5), (2, 1): (3, 2.5), (4, 3): (8, 1.25), (7, 6): (20, 10 / 14)}
    lines = set()
    for cell, path in SHORTEST.items():
        r = c = s = 0
        tot = np.zeros(2)
        for i, a in enumerate(path):
            ro, co, so, obs, obj, rew, done, bad = transition(50, 0, [r], [c], [s], [a])
            tot += obj[0]
            assert bool(done[0]) == (i == len(path) - 1) and not bad[0]
            r, c, s = int(ro[0]), int(co[0]), int(so[0])
        assert tuple(tot) == want[cell] and (r, c, s) == (0, 0, 0) and rew[0] == want[cell][0]
        lines.add('{:5f},{:5f}'.format(*tot))
    golden = os.path.join(ROOT, 'tests', 'golden', 'working_morl_dst', '78', 'ep', 'objs.txt')
    assert lines == set(open(golden).read().split())


def test_invalid_actions_act_as_up():
    """The host env maps an index outside 0..3 to 0; so does the rule."""
    for a in (-1, 4, 99):
        got = transition(50, 0, [3], [5], [7], [a])
        want = transition(50, 0, [3], [5], [7], [0])
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_header_under_the_host_sanitizers(tmp_path):
    """tests/cpp/dst_transition_check.cpp (its own main, pgm_dst.hpp alone) built with the address and
    undefined-behaviour sanitizers runs clean over the exhaustive set, and its lines are pgm_dst_transition's."""
    exe = tmp_path / 'dst_check'
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                    os.path.join(ROOT, 'pgmorl_amd', 'csrc'), os.path.join(ROOT, 'tests', 'cpp',
                                                                           'dst_transition_check.cpp'),
                    '-o', str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.replace('|', ' ').split() for ln in r.stdout.splitlines()]
    n = sum(len(exhaustive(ms)[0]) for ms, _ in SPECS)
    assert len(rows) == n and f'{n} cases' in r.stderr
    seen = 0
    for ms, tlb in SPECS:
        mine = [x for x in rows if (int(x[0]), int(x[1])) == (ms, tlb)]
        row, col, act, step = (np.array([int(x[i]) for x in mine], dtype=np.int32) for i in (2, 3, 4, 5))
        ro, co, so, obs, obj, rew, done, bad = transition(ms, tlb, row, col, step, act)
        ints = np.array([[int(x[i]) for i in (6, 7, 8, 15, 16)] for x in mine])
        flt = np.array([[float.fromhex(x[i]) for i in range(9, 15)] for x in mine])
        assert np.array_equal(ints, np.stack([ro, co, so, done, bad], -1))
        assert np.array_equal(flt, np.concatenate([obs, obj, rew[:, None]], -1))
        seen += len(mine)
    assert seen == n


# ------------------------------------------------------------------------------------------------ 2. argument checks
def _structs():
    st = EnvState(ONE, None, ONE, ONE, ONE, None)  # elapsed and s0 may be NULL
    ns = NormState(*([ONE] * 9), 0.995, 10.0, 10.0, 1e-8, 1, 1)
    return st, ns, RolloutBuf(*([ONE] * 9))


def _rollout(d=None, params=ONE, env=None, st=None, ns=None, rb=None, dref=True):
    s, n, r = _structs()
    d = Dims(2, 4, 8, 3, 4, 2, 64, 0) if d is None else d
    env = DstSpec(50, 0) if env is None else env
    return _lib.lib().pgm_rollout_dst(C.byref(d) if dref else None, params, C.byref(env), C.byref(st or s),
                                      C.byref(ns or n), C.byref(rb or r), None, 0, 0, None)


def _eval(d=None, params=ONE, env=None, mean=ONE, var=ONE, E=3, use_ob=1, out=ONE):
    d = Dims(2, 99, -3, 3, 4, 2, 64, 0) if d is None else d  # N and T are ignored
    env = DstSpec(50, 0) if env is None else env
    return _lib.lib().pgm_eval_dst(C.byref(d), params, C.byref(env), mean, var, E, use_ob, 1, 0.99, out, None)


def test_argument_errors():
    """Every refusal of the ABI table returns before any device call (this host has no device), in the table's order."""
    L = _lib.lib()
    inv, shape, unsup = _lib.PGM_E_INVALID_ARG, _lib.PGM_E_SHAPE, _lib.PGM_E_UNSUPPORTED
    # NULL pointers
    assert _rollout(dref=False) == inv and _rollout(params=None) == inv
    st, ns, rb = _structs()
    st.s = None
    assert _rollout(st=st) == inv
    st, ns, rb = _structs()
    ns.ret_var = None
    assert _rollout(ns=ns) == inv
    for field in ('obs', 'actions', 'logp', 'values', 'rewards', 'masks', 'bad_masks'):
        st, ns, rb = _structs()
        setattr(rb, field, None)
        assert _rollout(rb=rb) == inv, field
    assert L.pgm_rollout_dst(C.byref(Dims(2, 4, 8, 3, 4, 2, 64, 0)), ONE, None, C.byref(st), C.byref(ns),
                             C.byref(_structs()[2]), None, 0, 0, None) == inv
    assert _eval(params=None) == inv and _eval(out=None) == inv and _eval(mean=None) == inv and _eval(var=None) == inv
    assert L.pgm_eval_dst(None, ONE, C.byref(DstSpec(50, 0)), ONE, ONE, 1, 1, 1, 0.99, ONE, None) == inv
    # (a NULL pointer outranks bad dims)
    assert _rollout(d=Dims(0, 4, 8, 3, 4, 2, 64, 0), params=None) == inv
    # check_dims
    assert _rollout(d=Dims(0, 4, 8, 3, 4, 2, 64, 0)) == shape and _eval(d=Dims(0, 4, 8, 3, 4, 2, 64, 0)) == shape
    assert _rollout(d=Dims(2, 9, 8, 3, 4, 2, 64, 0)) == unsup and b'N=9' in L.pgm_last_error()
    assert _rollout(d=Dims(2, 4, 8, 3, 4, 2, 32, 0)) == unsup and b'hidden size' in L.pgm_last_error()
    assert _eval(d=Dims(2, 4, 8, 3, 4, 2, 32, 0)) == unsup and b'hidden size' in L.pgm_last_error()
    # the dim set
    for call, name in ((_rollout, b'pgm_rollout_dst'), (_eval, b'pgm_eval_dst')):
        assert call(d=Dims(2, 4, 8, 17, 6, 2, 64, 0)) == unsup
        assert b'Categorical' in L.pgm_last_error() and name in L.pgm_last_error()
        # LN = 1, with a message (and it outranks T, eval_num and max_steps)
        assert call(d=Dims(2, 4, 0, 3, 4, 2, 64, 1), env=DstSpec(0, 0)) == unsup
        assert b'LayerNorm' in L.pgm_last_error() and name in L.pgm_last_error()
    assert _eval(d=Dims(2, 4, 8, 3, 4, 2, 64, 1), E=0) == unsup
    # T <= 0 (outranks max_steps)
    assert _rollout(d=Dims(2, 4, 0, 3, 4, 2, 64, 0), env=DstSpec(0, 0)) == shape
    # eval_num outside 1..8 (outranks max_steps)
    for E in (0, 9, -1):
        assert _eval(E=E, env=DstSpec(0, 0)) == inv and b'eval_num' in L.pgm_last_error()
    # max_steps <= 0
    for ms in (0, -5):
        assert _rollout(env=DstSpec(ms, 0)) == inv and b'max_steps' in L.pgm_last_error()
        assert _eval(env=DstSpec(ms, 1)) == inv and b'max_steps' in L.pgm_last_error()
    # without use_ob_rms the statistics may be NULL: the call then passes validation, so it is not made here
    # pgm_dst_transition: NULL pointers, negative n, max_steps; n = 0 is fine
    a = np.zeros(1, dtype=np.int32)
    f = np.zeros(3)
    ok = [C.byref(DstSpec(50, 0)), 1] + [_p(a)] * 7 + [_p(f), _p(f), _p(f), _p(a), _p(a)]
    for i in [0] + list(range(2, 14)):
        args = list(ok)
        args[i] = None
        assert L.pgm_dst_transition(*args) == inv, i
    assert L.pgm_dst_transition(*(ok[:1] + [-1] + ok[2:])) == inv
    assert L.pgm_dst_transition(*([C.byref(DstSpec(0, 0))] + ok[1:])) == inv and b'max_steps' in L.pgm_last_error()
    assert L.pgm_dst_transition(*(ok[:1] + [0] + ok[2:])) == _lib.PGM_OK


# ------------------------------------------------------------------------------------------------ 3. feature bit, refusals
def test_feature_bit():
    assert _lib.lib().pgm_abi_features() & 2 and _lib.features() & _lib.FEATURE_DST_DEVICE
    assert _lib.FEATURE_DST_DEVICE == 2 and _lib.lib().pgm_abi_features() & _lib.FEATURE_CATEGORICAL
    assert _lib.lib().pgm_abi_version() == 5 and _lib.lib().pgm_abi_minor() == 1  # the version pair is unchanged
    _lib.require_dst_device()
    assert C.sizeof(DstSpec) == 8


def test_taskbatch_refusals():
    from pgmorl_amd.runtime import TaskBatch
    with pytest.raises(PGMError, match='host_env'):  # neither: the refusal from before, now naming both options
        TaskBatch(ENV, 2, device='cpu')
    with pytest.raises(PGMError, match='device_env'):
        TaskBatch(ENV, 2, device='cpu')
    with pytest.raises(PGMError, match='exactly one'):
        TaskBatch(ENV, 2, device='cpu', host_env=DeepSeaTreasureHostVecEnv(ENV, 2, 4), device_env=True)
    with pytest.raises(PGMError, match='Categorical'):
        TaskBatch(ENV, 2, device='cpu', layernorm=True, device_env=True)
    with pytest.raises(PGMError, match='eval_num'):
        TaskBatch(ENV, 2, device='cpu', device_env=True, eval_num=9)


def test_cli_refusals_leave_no_save_dir(tmp_path):
    from pgmorl_amd.run import get_parser, main
    assert get_parser().parse_args(['--device-env']).device_env is True
    assert get_parser().parse_args([]).device_env is False
    prev = torch.get_default_dtype()
    try:
        for i, (env, extra, msg) in enumerate(((ENV, [], '--device-env'),
                                               (ENV, ['--device-env', '--host-env', 'dst'], 'together with --host-env'),
                                               ('MO-Hopper-v2', ['--device-env', '--host-env', 'synth'],
                                                'together with --host-env'),
                                               (ENV, ['--device-env', '--layernorm'], 'Categorical'))):
            save = tmp_path / f'run{i}'
            with pytest.raises(PGMError, match=msg):
                main(['--env-name', env, '--obj-num', '2', '--save-dir', str(save)] + extra)
            assert not save.exists()
    finally:
        torch.set_default_dtype(prev)


def test_population_threads_the_flag():
    """MOPGPopulation reads args.device_env (the --device-env flag) and hands it to its TaskBatch."""
    from pgmorl_amd.mopg import MOPGPopulation
    from pgmorl_amd.run import get_parser, merge_argv
    args = get_parser().parse_args(merge_argv(['--env-name', ENV, '--device-env']))
    assert MOPGPopulation(args, device='cpu').device_env is True
    assert MOPGPopulation(args, device='cpu', device_env=False).device_env is False
    args = get_parser().parse_args(merge_argv(['--env-name', ENV, '--host-env', 'dst']))
    assert MOPGPopulation(args, device='cpu').device_env is False
