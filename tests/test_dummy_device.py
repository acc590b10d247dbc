"""The device MO-Dummy envs without a device: the env rule (pgm_dummy_transition, the inline function the kernels call)
against DummyMOHostVecEnv bit for bit, known answers, the argument checks of the new entry points, the feature bit, the
envspec lists, the parameter layout at the new dims, the CLI parser, and the episode ends of the reference rollouts
the GPU tests use."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from pgmorl_amd import _lib, envspec
from pgmorl_amd._lib import Dims, DummySpec, EnvState, NormState, PGMError, RolloutBuf
from pgmorl_amd.hostenv import DummyMOHostVecEnv, check_spec

from . import dummy_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = C.c_void_p(1)  # a non-NULL pointer that no validated-away call dereferences
SPECS = [(K, ms, bound, tlb) for K in (2, 3) for ms, bound in ((500, 5.0), (12, 1.25)) for tlb in (0, 1)]
NAMES = ('state', 'step', 'episode', 'obj', 'reward', 'done', 'bad')


def _same(got, want, what=''):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype == np.float64:
            assert w.dtype == np.float64 and np.array_equal(g.view(np.int64), w.view(np.int64)), f'{name} {what}'
        else:
            np.testing.assert_array_equal(g.astype(np.int64), w.astype(np.int64), err_msg=f'{name} {what}')


def _grid(K, ms, bound, tlb, R=3):
    state, step, episode, action = dr.grid_cases(ms, bound)
    n = len(step)
    table = envspec.dummy_reset_table(0, n, R)
    return state, step, episode, np.arange(n, dtype=np.int32), action, table


# ------------------------------------------------------------------------------------------------ 1. the env rule
@pytest.mark.parametrize('K,ms,bound,tlb', SPECS)
def test_transition_matches_the_host_env_on_the_grid(K, ms, bound, tlb):
    """Every output exactly, the fp64 ones bit for bit; the kinds of transition that must occur among the cases do."""
    state, step, episode, env, action, table = _grid(K, ms, bound, tlb)
    got = dr.transition(K, state, step, episode, env, action, table, ms, bound, tlb)
    want = dr.host_step(K, state, step, episode, action, ms, bound, tlb, R=3)
    _same(got, want)
    s2, so, eo, obj, rew, done, bad = got
    ac = np.clip(action.astype(np.float64), -1, 1)
    vel = (state[:, 2:4] + ac * 0.1) * 0.95
    land = state[:, :2] + vel
    r = np.sqrt(land[:, 0] * land[:, 0] + land[:, 1] * land[:, 1])
    out, limit = r > bound, step + 1 >= ms
    np.testing.assert_array_equal(done, (out | limit).astype(np.int32))
    np.testing.assert_array_equal(bad, ((out | limit) & (step + 1 == ms)).astype(np.int32) * tlb)
    assert (out & limit).any() and (out & ~limit).any() and (~out & limit).any() and (~out & ~limit).any()
    if tlb:
        assert bad[out & limit].all(), 'leaving the disc on the limit step is a time-limit end'
    near = np.abs(r - bound) < 1e-11
    assert (near & out).any() and (near & ~out).any(), 'landing points within 1e-12 of the bound on both sides'
    assert (np.abs(action) > 1).any() and (np.abs(action) == 1).any()
    live = done == 0
    assert (so[live] == step[live] + 1).all() and (eo[live] == episode[live]).all()
    d = done == 1
    assert (eo[d] == episode[d] + 1).all() and not so[d].any() and not s2[d, 2:].any()
    assert np.array_equal(s2[d, :2], table[env[d], eo[d] % 3])
    assert np.array_equal(s2[live, :2], land[live]) and obj.shape == (len(step), K)
    if K == 3:
        assert np.array_equal(obj[:, 2], bound - r)


@pytest.mark.parametrize('K,tlb', [(2, 1), (3, 0)])
def test_random_trajectories_with_resets_and_wraparound(K, tlb):
    """10,000 random 60-step trajectories at (max_steps 12, bound 1.25, R = 3): pgm_dummy_transition fed its own
    outputs stays on DummyMOHostVecEnv (10,000 envs of one task, one reset-table row each) bit for bit at every step;
    the episode counters pass R and the table wraps around."""
    n, steps, R, ms, bound = 10000, 60, 3, 12, 1.25
    he = DummyMOHostVecEnv(dr.ENVS[K], 1, n, seed=5, max_steps=ms, bound=bound, time_limit_is_bad=bool(tlb), R=R)
    obs = he.reset()[0]
    table = envspec.dummy_reset_table(5, n, R)
    assert np.array_equal(obs[:, :2], table[:, 0]) and not obs[:, 2:].any()
    state, step, episode = obs.copy(), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    env = np.arange(n, dtype=np.int32)
    rng = np.random.RandomState(1)
    ends = np.zeros(2, dtype=np.int64)
    for t in range(steps):
        action = (rng.randn(n, 2) * 1.5).astype(np.float32)
        got = dr.transition(K, state, step, episode, env, action, table, ms, bound, tlb)
        o, rew, done, bad, obj = he.step(action[None])
        _same(got, (o[0], he._st['step'][0], he._st['episode'][0], obj[0], rew[0], done[0], bad[0]), f'step {t}')
        state, step, episode = got[0], got[1], got[2]
        ends += (int((got[5] == 1).sum()), int((got[6] == 1).sum()))
    assert episode.max() > R and ends[0] > n and (ends[1] > 0) == bool(tlb)


def test_header_under_the_host_sanitizers(tmp_path):
    """tests/cpp/dummy_transition_check.cpp (its own main, pgm_dummy.hpp alone) built with the address and
    undefined-behaviour sanitizers runs clean over the grid of every spec, and its lines are pgm_dummy_transition's."""
    exe = tmp_path / 'dummy_check'
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'pgmorl_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'cpp', 'dummy_transition_check.cpp'), '-o', str(exe)], check=True)
    text, want = [], []
    hx = lambda v: ' '.join(float(x).hex() for x in np.asarray(v, dtype=np.float64).reshape(-1))
    for K, ms, bound, tlb in SPECS:
        state, step, episode, env, action, table = _grid(K, ms, bound, tlb)
        n = len(step)
        text.append(f'{ms} {tlb} {float(bound).hex()} {K} {table.shape[1]} {table.shape[0]} {n}\n{hx(table)}\n')
        for i in range(n):
            text.append(f'{hx(state[i])} {step[i]} {episode[i]} {env[i]} {hx(action[i])}\n')
        want.append((K, dr.transition(K, state, step, episode, env, action, table, ms, bound, tlb)))
    r = subprocess.run([str(exe)], input=''.join(text), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    total = sum(len(w[1][1]) for w in want)
    assert len(rows) == total and f'{total} cases' in r.stderr
    at = 0
    for K, (s2, so, eo, obj, rew, done, bad) in want:
        mine = rows[at:at + len(so)]
        at += len(so)
        flt = np.array([[float.fromhex(x) for x in row[:10]] for row in mine])
        ints = np.array([[int(x) for x in row[10:]] for row in mine])
        obj3 = np.concatenate([obj, np.zeros((len(so), 3 - K))], -1)
        assert np.array_equal(flt.view(np.int64), np.concatenate([s2, obj3, rew[:, None]], -1).view(np.int64))
        assert np.array_equal(ints, np.stack([so, eo, done, bad], -1))


# ------------------------------------------------------------------------------------------------ 2. known answers
def _one(K, state, step, action, **kw):
    table = envspec.dummy_reset_table(0, 1, 2)
    return dr.transition(K, [state], [step], [0], [0], [action], table, **kw)


def test_known_answers():
    s2, so, eo, obj, rew, done, bad = _one(2, np.zeros(6), 0, (1.0, 0.0))
    assert s2[0, 2] == 0.1 * 0.95 == 0.095 and s2[0, 3] == 0 and s2[0, 0] == 0.095 and s2[0, 1] == 0
    assert obj[0, 0] == 0.095 and obj[0, 1] == 1 / 1.1 and rew[0] == 0.095 + 0.1 * (1 / 1.1)
    assert s2[0, 4] == 0.095 and s2[0, 5] == 1.0 and so[0] == 1 and not done[0] and not bad[0]
    s2, so, eo, obj, rew, done, bad = _one(3, np.zeros(6), 0, (0.0, 0.0))
    assert obj[0, 1] == 10.0 and obj[0, 0] == 0 and obj[0, 2] == 5.0 and not s2.any()
    # a constant action (1, 0) from rest at the origin: vel_n = 0.1 q (1 - q^n) / (1 - q), q = 0.95, so
    # pos_n = (0.1 q / (1 - q)) (n - q (1 - q^n) / (1 - q)); the env leaves the disc of radius 5 at the first n with
    # pos_n > 5
    q = 0.95
    pos = lambda n: (0.1 * q / (1 - q)) * (n - q * (1 - q ** n) / (1 - q))
    leave = next(n for n in range(1, 500) if pos(n) > 5.0)
    assert pos(leave - 1) < 5.0 - 1e-6 and pos(leave) > 5.0 + 1e-6  # (far from the decision: the closed form decides)
    state, step, length = np.zeros(6), 0, 0
    while True:
        s2, so, eo, obj, rew, done, bad = _one(2, state, step, (1.0, 0.0))
        length += 1
        if done[0]:
            break
        state, step = s2[0], int(so[0])
        assert abs(state[0] - pos(length)) < 1e-9
    assert length == leave and not bad[0] and eo[0] == 1 and so[0] == 0
    assert np.array_equal(s2[0, :2], envspec.dummy_reset_table(0, 1, 2)[0, 1])
    # the same walk under a limit one step before it leaves: a time-limit end (or a termination when so reported)
    for tlb in (0, 1):
        state, step = np.zeros(6), 0
        for n in range(1, leave):
            s2, so, eo, obj, rew, done, bad = _one(2, state, step, (1.0, 0.0), max_steps=leave - 1, tlb=tlb)
            state, step = s2[0], int(so[0])
        assert done[0] and bad[0] == tlb


def test_reset_table():
    t = envspec.dummy_reset_table(3, 4)
    assert t.shape == (4, 256, 2) and t.dtype == np.float64 and (np.abs(t) <= 1).all() and envspec.DUMMY_RESETS == 256
    assert np.array_equal(envspec.dummy_reset_table(4, 2, 7), envspec.dummy_reset_table(3, 3, 7)[1:])  # keyed by seed + i
    assert np.array_equal(t[1, :5], envspec.dummy_reset_table(3, 2, 5)[1])  # a shorter table is a prefix
    assert len(np.unique(t.reshape(-1))) == t.size and abs(t.mean()) < 0.05
    assert not np.array_equal(t[0, 0], 2 * envspec.reset_state(2, 3))  # a stream of its own
    with pytest.raises(ValueError, match='R'):
        envspec.dummy_reset_table(0, 1, 0)
    he = DummyMOHostVecEnv('MO-Dummy3-v0', 2, 3, seed=3)
    assert np.array_equal(he.reset()[1, :, :2], t[:3, 0]) and he.dims() == (6, 2, 3) and he.R == 256
    assert np.array_equal(he.eval_reset(4)[0, :, :2], t[:, 0])


# ------------------------------------------------------------------------------------------------ 3. argument checks
def _structs():
    st = EnvState(ONE, ONE, ONE, ONE, ONE, None)  # s0 may be NULL
    ns = NormState(*([ONE] * 9), 0.995, 10.0, 10.0, 1e-8, 1, 1)
    return st, ns, RolloutBuf(*([ONE] * 9))


def _spec(ms=500, tlb=1, bound=5.0, table=ONE, R=256, count=8):
    return DummySpec(ms, tlb, bound, table, R, count)


def _rollout(d=None, params=ONE, env=None, st=None, episode=ONE, ns=None, rb=None, dref=True, eref=True):
    s, n, r = _structs()
    d = Dims(2, 4, 8, 6, 2, 2, 64, 0) if d is None else d
    env = _spec() if env is None else env
    return _lib.lib().pgm_rollout_dummy(C.byref(d) if dref else None, params, C.byref(env) if eref else None,
                                        C.byref(st or s), episode, C.byref(ns or n), C.byref(rb or r), None, 0, 0, None)


def _eval(d=None, params=ONE, env=None, mean=ONE, var=ONE, E=3, use_ob=1, out=ONE):
    d = Dims(2, 99, -3, 6, 2, 3, 64, 0) if d is None else d  # N and T are ignored
    env = _spec() if env is None else env
    return _lib.lib().pgm_eval_dummy(C.byref(d), params, C.byref(env), mean, var, E, use_ob, 1, 0.99, out, None)


def test_argument_errors():
    """Every refusal returns before any device call (this host has no device), with a message."""
    L = _lib.lib()
    inv, shape, unsup = _lib.PGM_E_INVALID_ARG, _lib.PGM_E_SHAPE, _lib.PGM_E_UNSUPPORTED
    # NULL pointers
    assert _rollout(dref=False) == inv and _rollout(params=None) == inv and _rollout(eref=False) == inv
    assert _rollout(episode=None) == inv and b'null pointer' in L.pgm_last_error()
    assert _rollout(env=_spec(table=None)) == inv
    for field in ('s', 'elapsed', 'obj_acc', 'obj_acc_valid', 'ret'):
        st, ns, rb = _structs()
        setattr(st, field, None)
        assert _rollout(st=st) == inv, field
    st, ns, rb = _structs()
    ns.ret_var = None
    assert _rollout(ns=ns) == inv
    for field in ('obs', 'actions', 'logp', 'values', 'rewards', 'masks', 'bad_masks'):
        st, ns, rb = _structs()
        setattr(rb, field, None)
        assert _rollout(rb=rb) == inv, field
    assert _eval(params=None) == inv and _eval(out=None) == inv and _eval(mean=None) == inv and _eval(var=None) == inv
    assert _eval(env=_spec(table=None)) == inv and b'pgm_eval_dummy' in L.pgm_last_error()
    assert _rollout(d=Dims(0, 4, 8, 6, 2, 2, 64, 0), params=None) == inv  # (a NULL pointer outranks bad dims)
    # check_dims
    assert _rollout(d=Dims(0, 4, 8, 6, 2, 2, 64, 0)) == shape and _eval(d=Dims(0, 4, 8, 6, 2, 2, 64, 0)) == shape
    assert _rollout(d=Dims(2, 9, 8, 6, 2, 2, 64, 0)) == unsup and b'N=9' in L.pgm_last_error()
    assert _rollout(d=Dims(2, 4, 8, 6, 2, 2, 32, 0)) == unsup and b'hidden size' in L.pgm_last_error()
    assert _eval(d=Dims(2, 4, 8, 6, 2, 3, 32, 0)) == unsup and b'hidden size' in L.pgm_last_error()
    # the dim set
    for call, name in ((_rollout, b'pgm_rollout_dummy'), (_eval, b'pgm_eval_dummy')):
        for dims in ((8, 2, 2), (17, 6, 2), (6, 2, 4), (6, 3, 2), (19, 6, 2)):
            assert call(d=Dims(2, 4, 8, *dims, 64, 0)) == unsup
            assert b'MO-Dummy' in L.pgm_last_error() and name in L.pgm_last_error()
        # LN outside {0, 1} (it outranks T, eval_num and the spec); LN = 1 is allowed
        assert call(d=Dims(2, 4, 0, 6, 2, 2, 64, 2), env=_spec(ms=0)) == inv and b'LN' in L.pgm_last_error()
    # T <= 0 (outranks the spec)
    assert _rollout(d=Dims(2, 4, 0, 6, 2, 2, 64, 1), env=_spec(ms=0)) == shape and b'T must' in L.pgm_last_error()
    # eval_num outside 1..8 (outranks the spec)
    for E in (0, 9, -1):
        assert _eval(E=E, env=_spec(ms=0)) == inv and b'eval_num' in L.pgm_last_error()
    # the spec: max_steps, bound, R, the rows of the table
    for call in (_rollout, _eval):
        for ms in (0, -5):
            assert call(env=_spec(ms=ms)) == inv and b'max_steps' in L.pgm_last_error()
        for b in (0.0, -1.0, float('nan')):
            assert call(env=_spec(bound=b)) == inv and b'bound' in L.pgm_last_error()
        for R in (0, -3):
            assert call(env=_spec(R=R)) == inv and b'R =' in L.pgm_last_error()
        assert call(env=_spec(count=2)) == inv and b'reset_count' in L.pgm_last_error()  # N = 4 envs, E = 3 episodes
    # pgm_dummy_transition: NULL pointers, negative n, K, the spec, env / episode out of range; n = 0 is fine
    i32, f64, f32 = np.zeros(1, dtype=np.int32), np.zeros(6), np.zeros(2, dtype=np.float32)
    tab = np.zeros((1, 2, 2))
    p = lambda a: C.c_void_p(a.ctypes.data)
    sp = DummySpec(500, 1, 5.0, p(tab), 2, 1)
    ok = [C.byref(sp), 2, 1, p(f64), p(i32), p(i32), p(i32), p(f32), p(f64), p(i32), p(i32), p(f64), p(f64), p(i32), p(i32)]
    assert L.pgm_dummy_transition(*ok) == _lib.PGM_OK
    for i in [0] + list(range(3, 15)):
        args = list(ok)
        args[i] = None
        assert L.pgm_dummy_transition(*args) == inv, i
    assert L.pgm_dummy_transition(*(ok[:2] + [-1] + ok[3:])) == inv
    assert L.pgm_dummy_transition(*(ok[:2] + [0] + ok[3:])) == _lib.PGM_OK
    for K in (1, 4):
        assert L.pgm_dummy_transition(*(ok[:1] + [K] + ok[2:])) == unsup and b'K=' in L.pgm_last_error()
    for bad_spec, word in ((DummySpec(0, 1, 5.0, p(tab), 2, 1), b'max_steps'), (DummySpec(5, 1, 0.0, p(tab), 2, 1), b'bound'),
                           (DummySpec(5, 1, 5.0, p(tab), 0, 1), b'R ='), (DummySpec(5, 1, 5.0, p(tab), 2, 0), b'reset_count'),
                           (DummySpec(5, 1, 5.0, None, 2, 1), b'null')):
        assert L.pgm_dummy_transition(*([C.byref(bad_spec)] + ok[1:])) == inv and word in L.pgm_last_error()
    one, neg = np.ones(1, dtype=np.int32), np.full(1, -1, dtype=np.int32)
    assert L.pgm_dummy_transition(*(ok[:6] + [p(one)] + ok[7:])) == inv and b'env 1' in L.pgm_last_error()
    assert L.pgm_dummy_transition(*(ok[:5] + [p(neg)] + ok[6:])) == inv and b'episode -1' in L.pgm_last_error()


# ------------------------------------------------------------------------------------------------ 4. bit, lists, layout, CLI
def test_feature_bit():
    assert _lib.lib().pgm_abi_features() == 7 and _lib.features() & _lib.FEATURE_DUMMY_DEVICE
    assert _lib.FEATURE_DUMMY_DEVICE == 4
    assert _lib.lib().pgm_abi_version() == 5 and _lib.lib().pgm_abi_minor() == 1  # the version pair is unchanged
    _lib.require_dummy_device()
    assert C.sizeof(DummySpec) == 32 and DummySpec.bound.offset == 8 and DummySpec.reset_table.offset == 16
    assert C.sizeof(_lib.DstSpec) == 8 and C.sizeof(Dims) == 32  # existing structs keep their layout


def test_envspec_lists():
    assert envspec.native_env_names() == ['MO-Dummy-v0', 'MO-Dummy3-v0']
    assert len(envspec.env_names()) == 7 and envspec.discrete_env_names() == ['MO-DeepSeaTreasure-v0']
    assert not set(envspec.native_env_names()) & set(envspec.env_names())
    for name, K in (('MO-Dummy-v0', 2), ('MO-Dummy3-v0', 3)):
        sp = envspec.make_spec(name)
        assert (sp['obs_dim'], sp['act_dim'], sp['obj_num'], sp['max_episode_steps'], sp['bound']) == (6, 2, K, 500, 5.0)
        assert sp['native'] == 'dummy' and not sp.get('discrete') and 'U' not in sp and 'd' not in sp
        assert np.array_equal(sp['act_lo'], [-1, -1]) and np.array_equal(sp['act_hi'], [1, 1])
    with pytest.raises(ValueError, match='MO-Dummy3-v0'):
        envspec.make_spec('MO-Dummy4-v0')


@pytest.mark.parametrize('K', [2, 3])
@pytest.mark.parametrize('ln', [False, True])
def test_param_layout_round_trip(K, ln):
    from oracle.policy import make_policy
    from pgmorl_amd.layout import ParamLayout
    lay = ParamLayout(6, 2, K, layernorm=ln)
    torch.manual_seed(K)
    sd = make_policy(6, 2, K, layernorm=ln).state_dict()
    flat = lay.flatten(sd)
    assert flat.shape == (lay.total,) and lay.total % 64 == 0
    back = lay.unflatten(torch.from_numpy(flat))
    assert list(back) == list(sd) and all(torch.equal(back[k].double(), sd[k].float().double()) for k in sd)
    assert sd['base.actor.0.weight'].shape == (64, 6) and sd['base.critic_linear.weight'].shape == (K, 64)
    # 19/6/2 stays outside the dim sets (the message lists the new ones)
    d = Dims(1, 1, 1, 19, 6, 2, 64, 0)
    assert _lib.lib().pgm_act_forward(C.byref(d), ONE, ONE, ONE, 0, ONE, ONE, ONE, None) == _lib.PGM_E_UNSUPPORTED
    msg = _lib.lib().pgm_last_error()
    assert b'unsupported dims' in msg and b'6/2/2' in msg and b'6/2/3' in msg


def test_cli_parser_and_host_env_spec():
    from pgmorl_amd.mopg import MOPGPopulation
    from pgmorl_amd.run import get_parser, merge_argv
    for name, K in (('MO-Dummy-v0', 2), ('MO-Dummy3-v0', 3)):
        args = get_parser().parse_args(merge_argv(['--env-name', name, '--obj-num', str(K)]))
        assert args.env_name == name and args.host_env is None and args.device_env is False and args.rng == 'device'
        pop = MOPGPopulation(args, device='cpu')
        assert pop.host_env_factory is None and (pop.layout.O, pop.layout.A, pop.layout.K) == (6, 2, K)
        assert check_spec('dummy', name) is DummyMOHostVecEnv
        args = get_parser().parse_args(merge_argv(['--env-name', name, '--host-env', 'dummy', '--rng', 'host']))
        assert MOPGPopulation(args, device='cpu').host_env_factory is DummyMOHostVecEnv
    with pytest.raises(ValueError, match='MO-Dummy envs only'):
        check_spec('dummy', 'MO-Hopper-v2')
    with pytest.raises(ValueError, match='no SynthMO stand-in'):
        check_spec('synth', 'MO-Dummy-v0')
    with pytest.raises(ValueError):
        check_spec('dst', 'MO-Dummy-v0')


def test_taskbatch_defaults_and_refusals():
    from pgmorl_amd.runtime import TaskBatch
    tb = TaskBatch('MO-Dummy3-v0', 2, num_processes=3, num_steps=8, device='cpu', seed=3, eval_num=2)
    assert tb.dummy_env and not tb.device_env and not tb.discrete and tb.host_env is None and (tb.O, tb.A, tb.K) == (6, 2, 3)
    assert (tb.mode.max_steps, tb.mode.bound, tb.mode.time_limit_is_bad, tb.mode.R) == (500, 5.0, True, 256)
    assert tb.episode.shape == (2, 3) and tb.episode.dtype == torch.int32 and tb.noise.shape == (8, 3, 2)
    assert np.array_equal(tb.mode._dummy_train.numpy(), envspec.dummy_reset_table(3, 3))
    assert np.array_equal(tb.mode._dummy_eval.numpy(), envspec.dummy_reset_table(3, 2))
    assert tb.mode.c_dummy.reset_count == 3 and tb.mode.c_dummy_eval.reset_count == 2 and tb.mode.c_dummy.time_limit_is_bad == 1
    tb = TaskBatch('MO-Dummy-v0', 1, num_processes=2, num_steps=8, device='cpu', device_env=True, layernorm=True,
                   max_steps=12, bound=1.25, time_limit_is_bad=False, R=3)
    assert tb.dummy_env and tb.layernorm and (tb.mode.max_steps, tb.mode.bound, tb.mode.time_limit_is_bad, tb.mode.R) == (12, 1.25, False, 3)
    with pytest.raises(PGMError, match='eval_num'):
        TaskBatch('MO-Dummy-v0', 1, device='cpu', eval_num=9)
    with pytest.raises(PGMError, match='must be positive'):
        TaskBatch('MO-Dummy-v0', 1, device='cpu', R=0)
    with pytest.raises(TypeError):
        TaskBatch('MO-Dummy-v0', 1, 4, 8, 0, 1, 0.995, 0.95, True, True, True, True, True, 0.2, 10, 32, 0.5, 0.0, 0.5,
                  1e-5, True, 'cpu', None, False, None, False, 12)  # max_steps is keyword-only
    with pytest.raises(PGMError, match='pgm_dummy_transition'):
        tb.env_step(torch.zeros(1, 2, 2))


# ------------------------------------------------------------------------------------------------ 5. the reference cases
@pytest.mark.parametrize('K', [2, 3])
@pytest.mark.parametrize('short', [False, True], ids=['defaults', 'limit12'])
def test_reference_rollouts_contain_both_episode_ends(K, short):
    """The reference rollouts the GPU tests compare against, from the reference alone: at (max_steps 12, bound 1.25)
    at least 3 true terminals and 3 time-limit ends per task, at the defaults at least 2 true terminals; the seed is
    the first counting up from 0 that meets the input rule, and every skipped seed violates it."""
    seed, (pols, noise, refs, bad, counts), skipped = dr.reference_case(K, short)
    print(f'K {K} short {short}: seed {seed}, (terminals, time-limit ends) per task {counts}, skipped {skipped}')
    assert not bad and sorted(skipped) == list(range(seed))
    for s, why in skipped.items():
        again = dr.rollout_case(K, 2, 4, 48, 2, s, dict(dr.SHORT) if short else {})[3]
        assert again and again == why, f'seed {s} was skipped without a violation'
    for term, limit in counts:
        assert term >= (3 if short else 2), counts
        if short:
            assert limit >= 3, counts
