"""Device env plug-ins on the CPU: the plug-in libraries build with the cross-compiler and load without a device, so
everything but the two kernels is checked here -- the header contract (info, the build cache, the headers that must
fail to build), the host functions against the numpy restatements of tests/envplug_envs.py bit for bit, the argument
refusals of the launch entry points in their documented order, the Python layers and the CLI refusals."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from pgmorl_amd import _lib, build, envplug, envspec
from pgmorl_amd._lib import Dims, EnvState, NormState, PGMError, PPOHParams, RolloutBuf
from pgmorl_amd.envplug import EnvPlugin
from pgmorl_amd.hostenv import PluginHostVecEnv

from . import dummy_ref as dr
from . import envplug_envs as pe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = (pe.Line, pe.Chain, pe.PlugDummy, pe.Wide)
ENVS = pytest.mark.parametrize('env', ALL + (pe.NoLimit,), ids=lambda e: e.NAME)


@pytest.fixture(scope='module')
def plugins():
    """Every test plug-in, built in one batch (at most four compile processes) and loaded once."""
    build.build_envs([pe.header(e.NAME) for e in ALL + (pe.NoLimit,)])
    return {e.NAME: EnvPlugin(pe.header(e.NAME)) for e in ALL + (pe.NoLimit,)}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _assert_same(got, want, what):
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(_bits(got[k]), _bits(want[k])), \
            f'{k} differs {what}: {got[k][:4]} vs {want[k][:4]}'


# ------------------------------------------------------------------------------------------------ 1. info
@ENVS
def test_info(plugins, env):
    pl = plugins[env.NAME]
    assert pl.info == pe.info(env) and pl.dims() == (env.O, env.A, env.K) and pl.DISCRETE is env.DISCRETE
    assert pl.h.pgm_envplug_abi() == envplug.PGM_ENVPLUG_ABI == 1
    assert pl.h.pgm_envplug_info(None) == _lib.PGM_E_INVALID_ARG and 'pgm_envplug_info' in pl.last_error()


# ------------------------------------------------------------------------------------------------ 2. the build cache
def test_build_cache(tmp_path, monkeypatch):
    """The library's directory is named by the hash of the header and the sources: a second build_env compiles
    nothing, a changed header is another library, and the plug-in batch uses at most four compile processes."""
    hdr = tmp_path / 'cached.hpp'
    shutil.copy(pe.header('nolimit'), hdr)
    calls = []
    real = subprocess.run
    monkeypatch.setattr(build.subprocess, 'run', lambda cmd, **kw: (calls.append(cmd), real(cmd, **kw))[1])
    lib1 = build.build_env(str(hdr))
    try:
        assert len(calls) == 1 and calls[0][-1].startswith(lib1) and '-include' in calls[0]
        assert all(f in calls[0] for f in build.FLAGS), 'build.FLAGS are used'
        rel = os.path.relpath(lib1, os.path.join(ROOT, 'pgmorl_amd', 'build_env'))
        stem, name = os.path.split(rel)
        assert name == 'libpgm_env.so' and stem.startswith('cached-') and len(stem) == len('cached-') + 12
        assert build.build_env(str(hdr)) == lib1 and len(calls) == 1, 'a second call does not recompile'
        os.utime(hdr)  # the hash is of the contents: a new mtime alone is not a change
        assert build.build_env(str(hdr)) == lib1 and len(calls) == 1
        hdr.write_text(hdr.read_text().replace('MAX_STEPS = 7', 'MAX_STEPS = 9'))
        lib2 = build.build_env(str(hdr))
        assert lib2 != lib1 and len(calls) == 2, 'a touched header does'
        assert EnvPlugin(str(hdr)).MAX_STEPS == 9
        assert build.build_env(str(hdr), force=True) == lib2 and len(calls) == 3
    finally:
        for lib in (lib1, locals().get('lib2')):
            if lib:
                shutil.rmtree(os.path.dirname(lib), ignore_errors=True)
    assert build.ENV_MAX_JOBS == 4
    with pytest.raises(RuntimeError, match='no env header'):
        build.build_env(str(tmp_path / 'missing.hpp'))


# ------------------------------------------------------------------------------------------------ 3. headers that fail
BROKEN = [('O = 5', 'O = 33', r'pgm_user_env::O outside 1 <= O <= 32', '33'),
          ('A = 1,', 'A = 9,', r'pgm_user_env::A above the limit A <= 8', '9'),
          ('K = 2', 'K = 4', r'pgm_user_env::K outside 1 <= K <= 3', '4'),
          ('SD = 2', 'SD = 17', r'pgm_user_env::SD outside 0 <= SD <= 16', '17'),
          ('MAX_STEPS = 40', 'MAX_STEPS = 0', r'pgm_user_env::MAX_STEPS must be positive', '0'),
          ('static void observe', 'static void observe_', r'pgm_user_env::observe is missing', None)]


@pytest.mark.parametrize('old,new,msg,value', BROKEN, ids=[b[1].strip(',') for b in BROKEN])
def test_broken_headers_fail_to_build(tmp_path, old, new, msg, value):
    text = open(pe.header('line')).read()
    assert text.count(old) == 1
    hdr = tmp_path / 'broken.hpp'
    hdr.write_text(text.replace(old, new))
    with pytest.raises(RuntimeError) as e:
        build.build_env(str(hdr))
    err = str(e.value)
    assert msg in err, err[-1500:]
    if value is not None:  # the compiler prints the evaluated comparison beside the message
        assert f"'{value} " in err or f' {value}' in err, err[-1500:]
    assert not os.path.exists(os.path.dirname(build.env_lib_path(str(hdr)))), 'nothing is left behind'
    with pytest.raises(PGMError, match='env plug-in'):
        EnvPlugin(str(hdr))


def test_categorical_header_needs_two_actions(tmp_path):
    text = open(pe.header('chain')).read()
    hdr = tmp_path / 'one_action.hpp'
    hdr.write_text(text.replace('A = 3,', 'A = 1,'))
    with pytest.raises(RuntimeError, match=r'Categorical head: A >= 2 actions'):
        build.build_env(str(hdr))


# ------------------------------------------------------------------------------------------------ 4. host functions
def _grid(env, rng):
    """States just inside and outside each terminal, elapsed 0, 1, limit - 2, limit - 1, actions inside, on and
    beyond the clip; R = 3, two table rows."""
    table = envspec.plugin_reset_table(5, 2, 3, env.RW)
    L = env.MAX_STEPS
    eps = 2.0 ** -40
    if env.DISCRETE:
        acts = [0, 1, 2]
    else:
        vals = [0.0, 0.5, -0.999, 1.0, -1.0, float(np.nextafter(np.float32(1), np.float32(2))), -1.5, 3.0]
        acts = [np.roll(np.resize(vals, env.A), j).astype(np.float32) for j in range(len(vals))]
    states = []
    if env is pe.Line:
        for x in (0.0, 1.5 - eps, 1.5, 1.5 + eps, -1.5 + eps, -1.5 - eps, 1.3, -1.4):
            for v in (0.0, 0.1, -0.1):
                states.append((np.array([x, v]), np.array([3], dtype=np.int32)))
    elif env is pe.Chain:
        for i in range(0, 7):
            states.append((np.zeros(0), np.array([i, 2], dtype=np.int32)))
    elif env is pe.PlugDummy:
        for px in (0.0, 4.9, 5.0 - eps, 5.0, 5.0 + eps, -4.95):
            for vx in (0.0, 0.08, -0.08):
                states.append((np.array([px, 0.01, vx, 0.0, 1.25, 2.5]), np.array([7], dtype=np.int32)))
    elif env is pe.Wide:
        for s0 in (0.0, 0.3, 0.6 - eps, 0.6, 0.5, -0.4):
            sd = rng.uniform(-0.3, 0.3, 16)
            sd[0], sd[1] = s0, 0.0
            states.append((sd, np.array([2, 5, 0, 4], dtype=np.int32)))
    else:
        states.append((np.array([0.25]), np.zeros(0, dtype=np.int32)))
    items = []
    for sd, si in states:
        for el in sorted({0, 1, max(L - 2, 0), L - 1}):
            for a in acts:
                for episode, row in ((0, 0), (2, 1), (7, 0)):
                    si2 = si.copy()
                    if env in (pe.Line, pe.PlugDummy, pe.Wide) and len(si2):
                        si2[0] = el  # the header's own step counter runs with the caller's
                    if env is pe.Chain:
                        si2[1] = el
                    if env is pe.Wide:
                        si2[3] = 2 * el
                    items.append((sd, si2, el, episode, row, a))
    cols = list(zip(*items))
    act = np.array(cols[5], dtype=np.int32) if env.DISCRETE else np.stack(cols[5]).astype(np.float32)
    return (np.stack(cols[0]).reshape(len(items), env.SD), np.stack(cols[1]).reshape(len(items), env.SI),
            np.array(cols[2], dtype=np.int32), np.array(cols[3], dtype=np.int32), np.array(cols[4], dtype=np.int32), act,
            table)


@ENVS
def test_transition_equals_numpy_on_the_grid(plugins, env):
    pl = plugins[env.NAME]
    sd, si, el, ep, row, act, table = _grid(env, np.random.RandomState(0))
    got = pl.transition(sd, si, el, ep, row, act, table)
    want = pe.transition(env, sd, si, el, ep, row, act, table)
    _assert_same(got, want, f'({env.NAME}, {len(el)} grid items)')
    assert got['done'].any() and not got['done'].all()
    forced = el == env.MAX_STEPS - 1
    assert (got['done'][forced] == 1).all() and (got['bad'][forced] == 1).all(), 'the forced limit'
    assert (got['elapsed'][got['done'] == 1] == 0).all() and (got['episode'] == ep + got['done']).all()
    if env not in (pe.NoLimit,):
        assert ((got['done'] == 1) & (got['bad'] == 0)).any(), 'true terminals occur on the grid'
    wrap = (got['done'] == 1) & (ep == 2)  # episode 3 of R = 3: entry 0 again
    s0, i0, o0 = pl.reset(row[wrap], np.zeros(wrap.sum(), dtype=np.int32), table)
    assert wrap.any() and np.array_equal(_bits(got['sd'][wrap]), _bits(s0)) and np.array_equal(got['obs'][wrap], o0)


@ENVS
def test_random_trajectories_equal_numpy(plugins, env):
    """2,000 random 60-step trajectories with resets and wrap-around at R = 3: the compiled header and the numpy
    restatement stay bit-equal, each on its own state."""
    pl, n, rng = plugins[env.NAME], 2000, np.random.RandomState(1)
    table = envspec.plugin_reset_table(3, 8, 3, env.RW)
    row = (np.arange(n) % 8).astype(np.int32)
    zero = np.zeros(n, dtype=np.int32)
    sd, si, obs = pl.reset(row, zero, table)
    _assert_same({'sd': sd, 'si': si, 'obs': obs}, dict(zip(('sd', 'si', 'obs'), pe.reset(env, row, zero, table))),
                 'after reset')
    a = {'sd': sd, 'si': si, 'elapsed': zero.copy(), 'episode': zero.copy()}
    b = {k: v.copy() for k, v in a.items()}
    ends = bads = 0
    for t in range(60):
        act = (rng.randint(0, env.A, n).astype(np.int32) if env.DISCRETE
               else (rng.randn(n, env.A) * 1.2).astype(np.float32))
        a = pl.transition(a['sd'], a['si'], a['elapsed'], a['episode'], row, act, table)
        b = pe.transition(env, b['sd'], b['si'], b['elapsed'], b['episode'], row, act, table)
        _assert_same(a, b, f'({env.NAME}, step {t})')
        ends += int(a['done'].sum())
        bads += int(a['bad'].sum())
    assert ends > n // 4 and int(a['episode'].max()) >= 3, 'episodes end and the table wraps (episode 3 of R = 3)'
    if env.MAX_STEPS < 60:
        assert bads > 0


def test_forced_limit_ends_a_header_that_never_does(plugins):
    pl = plugins['nolimit']
    table = envspec.plugin_reset_table(0, 1, 2, 1)
    st = dict(zip(('sd', 'si'), pl.reset([0], [0], table)[:2]), elapsed=[0], episode=[0])
    flags = []
    for t in range(15):
        st = pl.transition(st['sd'], st['si'], st['elapsed'], st['episode'], [0], np.zeros((1, 1), np.float32), table)
        flags.append((int(st['done'][0]), int(st['bad'][0]), int(st['elapsed'][0]), int(st['episode'][0])))
    assert flags[6] == (1, 1, 0, 1) and flags[13] == (1, 1, 0, 2)
    assert [f[0] for f in flags] == [int(t % 7 == 6) for t in range(15)]
    assert st['sd'][0, 0] == table[0, 0, 0] + 1.0  # episode 2 of R = 2 starts at entry 0 again, one step in


# ------------------------------------------------------------------------------------------------ 5. plugdummy = dummy
def test_plugdummy_equals_pgm_dummy_transition(plugins):
    """plugdummy.hpp's host function equals pgm_dummy_transition (MO-Dummy-v0: 500 steps, bound 5, the limit reported
    as a time-limit end) on a grid of the kind tests/test_dummy_device.py uses, with both reset tables built from one
    uniform array."""
    pl = plugins['plugdummy']
    sd, si, el, ep, row, act, utable = _grid(pe.PlugDummy, np.random.RandomState(0))
    dtable = 2.0 * utable - 1.0
    got = pl.transition(sd, si, el, ep, row, act, utable)
    s2, so, eo, obj, rew, done, bad = dr.transition(2, sd, el, ep, row, act, dtable, 500, 5.0, True)
    L = _lib.lib()
    n = len(el)
    spec = _lib.DummySpec(500, 1, 5.0, C.c_void_p(dtable.ctypes.data), 3, 2)
    out = [np.zeros((n, 6)), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 2)), np.zeros(n),
           np.zeros(n, np.int32), np.zeros(n, np.int32)]
    ptr = lambda x: C.c_void_p(np.ascontiguousarray(x).ctypes.data)  # noqa: E731
    sdc, elc, epc, rowc, actc = (np.ascontiguousarray(x) for x in (sd, el, ep, row, act))
    _lib.check(L.pgm_dummy_transition(C.byref(spec), 2, n, ptr(sdc), ptr(elc), ptr(epc), ptr(rowc), ptr(actc),
                                      *(ptr(o) for o in out)), 'pgm_dummy_transition')
    for name, mine, lib_out, ref in (('state', got['sd'], out[0], s2), ('step', got['elapsed'], out[1], so),
                                     ('episode', got['episode'], out[2], eo), ('obj', got['obj'], out[3], obj),
                                     ('reward', got['reward'], out[4], rew), ('done', got['done'], out[5], done),
                                     ('bad', got['bad'], out[6], bad)):
        assert np.array_equal(_bits(mine), _bits(lib_out)), f'{name}: plug-in vs pgm_dummy_transition'
        assert np.array_equal(_bits(mine), _bits(np.asarray(ref).astype(mine.dtype))), f'{name}: vs dummy_ref'
    assert np.array_equal(got['si'][:, 0], got['elapsed']) and np.array_equal(_bits(got['obs']), _bits(got['sd']))
    assert got['done'].any() and ((got['done'] == 1) & (got['bad'] == 0)).any()


# ------------------------------------------------------------------------------------------------ 6. sanitizers
@pytest.mark.parametrize('env', [pe.Wide, pe.Chain], ids=lambda e: e.NAME)
def test_header_under_the_host_sanitizers(tmp_path, plugins, env):
    """tests/cpp/envplug_transition_check.cpp (its own main; the header and pgm_envplug.hpp alone, no HIP) built with
    the address and undefined-behaviour sanitizers runs clean over the grid, and its lines are the host function's."""
    exe = tmp_path / 'envplug_check'
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'include'), '-include', pe.header(env.NAME),
                    os.path.join(ROOT, 'tests', 'cpp', 'envplug_transition_check.cpp'), '-o', str(exe)], check=True)
    sd, si, el, ep, row, act, table = _grid(env, np.random.RandomState(0))
    n = len(el)
    hx = lambda v: ' '.join(float(x).hex() for x in np.asarray(v, dtype=np.float64).reshape(-1))  # noqa: E731
    ix = lambda v: ' '.join(str(int(x)) for x in np.asarray(v).reshape(-1))  # noqa: E731
    text = [f'{table.shape[1]} {table.shape[0]} {n}\n{hx(table)}\n']
    for i in range(n):
        a = ix(act[i]) if env.DISCRETE else hx(act[i])
        text.append(f'{hx(sd[i])} {ix(si[i])} {el[i]} {ep[i]} {row[i]} {a}\n')
    r = subprocess.run([str(exe)], input=''.join(text), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert f'{n} cases' in r.stderr
    want = plugins[env.NAME].transition(sd, si, el, ep, row, act, table)
    rows = r.stdout.splitlines()
    assert len(rows) == n
    flt = np.array([[float.fromhex(x) for x in ln.split('|')[0].split()] for ln in rows])
    ints = np.array([[int(x) for x in ln.split('|')[1].split()] for ln in rows])
    wf = np.concatenate([want['sd'], want['obs'], want['obj'], want['reward'][:, None]], -1)
    wi = np.concatenate([want['si'], np.stack([want['elapsed'], want['episode'], want['done'], want['bad']], -1)], -1)
    assert np.array_equal(flt.view(np.int64), wf.view(np.int64)) and np.array_equal(ints, wi)


# ------------------------------------------------------------------------------------------------ 7. argument refusals
def _launch_args(pl, **over):
    """Both launch entry points' arguments with non-NULL dummies (never dereferenced: every call here is refused)."""
    x = C.c_void_p(0x1000)
    d = Dims(2, 3, 8, pl.O, pl.A, pl.K, 64, 0)
    for k, v in over.pop('dims', {}).items():
        setattr(d, k, v)
    st = EnvState(x, x, x, x, x, x)
    ns = NormState(x, x, x, x, x, x, x, x, x, 0.99, 10.0, 10.0, 1e-8, 1, 1)
    rb = RolloutBuf(x, x, x, x, x, x, x, x, x)
    a = dict(d=C.byref(d), params=x, sd=x, si=x, episode=x, table=x, R=3, reset_count=8, st=C.byref(st),
             ns=C.byref(ns), rb=C.byref(rb), ob_mean=x, ob_var=x, eval_num=2, objs=x)
    a.update(over)
    keep = (d, st, ns, rb)
    return a, keep


def _rollout(pl, **over):
    a, keep = _launch_args(pl, **over)
    rc = pl.h.pgm_envplug_rollout(a['d'], a['params'], a['sd'], a['si'], a['episode'], a['table'], a['R'],
                                  a['reset_count'], a['st'], a['ns'], a['rb'], None, 0, 0, None)
    return rc, pl.last_error()


def _eval(pl, **over):
    a, keep = _launch_args(pl, **over)
    rc = pl.h.pgm_envplug_eval(a['d'], a['params'], a['table'], a['R'], a['reset_count'], a['ob_mean'], a['ob_var'],
                               a['eval_num'], 1, 1, 0.99, a['objs'], None)
    return rc, pl.last_error()


@pytest.mark.parametrize('name', ['line', 'chain'])
def test_launch_refusals_in_the_documented_order(plugins, name):
    """NULL pointers; check_dims (H, N); d->O/A/K against the compiled constants; d->LN; T / eval_num; R and
    reset_count -- each refusal names its entry point, and an earlier item wins over every later one."""
    pl = plugins[name]
    E = _lib
    later = dict(R=0, reset_count=0)  # items 5-6 broken as well: the earlier item must still be the one reported
    for call, what, extra in ((_rollout, 'pgm_envplug_rollout', {}), (_eval, 'pgm_envplug_eval', dict(eval_num=9))):
        bad_all = dict(later, **extra)
        rc, msg = call(pl, params=None, dims=dict(H=32, O=pl.O + 1, LN=1, T=0), **bad_all)
        assert rc == E.PGM_E_INVALID_ARG and msg.startswith(what) and 'null pointer' in msg
        rc, msg = call(pl, dims=dict(H=32, O=pl.O + 1, LN=1, T=0), **bad_all)
        assert rc == E.PGM_E_UNSUPPORTED and msg.startswith(what) and 'hidden size 32' in msg
        rc, msg = call(pl, dims=dict(O=pl.O + 1, LN=1, T=0), **bad_all)
        assert rc == E.PGM_E_UNSUPPORTED and msg.startswith(what) and 'compiled for' in msg and f'O={pl.O + 1}' in msg
        for k in ('A', 'K'):
            rc, msg = call(pl, dims={k: getattr(pl, k) + 1})
            assert rc == E.PGM_E_UNSUPPORTED and 'compiled for' in msg
        rc, msg = call(pl, dims=dict(LN=1, T=0), **bad_all)
        assert rc == E.PGM_E_UNSUPPORTED and msg.startswith(what) and 'LN = 1' in msg and 'plain towers' in msg
    rc, msg = _rollout(pl, dims=dict(N=9))
    assert rc == _lib.PGM_E_UNSUPPORTED and 'N=9' in msg
    rc, msg = _rollout(pl, dims=dict(T=0), **later)
    assert rc == E.PGM_E_SHAPE and msg == 'pgm_envplug_rollout: T must be positive'
    for en in (0, 9):
        rc, msg = _eval(pl, eval_num=en, **later)
        assert rc == E.PGM_E_INVALID_ARG and msg.startswith('pgm_envplug_eval') and f'eval_num={en}' in msg
    for call, what, need in ((_rollout, 'pgm_envplug_rollout', 3), (_eval, 'pgm_envplug_eval', 2)):
        rc, msg = call(pl, R=0, reset_count=0)
        assert rc == E.PGM_E_INVALID_ARG and msg.startswith(what) and 'R = 0' in msg
        rc, msg = call(pl, reset_count=need - 1)
        assert rc == E.PGM_E_INVALID_ARG and msg.startswith(what) and f'the call reads {need}' in msg
    for k in ('episode', 'st', 'ns', 'rb', 'table') + (('sd',) if pl.SD else ()) + (('si',) if pl.SI else ()):
        rc, msg = _rollout(pl, **{k: None})
        assert rc == E.PGM_E_INVALID_ARG and 'null pointer' in msg, k
    for k in ('objs', 'ob_mean', 'table'):
        rc, msg = _eval(pl, **{k: None})
        assert rc == E.PGM_E_INVALID_ARG and 'null pointer' in msg, k


def test_host_function_refusals(plugins):
    pl = plugins['chain']
    table = envspec.plugin_reset_table(0, 2, 3, 1)
    si = np.array([[3, 0]], dtype=np.int32)
    for kw, msg in ((dict(row=[2]), 'row 2'), (dict(episode=[-1]), 'episode -1'), (dict(action=[3]), 'action index 3'),
                    (dict(elapsed=[-1]), 'elapsed -1')):
        a = dict(elapsed=[0], episode=[0], row=[0], action=[1])
        a.update(kw)
        with pytest.raises(PGMError, match=msg):
            pl.transition(np.zeros((1, 0)), si, a['elapsed'], a['episode'], a['row'], a['action'], table)
    with pytest.raises(PGMError, match='row 5'):
        pl.reset([5], [0], table)
    with pytest.raises(PGMError, match=r'\[rows\]\[R\]\[1\]'):
        pl.reset([0], [0], np.zeros((2, 3, 2)))


# ------------------------------------------------------------------------------------------------ 8. Python layers
def test_plugin_reset_table_known_answers():
    t = envspec.plugin_reset_table(7, 3, 4, 2)
    assert t.shape == (3, 4, 2) and t.dtype == np.float64 and (t >= 0).all() and (t < 1).all()
    for i in range(3):  # row i: the splitmix64 uniforms of env seed 7 + i under the plug-in stream constant
        assert np.array_equal(t[i].reshape(-1), envspec._uniforms(envspec.PLUGIN_RESET_STREAM + 7 + i, 8))
    assert np.array_equal(envspec.plugin_reset_table(8, 2, 4, 2), t[1:])
    assert np.array_equal(envspec.plugin_reset_table(7, 3, 2, 2)[:, :, :], t[:, :2])  # a prefix of the same stream
    # dummy_reset_table's construction without the 2 u - 1, under another stream constant
    assert envspec.PLUGIN_RESET_STREAM not in (envspec.DUMMY_RESET_STREAM, 0x5EED0000)
    d = envspec.dummy_reset_table(7, 3, 4)
    u = np.stack([envspec._uniforms(envspec.DUMMY_RESET_STREAM + 7 + i, 8).reshape(4, 2) for i in range(3)])
    assert np.array_equal(d, 2.0 * u - 1.0)
    # splitmix64 of state 0: the published first output 0xE220A8397B1DCDAF
    assert envspec._uniforms(0, 1)[0] == (0xE220A8397B1DCDAF >> 11) / float(1 << 53)
    assert envspec.plugin_reset_table(0, 1, 3, 0).shape == (1, 3, 0)
    with pytest.raises(ValueError, match='R = 0'):
        envspec.plugin_reset_table(0, 1, 0, 2)


@pytest.mark.parametrize('env', ALL, ids=lambda e: e.NAME)
def test_plugin_host_vec_env_protocol(plugins, env):
    """Shapes and dtypes of the HostVecEnv protocol, and the compiled header behind it equals the numpy restatement
    behind the same protocol over a few steps (training and evaluation, an ended episode standing still)."""
    P, N, E = 2, 3, 4
    he = PluginHostVecEnv(plugins[env.NAME], P, N, seed=2, R=3)
    ne = pe.NumpyPluginHostVecEnv(env, P, N, seed=2, R=3)
    assert he.dims() == (env.O, env.A, env.K) and he.discrete is env.DISCRETE and he.capacity == P and he.N == N
    o1, o2 = he.reset(), ne.reset()
    assert o1.shape == (P, N, env.O) and o1.dtype == np.float64 and np.array_equal(o1, o2)
    rng = np.random.RandomState(0)
    for t in range(env.MAX_STEPS + 3 if env.MAX_STEPS < 50 else 12):
        act = rng.randint(0, env.A, (P, N)).astype(np.int32) if env.DISCRETE else rng.randn(P, N, env.A).astype(np.float32)
        a, b = he.step(act), ne.step(act)
        for x, y, shape, dt in zip(a, b, ((P, N, env.O), (P, N), (P, N), (P, N), (P, N, env.K)),
                                   (np.float64, np.float64, bool, bool, np.float64)):
            assert x.shape == shape and x.dtype == dt and np.array_equal(x, y)
    if env.MAX_STEPS < 50:
        assert a[2].shape == (P, N) and he._st['episode'].max() >= 1
    o1, o2 = he.eval_reset(E), ne.eval_reset(E)
    assert o1.shape == (P, E, env.O) and np.array_equal(o1, o2)
    ended = np.zeros((P, E), dtype=bool)
    for t in range(min(env.MAX_STEPS, 45)):
        act = rng.randint(0, env.A, (P, E)).astype(np.int32) if env.DISCRETE else rng.randn(P, E, env.A).astype(np.float32)
        (ob, oj, dn), (ob2, oj2, dn2) = he.eval_step(act), ne.eval_step(act)
        assert ob.shape == (P, E, env.O) and oj.shape == (P, E, env.K) and dn.shape == (P, E) and dn.dtype == bool
        assert np.array_equal(ob, ob2) and np.array_equal(oj, oj2) and np.array_equal(dn, dn2)
        assert (oj[ended] == 0).all() and (dn | ~ended).all(), 'an ended episode adds nothing and stays ended'
        ended = dn
    if env.MAX_STEPS <= 45:
        assert ended.all(), 'every evaluation episode ends within MAX_STEPS steps'
    he.set_active(1)
    assert he.reset().shape == (1, N, env.O)
    with pytest.raises(ValueError):
        he.set_active(P + 1)


def test_registration(plugins):
    pl = plugins['line']
    assert pl.register('PlugReg-Line-v0') == 'PlugReg-Line-v0'
    sp = envspec.make_spec('PlugReg-Line-v0')
    assert (sp['obs_dim'], sp['act_dim'], sp['obj_num']) == (5, 1, 2) and sp['user'] and not sp.get('discrete')
    plugins['chain'].register('PlugReg-Chain-v0')
    assert envspec.make_spec('PlugReg-Chain-v0')['discrete'] is True
    pl.register('PlugReg-Line-v0')  # the same dims again: accepted
    for known in ('MO-Hopper-v2', 'MO-DeepSeaTreasure-v0', 'MO-Dummy-v0'):
        with pytest.raises(ValueError, match="one of envspec's own envs"):
            pl.register(known)
    with pytest.raises(ValueError, match='already registered'):
        plugins['wide'].register('PlugReg-Line-v0')
    assert envplug.as_plugin(pl) is pl and envplug.as_plugin(pl.header).dims() == pl.dims()


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_taskbatch_refusals(plugins):
    from pgmorl_amd.runtime import TaskBatch
    pl = plugins['line']
    he = lambda: PluginHostVecEnv(pl, 2, 4)  # noqa: E731
    kw = dict(device='cpu', env_plugin=pl)
    with pytest.raises(PGMError, match='host_env=... and device_env=True are other places'):
        TaskBatch('PlugTB-v0', 2, host_env=he(), **kw)
    with pytest.raises(PGMError, match='host_env=... and device_env=True are other places'):
        TaskBatch('PlugTB-v0', 2, device_env=True, **kw)
    with pytest.raises(PGMError, match='layernorm=True with env_plugin'):
        TaskBatch('PlugTB-v0', 2, layernorm=True, **kw)
    with pytest.raises(PGMError, match='eval_num=9 with env_plugin'):
        TaskBatch('PlugTB-v0', 2, eval_num=9, **kw)
    with pytest.raises(PGMError, match='num_processes=9 with env_plugin'):
        TaskBatch('PlugTB-v0', 2, num_processes=9, **kw)
    assert 'PlugTB-v0' not in envspec.user_env_names(), 'a refused batch registers nothing'
    with pytest.raises(PGMError, match="one of envspec's own envs"):
        TaskBatch('MO-Hopper-v2', 2, **kw)
    with pytest.raises(PGMError, match='does not build|no env header'):
        TaskBatch('PlugTB-v0', 2, device='cpu', env_plugin=os.path.join(ROOT, 'tests', 'envplug', 'absent.hpp'))
    # every existing refusal keeps its text: a registered third-party env with neither host_env nor env_plugin
    pl.register('PlugTB-registered-v0')
    with pytest.raises(PGMError, match='host-stepped only: TaskBatch needs host_env'):
        TaskBatch('PlugTB-registered-v0', 2, device='cpu')


def test_cli_refuses_before_the_save_dir(tmp_path):
    from pgmorl_amd.run import main
    line = pe.header('line')
    broken = tmp_path / 'broken.hpp'
    broken.write_text(open(line).read().replace('K = 2', 'K = 4'))
    prev = torch.get_default_dtype()
    try:
        cases = ((['--env-plugin', line, '--env-name', 'MO-Hopper-v2'], "one of envspec's own envs"),
                 (['--env-plugin', line, '--env-name', 'PlugCli-v0', '--layernorm'], 'plain towers'),
                 (['--env-plugin', line, '--env-name', 'PlugCli-v0', '--device-env'], '--device-env with --env-plugin'),
                 (['--env-plugin', line, '--env-name', 'PlugCli-v0', '--host-env', 'synth'], '--host-env synth with'),
                 (['--env-plugin', line, '--env-name', 'PlugCli-v0', '--host-env', 'tests.anydims_envs:make_env'],
                  'with --env-plugin'),
                 (['--env-plugin', str(broken), '--env-name', 'PlugCli-v0'], 'K outside 1 <= K <= 3'),
                 (['--env-plugin', str(tmp_path / 'absent.hpp'), '--env-name', 'PlugCli-v0'], 'no env header'),
                 (['--env-name', 'PlugCli-v0', '--host-env', 'plugin'], 'pass --env-plugin'))
        for i, (extra, msg) in enumerate(cases):
            save = tmp_path / f'run{i}'
            with pytest.raises((PGMError, ValueError), match=msg):
                main(['--obj-num', '2', '--save-dir', str(save)] + extra)
            assert not save.exists(), extra
    finally:
        torch.set_default_dtype(prev)


# ------------------------------------------------------------------------------------------------ 10. libpgm.so untouched
def test_libpgm_is_untouched(plugins):
    """The capability lives in a library of its own: libpgm.so's feature mask, version pair and struct sizes are as
    before, it exports no plug-in symbol, and a plug-in library exports none of libpgm.so's entry points."""
    L = _lib.lib()
    assert L.pgm_abi_feature_mask() == 15 and L.pgm_abi_features() == 7
    assert L.pgm_abi_version() == 5 and L.pgm_abi_minor() == 1
    assert C.sizeof(Dims) == 32 and C.sizeof(RolloutBuf) == 72 and C.sizeof(PPOHParams) == 48
    assert C.sizeof(EnvState) == 48 and C.sizeof(NormState) == 112
    for name in envplug.SIGS:
        assert not hasattr(L, name), name
    h = plugins['line'].h
    for name in ('pgm_abi_version', 'pgm_rollout', 'pgm_ppo_update_any', 'pgm_last_error'):
        assert not hasattr(h, name), name
    assert 'pgm_envplug.hip' not in build.SOURCES and 'pgm_envplug.hpp' not in build.HEADERS


# ------------------------------------------------------------------------------------------------ the recorded seeds
@pytest.mark.parametrize('env', [pe.Line, pe.Chain], ids=lambda e: e.NAME)
def test_mopg_seed_is_the_first_that_passes(env):
    """The seed recorded for the MOPG case against the reference (tests/envplug_ref.py) is the first from
    0 at which the reference alone meets every condition; the margins are those recorded."""
    from . import envplug_ref as er
    seed = er.MOPG_SEEDS[env.NAME]
    for earlier in range(seed):
        assert er.mopg_case(env, earlier)[5], 'an earlier seed meets the conditions'
    name, args, pols, w, refs, bad, m = er.mopg_case(env, seed)
    assert not bad, bad
    assert all(m[k] >= er.MARGIN for k in (('uniform', 'logit') if env.DISCRETE else ('env',))), m


def test_chain_eval_seeds():
    from . import envplug_ref as er
    for E in (1, 8):
        for use_ob in (0, 1):
            seed, (pols, rms, want, bad, m) = er.chain_eval_seed(E, use_ob)
            assert seed == 0 and not bad and m['logit'] >= er.MARGIN, (E, use_ob, seed, bad, m)
