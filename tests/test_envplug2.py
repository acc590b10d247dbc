"""Contract 2 of the device env plug-ins (include/pgm_envplug.h: runtime parameters, per-step uniforms) on the CPU: the
five headers of tests/envplug2 build and the ones that must not fail with a message naming the member; info_ex and
params; the env-noise stream against oracle/streams.py; the host functions against the numpy restatements of
tests/envplug2_envs.py bit for bit; line2.hpp against line.hpp; the refusals of the entry points in their documented
order, of TaskBatch and of the CLI; the headers under the host sanitizers in a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import streams
from pgmorl_amd import _lib, build, envplug, envspec
from pgmorl_amd._lib import PGMError
from pgmorl_amd.envplug import EnvPlugin
from pgmorl_amd.hostenv import PluginHostVecEnv

from . import envplug2_envs as p2
from . import envplug_envs as pe
from .test_envplug import _assert_same, _bits, _launch_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = (p2.Slip, p2.Gather, p2.ParMax, p2.NoiseMax, p2.Line2)
ENVS = pytest.mark.parametrize('env', ALL, ids=lambda e: e.NAME)
# two parameter sets per header: the defaults and another one (None where the header has no parameter)
OTHER = {'slip': {'slip': 0.6, 'wind': -0.125}, 'gather': {'p_attack': 0.5},
         'parmax': dict({f'p{i}': 0.0625 * (i - 7) for i in range(16)}, p0=1.0, p1=0.5), 'noisemax': None,
         'line2': None}


@pytest.fixture(scope='module')
def plugins():
    hs = [p2.header(e.NAME) for e in ALL] + [pe.header('line')]
    build.build_envs(hs)
    d = {e.NAME: EnvPlugin(p2.header(e.NAME)) for e in ALL}
    d['line'] = EnvPlugin(pe.header('line'))
    return d


# ------------------------------------------------------------------------------------------------ 1. build, info
@ENVS
def test_info_ex_and_params(plugins, env):
    pl = plugins[env.NAME]
    assert pl.info == p2.info(env) and (pl.CONTRACT, pl.NP, pl.NW) == (2, env.NP, env.NW)
    assert tuple(pl.par_names) == env.PAR_NAMES and np.array_equal(pl.par_default, np.array(env.PAR_DEFAULT))
    assert pl.h.pgm_envplug_abi() == envplug.PGM_ENVPLUG_ABI == 1 and pl.h.pgm_envplug_contract() == 2
    out = (C.c_int32 * 11)()
    assert pl.h.pgm_envplug_info_ex(out) == 0 and list(out)[8:] == [2, env.NP, env.NW]
    assert pl.h.pgm_envplug_info_ex(None) == _lib.PGM_E_INVALID_ARG and 'pgm_envplug_info_ex' in pl.last_error()
    names = ','.join(env.PAR_NAMES)
    buf = C.create_string_buffer(len(names) + 1)
    assert pl.h.pgm_envplug_params(buf, len(buf), None) == 0 and buf.value.decode() == names
    if names:
        assert pl.h.pgm_envplug_params(buf, len(names), None) == _lib.PGM_E_INVALID_ARG
        assert pl.last_error().startswith('pgm_envplug_params')


def test_contract_1_header_reports_1_0_0(plugins):
    pl = plugins['line']
    assert (pl.CONTRACT, pl.NP, pl.NW) == (1, 0, 0) and pl.par_names == [] and pl.par_default.size == 0
    assert pl.h.pgm_envplug_contract() == 1
    out = (C.c_int32 * 11)()
    assert pl.h.pgm_envplug_info_ex(out) == 0 and list(out) == list(pe.info(pe.Line).values()) + [1, 0, 0]


BROKEN = [('slip', 'NP = 2, NW = 1;', 'NW = 1;', 'pgm_user_env::NP is missing'),
          ('slip', 'NP = 2, NW = 1;', 'NP = 2;', 'pgm_user_env::NW is missing'),
          ('parmax', 'NP = 16,', 'NP = 17,', 'pgm_user_env::NP outside 0 <= NP <= 16'),
          ('noisemax', 'NW = 4;', 'NW = 5;', 'pgm_user_env::NW outside 0 <= NW <= 4'),
          ('gather', 'static constexpr const char* PAR_NAMES = "p_attack";', '', 'pgm_user_env::PAR_NAMES is missing'),
          ('gather', 'static constexpr double PAR_DEFAULT[NP] = {0.1};', '', 'pgm_user_env::PAR_DEFAULT is missing'),
          ('slip', '"slip,wind"', '"slip"', 'pgm_user_env::PAR_NAMES must hold NP comma-separated identifiers'),
          ('slip', '"slip,wind"', '"slip,wind,gust"', 'pgm_user_env::PAR_NAMES must hold NP comma-separated'),
          ('slip', '"slip,wind"', '"slip,2wind"', 'pgm_user_env::PAR_NAMES must hold NP comma-separated'),
          ('line2', 'CONTRACT = 2,', 'CONTRACT = 3,', 'pgm_user_env::CONTRACT must be 1 or 2')]


@pytest.mark.parametrize('name,old,new,msg', BROKEN, ids=[f'{b[0]}-{i}' for i, b in enumerate(BROKEN)])
def test_broken_contract_2_headers_fail_to_build(tmp_path, name, old, new, msg):
    text = open(p2.header(name)).read()
    assert text.count(old) == 1
    if 'NP = 2, NW = 1;' == old and new == 'NW = 1;':  # (the array bound of PAR_DEFAULT must still compile)
        text = text.replace('PAR_DEFAULT[NP]', 'PAR_DEFAULT[2]')
    hdr = tmp_path / 'broken2.hpp'
    hdr.write_text(text.replace(old, new))
    with pytest.raises(RuntimeError) as e:
        build.build_env(str(hdr))
    assert msg in str(e.value), str(e.value)[-2000:]
    assert not os.path.exists(os.path.dirname(build.env_lib_path(str(hdr)))), 'nothing is left behind'


# ------------------------------------------------------------------------------------------------ 2. the stream
def test_uniforms_are_the_restated_stream(plugins):
    """pgm_envplug_uniforms = (hash_at(seed, i) >> 11) 2^-53 at the first, a middle and the last index of a block, at
    a 64-bit seed and start; in [0, 1); and the env stream of a rollout seed is not its action stream."""
    pl = plugins['slip']
    for seed, start, n in ((0, 0, 257), (7, 1000, 64), ((1 << 63) + 5, (1 << 40) + 3, 33)):
        got = pl.uniforms(seed, start, n)
        want = p2.u53(seed, start, n)
        for i in (0, n // 2, n - 1):
            assert got[i] == want[i] == float(int(streams.hash_at(seed, start + i)) >> 11) / float(1 << 53), (seed, i)
        assert np.array_equal(got, want) and (got >= 0).all() and (got < 1).all()
    assert np.array_equal(plugins['line'].uniforms(7, 1000, 64), pl.uniforms(7, 1000, 64)), 'one stream, any header'
    assert pl.uniforms(3, 0, 0).shape == (0,)
    assert pl.h.pgm_envplug_uniforms(0, 0, 4, None) == _lib.PGM_E_INVALID_ARG
    for seed in (0, 1, 12345):
        es = envplug.env_seed(seed)
        assert es == p2.env_seed(seed) == seed ^ envplug.ENV_SEED_XOR and es != seed
        idx = np.arange(64, dtype=np.uint64)
        assert not (streams.hash_at(es, idx) == streams.hash_at(seed, idx)).any(), 'another stream than the actions\''
    assert envplug.env_seed(-1) == (2 ** 64 - 1) ^ envplug.ENV_SEED_XOR


# ------------------------------------------------------------------------------------------------ 3. host functions
def _grid(env, rng):
    """tests/test_envplug.py's grid with the uniforms: states just inside and outside each terminal, elapsed 0, 1,
    limit - 2, limit - 1, actions inside, on and beyond the clip, w on both sides of every threshold; R = 3."""
    table = envspec.plugin_reset_table(5, 2, 3, env.RW)
    L = env.MAX_STEPS
    eps = 2.0 ** -40
    acts = list(range(env.A)) if env.DISCRETE else [np.array([v], dtype=np.float32) for v in
                                                     (0.0, 0.5, -0.999, 1.0, -1.0, 1.0000001, -1.5, 3.0)]
    ws = {0: [np.zeros(0)],
          1: [np.array([v]) for v in (0.0, 0.2 - eps, 0.2, 0.6 - eps, 0.6, 1.0 - 2.0 ** -53)],
          3: [np.array(v) for v in ((0.05, 0.5, 0.5), (0.1, 0.95, 0.1), (0.3, 0.1, 0.85), (0.5, 0.9, 0.8),
                                    (0.999, 0.0, 0.0))],
          4: [np.array(v) for v in ((0.0, 0.0, 0.0, 0.0), (0.5, 0.25, 0.75, 0.125), (0.999, 0.999, 0.0, 0.999))]}[env.NW]
    states = []
    if env is p2.Slip:
        states = [(np.array([x, 0.01]), np.zeros(0, np.int32))
                  for x in (0.0, 1.0 - eps, 1.0, 0.95, -0.99, -1.0 + eps, 0.7, -0.75)]
    elif env is p2.Gather:
        states = [(np.zeros(0), np.array([x, y, c], dtype=np.int32)) for x in range(3) for y in range(3)
                  for c in (0, 1, 2, 3)]
    elif env is p2.ParMax:
        states = [(np.array([x]), np.zeros(0, np.int32)) for x in (0.0, 1.9, 2.0, -2.0 + eps, 2.2, -1.5, 0.3)]
    elif env is p2.NoiseMax:
        states = [(np.array([x]), np.zeros(0, np.int32)) for x in (0.0, 0.6 - eps, 0.6, 0.45, -0.5, -0.6 + eps)]
    else:
        states = [(np.array([x, v]), np.array([3], dtype=np.int32))
                  for x in (0.0, 1.5 - eps, 1.5, 1.5 + eps, -1.5 - eps, 1.3) for v in (0.0, 0.1, -0.1)]
    items = []
    for sd, si in states:
        for el in sorted({0, 1, max(L - 2, 0), L - 1}):
            for a in acts:
                for w in ws:
                    for episode, row in ((0, 0), (2, 1)):
                        si2 = si.copy()
                        if env is p2.Line2:
                            si2[0] = el
                        items.append((sd, si2, el, episode, row, a, w))
    cols = list(zip(*items))
    n = len(items)
    act = np.array(cols[5], dtype=np.int32) if env.DISCRETE else np.stack(cols[5]).astype(np.float32)
    return (np.stack(cols[0]).reshape(n, env.SD), np.stack(cols[1]).reshape(n, env.SI),
            np.array(cols[2], dtype=np.int32), np.array(cols[3], dtype=np.int32), np.array(cols[4], dtype=np.int32), act,
            np.stack(cols[6]).reshape(n, env.NW), table)


def _par_sets(env):
    return [p2.par_vector(env)] + ([p2.par_vector(env, OTHER[env.NAME])] if OTHER[env.NAME] else [])


@ENVS
def test_host_functions_equal_numpy_on_the_grid(plugins, env):
    pl = plugins[env.NAME]
    sd, si, el, ep, row, act, w, table = _grid(env, np.random.RandomState(0))
    outs = []
    for par in _par_sets(env):
        got = pl.transition(sd, si, el, ep, row, act, table, par=par, w=w)
        want = p2.transition(env, sd, si, el, ep, row, act, table, par, w)
        _assert_same(got, want, f'({env.NAME}, {len(el)} grid items, par {par})')
        assert got['done'].any() and not got['done'].all()
        forced = el == env.MAX_STEPS - 1
        assert (got['done'][forced] == 1).all() and (got['bad'][forced] == 1).all(), 'the forced limit'
        assert (got['elapsed'][got['done'] == 1] == 0).all() and (got['episode'] == ep + got['done']).all()
        assert ((got['done'] == 1) & (got['bad'] == 0)).any(), 'true terminals occur on the grid'
        wrap = (got['done'] == 1) & (ep == 2)  # the auto-reset: episode 3 of R = 3 is entry 0 again
        s0, i0, o0 = pl.reset(row[wrap], np.zeros(wrap.sum(), dtype=np.int32), table, par=par)
        r0 = p2.reset(env, row[wrap], np.zeros(wrap.sum(), dtype=np.int32), table, par)
        assert wrap.any() and np.array_equal(_bits(got['sd'][wrap]), _bits(s0)) and np.array_equal(got['obs'][wrap], o0)
        _assert_same({'sd': s0, 'si': i0, 'obs': o0}, dict(zip(('sd', 'si', 'obs'), r0)), 'reset_ex')
        outs.append(got)
    if len(outs) == 2:
        assert not np.array_equal(outs[0]['obj'], outs[1]['obj']), 'the parameters enter the step'
    if env.NW:  # the uniforms enter the step: the same items under other words
        other = pl.transition(sd, si, el, ep, row, act, table, par=_par_sets(env)[0], w=(w + 0.5) % 1.0)
        assert any(not np.array_equal(other[k], outs[0][k]) for k in ('obj', 'sd', 'si', 'done'))
    assert np.array_equal(pl.transition(sd, si, el, ep, row, act, table, w=w)['obj'], outs[0]['obj']), 'par=None: defaults'


def test_every_parameter_of_parmax_enters_an_objective(plugins):
    pl, env = plugins['parmax'], p2.ParMax
    sd, si, el, ep, row, act, w, table = _grid(env, None)
    base = pl.transition(sd, si, el, ep, row, act, table)['obj']
    for i in range(16):
        par = p2.par_vector(env)
        par[i] += 0.5
        assert not np.array_equal(pl.transition(sd, si, el, ep, row, act, table, par=par)['obj'], base), f'p{i}'


def test_line2_is_line(plugins):
    """The contract-2 restatement of line.hpp equals line.hpp bit for bit: transition_ex vs transition, reset_ex vs
    reset; and the contract-1 library takes the _ex calls with NULL env_par / w."""
    a, b = plugins['line2'], plugins['line']
    sd, si, el, ep, row, act, w, table = _grid(p2.Line2, None)
    _assert_same(a.transition(sd, si, el, ep, row, act, table), b.transition(sd, si, el, ep, row, act, table), 'line2')
    for x, y in zip(a.reset(row, ep, table), b.reset(row, ep, table)):
        assert np.array_equal(_bits(x), _bits(y))
    want = b.transition(sd, si, el, ep, row, act, table)
    n = len(el)
    o = {k: np.zeros_like(v) for k, v in want.items()}
    ptr = lambda x: C.c_void_p(np.ascontiguousarray(x).ctypes.data)  # noqa: E731
    keep = [np.ascontiguousarray(x) for x in (sd, si, el, ep, row, act, table)]
    rc = b.h.pgm_envplug_transition_ex(n, *(ptr(x) for x in keep[:6]), ptr(keep[6]), 3, 2, None, None,
                                       *(ptr(o[k]) for k in ('sd', 'si', 'elapsed', 'episode', 'obs', 'obj', 'reward',
                                                             'done', 'bad')))
    assert rc == 0, b.last_error()
    _assert_same(o, want, 'pgm_envplug_transition_ex of a contract-1 library')


# ------------------------------------------------------------------------------------------------ 4. refusals
def _rollout_ex(pl, env_par=C.c_void_p(0x1000), **over):
    a, keep = _launch_args(pl, **over)
    rc = pl.h.pgm_envplug_rollout_ex(a['d'], a['params'], a['sd'], a['si'], a['episode'], a['table'], a['R'],
                                     a['reset_count'], a['st'], a['ns'], a['rb'], None, 0, 0, env_par, None, 0, None)
    return rc, pl.last_error()


def _eval_ex(pl, env_par=C.c_void_p(0x1000), **over):
    a, keep = _launch_args(pl, **over)
    rc = pl.h.pgm_envplug_eval_ex(a['d'], a['params'], a['table'], a['R'], a['reset_count'], a['ob_mean'], a['ob_var'],
                                  a['eval_num'], 1, 1, 0.99, a['objs'], env_par, 0, None)
    return rc, pl.last_error()


@pytest.mark.parametrize('name', ['slip', 'gather'])
def test_contract_2_library_refuses_the_old_entry_points(plugins, name):
    pl = plugins[name]
    a, keep = _launch_args(pl)
    x = C.c_void_p(0x1000)
    calls = (('pgm_envplug_rollout', lambda: pl.h.pgm_envplug_rollout(
                  a['d'], a['params'], a['sd'], a['si'], a['episode'], a['table'], 3, 8, a['st'], a['ns'], a['rb'], None,
                  0, 0, None)),
             ('pgm_envplug_eval', lambda: pl.h.pgm_envplug_eval(a['d'], a['params'], a['table'], 3, 8, x, x, 2, 1, 1,
                                                                0.99, a['objs'], None)),
             ('pgm_envplug_transition', lambda: pl.h.pgm_envplug_transition(0, *([x] * 7), 3, 2, *([x] * 9))),
             ('pgm_envplug_reset', lambda: pl.h.pgm_envplug_reset(0, x, x, x, 3, 2, x, x, x)))
    for what, call in calls:
        assert call() == _lib.PGM_E_UNSUPPORTED
        msg = pl.last_error()
        assert msg.startswith(what + ':') and f'{what}_ex' in msg and 'CONTRACT = 2' in msg, msg


@pytest.mark.parametrize('name', ['slip', 'gather', 'line'])
def test_ex_refusals_in_the_documented_order(plugins, name):
    """The order of pgm_envplug_rollout / _eval (NULL pointers; check_dims; the compiled dims; LN; T / eval_num; R;
    reset_count), then env_par NULL with NP > 0 -- every item with every later one wrong as well, every message
    starting with the _ex entry point's name.  A contract-1 library has no last item: NULL env_par is accepted (the
    call then fails nowhere before the launch, which these dummies must not reach, so it is not made)."""
    pl, E = plugins[name], _lib
    for call, what, extra, need in ((_rollout_ex, 'pgm_envplug_rollout_ex', {}, 3),
                                    (_eval_ex, 'pgm_envplug_eval_ex', dict(eval_num=9), 2)):
        later = dict(R=0, reset_count=0, env_par=None)
        bad_all = dict(later, **extra)
        rc, msg = call(pl, params=None, dims=dict(H=32, O=pl.O + 1, LN=1, T=0), **bad_all)
        assert rc == E.PGM_E_INVALID_ARG and msg.startswith(what + ':') and 'null pointer' in msg
        rc, msg = call(pl, dims=dict(H=32, O=pl.O + 1, LN=1, T=0), **bad_all)
        assert rc == E.PGM_E_UNSUPPORTED and msg.startswith(what + ':') and 'hidden size 32' in msg
        rc, msg = call(pl, dims=dict(O=pl.O + 1, LN=1, T=0), **bad_all)
        assert rc == E.PGM_E_UNSUPPORTED and msg.startswith(what + ':') and 'compiled for' in msg
        rc, msg = call(pl, dims=dict(LN=1, T=0), **bad_all)
        assert rc == E.PGM_E_UNSUPPORTED and msg.startswith(what + ':') and 'LN = 1' in msg
        if call is _rollout_ex:
            rc, msg = call(pl, dims=dict(T=0), **later)
            assert rc == E.PGM_E_SHAPE and msg == f'{what}: T must be positive'
        else:
            rc, msg = call(pl, **bad_all)
            assert rc == E.PGM_E_INVALID_ARG and msg.startswith(what + ':') and 'eval_num=9' in msg
        rc, msg = call(pl, **later)
        assert rc == E.PGM_E_INVALID_ARG and msg.startswith(what + ':') and 'R = 0' in msg
        rc, msg = call(pl, reset_count=need - 1, env_par=None)
        assert rc == E.PGM_E_INVALID_ARG and msg.startswith(what + ':') and f'the call reads {need}' in msg
        if pl.NP > 0:
            rc, msg = call(pl, env_par=None)
            assert rc == E.PGM_E_INVALID_ARG and msg.startswith(what + ':') and 'env_par' in msg and f'NP = {pl.NP}' in msg


def test_host_ex_refusals(plugins):
    pl = plugins['slip']
    table = envspec.plugin_reset_table(0, 2, 3, 1)
    args = (np.zeros((1, 2)), np.zeros((1, 0), np.int32), [0], [0], [0], np.zeros((1, 1), np.float32), table)
    with pytest.raises(PGMError, match='NW = 1 uniforms per step'):
        pl.transition(*args)
    with pytest.raises(PGMError, match='NP = 2'):
        pl.transition(*args, par=[0.1], w=[[0.5]])
    with pytest.raises(PGMError, match='row 5'):
        pl.reset([5], [0], table)
    x = C.c_void_p(0x1000)
    one = np.zeros(1, np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = pl.h.pgm_envplug_transition_ex(1, x, x, ptr(one), ptr(one), ptr(one), x, x, 3, 2, None, x, *([x] * 9))
    assert rc == _lib.PGM_E_INVALID_ARG and pl.last_error().startswith('pgm_envplug_transition_ex:') \
        and 'env_par' in pl.last_error()
    rc = pl.h.pgm_envplug_transition_ex(1, x, x, ptr(one), ptr(one), ptr(one), x, x, 3, 2, x, None, *([x] * 9))
    assert rc == _lib.PGM_E_INVALID_ARG and 'w is a null pointer' in pl.last_error()
    rc = pl.h.pgm_envplug_transition_ex(1, x, x, ptr(one), ptr(one), ptr(one), x, x, 0, 2, None, None, *([x] * 9))
    assert rc == _lib.PGM_E_INVALID_ARG and 'R = 0' in pl.last_error(), 'the existing order comes first'
    rc = pl.h.pgm_envplug_reset_ex(1, ptr(one), ptr(one), x, 3, 2, None, x, x, x)
    assert rc == _lib.PGM_E_INVALID_ARG and pl.last_error().startswith('pgm_envplug_reset_ex:')


def test_par_vector(plugins):
    pl = plugins['slip']
    assert np.array_equal(pl.par_vector(), [0.2, 0.05]) and np.array_equal(pl.par_vector({'wind': 1}), [0.2, 1.0])
    with pytest.raises(PGMError, match="'gust' is not a runtime parameter of slip.hpp"):
        pl.par_vector({'gust': 1.0})
    with pytest.raises(PGMError, match='must be a finite number'):
        pl.par_vector({'wind': 'strong'})
    for name in ('noisemax', 'line'):
        with pytest.raises(PGMError, match='has no runtime parameters'):
            plugins[name].par_vector({'wind': 1.0})
        assert plugins[name].par_vector({}).size == 0


def test_taskbatch_refusals_of_env_params(plugins):
    from pgmorl_amd.runtime import TaskBatch
    with pytest.raises(PGMError, match="'gust' is not a runtime parameter"):
        TaskBatch('Plug2TB-v0', 2, device='cpu', env_plugin=plugins['slip'], env_params={'gust': 1.0})
    with pytest.raises(PGMError, match='has no runtime parameters'):
        TaskBatch('Plug2TB-v0', 2, device='cpu', env_plugin=plugins['noisemax'], env_params={'wind': 1.0})
    with pytest.raises(PGMError, match='has no runtime parameters'):
        TaskBatch('Plug2TB-v0', 2, device='cpu', env_plugin=plugins['line'], env_params={'wind': 1.0})
    assert 'Plug2TB-v0' not in envspec.user_env_names(), 'a refused batch registers nothing'
    with pytest.raises(PGMError, match='this batch has no plug-in'):
        TaskBatch('MO-Hopper-v2', 2, device='cpu', env_params={'wind': 1.0})
    with pytest.raises(PGMError, match="'gust' is not a runtime parameter"):
        PluginHostVecEnv(plugins['slip'], 2, 3, env_params={'gust': 1.0})


def test_cli_refuses_env_param_before_the_save_dir(tmp_path):
    from pgmorl_amd.run import main
    slip, line = p2.header('slip'), pe.header('line')
    prev = torch.get_default_dtype()
    try:
        cases = ((['--env-name', 'MO-Hopper-v2', '--env-param', 'wind=0.1'], 'it needs --env-plugin'),
                 (['--env-plugin', slip, '--env-name', 'Plug2Cli-v0', '--env-param', 'gust=0.1'],
                  "'gust' is not a runtime parameter"),
                 (['--env-plugin', slip, '--env-name', 'Plug2Cli-v0', '--env-param', 'wind'], 'expected NAME=VALUE'),
                 (['--env-plugin', slip, '--env-name', 'Plug2Cli-v0', '--env-param', 'wind=strong'], 'finite number'),
                 (['--env-plugin', slip, '--env-name', 'Plug2Cli-v0', '--host-env', 'plugin', '--env-param', 'gust=1'],
                  "'gust' is not a runtime parameter"),
                 (['--env-plugin', line, '--env-name', 'Plug2CliLine-v0', '--env-param', 'wind=0.1'],
                  'has no runtime parameters'))
        for i, (extra, msg) in enumerate(cases):
            save = tmp_path / f'run{i}'
            with pytest.raises(PGMError, match=msg):
                main(['--obj-num', '2', '--save-dir', str(save)] + extra)
            assert not save.exists(), extra
    finally:
        torch.set_default_dtype(prev)


# ------------------------------------------------------------------------------------------------ 5. the host env
@pytest.mark.parametrize('env', [p2.Slip, p2.Gather, p2.NoiseMax], ids=lambda e: e.NAME)
def test_plugin_host_vec_env_feeds_the_stream(plugins, env):
    """hostenv.PluginHostVecEnv against the numpy restatement behind the same protocol: the parameters, the stream of
    the rollout's env seed at (t N + n) NW + j restarted by begin_rollout, fed uniforms, the evaluation's stream at
    (e MAX_STEPS + it) NW + j -- equal outputs; the words do not depend on the task."""
    P, N, E, T = 2, 3, 4, 14
    kw = dict(seed=2, R=3, env_params=OTHER[env.NAME])
    he, ne = PluginHostVecEnv(plugins[env.NAME], P, N, **kw), p2.NumpyPlugin2HostVecEnv(env, P, N, **kw)
    rng = np.random.RandomState(0)
    fed = rng.rand(T, N, env.NW)
    for r, noise in enumerate((None, fed, None)):
        if r == 0:
            assert np.array_equal(he.reset(), ne.reset())
        he.begin_rollout(envplug.env_seed(10 + r), noise)
        ne.begin_rollout(p2.env_seed(10 + r), noise)
        for t in range(T):
            act = (np.broadcast_to(rng.randint(0, env.A, (1, N)), (P, N)).astype(np.int32) if env.DISCRETE
                   else np.broadcast_to(rng.randn(1, N, env.A), (P, N, env.A)).astype(np.float32))
            a, b = he.step(act), ne.step(act)
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and np.array_equal(x, y), (r, t)
            assert np.array_equal(a[0][0], a[0][1]) and np.array_equal(a[4][0], a[4][1]), 'the same noise for every task'
    assert he._st['episode'].max() >= 1
    assert np.array_equal(he.eval_reset(E), ne.eval_reset(E))
    for t in range(env.MAX_STEPS):
        act = (rng.randint(0, env.A, (P, E)).astype(np.int32) if env.DISCRETE
               else rng.randn(P, E, env.A).astype(np.float32))
        for x, y in zip(he.eval_step(act), ne.eval_step(act)):
            assert np.array_equal(x, y), t


# ------------------------------------------------------------------------------------------------ the recorded cases
@pytest.mark.parametrize('N', [1, 3, 8])
@pytest.mark.parametrize('env', [p2.Slip, p2.Gather], ids=lambda e: e.NAME)
def test_recorded_conditions(env, N):
    """The parameters and seeds recorded for the GPU case fused-vs-host-stepped (tests/envplug2_ref.py COND) make its
    first rollout, replayed here by the fp64 reference, contain a true terminal, a forced limit, two auto-resets and
    steps on both sides of w0 < p; the counts are those recorded."""
    from . import envplug2_ref as r2
    c = r2.conditions(env, N)
    assert r2.meets(c), c
    assert tuple(c[k] for k in ('terminals', 'limits', 'resets', 'below', 'above')) == r2.COUNTS[env.NAME, N], c


def test_mopg_seed_is_the_first_that_passes():
    from . import envplug2_ref as r2
    for earlier in range(r2.MOPG_SEED):
        assert r2.mopg_case(p2.Slip, earlier)[5], 'an earlier seed meets the conditions'
    name, args, pols, w, refs, bad, m = r2.mopg_case(p2.Slip, r2.MOPG_SEED)
    assert not bad, bad
    assert m['env'] >= r2.MARGIN, m


# ------------------------------------------------------------------------------------------------ 6. sanitizers
@ENVS
def test_contract_2_header_under_the_host_sanitizers(tmp_path, plugins, env):
    """tests/cpp/envplug2_transition_check.cpp (its own main; the header and pgm_envplug.hpp alone, no HIP) built with
    the address and undefined-behaviour sanitizers runs clean over the grid with the parameters and the uniforms in
    exact-size heap arrays, and its lines are the host function's.  No sanitizer touches code loaded into python."""
    exe = tmp_path / 'envplug2_check'
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'include'), '-include', p2.header(env.NAME),
                    os.path.join(ROOT, 'tests', 'cpp', 'envplug2_transition_check.cpp'), '-o', str(exe)], check=True)
    sd, si, el, ep, row, act, w, table = _grid(env, np.random.RandomState(0))
    par = _par_sets(env)[-1]
    n = len(el)
    hx = lambda v: ' '.join(float(x).hex() for x in np.asarray(v, dtype=np.float64).reshape(-1))  # noqa: E731
    ix = lambda v: ' '.join(str(int(x)) for x in np.asarray(v).reshape(-1))  # noqa: E731
    text = [f'{table.shape[1]} {table.shape[0]} {n}\n{hx(par)}\n{hx(table)}\n']
    for i in range(n):
        a = ix(act[i]) if env.DISCRETE else hx(act[i])
        text.append(f'{hx(sd[i])} {ix(si[i])} {el[i]} {ep[i]} {row[i]} {a} {hx(w[i])}\n')
    r = subprocess.run([str(exe)], input=''.join(text), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert f'{n} cases' in r.stderr
    want = plugins[env.NAME].transition(sd, si, el, ep, row, act, table, par=par, w=w)
    rows = r.stdout.splitlines()
    assert len(rows) == n + 1
    flt = np.array([[float.fromhex(x) for x in ln.split('|')[0].split()] for ln in rows[:n]])
    ints = np.array([[int(x) for x in ln.split('|')[1].split()] for ln in rows[:n]])
    wf = np.concatenate([want['sd'], want['obs'], want['obj'], want['reward'][:, None]], -1)
    wi = np.concatenate([want['si'], np.stack([want['elapsed'], want['episode'], want['done'], want['bad']], -1)], -1)
    assert np.array_equal(flt.view(np.int64), wf.view(np.int64)) and np.array_equal(ints, wi)
    stream = np.array([float.fromhex(x) for x in rows[n].split()])
    assert np.array_equal(stream, p2.u53(7, 0, env.NW + 1)), 'u53 of the g++ build'
