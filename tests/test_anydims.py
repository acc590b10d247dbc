"""The runtime-dim kernel family without a device: the feature bit, the argument checks of every *_any entry point in
their documented order, the workspace size, envspec.register_env / hostenv.register_from_spec, the parameter layout at
dims no kernel is compiled for, the refusals of TaskBatch and the CLI, and the conditions on the GPU tests' inputs
(tests/anydims_ref.py), judged from the reference alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from pgmorl_amd import _lib, envspec
from pgmorl_amd._lib import Dims, PGMError, PPOHParams, RolloutBuf
from pgmorl_amd.hostenv import GymHostVecEnv, check_spec, register_from_spec
from pgmorl_amd.layout import ParamLayout
from pgmorl_amd.policy import new_policy

from . import anydims_envs as envs
from . import anydims_ref as ar

ONE = C.c_void_p(1)  # a non-NULL pointer that no validated-away call dereferences
SPEC = 'tests.anydims_envs:make_env'
UNS, INV, SHP = _lib.PGM_E_UNSUPPORTED, _lib.PGM_E_INVALID_ARG, _lib.PGM_E_SHAPE


def test_feature_bit():
    """Bit 8 is set in the library's full mask, pgm_abi_feature_mask().  pgm_abi_features() itself keeps the value the
    existing callers compare for equality (tests/test_dummy_device.py pins == 7), so the new bit cannot appear there."""
    L = _lib.lib()
    assert _lib.FEATURE_ANY_DIMS == 8 and L.pgm_abi_feature_mask() & 8 and _lib.features() & _lib.FEATURE_ANY_DIMS
    assert L.pgm_abi_feature_mask() & 7 == 7 and L.pgm_abi_feature_mask() == L.pgm_abi_features() | 8
    assert _lib.lib().pgm_abi_version() == 5 and _lib.lib().pgm_abi_minor() == 1  # the version pair is unchanged
    _lib.require_any_dims()
    assert C.sizeof(Dims) == 32 and C.sizeof(RolloutBuf) == 72 and C.sizeof(PPOHParams) == 48  # no struct changed size


# ------------------------------------------------------------------------------------------------ argument checks
def _calls(d, head=0, t=0, E=3, hp=None, rb=None, null=None):
    """Every new entry point on dims d with non-NULL dummies (never dereferenced: the call is refused).  null: the
    name of the entry point whose first required pointer after the dims is NULL."""
    L = _lib.lib()
    rb = rb or RolloutBuf(*([ONE] * 9))
    hp = hp or PPOHParams(0.2, 0.5, 0.0, 0.5, 1e-5, 0.9, 0.999, 0.0, 1, 2, 1, 0)
    st, ns = _lib.EnvState(ONE, ONE, ONE, ONE, ONE, ONE), _lib.NormState(*([ONE] * 9), 0.995, 10.0, 10.0, 1e-8, 1, 1)
    prm = lambda name: None if null == name else ONE
    return {
        'pgm_rollout_act_any': lambda: L.pgm_rollout_act_any(C.byref(d), head, prm('pgm_rollout_act_any'),
                                                             C.byref(rb), t, ONE, ONE, None),
        'pgm_eval_act_any': lambda: L.pgm_eval_act_any(C.byref(d), head, prm('pgm_eval_act_any'), ONE, ONE, 1, ONE, E,
                                                       ONE, None),
        'pgm_env_ingest_any': lambda: L.pgm_env_ingest_any(C.byref(d), C.byref(st), C.byref(ns), C.byref(rb),
                                                           t if t <= d.T else d.T, prm('pgm_env_ingest_any'), ONE, ONE,
                                                           ONE, ONE, None),
        'pgm_ppo_update_any': lambda: L.pgm_ppo_update_any(C.byref(d), head, C.byref(hp), prm('pgm_ppo_update_any'),
                                                           ONE, ONE, ONE, ONE, ONE, C.byref(rb), ONE, ONE, None),
    }


def _refused(calls, rc, word, skip=()):
    L = _lib.lib()
    for name, call in calls.items():
        if name in skip:
            continue
        assert call() == rc, (name, L.pgm_last_error())
        err = L.pgm_last_error()
        assert word in err and name.encode() in err, (name, err)


GOOD = (2, 4, 8, 5, 1, 2, 64, 0)  # P, N, T, O, A, K, H, LN


def _dims(**kw):
    f = dict(zip(('P', 'N', 'T', 'O', 'A', 'K', 'H', 'LN'), GOOD))
    f.update(kw)
    return Dims(*(f[k] for k in ('P', 'N', 'T', 'O', 'A', 'K', 'H', 'LN')))


def test_argument_errors_in_order():
    """NULL pointers, then check_dims (H, N), then the range (O, A, K, head, Categorical A < 2), then LN, then the step
    index / E / the minibatch shape: each refused before any device work (this host has no device), the message naming
    the entry point; an earlier item wins over a later one."""
    L = _lib.lib()
    bad_all = _dims(H=32, O=40, LN=1)  # every later item is wrong as well
    # 1. NULL pointers first
    for name in _calls(bad_all):
        assert _calls(bad_all, null=name)[name]() == INV and b'null' in L.pgm_last_error() \
            and name.encode() in L.pgm_last_error(), name
    nb = RolloutBuf(*([ONE] * 9))
    nb.obs = None
    _refused(_calls(bad_all, rb=nb), INV, b'null', skip=('pgm_eval_act_any',))  # (it takes no rollout storage)
    assert L.pgm_rollout_act_any(None, 0, ONE, C.byref(nb), 0, ONE, ONE, None) == INV
    assert L.pgm_ppo_update_any(C.byref(_dims()), 0, C.byref(PPOHParams()), ONE, ONE, ONE, ONE, ONE, ONE,
                                C.byref(RolloutBuf(*([ONE] * 9))), ONE, None, None) == INV  # the workspace
    # 2. check_dims
    _refused(_calls(_dims(H=32, O=40, LN=1)), UNS, b'hidden size')
    _refused(_calls(_dims(N=9, O=40, LN=1)), UNS, b'N=9', skip=('pgm_eval_act_any',))  # (eval ignores N)
    # 3. the range, each limit named
    _refused(_calls(_dims(O=33, LN=1), t=99, E=9), UNS, b'obs_dim 33')
    _refused(_calls(_dims(A=9, LN=1), t=99, E=9), UNS, b'A = 9')
    _refused(_calls(_dims(K=4, LN=1), t=99, E=9), UNS, b'K = 4')
    _refused(_calls(_dims(LN=1), head=2, t=99, E=9), UNS, b'head = 2', skip=('pgm_env_ingest_any',))
    _refused(_calls(_dims(A=1, LN=1), head=1, t=99, E=9), UNS, b'A >= 2', skip=('pgm_env_ingest_any',))
    # 4. LayerNorm
    _refused(_calls(_dims(LN=1), t=99, E=9), UNS, b'LayerNorm')
    # 5. the step index, E, the minibatch shape
    d = _dims()
    for head in (0, 1):
        dd = _dims(A=3)
        for t in (9, -1):
            assert _calls(dd, head=head, t=t)['pgm_rollout_act_any']() == SHP and b'step t' in L.pgm_last_error()
        for E in (0, 9):
            assert _calls(dd, head=head, E=E)['pgm_eval_act_any']() == SHP and b'E=' in L.pgm_last_error()
        hp = PPOHParams(0.2, 0.5, 0.0, 0.5, 1e-5, 0.9, 0.999, 0.0, 0, 2, 1, 0)  # ppo_epoch 0
        assert _calls(dd, head=head, hp=hp)['pgm_ppo_update_any']() == SHP and b'bad shape' in L.pgm_last_error()
        hp = PPOHParams(0.2, 0.5, 0.0, 0.5, 1e-5, 0.9, 0.999, 0.0, 1, 33, 1, 0)  # more minibatches than rows
        assert _calls(dd, head=head, hp=hp)['pgm_ppo_update_any']() == SHP
    st, ns = _lib.EnvState(ONE, ONE, ONE, ONE, ONE, ONE), _lib.NormState(*([ONE] * 9), 0.995, 10.0, 10.0, 1e-8, 1, 1)
    rb = RolloutBuf(*([ONE] * 9))
    for t in (8, -2):
        assert L.pgm_env_ingest_any(C.byref(d), C.byref(st), C.byref(ns), C.byref(rb), t, ONE, ONE, ONE, ONE, ONE,
                                    None) == SHP and b'pgm_env_ingest_any' in L.pgm_last_error()
    # t < T needs the random stream and action_out; t >= 0 the transition
    assert L.pgm_rollout_act_any(C.byref(d), 0, ONE, C.byref(rb), 0, None, ONE, None) == INV
    assert L.pgm_rollout_act_any(C.byref(d), 0, ONE, C.byref(rb), 0, ONE, None, None) == INV
    assert L.pgm_env_ingest_any(C.byref(d), C.byref(st), C.byref(ns), C.byref(rb), 0, ONE, None, ONE, ONE, ONE,
                                None) == INV


def test_existing_entry_points_still_refuse_unknown_dims():
    L = _lib.lib()
    d, rb = _dims(), RolloutBuf(*([ONE] * 9))
    assert L.pgm_rollout_act(C.byref(d), ONE, C.byref(rb), 0, ONE, ONE, None) == UNS
    assert L.pgm_rollout_act_cat(C.byref(d), ONE, C.byref(rb), 0, ONE, ONE, None) == UNS


def test_workspace_bytes():
    L = _lib.lib()
    sizes = [L.pgm_ppo_update_any_workspace_bytes(C.byref(Dims(P, 4, 64, 5, 1, 2, 64, 0))) for P in range(1, 130)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and all(s >= (2 * P + 1) * 8 for P, s in enumerate(sizes, 1))
    assert L.pgm_ppo_update_any_workspace_bytes(None) == 0


# ------------------------------------------------------------------------------------------------ registration
def test_register_env():
    envspec.register_env('Reg-A', 5, 1, 2)
    envspec.register_env('Reg-A', 5, 1, 2)  # the same dims again: accepted
    envspec.register_env('Reg-B', 2, 3, 3, discrete=True)
    assert {'Reg-A', 'Reg-B'} <= set(envspec.user_env_names())
    assert envspec.make_spec('Reg-A') == {'name': 'Reg-A', 'obs_dim': 5, 'act_dim': 1, 'obj_num': 2, 'user': True}
    sp = envspec.make_spec('Reg-B')
    assert sp['user'] and sp['discrete'] and (sp['obs_dim'], sp['act_dim'], sp['obj_num']) == (2, 3, 3)
    with pytest.raises(ValueError, match='already registered'):
        envspec.register_env('Reg-A', 6, 1, 2)
    for known in ('MO-Hopper-v2', 'MO-DeepSeaTreasure-v0', 'MO-Dummy-v0'):
        with pytest.raises(ValueError, match='own envs'):
            envspec.register_env(known, 5, 1, 2)
    for bad, word in (((33, 1, 2, False), 'obs_dim'), ((0, 1, 2, False), 'obs_dim'), ((5, 9, 2, False), 'action dims'),
                      ((5, 0, 2, False), 'action dims'), ((5, 1, 4, False), 'objectives'),
                      ((5, 1, 0, False), 'objectives'), ((5, 1, 2, True), 'actions'), ((5, 9, 2, True), 'actions')):
        with pytest.raises(ValueError, match=word):
            envspec.register_env('Reg-bad', *bad[:3], discrete=bad[3])
    assert 'Reg-bad' not in envspec.user_env_names()
    with pytest.raises(ValueError, match='unknown env'):  # an unregistered unknown name raises as before
        envspec.make_spec('Reg-unknown')
    # the built-in lists are untouched
    assert len(envspec.env_names()) == 7 and not set(envspec.user_env_names()) & set(envspec.env_names())


def test_register_from_spec(monkeypatch):
    assert register_from_spec('synth', 'Spec-unknown') is False and register_from_spec(SPEC, 'MO-Hopper-v2') is False
    for bad in ('synth', 'dst', 'dummy'):
        with pytest.raises(ValueError):  # those step envspec's own envs only
            check_spec(bad, 'Spec-unknown')
    assert envs.CONT not in envspec.env_names()
    # a name nothing has registered, behind a callable of its own: True on the first call, False on the repeat
    monkeypatch.setattr(envs, 'make_fresh', lambda name, seed, rank: envs.TinyDiscEnv(seed + rank), raising=False)
    fresh = 'tests.anydims_envs:make_fresh'
    assert 'Spec-fresh-v0' not in envspec.user_env_names()
    assert register_from_spec(fresh, 'Spec-fresh-v0', 0) is True and 'Spec-fresh-v0' in envspec.user_env_names()
    assert register_from_spec(fresh, 'Spec-fresh-v0', 0) is False
    sp = envspec.make_spec('Spec-fresh-v0')
    assert (sp['obs_dim'], sp['act_dim'], sp['obj_num'], sp.get('discrete'), sp['user']) == (2, 3, 3, True, True)
    register_from_spec(SPEC, envs.CONT, 0)  # (another test may have registered these two already)
    register_from_spec(SPEC, envs.DISC, 0)
    assert envspec.make_spec(envs.CONT)['obs_dim'] == 5 and not envspec.make_spec(envs.CONT).get('discrete')
    sp = envspec.make_spec(envs.DISC)
    assert (sp['obs_dim'], sp['act_dim'], sp['obj_num'], sp['discrete'], sp['user']) == (2, 3, 3, True, True)
    factory = check_spec(SPEC, envs.CONT, 0)  # compares against the registered dims
    he = factory(envs.CONT, 1, 2, 0)
    assert isinstance(he, GymHostVecEnv) and he.dims() == (5, 1, 2)
    he.close()
    for bad in ('synth', 'dst', 'dummy'):
        with pytest.raises(ValueError, match='third-party'):
            check_spec(bad, envs.DISC)
    with pytest.raises(ValueError, match='unknown env'):  # the callable refuses the name: nothing is registered
        register_from_spec(SPEC, 'Spec-unknown')
    assert 'Spec-unknown' not in envspec.user_env_names()
    with pytest.raises(ValueError, match='cannot import'):
        register_from_spec('tests.no_such_module:make_env', 'Spec-unknown')


def test_tiny_envs_are_deterministic_per_seed_and_rank():
    for name, act in ((envs.CONT, np.array([0.7], dtype=np.float32)), (envs.DISC, 2)):
        runs = []
        for _ in range(2):
            e = envs.make_env(name, 3, 1)
            tr = [e.reset()]
            for _ in range(30):
                o, r, done, info = e.step(act)
                tr.append(np.concatenate([o, [r, done], info['obj']]))
                if done:
                    assert 'bad_transition' not in info  # driven to the bound / the end of the chain: a true terminal
                    tr.append(e.reset())
            runs.append(np.concatenate(tr))
        assert np.array_equal(*runs)

        def starts(rank):  # the start states of six episodes (one step each)
            e, out = envs.make_env(name, 3, rank), []
            for _ in range(6):
                out.append(e.reset())
                e.step(act)
            return np.concatenate(out)
        assert not np.array_equal(starts(1), starts(2)) and np.array_equal(starts(2), starts(2))
        e = envs.make_env(name, 3, 1)
        assert np.array_equal(e.reset(), e.reset())  # no step in between: the same episode again (a probe is harmless)
    e = envs.make_env(envs.DISC, 0, 0)
    e.reset()
    flags = [e.step(1) for _ in range(envs.DISC_LIMIT)]
    assert flags[-1][2] and flags[-1][3].get('bad_transition') and not flags[-2][2]  # staying: the time limit


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize('dims,discrete', [((5, 1, 2), False), ((2, 3, 3), True)])
def test_param_layout_roundtrip(dims, discrete):
    torch.manual_seed(4)
    pol = new_policy(*dims, discrete=discrete)
    sd = pol.state_dict()
    lay = ParamLayout(*dims, discrete=discrete)
    flat = lay.flatten(sd, dtype=np.float64)
    back = lay.unflatten(flat)
    assert list(back.keys()) == list(sd.keys()) and flat.size == lay.total and lay.total % 64 == 0
    for k in sd:
        assert torch.equal(back[k], sd[k]), k
    O, A, K = dims
    n = 2 * (O * 64 + 64 + 64 * 64 + 64) + 64 * K + K + 64 * A + A + (0 if discrete else A)
    assert sum(v.numel() for v in sd.values()) == n


# ------------------------------------------------------------------------------------------------ refusals
def test_taskbatch_refusals():
    from pgmorl_amd.runtime import TaskBatch
    name = ar.env_of((5, 1, 2), False)
    he = lambda: GymHostVecEnv(envs.make_env, envs.CONT, 2, 4)
    with pytest.raises(PGMError, match='host_env'):
        TaskBatch(name, 2, device='cpu')
    with pytest.raises(PGMError, match='plain towers'):
        TaskBatch(name, 2, device='cpu', layernorm=True, host_env=he())
    with pytest.raises(PGMError, match='device'):
        TaskBatch(name, 2, device='cpu', device_env=True, host_env=he())
    with pytest.raises(PGMError, match='at most 8'):
        TaskBatch(name, 2, device='cpu', eval_num=9, host_env=he())
    with pytest.raises(PGMError, match='obs_dim <= 32'):  # any_dims=True on an env outside the family's range
        TaskBatch('MO-Humanoid-v2', 2, device='cpu', any_dims=True, host_env=he())
    with pytest.raises(PGMError, match='host_env'):
        TaskBatch('MO-Hopper-v2', 2, device='cpu', any_dims=True)


def test_cli_refuses_before_the_save_dir(tmp_path, monkeypatch):
    from pgmorl_amd.run import main
    import tests.anydims_envs as mod

    class Wide(envs.TinyContEnv):
        def _obs(self):
            return np.zeros(33)
    monkeypatch.setattr(mod, 'make_wide', lambda name, seed, rank: Wide(seed + rank), raising=False)
    prev = torch.get_default_dtype()
    try:
        cases = ((['--env-name', envs.CONT, '--host-env', SPEC, '--layernorm'], 'plain towers'),
                 (['--env-name', 'Wide-v0', '--host-env', 'tests.anydims_envs:make_wide'], 'obs_dim 33'),
                 (['--env-name', 'Cli-unknown', '--host-env', SPEC], 'unknown env'),
                 (['--env-name', 'Cli-unknown', '--host-env', 'synth'], 'unknown env'))
        for i, (extra, msg) in enumerate(cases):
            save = tmp_path / f'run{i}'
            with pytest.raises((PGMError, ValueError), match=msg):
                main(['--obj-num', '2', '--save-dir', str(save)] + extra)
            assert not save.exists()
    finally:
        torch.set_default_dtype(prev)


# ------------------------------------------------------------------------------------------------ test inputs
@pytest.mark.parametrize('dims,discrete,shape,row', ar.UPDATE_CASES + ar.COMPILED_CASES)
def test_update_inputs_meet_the_conditions(dims, discrete, shape, row):
    """branch_inputs' shares, margins and fp32-arm agreement at every Adam step of every task at the recorded seed
    (update_case asserts them), plus row f's entropy condition on the Categorical head."""
    _, results, worst = ar.update_case(dims, discrete, shape, row)
    P, T, N, E, M = ar.SHAPES[shape]
    assert len(results) == P and all(len(r[3]) == E * M for r in results)
    if row == 'f' and discrete:
        assert worst['entropy term, x band'] > 10.0
    print(dims, discrete, shape, row, ar.UPDATE_SEEDS[(dims, discrete, shape, row)],
          {k: float(f'{v:.3g}') for k, v in worst.items()})


LATER_SEEDS = sorted((c for c, s in ar.UPDATE_SEEDS.items() if s > ar.bi.BASE_SEED), key=str)


def test_later_seeds_cover_every_recorded_exception():
    assert len(LATER_SEEDS) == 9 and all(ar.UPDATE_SEEDS[c] < ar.bi.BASE_SEED + ar.SEED_TRIES for c in LATER_SEEDS)
    assert all(s == ar.bi.BASE_SEED for c, s in ar.UPDATE_SEEDS.items() if c not in LATER_SEEDS)  # nothing below it


@pytest.mark.parametrize('dims,discrete,shape,row', LATER_SEEDS)
def test_update_seed_is_the_first_that_passes(dims, discrete, shape, row):
    """Every case whose recorded seed is above the base: each seed below it misses a condition of the reference's."""
    for earlier in range(ar.bi.BASE_SEED, ar.UPDATE_SEEDS[(dims, discrete, shape, row)]):
        assert ar.evaluate_update(dims, discrete, shape, row, earlier, stop_early=True)[2], (dims, discrete, earlier)
