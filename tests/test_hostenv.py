"""Host-stepped environments, host side: ABI minor 1 and the argument validation of pgm_rollout_act / pgm_env_ingest /
pgm_eval_act (no kernel is launched: every case returns before any device work), SynthHostVecEnv against the oracle's
SynthEnv, GymHostVecEnv over fake env classes in both step APIs, and the --host-env flag."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.vecenv import SynthEnv
from pgmorl_amd import _lib, envspec
from pgmorl_amd._lib import Dims, EnvState, NormState, RolloutBuf
from pgmorl_amd.hostenv import GymHostVecEnv, SynthHostVecEnv, check_spec, resolve
from pgmorl_amd.run import get_parser, main, merge_argv

DUMMY = 0x1000  # never dereferenced: the calls below fail validation first


def _p(v=DUMMY):
    return C.c_void_p(v)


def _dims(T=8, O=11, A=3, K=2, LN=0, P=2, N=4):
    return Dims(P, N, T, O, A, K, 64, LN)


def _rb():
    return RolloutBuf(*([DUMMY] * 9))


def _state():
    return EnvState(None, None, DUMMY, DUMMY, DUMMY, None)  # s, elapsed, s0 may be NULL for the ingest


def _norm():
    return NormState(*([DUMMY] * 9), 0.995, 10.0, 10.0, 1e-8, 1, 1)


def test_abi_minor():
    assert _lib.lib().pgm_abi_minor() == 1 == _lib.PGM_ABI_MINOR
    assert _lib.lib().pgm_abi_version() == 5


def _act(d, params=DUMMY, rb=None, t=0, noise=DUMMY, out=DUMMY):
    rb = _rb() if rb is None else rb
    return _lib.lib().pgm_rollout_act(C.byref(d), _p(params), C.byref(rb), t, _p(noise), _p(out), _p(0))


def test_rollout_act_validates_before_any_device_work():
    d = _dims(T=8)
    assert _act(d, params=0) == _lib.PGM_E_INVALID_ARG
    rb = _rb()
    rb.values = None
    assert _act(d, rb=rb) == _lib.PGM_E_INVALID_ARG
    assert _lib.lib().pgm_rollout_act(None, _p(), C.byref(_rb()), 0, _p(), _p(), _p(0)) == _lib.PGM_E_INVALID_ARG
    assert _act(d, t=9) == _lib.PGM_E_SHAPE
    assert _act(d, t=-2) == _lib.PGM_E_SHAPE
    assert _act(d, t=-1) == _lib.PGM_E_SHAPE
    assert _act(d, t=3, noise=0) == _lib.PGM_E_INVALID_ARG      # noise is required for t < T
    assert _act(d, t=3, out=0) == _lib.PGM_E_INVALID_ARG
    assert _act(_dims(O=376, A=17, K=2, LN=1)) == _lib.PGM_E_UNSUPPORTED
    assert b'LayerNorm' in _lib.lib().pgm_last_error()
    assert _act(_dims(LN=2)) == _lib.PGM_E_INVALID_ARG
    assert _act(_dims(N=9)) == _lib.PGM_E_UNSUPPORTED            # check_dims: N <= 8


def _ingest(d, st=None, ns=None, rb=None, t=0, obs=DUMMY, obj=DUMMY, rew=DUMMY, done=DUMMY, bad=DUMMY):
    st, ns, rb = _state() if st is None else st, _norm() if ns is None else ns, _rb() if rb is None else rb
    return _lib.lib().pgm_env_ingest(C.byref(d), C.byref(st), C.byref(ns), C.byref(rb), t, _p(obs), _p(obj), _p(rew),
                                     _p(done), _p(bad), _p(0))


def test_env_ingest_validates_before_any_device_work():
    d = _dims(T=8)
    assert _ingest(d, obs=0) == _lib.PGM_E_INVALID_ARG
    st = _state()
    st.ret = None
    assert _ingest(d, st=st) == _lib.PGM_E_INVALID_ARG
    ns = _norm()
    ns.ret_var = None
    assert _ingest(d, ns=ns) == _lib.PGM_E_INVALID_ARG
    rb = _rb()
    rb.bad_masks = None
    assert _ingest(d, rb=rb) == _lib.PGM_E_INVALID_ARG
    for t in (9, 8, -2):  # valid: -1 (reset) and [0, T)
        assert _ingest(d, t=t) == _lib.PGM_E_SHAPE
    for kw in ({'obj': 0}, {'rew': 0}, {'done': 0}, {'bad': 0}):  # required for t >= 0
        assert _ingest(d, t=2, **kw) == _lib.PGM_E_INVALID_ARG
    assert _ingest(_dims(O=376, A=17, K=2, LN=1)) == _lib.PGM_E_UNSUPPORTED
    assert _ingest(_dims(LN=2)) == _lib.PGM_E_INVALID_ARG


def _eval_act(d, params=DUMMY, mean=DUMMY, var=DUMMY, use=1, obs=DUMMY, E=1, out=DUMMY):
    return _lib.lib().pgm_eval_act(C.byref(d), _p(params), _p(mean), _p(var), use, _p(obs), E, _p(out), _p(0))


def test_eval_act_validates_before_any_device_work():
    d = _dims()
    assert _eval_act(d, params=0) == _lib.PGM_E_INVALID_ARG
    assert _eval_act(d, obs=0) == _lib.PGM_E_INVALID_ARG
    assert _eval_act(d, out=0) == _lib.PGM_E_INVALID_ARG
    assert _eval_act(d, mean=0) == _lib.PGM_E_INVALID_ARG        # required with use_ob_rms
    assert _eval_act(d, E=0) == _lib.PGM_E_SHAPE
    assert _eval_act(d, E=9) == _lib.PGM_E_SHAPE
    assert _eval_act(_dims(O=376, A=17, K=2, LN=1)) == _lib.PGM_E_UNSUPPORTED
    assert _eval_act(_dims(LN=2)) == _lib.PGM_E_INVALID_ARG
    assert _eval_act(_dims(N=99, T=-5), E=0) == _lib.PGM_E_SHAPE  # N and T are ignored: only E is at fault


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('env', ['MO-Hopper-v3', 'MO-Walker2d-v2', 'MO-Humanoid-v2'])
def test_synth_host_env_is_the_oracle_synth_env(env):
    """60 steps across two auto-resets (max_episode_steps = 25), N = 3, P = 2 tasks fed the same actions: the same fp64
    formula as oracle.vecenv.SynthEnv.  The matrix products are summed in another order (einsum over the batch vs
    one BLAS gemv per env), so observations / objectives agree to 1e-14 absolute, not bitwise; flags are exact and the
    two tasks' copies are bitwise identical."""
    P, N, steps, tmax, seed = 2, 3, 60, 25, 4
    spec = dict(envspec.make_spec(env), max_episode_steps=tmax)
    O, A = spec['obs_dim'], spec['act_dim']
    he = SynthHostVecEnv(env, P, N, seed=seed, max_episode_steps=tmax)
    assert he.dims() == (O, A, spec['obj_num']) and (he.P, he.N) == (P, N)
    ref = [SynthEnv(spec, s0) for s0 in envspec.reset_table(O, seed, N)]
    obs = he.reset()
    assert obs.dtype == np.float64 and obs.shape == (P, N, O)
    for n in range(N):
        np.testing.assert_array_equal(obs[0, n], ref[n].reset())
    np.testing.assert_array_equal(obs[0], obs[1])
    rng = np.random.RandomState(1)
    ndone = 0
    for t in range(steps):
        act = (rng.randn(N, A) * 1.5).astype(np.float32)  # beyond the action clip now and then
        obs, rew, done, bad, obj = he.step(np.broadcast_to(act, (P, N, A)))
        assert rew.shape == (P, N) and not rew.any()
        for n in range(N):
            o, r, d, info = ref[n].step(act[n])
            if d:
                o = ref[n].reset()
            np.testing.assert_allclose(obs[0, n], o, rtol=0, atol=1e-14, err_msg=f'obs t={t}')
            np.testing.assert_allclose(obj[0, n], info['obj'], rtol=0, atol=1e-14, err_msg=f'obj t={t}')
            assert bool(done[0, n]) == bool(d) and bool(bad[0, n]) == ('bad_transition' in info)
            ndone += int(d)
        for x in (obs, rew, done, bad, obj):
            np.testing.assert_array_equal(x[0], x[1])
    assert ndone == 2 * N


def test_synth_host_env_eval_side_and_set_active():
    he = SynthHostVecEnv('MO-Hopper-v2', 3, 2, seed=5, max_episode_steps=4)
    he.set_active(2)
    assert he.reset().shape == (2, 2, 11)
    obs = he.eval_reset(3)
    np.testing.assert_array_equal(obs[1], envspec.reset_table(11, 5, 3))  # episode e seeded seed + e
    for i in range(4):
        obs, obj, done = he.eval_step(np.zeros((2, 3, 3), dtype=np.float32))
        assert obs.shape == (2, 3, 11) and obj.shape == (2, 3, 2) and done.all() == (i == 3)
    with pytest.raises(ValueError):
        he.set_active(4)


# ---------------------------------------------------------------------------------------------------------------
class _Space:
    shape = (2,)


class FakeEnv:
    """obs = [seed, episode, step]; obj = [step, sum(action)]; reward = step / 2.  Episode 0 ends in a true terminal
    state at step ``term_at`` (if set); every other episode at the time limit ``horizon``."""
    action_space = _Space()
    obj_dim = 2

    def __init__(self, seed, api, horizon=4, term_at=None, tl_key='bad_transition'):
        self.seed_, self.api, self.horizon, self.term_at, self.tl_key = seed, api, horizon, term_at, tl_key
        self.ep, self.k, self.closed = -1, 0, False

    def _obs(self):
        return np.array([self.seed_, self.ep, self.k], dtype=np.float32)

    def reset(self):
        self.ep += 1
        self.k = 0
        return (self._obs(), {}) if self.api == 5 else self._obs()

    def step(self, a):
        self.k += 1
        term = self.ep == 0 and self.term_at is not None and self.k == self.term_at
        trunc = not term and self.k >= self.horizon
        info = {'obj': np.array([self.k, float(np.sum(a))])}
        if self.api == 5:
            return self._obs(), self.k / 2, term, trunc, info
        if trunc:
            info[self.tl_key] = True
        return self._obs(), self.k / 2, term or trunc, info

    def close(self):
        self.closed = True


def _fake_factory(api, tl_key='bad_transition', log=None):
    def make_env(env_name, seed, rank):
        e = FakeEnv(seed + rank, api, term_at=2 if rank == 1 else None, tl_key=tl_key)
        if log is not None:
            log.append(e)
        return e
    return make_env


@pytest.mark.parametrize('api,tl_key', [(4, 'bad_transition'), (4, 'TimeLimit.truncated'), (5, None)])
def test_gym_host_env_both_step_apis(api, tl_key):
    P, N, seed = 2, 2, 10
    he = GymHostVecEnv(_fake_factory(api, tl_key), 'Fake-v0', P, N, seed=seed)
    assert he.dims() == (3, 2, 2)
    obs = he.reset()
    assert obs.dtype == np.float64 and obs.shape == (P, N, 3)
    ep0 = obs[:, 0, 1].copy()  # (probe_dims has reset env (0, 0) once already: task 0 is one episode ahead)
    np.testing.assert_array_equal(obs[:, :, 0], [[seed, seed + 1]] * P)  # rank n of every task: seed + n
    act = np.full((P, N, 2), 0.25, dtype=np.float32)
    # step 1: nothing ends
    obs, rew, done, bad, obj = he.step(act)
    assert rew.dtype == np.float64 and not done.any() and not bad.any()
    np.testing.assert_array_equal(rew, np.full((P, N), 0.5))
    np.testing.assert_array_equal(obs[:, :, 2], np.ones((P, N)))
    # step 2: env rank 1 reaches its TRUE terminal state: done without bad; obs is the reset observation of the next
    # episode, obj / reward are the terminal step's
    obs, rew, done, bad, obj = he.step(act)
    np.testing.assert_array_equal(done, [[False, True]] * P)
    assert not bad.any()
    np.testing.assert_array_equal(obs[:, 1], [[seed + 1, 1, 0]] * P)
    np.testing.assert_array_equal(obj[:, 1], [[2, 0.5]] * P)
    np.testing.assert_array_equal(rew[:, 1], [1.0] * P)
    # steps 3, 4: env rank 0 hits the time limit at its 4th step: done with bad
    he.step(act)
    obs, rew, done, bad, obj = he.step(act)
    np.testing.assert_array_equal(done, [[True, False]] * P)
    np.testing.assert_array_equal(bad, [[True, False]] * P)
    np.testing.assert_array_equal(obs[:, 0], [[seed, ep0[p] + 1, 0] for p in range(P)])
    np.testing.assert_array_equal(obj[:, 0], [[4, 0.5]] * P)
    he.close()


def test_gym_host_env_eval_episodes_are_seeded_seed_plus_eval_id():
    made = []
    he = GymHostVecEnv(_fake_factory(5, log=made), 'Fake-v0', 2, 1, seed=7, workers=4)
    n_train = len(made)
    obs = he.eval_reset(3)
    assert obs.shape == (2, 3, 3)
    np.testing.assert_array_equal(obs[:, :, 0], [[7, 8, 9]] * 2)
    ev = made[n_train:]
    assert [e.seed_ for e in ev] == [7, 8, 9] * 2
    act = np.zeros((2, 3, 2), dtype=np.float32)
    # eval env rank 1 ends (true terminal) at its step 2, the others at the horizon 4; an ended episode is not stepped
    for i in range(1, 5):
        obs, obj, done = he.eval_step(act)
        np.testing.assert_array_equal(done, [[i >= 4, i >= 2, i >= 4]] * 2)
    assert [e.k for e in ev[:3]] == [4, 2, 4]
    he.eval_reset(1)  # fresh env objects every evaluation; the previous ones are closed
    assert all(e.closed for e in ev)
    np.testing.assert_array_equal(he.step(np.zeros((2, 1, 2), dtype=np.float32))[0][:, 0, 0], [7, 7])
    he.close()


# ---------------------------------------------------------------------------------------------------------------
def make_wrong_dims_env(env_name, seed, rank):
    """--host-env tests.test_hostenv:make_wrong_dims_env: dims (3, 2, 2), no SynthMO env has them."""
    return FakeEnv(seed + rank, 4)


def test_cli_parses_host_env():
    assert get_parser().parse_args(merge_argv([])).host_env is None
    assert get_parser().parse_args(merge_argv(['--host-env', 'synth'])).host_env == 'synth'
    assert get_parser().parse_args(merge_argv(['--host-env', 'a.b:c'])).host_env == 'a.b:c'
    assert resolve('synth') is SynthHostVecEnv
    assert check_spec('synth', 'MO-Hopper-v3') is SynthHostVecEnv


@pytest.mark.parametrize('spec', ['tests.test_hostenv:make_wrong_dims_env', 'no_such_module_xyz:make_env',
                                  'tests.test_hostenv:no_such_callable', 'not-a-spec'])
def test_cli_refuses_bad_host_env_before_the_save_dir(tmp_path, spec, monkeypatch):
    import pgmorl_amd.morl as morl
    monkeypatch.setattr(morl, 'run', lambda *a, **k: pytest.fail('run() was reached'))
    prev = torch.get_default_dtype()
    save = tmp_path / 'run'
    try:
        with pytest.raises(_lib.PGMError) as ei:
            main(['--host-env', spec, '--env-name', 'MO-Hopper-v2', '--save-dir', str(save)])
    finally:
        torch.set_default_dtype(prev)
    assert '--host-env' in str(ei.value)
    if 'wrong_dims' in spec:
        assert '(3, 2, 2)' in str(ei.value) and '(11, 3, 2)' in str(ei.value)
    assert not save.exists()
