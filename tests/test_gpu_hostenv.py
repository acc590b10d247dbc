"""Host-stepped environments on the device (pgm_rollout_act / pgm_env_ingest / pgm_eval_act, TaskBatch(host_env=...),
--host-env) against the CPU oracle on identical inputs.  Bands are those of the fused-path tests they mirror
(tests/test_gpu_kernels.py, tests/test_gpu_layernorm.py), named at each use."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import ppo as oppo
from oracle.mopg import initial_sample, mopg_worker
from oracle.vecenv import RunningMeanStd, SynthEnv, VecNormalizedSynth
from pgmorl_amd import _lib, envspec
from pgmorl_amd._lib import Dims, PGMError
from pgmorl_amd.hostenv import GymHostVecEnv, SynthHostVecEnv
from pgmorl_amd.runtime import TaskBatch

from .helpers import fp32_policies, perturb, small_args, weights_grid
from .test_gpu_kernels import _batch_with_policies, _close, _noise_fn, _oracle_rollout, _teacher_forced_check
from .test_gpu_layernorm import _ln_batch

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
PLAIN = dict(v=(2e-5, 1e-5), a=(2e-5, 1e-5), lp=(5e-5, 1e-5))  # test_act_forward
LNB = dict(v=(5e-5, 1e-4), a=(5e-5, 1e-4), lp=(2e-4, 1e-4))    # test_act_forward_ln


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _make(env, P, N, T, ln, **kw):
    return (_ln_batch if ln else _batch_with_policies)(env, P, N, T, **kw)


# ------------------------------------------------------------------------------------------------ 1. pgm_rollout_act
@pytest.mark.parametrize('env,N,ln', [('MO-Walker2d-v2', 4, False), ('MO-Swimmer-v2', 4, False),
                                      ('MO-Hopper-v3', 8, False), ('MO-Humanoid-v2', 3, False),
                                      ('MO-Hopper-v2', 4, True)])
def test_rollout_act(gpu, env, N, ln):
    """Policy.act of step t in {0, 2, 4} and the bootstrap get_value (t = T = 5) on given observations against
    oracle.policy; only slot t of values / actions / logp may change, action_out is the stored action bitwise."""
    P, T = 3, 5
    spec, tb, pols = _make(env, P, N, T, ln)
    O, A, K = spec['obs_dim'], spec['act_dim'], spec['obj_num']
    band = LNB if ln else PLAIN
    g = torch.Generator().manual_seed(11)
    obs = torch.randn(P, T + 1, N, O, generator=g).float()
    noise = torch.randn(T, N, A, generator=g).float()
    tb.obs.copy_(obs)
    tb.noise.copy_(noise)
    out = torch.empty(P, N, A, device=gpu)
    for t in (0, 2, 4, 5):
        for x in (tb.values, tb.actions, tb.logp, out):
            x.fill_(SENTINEL)
        last = t == T
        _lib.check(_lib.lib().pgm_rollout_act(C.byref(tb.dims), _ptr(tb.params), C.byref(tb.c_rb), t,
                                              _ptr(None if last else tb.noise), _ptr(None if last else out),
                                              _stream()), 'pgm_rollout_act')
        val, act, lp, ao = tb.values.cpu(), tb.actions.cpu(), tb.logp.cpu(), out.cpu()
        assert torch.equal(tb.obs.cpu(), obs), 'observations were written'
        keep = torch.ones(T + 1, dtype=torch.bool)
        keep[t] = False
        assert (val[:, keep] == SENTINEL).all(), f't={t}: values outside slot t changed'
        assert (act[:, keep[:T]] == SENTINEL).all() and (lp[:, keep[:T]] == SENTINEL).all(), \
            f't={t}: actions / logp outside slot t changed'
        if last:
            assert (ao == SENTINEL).all()
        else:
            assert torch.equal(ao, act[:, t]), 'action_out is not the stored action'
        for p in range(P):
            with torch.no_grad():
                if last:
                    rv = pols[p].get_value(obs[p, t].double())
                else:
                    rv, ra, rlp = pols[p].act(obs[p, t].double(), noise=noise[t].double())
            _close(val[p, t], rv, *band['v'], f'value t={t}')
            if not last:
                _close(act[p, t], ra, *band['a'], f'action t={t}')
                _close(lp[p, t], rlp[:, 0], *band['lp'], f'log_prob t={t}')


# ------------------------------------------------------------------------------------------------ 2. pgm_env_ingest
class _RefVecNormalize:
    """VecNormalize.step_wait / reset on supplied transitions with a non-zero scalar reward, in fp64 on
    oracle.vecenv.RunningMeanStd (oracle/vecenv.py restates the zero-reward case of the same lines)."""

    def __init__(self, N, O, gamma, use_ob, use_obj, clipob=10.0, cliprew=10.0, eps=1e-8):
        self.ob_rms = RunningMeanStd(shape=(O,)) if use_ob else None
        self.ret_rms = RunningMeanStd(shape=())
        self.obj_rms = RunningMeanStd(shape=()) if use_obj else None
        self.gamma, self.clipob, self.cliprew, self.eps = gamma, clipob, cliprew, eps
        self.ret, self.obj = np.zeros(N), None

    def _obfilt(self, obs):
        if self.ob_rms is None:
            return obs
        self.ob_rms.update(obs)
        return np.clip((obs - self.ob_rms.mean) / np.sqrt(self.ob_rms.var + self.eps), -self.clipob, self.clipob)

    def reset(self, obs):
        self.ret = np.zeros_like(self.ret)
        return self._obfilt(obs)

    def step(self, obs, rews, dones, objs):
        self.ret = self.ret * self.gamma + rews
        self.obj = self.obj * self.gamma + objs if self.obj is not None else objs.copy()
        obs = self._obfilt(obs)
        self.ret_rms.update(self.ret)
        if self.obj_rms is not None:
            self.obj_rms.update(self.obj)
            objs = np.clip(objs / np.sqrt(self.obj_rms.var + self.eps), -self.cliprew, self.cliprew)
        self.ret[dones] = 0.0
        self.obj[dones] = 0.0
        return obs, objs


def _ingest(tb, t, obs, obj=None, rew=None, done=None, bad=None):
    dev = tb.dev
    d = [None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dt).to(dev)
         for x, dt in ((obs, torch.float64), (obj, torch.float64), (rew, torch.float64), (done, torch.int32),
                       (bad, torch.int32))]
    _lib.check(_lib.lib().pgm_env_ingest(C.byref(tb.dims), C.byref(tb.c_state), C.byref(tb.c_norm), C.byref(tb.c_rb),
                                         t, *(_ptr(x) for x in d), _stream()), 'pgm_env_ingest')


INGEST_ENVS = {(8, 2): 'MO-Swimmer-v2', (11, 3): 'MO-Hopper-v3', (17, 2): 'MO-Walker2d-v2', (376, 2): 'MO-Humanoid-v2'}


@pytest.mark.parametrize('use_ob,use_obj', [(1, 1), (1, 0), (0, 0)])
@pytest.mark.parametrize('O,K,N', [(8, 2, 1), (11, 3, 3), (17, 2, 8), (376, 2, 8)])
def test_env_ingest(gpu, O, K, N, use_ob, use_obj):
    """A reset and 12 scripted transitions per task (seeded random observations / objectives, non-zero rewards, a done
    without bad, a done with bad, two envs done in one step, a done in the last step) against _RefVecNormalize.
    Bands of test_env_reset_step_vecnormalize."""
    P, T, gamma = 2, 12, 0.995
    tb = TaskBatch(INGEST_ENVS[(O, K)], P, num_processes=N, num_steps=T, gamma=gamma, ob_rms=bool(use_ob),
                   obj_rms=bool(use_obj))
    ref = [_RefVecNormalize(N, O, gamma, use_ob, use_obj) for _ in range(P)]
    rng = np.random.RandomState(100 * O + 10 * N + 2 * use_ob + use_obj)
    done = np.zeros((T, P, N), dtype=bool)
    bad = np.zeros((T, P, N), dtype=bool)
    done[3, :, 0] = True                               # a true terminal: done without bad
    done[5, :, N - 1] = bad[5, :, N - 1] = True        # a time-limit end: done with bad
    done[7, :, :2] = True                              # two envs in one step (one when N = 1) ...
    bad[7, 0, 0] = True                                # ... of task 0, one at the time limit
    done[T - 1, 1, N // 2] = True                      # a done in the last step
    bad[T - 1, 1, N // 2] = True
    for name in ('obs', 'rewards', 'masks', 'bad_masks'):
        getattr(tb, name).fill_(SENTINEL)
    tb.ret.fill_(3.0)        # a reset must clear these
    tb.obj_valid.fill_(1)
    stores = ('obs', 'rewards', 'masks', 'bad_masks')

    def snap():
        return {k: getattr(tb, k).cpu().numpy().copy() for k in stores}

    def untouched(prev, cur, touched, what):
        for k in stores:
            keep = np.ones(cur[k].shape[1], dtype=bool)
            keep[touched[k]] = False
            np.testing.assert_array_equal(cur[k][:, keep], prev[k][:, keep], err_msg=f'{what}: {k} outside its slot')

    prev = snap()
    raw = rng.randn(P, N, O) * 0.4 + 0.2
    _ingest(tb, -1, raw)
    cur = snap()
    untouched(prev, cur, {'obs': 0, 'rewards': [], 'masks': 0, 'bad_masks': 0}, 'reset')
    for p in range(P):
        _close(cur['obs'][p, 0], ref[p].reset(raw[p]), 2e-6, 2e-6, 'reset obs')
    assert (cur['masks'][:, 0] == 1).all() and (cur['bad_masks'][:, 0] == 1).all()
    assert not tb.ret.cpu().numpy().any() and not tb.obj_valid.cpu().numpy().any()
    for t in range(T):
        prev = cur
        raw = rng.randn(P, N, O) * 0.4 + 0.2
        if t == 6:
            raw[:, :, 0] = 40.0                        # far outside: the clip at +-clipob
        robj = rng.randn(P, N, K) * 2.0 + 1.0
        rew = rng.randn(P, N) * 1.5 + 0.5
        _ingest(tb, t, raw, robj, rew, done[t], bad[t])
        cur = snap()
        untouched(prev, cur, {'obs': t + 1, 'rewards': t, 'masks': t + 1, 'bad_masks': t + 1}, f'step {t}')
        ret, acc = tb.ret.cpu().numpy(), tb.obj_acc.cpu().numpy()
        for p in range(P):
            o, r = ref[p].step(raw[p], rew[p], done[t, p], robj[p])
            _close(cur['obs'][p, t + 1], o, 2e-6, 2e-6, f'obs step {t}')
            _close(cur['rewards'][p, t], r, 1e-5, 1e-6, f'rewards step {t}')
            np.testing.assert_array_equal(cur['masks'][p, t + 1], np.where(done[t, p], 0.0, 1.0))
            np.testing.assert_array_equal(cur['bad_masks'][p, t + 1], np.where(bad[t, p], 0.0, 1.0))
            assert (ret[p][done[t, p]] == 0).all() and (acc[p][done[t, p]] == 0).all(), 'accumulators of done envs'
            _close(ret[p], ref[p].ret, 0, 1e-9, f'ret step {t}')
            _close(acc[p], ref[p].obj, 0, 1e-9, f'obj accumulator step {t}')
    n = 1e-4
    for _ in range(T):
        n = n + N  # the count as RunningMeanStd advances it
    for p in range(P):
        if use_ob:
            _close(tb.ob_mean[p].cpu(), ref[p].ob_rms.mean, 0, 1e-9, 'ob_rms.mean')
            _close(tb.ob_var[p].cpu(), ref[p].ob_rms.var, 0, 1e-9, 'ob_rms.var')
            assert float(tb.ob_count[p]) == ref[p].ob_rms.count == n + N  # (+ the reset's update)
        else:
            assert (tb.ob_mean[p] == 0).all() and (tb.ob_var[p] == 1).all() and float(tb.ob_count[p]) == 1e-4
        if use_obj:
            _close(tb.obj_mean[p].cpu(), ref[p].obj_rms.mean, 0, 1e-9, 'obj_rms.mean')
            _close(tb.obj_var[p].cpu(), ref[p].obj_rms.var, 0, 1e-9, 'obj_rms.var')
            assert float(tb.obj_count[p]) == ref[p].obj_rms.count == n
        else:
            assert (tb.obj_mean[p] == 0).all() and (tb.obj_var[p] == 1).all() and float(tb.obj_count[p]) == 1e-4
        _close(tb.ret_mean[p].cpu(), ref[p].ret_rms.mean, 0, 1e-9, 'ret_rms.mean')
        _close(tb.ret_var[p].cpu(), ref[p].ret_rms.var, 0, 1e-9, 'ret_rms.var')
        assert float(tb.ret_count[p]) == ref[p].ret_rms.count == n


# ------------------------------------------------------------------------------------------------ 3. pgm_eval_act
@pytest.mark.parametrize('use_ob', [1, 0])
@pytest.mark.parametrize('E', [1, 3, 8])
@pytest.mark.parametrize('env,ln', [('MO-Hopper-v3', False), ('MO-Humanoid-v2', False), ('MO-Hopper-v2', True)])
def test_eval_act(gpu, env, ln, E, use_ob):
    """The deterministic action on fp64 raw observations normalised with frozen statistics (mopg.py:36-39) against
    the oracle; bands of test_rollout_act."""
    P = 3
    spec, tb, pols = _make(env, P, 4, 8, ln, seed=5)
    O, A, K = spec['obs_dim'], spec['act_dim'], spec['obj_num']
    band = LNB if ln else PLAIN
    rng = np.random.RandomState(7 + E)
    rms = []
    for p in range(P):
        r = RunningMeanStd(shape=(O,))
        r.update(rng.randn(50, O) * 0.3 + 0.1)
        rms.append(r)
    mean = torch.tensor(np.stack([r.mean for r in rms]), device=gpu)
    var = torch.tensor(np.stack([r.var for r in rms]), device=gpu)
    raw = rng.randn(P, E, O) * 0.3 + 0.1
    raw[:, :, 1] = 9.0   # normalises far beyond the clip at 10
    raw[:, :, 2] = -9.0
    d_raw = torch.tensor(raw, device=gpu)
    out = torch.full((P, E, A), SENTINEL, device=gpu)
    d = Dims(P, 99, -3, O, A, K, 64, int(ln))  # N and T are ignored
    _lib.check(_lib.lib().pgm_eval_act(C.byref(d), _ptr(tb.params), _ptr(mean if use_ob else None),
                                       _ptr(var if use_ob else None), use_ob, _ptr(d_raw), E, _ptr(out), _stream()),
               'pgm_eval_act')
    got = out.cpu()
    for p in range(P):
        ob = raw[p]
        if use_ob:
            ob = np.clip((ob - rms[p].mean) / np.sqrt(rms[p].var + 1e-8), -10.0, 10.0)
            assert (np.abs(ob) == 10.0).any()
        with torch.no_grad():
            _, ra, _ = pols[p].act(torch.tensor(ob, dtype=torch.float64), deterministic=True)
        _close(got[p], ra, *band['a'], 'deterministic action')


# ------------------------------------------------------------------------------------------------ 4. host rollout
def _check_against(tb, dev, p, ro, what=''):
    """Bands of test_rollout."""
    _close(dev['obs'][p], ro.obs, 5e-5, 1e-4, 'obs' + what)
    _close(dev['actions'][p], ro.actions, 5e-5, 1e-4, 'actions' + what)
    _close(dev['logp'][p], ro.action_log_probs[..., 0], 2e-4, 1e-4, 'logp' + what)
    _close(dev['values'][p], ro.value_preds, 5e-5, 1e-4, 'values (incl. bootstrap)' + what)
    _close(dev['rewards'][p], ro.rewards, 5e-5, 1e-4, 'rewards' + what)
    np.testing.assert_array_equal(dev['masks'][p].numpy(), ro.masks[..., 0].numpy())
    np.testing.assert_array_equal(dev['bad_masks'][p].numpy(), ro.bad_masks[..., 0].numpy())


def _storage(tb):
    return {k: getattr(tb, k).cpu().clone() for k in ('obs', 'actions', 'logp', 'values', 'rewards', 'masks',
                                                      'bad_masks')}


def _host_batch(env, P, N, T, he, seed=3, **kw):
    spec = envspec.make_spec(env)
    tb = TaskBatch(env, P, num_processes=N, num_steps=T, host_env=he, **kw)
    gen = torch.Generator().manual_seed(seed + 100)
    pols = [perturb(p, 0.05, gen) for p in fp32_policies(spec, P, seed)]
    for p, pol in enumerate(pols):
        tb.set_task(p, pol.state_dict())
    return spec, tb, pols


@pytest.mark.parametrize('env,N,T,tmax,R', [('MO-Hopper-v2', 4, 48, 20, 1), ('MO-Walker2d-v2', 2, 64, None, 1),
                                            ('MO-Hopper-v3', 8, 40, None, 1), ('MO-Walker2d-v2', 2, 37, 30, 2)])
def test_host_rollout(gpu, env, N, T, tmax, R):
    """TaskBatch(host_env=SynthHostVecEnv).rollout with uploaded noise against the oracle rollout; tmax = 20 crosses
    two auto-resets inside T = 48; R = 2: two rollouts with the after_update carry (and a reset across the seam)."""
    P = 2
    he = SynthHostVecEnv(env, P, N, seed=0, max_episode_steps=tmax)
    spec, tb, pols = _host_batch(env, P, N, T, he)
    if tmax:
        spec = dict(spec, max_episode_steps=tmax)
    s0 = envspec.reset_table(spec['obs_dim'], 0, N)
    noise = torch.randn(R, T, N, spec['act_dim'], generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    with pytest.raises(PGMError, match='host-env'):
        tb.env_step(torch.zeros(P, N, spec['act_dim']))
    tb.env_reset()
    dev = []
    for r in range(R):
        tb.rollout(r, noise=noise[r].float(), carry=r > 0)
        dev.append(_storage(tb))
    for p in range(P):
        envs = VecNormalizedSynth(spec, s0, 0.995)
        ro = oppo.RolloutStorage(T, N, spec['obs_dim'], spec['act_dim'], spec['obj_num'])
        ro.obs[0].copy_(torch.from_numpy(envs.reset()).double())
        for r in range(R):
            if r > 0:
                ro.after_update()
            _oracle_rollout(pols[p], envs, ro, noise[r].float().double())
            _check_against(tb, dev[r], p, ro, f' (rollout {r})')
        if tmax:
            assert (ro.masks == 0).any()
        _close(tb.obj_var[p].cpu(), envs.obj_rms.var, 0, 1e-6, 'obj_rms.var')
        _close(tb.ob_var[p].cpu(), envs.ob_rms.var, 1e-9, 1e-6, 'ob_rms.var')


class _Box:
    def __init__(self, n):
        self.shape = (n,)


class _OracleGymEnv(SynthEnv):
    """The oracle's SynthEnv as a gym-style object (old step API): what GymHostVecEnv wraps."""

    def __init__(self, spec, s0):
        super().__init__(spec, s0)
        self.action_space, self.obj_dim = _Box(spec['act_dim']), spec['obj_num']


def test_host_rollout_humanoid_teacher_forced(gpu):
    """Humanoid N = 8, T = 40, teacher-forced as the fused Humanoid rollout test is: the host envs ARE the oracle's
    SynthEnv objects (through GymHostVecEnv), so the device is fed the oracle's transitions for its own actions and
    each step's policy and VecNormalize transition is compared on its own (_teacher_forced_check)."""
    env, P, N, T = 'MO-Humanoid-v2', 2, 8, 40
    spec = envspec.make_spec(env)
    he = GymHostVecEnv(lambda name, seed, rank: _OracleGymEnv(spec, envspec.reset_state(spec['obs_dim'], seed + rank)),
                       env, P, N, seed=0)
    _, tb, pols = _host_batch(env, P, N, T, he)
    s0 = envspec.reset_table(spec['obs_dim'], 0, N)
    noise = torch.randn(T, N, spec['act_dim'], generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    tb.env_reset()
    tb.rollout(0, noise=noise.float(), carry=False)
    for p in range(P):
        _teacher_forced_check(tb, p, pols[p], spec, s0, noise)
    he.close()


# ------------------------------------------------------------------------------------------------ 5. true terminals
# Hopper-v2, N = 4, T = 48, time limit 20: an episode also ends, as a TRUE terminal (done without bad_transition), when
# objective TERM_K of the step drops below TERM_THR.  Seed and threshold were chosen on the CPU from the oracle alone
# (the smallest seed, then the threshold on a 0.05 grid, at which every task's fp64 run has >= 3 true terminals and
# >= 1 time-limit end, the fp32 arm of the oracle takes the same decisions, and no objective comes within TERM_MARGIN
# of the threshold); test_true_termination re-asserts all of that before it looks at the device.
TERM_ENV, TERM_N, TERM_T, TERM_TMAX = 'MO-Hopper-v2', 4, 48, 20
# Result: seed 0, threshold 0.05 -- task 0 has 11 true terminals and 4 time-limit ends, task 1 has 3 and 6; the nearest
# objective stays 4.0e-3 from the threshold in both arms.
TERM_SEED, TERM_K, TERM_THR, TERM_MARGIN = 0, 1, 0.05, 1e-3


class _TermSynthEnv(SynthEnv):
    def step(self, a):
        o, r, done, info = super().step(a)
        self.last_obj = info['obj'][TERM_K]
        if self.last_obj < TERM_THR:  # a true terminal state takes precedence over the time limit
            info.pop('bad_transition', None)
            done = True
        return o, r, done, info


class _TermHostEnv(SynthHostVecEnv):
    def terminal(self, s, obj):
        return obj[..., TERM_K] < TERM_THR


def _term_policies(P):
    spec = envspec.make_spec(TERM_ENV)
    gen = torch.Generator().manual_seed(TERM_SEED + 100)
    return [perturb(p, 0.05, gen) for p in fp32_policies(spec, P, TERM_SEED)]


def _term_oracle(pol, noise, net=torch.float64):
    """The oracle rollout over _TermSynthEnv objects; net = float32: the oracle's fp32 arm (policy in fp32, envs and
    statistics fp64).  Returns (storage, envs, smallest |objective - threshold| seen)."""
    spec = dict(envspec.make_spec(TERM_ENV), max_episode_steps=TERM_TMAX)
    s0 = envspec.reset_table(spec['obs_dim'], 0, TERM_N)
    envs = VecNormalizedSynth(spec, s0, 0.995)
    envs.envs = [_TermSynthEnv(spec, x) for x in s0]
    ro = oppo.RolloutStorage(TERM_T, TERM_N, spec['obs_dim'], spec['act_dim'], spec['obj_num'])
    ro.obs[0].copy_(torch.from_numpy(envs.reset()).double())
    pol = copy.deepcopy(pol).to(net)
    margin = np.inf
    for t in range(TERM_T):
        with torch.no_grad():
            value, action, logp = (x.double() for x in pol.act(ro.obs[t].to(net), noise=noise[t]))
        obs, dones, infos = envs.step(action.numpy())
        margin = min(margin, min(abs(e.last_obj - TERM_THR) for e in envs.envs))
        obj = torch.tensor(np.stack([i['obj'] for i in infos]), dtype=torch.float64)
        masks = torch.tensor([[0.0] if d else [1.0] for d in dones], dtype=torch.float64)
        bad = torch.tensor([[0.0] if 'bad_transition' in i else [1.0] for i in infos], dtype=torch.float64)
        ro.insert(torch.from_numpy(obs).double(), action, logp, value, obj, masks, bad)
    with torch.no_grad():
        ro.value_preds[-1] = pol.get_value(ro.obs[-1].to(net)).double()
    return ro, envs, margin


def _term_noise():
    A = envspec.make_spec(TERM_ENV)['act_dim']
    return torch.randn(TERM_T, TERM_N, A, generator=torch.Generator().manual_seed(TERM_SEED + 4),
                       dtype=torch.float64).float().double()


def test_true_termination(gpu):
    """done without bad_transition from a rollout: masks = 0, bad_masks = 1, the GAE branch SynthMO's fixed-length
    episodes never feed.  masks / bad_masks exact, the rest in the bands of test_rollout, gae() on the device's storage
    against the oracle's compute_returns in the band of test_gae."""
    P, N, T = 2, TERM_N, TERM_T
    pols = _term_policies(P)
    noise = _term_noise()
    refs = []
    for p in range(P):
        ro, envs, margin = _term_oracle(pols[p], noise)
        ro32, _, margin32 = _term_oracle(pols[p], noise, torch.float32)
        m, b = ro.masks[1:, :, 0], ro.bad_masks[1:, :, 0]
        assert int(((m == 0) & (b == 1)).sum()) >= 3, 'true terminals in the oracle run'
        assert int(((m == 0) & (b == 0)).sum()) >= 1, 'time-limit ends in the oracle run'
        assert torch.equal(ro.masks, ro32.masks) and torch.equal(ro.bad_masks, ro32.bad_masks), 'fp32-arm decisions'
        assert min(margin, margin32) > TERM_MARGIN
        refs.append((ro, envs))
    he = _TermHostEnv(TERM_ENV, P, N, seed=0, max_episode_steps=TERM_TMAX)
    tb = TaskBatch(TERM_ENV, P, num_processes=N, num_steps=T, host_env=he, gamma=0.995, gae_lambda=0.95)
    for p, pol in enumerate(pols):
        tb.set_task(p, pol.state_dict())
    tb.env_reset()
    tb.rollout(0, noise=noise.float(), carry=False)
    tb.gae()
    dev = _storage(tb)
    got = tb.returns.cpu().numpy()
    for p in range(P):
        ro, envs = refs[p]
        _check_against(tb, dev, p, ro)
        _close(tb.obj_var[p].cpu(), envs.obj_rms.var, 0, 1e-6, 'obj_rms.var')
        _close(tb.ob_var[p].cpu(), envs.ob_rms.var, 1e-9, 1e-6, 'ob_rms.var')
        r, v = dev['rewards'][p].double(), dev['values'][p].double()
        m, b = dev['masks'][p].double().unsqueeze(-1), dev['bad_masks'][p].double().unsqueeze(-1)
        ret = torch.zeros(T + 1, N, r.shape[-1], dtype=torch.float64)
        oppo.compute_returns_inplace(r, v.clone(), m, b, ret, v[-1], True, 0.995, 0.95, True)
        _close(got[p, :T], ret[:T].numpy(), 1e-5, 1e-5, 'returns')


# ------------------------------------------------------------------------------------------------ 6. MOPG iterations
# The policy-init seed: the first, counting up from test_mopg_iterations_end_to_end's 0, at which the oracle's own
# fp32 arm (oracle.mopg.NET = float32) stays inside the eval band of both iterations of both tasks on the CPU.
# Seed 0 was taken: its fp32 arm is within 1e-5 of the fp64 objectives (~480, ~525), the band being 5e-2.
E2E_SEED = 0


def test_host_mopg_iterations_end_to_end(gpu):
    """Two host-stepped MOPG iterations (host rollout, GAE, scalarised PPO, host evaluation) against the oracle's
    mopg_worker; bands of test_mopg_iterations_end_to_end."""
    env, P, N, T, E, M, iters = 'MO-Hopper-v2', 2, 4, 32, 2, 4, 2
    args = small_args(env, num_steps=T, num_processes=N, ppo_epoch=E, num_mini_batch=M, num_env_steps=T * N * 10)
    spec = envspec.make_spec(env)
    A, B = spec['act_dim'], T * N
    he = SynthHostVecEnv(env, P, N, seed=0)
    tb = TaskBatch(env, P, num_processes=N, num_steps=T, ppo_epoch=E, num_mini_batch=M, host_env=he)
    fn = _noise_fn(T, N, A, E, B)
    w = weights_grid(spec['obj_num'], P)
    torch.manual_seed(E2E_SEED)
    samples = [initial_sample(args, spec) for _ in range(P)]
    for s in samples:
        with torch.no_grad():
            for prm in s.actor_critic.parameters():
                prm.copy_(prm.float().double())
    for p, s in enumerate(samples):
        tb.set_task(p, s.actor_critic.state_dict(), {}, s.env_params, w[p])
    tb.env_reset()
    total = int(args.num_env_steps) // T // N
    gpu_objs, gpu_params = [], []
    for j in range(iters):
        noise, perms = fn(j)
        tb.iteration(j, oppo.linear_lr(j, total, args.lr), noise=noise.float(), perms=torch.stack(perms).numpy(),
                     carry=j > 0, overlap_eval=True)  # (ignored in host-env mode: the evaluation follows the update)
        gpu_objs.append(tb.objs.cpu().numpy().copy())
        gpu_params.append(tb.params.cpu().numpy().copy())
    tb.check_update()
    s0_train = envspec.reset_table(spec['obs_dim'], 0, N)
    s0_eval = envspec.reset_table(spec['obs_dim'], 0, 1)
    for p in range(P):
        offs = mopg_worker(args, spec, s0_train, s0_eval, samples[p], w[p], 0, iters, noise_fn=fn)
        for j, off in enumerate(offs):
            ref = tb.layout.flatten(off.actor_critic.state_dict(), dtype=np.float64)
            _close(gpu_params[j][p], ref, 2e-5, 1e-4, f'params iter {j}')
            _close(gpu_objs[j][p], off.objs, 1e-3, 1e-4, f'eval objs iter {j}')


# ------------------------------------------------------------------------------------------------ 7. the CLI
def _cli_run(save, extra):
    from pgmorl_amd.run import main
    T, N = 32, 2
    argv = ['--env-name', 'MO-Hopper-v2', '--obj-num', '2', '--num-steps', str(T), '--num-processes', str(N),
            '--ppo-epoch', '1', '--num-mini-batch', '2', '--num-env-steps', str(T * N * 4), '--warmup-iter', '2',
            '--update-iter', '1', '--delta-weight', '0.5', '--selection-method', 'prediction-guided', '--save-dir',
            str(save), '--rl-log-interval', '1', '--rng', 'host', '--pbuffer-num', '100'] + extra
    prev = torch.get_default_dtype()
    try:
        main(argv)
    finally:
        torch.set_default_dtype(prev)


def test_cli_host_env_synth(gpu, tmp_path, capsys):
    """pgmorl_amd.run --host-env synth (warm-up of 2 iterations + 2 generations, T = 32): the full results tree and
    final/ are written, and the warm-up offspring objectives equal those of the same run on the device envs within
    twice the eval band (each run stands within one band of the same oracle)."""
    _cli_run(tmp_path / 'host', ['--host-env', 'synth'])
    _cli_run(tmp_path / 'dev', [])
    capsys.readouterr()
    for it in ('2', '3', '4'):
        for f in ('ep/objs.txt', 'population/objs.txt', 'population/optgraph.txt', 'elites/elites.txt',
                  'elites/weights.txt', 'elites/offsprings.txt'):
            assert os.path.exists(tmp_path / 'host' / it / f), f'{it}/{f}'
    for f in ('args.txt', 'log.txt', 'timing.json', 'final/objs.txt', 'final/EP_policy_0.pt'):
        assert os.path.exists(tmp_path / 'host' / f), f
    assert '--host-env' in open(tmp_path / 'host' / 'args.txt').read()
    final = np.loadtxt(tmp_path / 'host' / 'final' / 'objs.txt', delimiter=',', ndmin=2)
    assert final.shape[1] == 2 and np.isfinite(final).all()
    host = np.loadtxt(tmp_path / 'host' / '2' / 'elites' / 'offsprings.txt', delimiter=',', ndmin=2)
    dev = np.loadtxt(tmp_path / 'dev' / '2' / 'elites' / 'offsprings.txt', delimiter=',', ndmin=2)
    assert host.shape == dev.shape and host.shape[0] >= 4
    _close(host, dev, 2e-3, 2e-4, 'warm-up offspring objectives, host envs vs device envs')
