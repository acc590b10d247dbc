"""The fused SynthMO rollout, env-step and evaluation kernels on the branches a plain command line takes and the rest of
the suite never does: ob_rms / obj_rms switched off, the +-10 observation and reward clips firing, gamma != 0.995.

Every case compares the device (fp32) with the CPU oracle (fp64) given the same flags, gamma and preloaded statistics, in
the bands tests/test_gpu_kernels.py uses for the same quantities.  "Off" is also checked on the state: the statistics of a
switched-off normaliser hold recognisable values (SENT) before env_reset and must hold the same bits after every launch,
while the observations / rewards equal the oracle's raw ones: the kernels neither update nor read them.  ret_rms is
updated in every combination (vec_normalize.py:41) and compared in every rollout case.

That a case can fail is asserted on the oracle alone, before the device is looked at: flags off and flags on differ by
more than 0.1 (a thousand tolerances), the preloaded narrow ob_rms clips a tenth of the observations at each bound and
leaves a third inside, the reward clip fires, gamma changes obj_rms.var.

Kernels.  'auto' is the launcher's choice: the lane kernel (obs_dim <= 48, N in 1 / 2 / 4 / 8), the wide kernel
(Humanoid, the same N), the wave / wide evaluation; N = 6 is the block kernel's under either name.  'block' forces the
block rollout / evaluation kernel.  Humanoid rollouts use the teacher-forced check (see test_rollout)."""
import functools

import numpy as np
import pytest
import torch

from oracle import ppo as oppo
from oracle.mopg import evaluation as oracle_evaluation
from oracle.mopg import initial_sample, mopg_worker
from oracle.vecenv import RunningMeanStd, VecNormalizedSynth
from pgmorl_amd import envspec
from pgmorl_amd.runtime import TaskBatch

from . import test_gpu_runs as runs
from .helpers import fp32_policies, perturb, small_args, weights_grid
from .test_gpu_kernels import _close, _noise_fn, _oracle_rollout, _teacher_forced_check

pytestmark = pytest.mark.gpu

P = 2
WALKER, HOPPER2, HOPPER3, HUMANOID = 'MO-Walker2d-v2', 'MO-Hopper-v2', 'MO-Hopper-v3', 'MO-Humanoid-v2'
FF, FT, TF, TT = (False, False), (False, True), (True, False), (True, True)
KERNELS = ['auto', 'block']
# what a switched-off RunningMeanStd holds on the device: nothing a kernel would write, nothing it could read unnoticed
SENT = {'mean': 0.37, 'var': 2.5, 'count': 123.0}


# ------------------------------------------------------------------------------------------------ shared inputs
def _spec(env, steps=None):
    """The env's spec, its time limit cut to `steps` (a spec field; the device's copy is tb.c_spec.max_episode_steps)."""
    spec = envspec.make_spec(env)
    return spec if steps is None else dict(spec, max_episode_steps=steps)


@functools.lru_cache(maxsize=None)
def _pols(env, seed=3, scale=0.05):
    gen = torch.Generator().manual_seed(seed + 100)
    return tuple(perturb(pol, scale, gen) for pol in fp32_policies(envspec.make_spec(env), P, seed))


def _noise(spec, N, T, seed=4):
    return torch.randn(T, N, spec['act_dim'], generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _narrow_rms(O):
    """An ob_rms that clips on purpose: std 0.01 on the even features (a 100x gain on states in (-1, 1)), 1 on the odd
    ones, the mean +-0.05 in pairs; count 1e6, so the rollout's own updates leave it there."""
    r = RunningMeanStd(shape=(O,))
    f = np.arange(O)
    r.mean = np.where(f % 4 < 2, 0.05, -0.05)
    r.var = np.where(f % 2 == 0, 1e-4, 1.0)
    r.count = 1e6
    return r


@functools.lru_cache(maxsize=None)
def _oracle(env, N, T, ob_rms=True, obj_rms=True, gamma=0.995, steps=None, preload=False, seeds=(3, 4)):
    """The free-running oracle rollout of every task -> [(storage, env)]; computed once per case, shared by the kernels
    and the cases that compare two settings, and only read.  seeds: of the policies and of the action noise."""
    spec = _spec(env, steps)
    s0 = envspec.reset_table(spec['obs_dim'], 0, N)
    noise = _noise(spec, N, T, seeds[1]).float().double()
    out = []
    for pol in _pols(env, seeds[0]):
        envs = VecNormalizedSynth(spec, s0, gamma, ob_rms, obj_rms)
        if preload:
            envs.ob_rms = _narrow_rms(spec['obs_dim'])
        ro = oppo.RolloutStorage(T, N, spec['obs_dim'], spec['act_dim'], spec['obj_num'])
        ro.obs[0].copy_(torch.from_numpy(envs.reset()).double())
        _oracle_rollout(pol, envs, ro, noise)
        out.append((ro, envs))
    return out


def _kernel(monkeypatch, kernel):
    if kernel == 'block':
        monkeypatch.setenv('PGM_ROLLOUT_KERNEL', 'block')
        monkeypatch.setenv('PGM_EVAL_KERNEL', 'block')


def _batch(env, pols, N, T, steps=None, **kw):
    tb = TaskBatch(env, len(pols), num_processes=N, num_steps=T, **kw)
    if steps is not None:
        tb.spec = _spec(env, steps)
        tb.c_spec.max_episode_steps = steps
    for p, pol in enumerate(pols):
        tb.set_task(p, pol.state_dict())
    return tb


def _plant(tb, ob_rms, obj_rms):
    """SENT into the statistics that are switched off -> {tensor name: its bits}."""
    kept = {}
    for on, pre in ((ob_rms, 'ob'), (obj_rms, 'obj')):
        if not on:
            for k, v in SENT.items():
                getattr(tb, f'{pre}_{k}').fill_(v)
                kept[f'{pre}_{k}'] = getattr(tb, f'{pre}_{k}').clone()
    return kept


def _assert_kept(tb, kept, when):
    for name, bits in kept.items():
        assert torch.equal(getattr(tb, name), bits), f'{name} is switched off and was written {when}'


def _check_ret_rms(tb, p, envs):
    _close(tb.ret_mean[p].cpu(), envs.ret_rms.mean, 0, 1e-6, 'ret_rms.mean')
    _close(tb.ret_var[p].cpu(), envs.ret_rms.var, 0, 1e-6, 'ret_rms.var')
    assert float(tb.ret_count[p]) == pytest.approx(envs.ret_rms.count, rel=1e-12)


def _check_storage(dev, p, ro, what=''):
    """test_rollout's comparison of the rollout storage of task p (dev: the batch, or a dict of its tensors)."""
    get = dev.get if isinstance(dev, dict) else lambda k: getattr(dev, k).cpu()
    _close(get('obs')[p], ro.obs, 5e-5, 1e-4, 'obs' + what)
    _close(get('actions')[p], ro.actions, 5e-5, 1e-4, 'actions' + what)
    _close(get('logp')[p], ro.action_log_probs[..., 0], 2e-4, 1e-4, 'logp' + what)
    _close(get('values')[p], ro.value_preds, 5e-5, 1e-4, 'values (incl. bootstrap)' + what)
    _close(get('rewards')[p], ro.rewards, 5e-5, 1e-4, 'rewards' + what)
    np.testing.assert_array_equal(get('masks')[p].numpy(), ro.masks[..., 0].numpy())
    np.testing.assert_array_equal(get('bad_masks')[p].numpy(), ro.bad_masks[..., 0].numpy())


def _rollout_case(monkeypatch, kernel, env, N, T, ob_rms=True, obj_rms=True, gamma=0.995, steps=None, preload=False,
                  forced=False, seeds=(3, 4)):
    """env_reset + one rollout against the oracle with the same flags, gamma, time limit and preloaded ob_rms; the
    switched-off statistics keep SENT, ret_rms matches.  forced (always for Humanoid): the teacher-forced check."""
    _kernel(monkeypatch, kernel)
    spec, pols = _spec(env, steps), _pols(env, seeds[0])
    tb = _batch(env, pols, N, T, steps, ob_rms=ob_rms, obj_rms=obj_rms, gamma=gamma)
    kept = _plant(tb, ob_rms, obj_rms)
    stats = {'ob_rms': _narrow_rms(spec['obs_dim'])} if preload else {}
    for p in range(P):
        tb.set_env_params(p, stats)
    noise = _noise(spec, N, T, seeds[1])
    tb.env_reset()
    _assert_kept(tb, kept, 'by env_reset')
    tb.rollout(0, noise=noise.float(), carry=False)
    _assert_kept(tb, kept, 'by the rollout')
    s0 = envspec.reset_table(spec['obs_dim'], 0, N)
    for p in range(P):
        if forced or spec['obs_dim'] > 48:
            envs = _teacher_forced_check(tb, p, pols[p], spec, s0, noise, gamma, ob_rms, obj_rms, stats)
        else:
            ro, envs = _oracle(env, N, T, ob_rms, obj_rms, gamma, steps, preload, seeds)[p]
            _check_storage(tb, p, ro)
            if obj_rms:
                _close(tb.obj_var[p].cpu(), envs.obj_rms.var, 0, 1e-6, 'obj_rms.var')
            if ob_rms:
                _close(tb.ob_var[p].cpu(), envs.ob_rms.var, 1e-9, 1e-6, 'ob_rms.var')
        _check_ret_rms(tb, p, envs)


# ------------------------------------------------------------------------------------------------ A: flags off
# (env, N, T, time limit (None: the env's), the flag combinations): Walker 4 x 40 the baseline; Hopper-v3 K = 3 at N = 6
# (the block kernel, N no power of two) and at N = 8 (the lane kernel with two env slots per wave); Walker N = 1: one
# wave per role; the 12-step limit: two auto-resets to raw observations; T = 3 ends inside the reward drain; Humanoid
# N = 8: the wide kernel's split-half feature slot, N = 2: its small-N merge, the 5-step limit: its auto-reset
OFF_SHAPES = [(WALKER, 4, 40, None, (FF, FT, TF)), (HOPPER3, 6, 24, None, (FF,)), (HOPPER3, 8, 24, None, (FF,)),
              (WALKER, 1, 33, None, (FT, TF)), (WALKER, 2, 30, 12, (FF,)), (HOPPER2, 8, 3, None, (FF,)),
              (HUMANOID, 8, 24, None, (FF, FT, TF)), (HUMANOID, 2, 20, None, (FF,)), (HUMANOID, 4, 12, 5, (FF,))]
OFF_CASES = [(env, N, T, steps, ob, obj) for env, N, T, steps, flags in OFF_SHAPES for ob, obj in flags]


def _assert_flags_matter(env, N, T, ob_rms, obj_rms, steps):
    """Oracle alone: this case's observations (ob_rms off) and rewards are not what both flags on give."""
    off = _oracle(env, N, T, ob_rms, obj_rms, 0.995, steps)
    on = _oracle(env, N, T, True, True, 0.995, steps)
    for (ro, _), (ro_on, _) in zip(off, on):
        if not ob_rms:  # (with ob_rms on in both, obj_rms cannot reach the observations: the policy never sees a reward)
            assert float((ro.obs - ro_on.obs).abs().max()) > 0.1
        assert float((ro.rewards - ro_on.rewards).abs().max()) > 0.1
        if steps is not None:  # the lowered limit is crossed, twice where T allows
            assert int((ro.masks == 0).sum()) == N * (T // steps) and T // steps >= 2


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('env,N,T,steps,ob_rms,obj_rms', OFF_CASES)
def test_rollout_flags_off(gpu, monkeypatch, env, N, T, steps, ob_rms, obj_rms, kernel):
    _assert_flags_matter(env, N, T, ob_rms, obj_rms, steps)
    _rollout_case(monkeypatch, kernel, env, N, T, ob_rms, obj_rms, steps=steps)


def test_rollout_carry_short_flags_off(gpu):
    """test_rollout_carry_short's scheme (4 consecutive rollouts with the after_update carry) at Walker N = 4, T = 2 with
    both flags off: the switched-off statistics cross every launch boundary and the drain untouched."""
    env, N, T, R = WALKER, 4, 2, 4
    spec, pols = _spec(env), _pols(env, 9)
    tb = _batch(env, pols, N, T, ob_rms=False, obj_rms=False)
    kept = _plant(tb, False, False)
    s0 = envspec.reset_table(spec['obs_dim'], 0, N)
    noise = torch.randn(R, T, N, spec['act_dim'], generator=torch.Generator().manual_seed(10), dtype=torch.float64)
    tb.env_reset()
    dev = []
    for r in range(R):
        tb.rollout(r, noise=noise[r].float(), carry=r > 0)
        _assert_kept(tb, kept, f'by rollout {r}')
        dev.append({k: getattr(tb, k).cpu().clone() for k in ('obs', 'actions', 'logp', 'values', 'rewards', 'masks',
                                                                'bad_masks')})
    for p in range(P):
        envs = VecNormalizedSynth(spec, s0, 0.995, False, False)
        ro = oppo.RolloutStorage(T, N, spec['obs_dim'], spec['act_dim'], spec['obj_num'])
        ro.obs[0].copy_(torch.from_numpy(envs.reset()).double())
        for r in range(R):
            if r > 0:
                ro.after_update()
            _oracle_rollout(pols[p], envs, ro, noise[r].float().double())
            _check_storage(dev[r], p, ro, f' (rollout {r})')
        assert float(ro.obs.abs().max()) < 1.0  # raw states: tanh's range
        _check_ret_rms(tb, p, envs)


# ------------------------------------------------------------------------------------------------ B: env_reset / env_step
@pytest.mark.parametrize('ob_rms,obj_rms', [FF, FT, TF])
def test_env_reset_step_flags_off(gpu, ob_rms, obj_rms):
    """test_env_reset_step_vecnormalize (its bands) at Hopper-v2 N = 4 with a flag off: reset + 60 steps under a 25-step
    time limit, so env_kernel's auto-reset is crossed twice."""
    env, N, steps, limit = HOPPER2, 4, 60, 25
    spec = _spec(env, limit)
    tb = TaskBatch(env, P, num_processes=N, num_steps=4, ob_rms=ob_rms, obj_rms=obj_rms)
    tb.c_spec.max_episode_steps = limit
    kept = _plant(tb, ob_rms, obj_rms)
    s0 = envspec.reset_table(spec['obs_dim'], 0, N)
    ref = [VecNormalizedSynth(spec, s0, 0.995, ob_rms, obj_rms) for _ in range(P)]
    o_gpu = tb.env_reset().cpu().numpy()
    _assert_kept(tb, kept, 'by env_reset')
    for p in range(P):
        _close(o_gpu[p], ref[p].reset(), 1e-6, 1e-6, 'reset obs')
    rng = np.random.RandomState(3)
    resets = 0
    for t in range(steps):
        act = (rng.randn(P, N, spec['act_dim']) * 0.7).astype(np.float32)
        obs, rew, m, b = (x.cpu().numpy() for x in tb.env_step(torch.from_numpy(act).to(gpu)))
        for p in range(P):
            ro, rd, infos = ref[p].step(act[p].astype(np.float64))
            resets += int(rd.sum())
            _close(obs[p], ro, 2e-6, 2e-6, f'obs step {t}')
            _close(rew[p], np.stack([i['obj'] for i in infos]), 1e-5, 1e-6, f'reward step {t}')
            np.testing.assert_array_equal(m[p], np.where(rd, 0.0, 1.0))
            np.testing.assert_array_equal(b[p], [0.0 if 'bad_transition' in i else 1.0 for i in infos])
    assert resets == 2 * N * P
    _assert_kept(tb, kept, 'by env_step')
    for p in range(P):
        if ob_rms:
            _close(tb.ob_mean[p].cpu(), ref[p].ob_rms.mean, 0, 1e-9, 'ob_rms.mean')
            _close(tb.ob_var[p].cpu(), ref[p].ob_rms.var, 0, 1e-9, 'ob_rms.var')
            assert float(tb.ob_count[p]) == pytest.approx(ref[p].ob_rms.count, rel=1e-12)
        if obj_rms:
            _close(tb.obj_mean[p].cpu(), ref[p].obj_rms.mean, 0, 1e-9, 'obj_rms.mean')
            _close(tb.obj_var[p].cpu(), ref[p].obj_rms.var, 0, 1e-9, 'obj_rms.var')
            assert float(tb.obj_count[p]) == pytest.approx(ref[p].obj_rms.count, rel=1e-12)
        _check_ret_rms(tb, p, ref[p])


# ------------------------------------------------------------------------------------------------ C: the clips
# (Hopper-v3 N = 8 beside the N = 6 of the block kernel: the lane kernel's clip with two env slots per wave)
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('env,N,T', [(WALKER, 4, 40), (HOPPER3, 6, 24), (HOPPER3, 8, 24), (HUMANOID, 8, 24),
                                     (HUMANOID, 2, 20)])
def test_rollout_observation_clip(gpu, monkeypatch, env, N, T, kernel):
    """Both flags on and _narrow_rms preloaded on both sides: the observation clip produces both bounds and passes the
    values between them.  Teacher-forced for every env: the narrow features' 100x gain amplifies fp32 rounding in a
    free-running comparison.  (An element the oracle leaves within 1e-3 of a bound needs no exclusion: a flipped clip
    decision moves it by less than the band at |ref| = 10.)"""
    for ro, _ in _oracle(env, N, T, preload=True):
        hi, lo = float((ro.obs == 10.0).double().mean()), float((ro.obs == -10.0).double().mean())
        inside = float((ro.obs.abs() < 10.0).double().mean())
        assert hi >= 0.10 and lo >= 0.10 and inside >= 0.30, (hi, lo, inside)
    _rollout_case(monkeypatch, kernel, env, N, T, preload=True, forced=True)


@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('env,N,T,low', [(HOPPER3, 1, 24, False), (HUMANOID, 2, 20, True)])
def test_rollout_reward_clip(gpu, monkeypatch, env, N, T, low, kernel):
    """Fresh statistics at N <= 2: obj_rms.var starts from one or two envs' accumulators, and every task's first rewards
    clip at +10 (Humanoid: at -10 too; policy seed 0 and noise seed 5, under which its oracle does both)."""
    seeds = (0, 5)
    for ro, _ in _oracle(env, N, T, seeds=seeds):
        assert int((ro.rewards == 10.0).sum()) >= 1 and (not low or int((ro.rewards == -10.0).sum()) >= 1)
        assert int((ro.rewards.abs() < 10.0).sum()) >= 1
    _rollout_case(monkeypatch, kernel, env, N, T, seeds=seeds)


# ------------------------------------------------------------------------------------------------ D: gamma
@pytest.mark.parametrize('kernel', KERNELS)
@pytest.mark.parametrize('env,N,T', [(WALKER, 4, 40), (HUMANOID, 4, 20)])
def test_rollout_gamma(gpu, monkeypatch, env, N, T, kernel):
    """gamma = 0.9 in the discounted objective / return accumulators: obj_rms.var is a fraction of its value at 0.995, so
    a kernel that ignored NormState.gamma misses the rtol 1e-6 check on it (and the rewards scaled by it)."""
    for (_, e9), (_, e995) in zip(_oracle(env, N, T, gamma=0.9), _oracle(env, N, T)):
        assert (e9.obj_rms.var < 0.5 * e995.obj_rms.var).all(), (e9.obj_rms.var, e995.obj_rms.var)
    _rollout_case(monkeypatch, kernel, env, N, T, gamma=0.9)


def _eval_stats(O):
    """test_eval's per-task ob_rms."""
    rng = np.random.RandomState(2)
    out = []
    for _ in range(P):
        r = RunningMeanStd(shape=(O,))
        r.update(rng.randn(50, O) * 0.3 + 0.1)
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_eval(env, p, eval_num, raw, ob, gamma=0.995, steps=None):
    """oracle.mopg.evaluation of task p's evaluation policy; ob: 'off', 'sent' (ob_rms on, holding SENT) or 'stats'."""
    spec = _spec(env, steps)
    args = small_args(env, eval_num=eval_num, raw=raw, gamma=gamma, ob_rms=ob != 'off')
    rms = None
    if ob == 'sent':
        rms = RunningMeanStd(shape=(spec['obs_dim'],))
        rms.mean, rms.var = rms.mean + SENT['mean'], rms.var * SENT['var']
    elif ob == 'stats':
        rms = _eval_stats(spec['obs_dim'])[p]
    s0 = envspec.reset_table(spec['obs_dim'], 0, eval_num)
    return oracle_evaluation(args, spec, s0, _pols(env, 5, 0.1)[p], rms)


@pytest.mark.parametrize('kernel', ['waves', 'block'])
def test_eval_gamma(gpu, monkeypatch, kernel):
    """raw=False: the evaluation's discount is the batch's gamma (0.9 here), not 0.995."""
    monkeypatch.setenv('PGM_EVAL_KERNEL', kernel)
    env, eval_num = HOPPER3, 2
    spec, pols = _spec(env), _pols(env, 5, 0.1)
    tb = _batch(env, pols, 4, 8, eval_num=eval_num, raw=False, gamma=0.9)
    for p, r in enumerate(_eval_stats(spec['obs_dim'])):
        tb.set_env_params(p, {'ob_rms': r})
    objs = tb.evaluate().cpu().numpy()
    for p in range(P):
        ref = _oracle_eval(env, p, eval_num, False, 'stats', 0.9)
        other = _oracle_eval(env, p, eval_num, False, 'stats', 0.995)
        assert (np.abs(other - ref) > 100 * (1e-4 + 1e-5 * np.abs(ref))).all(), (ref, other)
        _close(objs[p], ref, 1e-4, 1e-5, 'evaluation objs')


# ------------------------------------------------------------------------------------------------ E: evaluation, ob_rms off
def _eval_off_case(monkeypatch, kernel, env, eval_num, raw, steps, atol, rtol):
    monkeypatch.setenv('PGM_EVAL_KERNEL', kernel)
    pols = _pols(env, 5, 0.1)
    tb = _batch(env, pols, 4, 8, steps, eval_num=eval_num, raw=raw, ob_rms=False)
    kept = _plant(tb, False, True)
    # oracle alone (task 0's first episode): an evaluation that read the planted statistics would be far outside the band
    ref0, read0 = (_oracle_eval(env, 0, 1, raw, ob, 0.995, steps) for ob in ('off', 'sent'))
    assert (np.abs(read0 - ref0) > 100 * (atol + rtol * np.abs(ref0))).any(), (ref0, read0)
    objs = tb.evaluate().cpu().numpy()
    _assert_kept(tb, kept, 'by the evaluation')
    for p in range(P):
        _close(objs[p], _oracle_eval(env, p, eval_num, raw, 'off', 0.995, steps), atol, rtol, f'{kernel} task {p}')


@pytest.mark.parametrize('kernel', ['waves', 'block'])
@pytest.mark.parametrize('raw', [True, False])
@pytest.mark.parametrize('env,eval_num', [(WALKER, 1), (HOPPER2, 11)])
def test_eval_ob_rms_off(gpu, monkeypatch, env, eval_num, raw, kernel):
    """TaskBatch(ob_rms=False): the policy sees the raw state (cast to fp32), whatever ob_mean / ob_var hold."""
    _eval_off_case(monkeypatch, kernel, env, eval_num, raw, None, 1e-4, 1e-5)


@pytest.mark.parametrize('kernel', ['wide', 'block'])
@pytest.mark.parametrize('eval_num,raw', [(1, True), (6, False)])
def test_eval_wide_ob_rms_off(gpu, monkeypatch, eval_num, raw, kernel):
    """Humanoid, episodes cut to 12 steps on both sides and test_eval_wide's band (see there)."""
    _eval_off_case(monkeypatch, kernel, HUMANOID, eval_num, raw, 12, 1e-3, 2e-4)


# ------------------------------------------------------------------------------------------------ F: end to end, grouped
def test_mopg_iterations_flags_off(gpu):
    """test_mopg_iterations_end_to_end (its shapes and bands) with ob_rms=False, obj_rms=False on both sides: the
    advantages are normalised with no variance behind a real flags-off rollout, iteration() carries the raw
    observations, and the env_params a task exports hold None for the switched-off statistics."""
    from pgmorl_amd.mopg import MOPGPopulation
    env, N, T, E, M, iters = HOPPER2, 4, 64, 2, 4, 2
    args = small_args(env, num_steps=T, num_processes=N, ppo_epoch=E, num_mini_batch=M, num_env_steps=T * N * 10,
                      ob_rms=False, obj_rms=False)
    spec = envspec.make_spec(env)
    A, K, O, B = spec['act_dim'], spec['obj_num'], spec['obs_dim'], T * N
    tb = TaskBatch(env, P, num_processes=N, num_steps=T, ppo_epoch=E, num_mini_batch=M, ob_rms=False, obj_rms=False)
    fn = _noise_fn(T, N, A, E, B)
    w = weights_grid(K, P)
    torch.manual_seed(0)
    samples = [initial_sample(args, spec) for _ in range(P)]
    for s in samples:
        assert s.env_params['ob_rms'] is None and s.env_params['obj_rms'] is None
        with torch.no_grad():
            for prm in s.actor_critic.parameters():
                prm.copy_(prm.float().double())
    for p, s in enumerate(samples):
        tb.set_task(p, s.actor_critic.state_dict(), {}, s.env_params, w[p])
    kept = _plant(tb, False, False)
    tb.env_reset()
    total = int(args.num_env_steps) // T // N
    gpu_objs, gpu_params = [], []
    for j in range(iters):
        noise, perms = fn(j)
        tb.iteration(j, oppo.linear_lr(j, total, args.lr), noise=noise.float(), perms=torch.stack(perms).numpy(),
                     carry=j > 0)
        gpu_objs.append(tb.objs.cpu().numpy().copy())
        gpu_params.append(tb.params.cpu().numpy().copy())
    _assert_kept(tb, kept, 'by iteration()')
    rec = torch.from_numpy(tb.new_stats64()).to(gpu)  # (a buffer of the record's size)
    tb.stats64_record(rec)
    st = tb.stat_views(rec.cpu().numpy())
    pop = MOPGPopulation(args, device='cuda')
    s0_train = envspec.reset_table(O, 0, N)
    s0_eval = envspec.reset_table(O, 0, 1)
    for p in range(P):
        offs = mopg_worker(args, spec, s0_train, s0_eval, samples[p], w[p], 0, iters, noise_fn=fn)
        for j, off in enumerate(offs):
            ref = tb.layout.flatten(off.actor_critic.state_dict(), dtype=np.float64)
            _close(gpu_params[j][p], ref, 2e-5, 1e-4, f'params iter {j}')
            _close(gpu_objs[j][p], off.objs, 1e-3, 1e-4, f'eval objs iter {j}')
        ep, want = pop._env_params(st, p, O, K), offs[-1].env_params
        assert ep['ob_rms'] is None and ep['obj_rms'] is None and want['ob_rms'] is None and want['obj_rms'] is None
        _close(ep['ret_rms'].var, want['ret_rms'].var, 0, 1e-6, 'exported ret_rms.var')
        assert ep['ret_rms'].mean == want['ret_rms'].mean == 0.0
        assert ep['ret_rms'].count == pytest.approx(want['ret_rms'].count, rel=1e-12)


@pytest.mark.parametrize('env,ln,N', [(WALKER, False, 4), (HUMANOID, False, 2), (HOPPER2, True, 3)])
def test_runs_entry_points_flags_off(gpu, env, ln, N):
    """test_gpu_runs' r1 with both flags off: one run through pgm_env_reset_runs / pgm_rollout_runs / pgm_eval_runs equals
    the plain entry points bit for bit over its sequence (reset, two rollouts, evaluation), and both leave the
    switched-off statistics as reset_stats made them."""
    n_tasks, E = 3, 3
    spec, pols = runs._policies(env, ln, n_tasks)
    noise = runs._noise(spec, N)
    off = dict(ob_rms=False, obj_rms=False)
    want = runs._sequence(runs._batch(env, ln, pols, N, E, seed=7, **off), noise)
    tb = runs._batch(env, ln, pols, N, E, run_seeds=[7], **off)
    tb.set_runs([0] * n_tasks)
    got = runs._sequence(tb, noise)
    runs._assert_equal(got, want, slice(None), 'num_runs = 1, flags off')
    for stage in ('reset', 'rollout0', 'rollout1'):
        for pre in ('ob', 'obj'):
            for k, fresh in (('mean', 0.0), ('var', 1.0), ('count', 1e-4)):
                v = got[stage][f'{pre}_{k}']
                assert torch.equal(v, torch.full_like(v, fresh)), f'{stage}: {pre}_{k} is switched off and was written'
        assert float(got[stage]['obs'].abs().max()) < 1.0  # raw states: tanh's range
    assert not torch.equal(got['rollout1']['ret_var'], torch.ones_like(got['rollout1']['ret_var']))
