"""Device-resident state of P MOPG tasks on one GPU and the per-iteration kernel sequence.

One ``TaskBatch`` owns every HBM buffer of P tasks (parameters + Adam state, env state, running
statistics, rollout storage) and drives the libpgm kernels on torch's current stream:

    rollout (T steps, fused act + env + VecNormalize + insert + bootstrap value)
      -> gae -> adv_normalize -> ppo_update -> eval

i.e. one iteration of MOPG_worker's loop body (morl/mopg.py:95-155) for all tasks at once.
torch is used only for device memory and the stream; every op is a libpgm kernel and raises if
the library is unavailable (no CPU fallback).

How the env is stepped is the batch's env mode (``tb.mode``); which policy / update kernels act on the storage is its
kernel family (``tb.family``).  Returns, advantages and the statistics are the same kernels on the same storage in every
combination (the table of combinations, and where a new mode or family plugs in).

Env modes:
  * ``SynthMode``: the SynthMO device envs, pgm_env_reset / pgm_rollout / pgm_eval; with ``run_seeds`` (the tasks of
    several runs in one population) the *_runs entry points;
  * ``HostMode``: ``host_env`` (a ``hostenv.HostVecEnv``) steps the envs on the host: the rollout is a per-step loop of
    rollout_act -> host ``step`` -> env_ingest, the evaluation a host episode loop over eval_act;
  * ``DstMode``: ``device_env=True`` on Deep Sea Treasure, the one discrete-action env with a device form:
    pgm_rollout_dst / pgm_eval_dst, one launch each, the grid world stepped inside the kernels;
  * ``DummyMode``: the MO-Dummy envs (envspec.native_env_names()), device envs by default: pgm_rollout_dummy /
    pgm_eval_dummy (``host_env=hostenv.DummyMOHostVecEnv(...)`` selects HostMode instead);
  * ``PluginMode``: ``env_plugin`` (an ``envplug.EnvPlugin`` or the path of a user env header, include/pgm_envplug.h):
    pgm_envplug_rollout / pgm_envplug_eval of the plug-in's library, *_ex for a contract-2 header.
Kernel families (``FAMILIES``): 'gauss' (compiled per dim set, Gaussian head, plain or LayerNorm towers), 'cat' (the
Categorical *_cat entry points), 'any' (the runtime-dim *_any entry points, either head).
"""
import ctypes as C
import time
from collections import namedtuple

import numpy as np
import torch

from . import envplug, envspec
from ._lib import (ANY_MAX_ACT, ANY_MAX_OBJ, ANY_MAX_OBS, Dims, DstSpec, DummySpec, EnvSpec, EnvState, NormState,
                   PGMError, PPOHParams, RolloutBuf, check, launch_opts, lib, require_any_dims, require_categorical,
                   require_dst_device, require_dummy_device, require_runs, require_tasks, TASK_HPARAM_FIELDS)
from .layout import ParamLayout

F32, F64, I32 = torch.float32, torch.float64, torch.int32
LN_MAX_OBS = 32  # layernorm=True: the five envs with obs_dim <= 32 (include/pgm_abi.h pgm_dims.LN)
HOST_EVAL_MAX = 8  # pgm_eval_act and the fused evaluations: evaluation episodes per task in one launch
UPDATE_TIMEOUT_MSG = ('pgm_ppo_update: a cross-workgroup exchange timed out (workspace word 2P set); the update '
                      'kernel\'s workgroups were not co-resident -- the parameters are invalid')
ENV_NOISE_MSG = 'rollout(env_noise=...): only a contract-2 env plug-in with NW > 0 takes env noise'


# the per-task settings of set_task_hparams: pgm_task_hparams' fields in order, then the GAE lambda
TASK_FIELDS = TASK_HPARAM_FIELDS + ('gae_lambda',)


def check_task_hparam(name, values, what='set_task_hparams'):
    """The host checks of one per-task setting (the kernels trust the device tables): finite, clip_param > 0,
    max_grad_norm > 0, 0 <= gae_lambda <= 1.  Returns the values as a float64 array; PGMError naming the field."""
    if name not in TASK_FIELDS:
        raise PGMError(f'{what}: {name!r} is not a per-task setting (one of {", ".join(TASK_FIELDS)})')
    try:
        v = np.asarray(values, dtype=np.float64)
    except (TypeError, ValueError):
        raise PGMError(f'{what}: {name}={values!r} is not a number or an array of numbers') from None
    if not np.all(np.isfinite(v)):
        raise PGMError(f'{what}: {name}={np.ravel(v).tolist()} must be finite')
    if name in ('clip_param', 'max_grad_norm') and not np.all(v > 0):
        raise PGMError(f'{what}: {name}={np.ravel(v).tolist()} must be > 0')
    if name == 'gae_lambda' and not np.all((v >= 0) & (v <= 1)):
        raise PGMError(f'{what}: {name}={np.ravel(v).tolist()} must be in [0, 1]')
    return v


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(name, *args, of=None):
    """Entry point `name` of libpgm.so, or of the plug-in `of`, on the current stream (every launch ends with it)."""
    if of is None:
        check(getattr(lib(), name)(*args, _stream()), name)
    else:
        of.check(getattr(of.h, name)(*args, _stream()), name)


# ---------------------------------------------------------------------------------------------- kernel families
# The entry points of one family of policy / update kernels and what their calls look like.  head: the act, evaluation
# and update calls take the head type (0 Gaussian, 1 Categorical) after the dims; tasks: the per-task-settings update
# pgm_ppo_update_tasks (and pgm_gae_tasks) exists; opts: the update takes launch_opts and pgm_ppo_update_reset clears
# its workspace (the others reset their own, smaller one); variant: update_variant() where there is no launch choice
Family = namedtuple('Family', 'rollout_act env_ingest eval_act ppo_update workspace_bytes head tasks opts variant')


def _family(sfx, env_ingest, head=False, gauss=False, variant=None):
    return Family(f'pgm_rollout_act{sfx}', env_ingest, f'pgm_eval_act{sfx}', f'pgm_ppo_update{sfx}',
                  f'pgm_ppo_update{sfx}_workspace_bytes', head, gauss, gauss, variant)


FAMILIES = {'gauss': _family('', 'pgm_env_ingest', gauss=True),
            'cat': _family('_cat', 'pgm_env_ingest', variant='ppo_update_cat_kernel (one workgroup per tower)'),
            'any': _family('_any', 'pgm_env_ingest_any', head=True, variant='ppo_update_any_kernel')}


# ---------------------------------------------------------------------------------------------- env modes
class EnvMode:
    """One way of stepping the env.  A mode owns its constructor checks, defaults and allocations (``setup``: per-task
    tensors through ``tb.z``, mode-wide constants on the mode), what it rebuilds per ``set_active`` (``views``) and the
    operations ``reset`` / ``rollout`` / ``evaluate``; the facts below are all the batch's other methods know of it."""
    name = None          # what set_task_hparams' refusal calls the mode (None: SynthMode, which has the settings)
    no_step = None       # env_step's refusal (None: the mode has the single-step kernel)
    fused_noise = False  # the rollout draws its action noise in-kernel: iteration() pre-draws none
    overlap = True       # the evaluation is a launch that can run beside the next rollout
    run_seeds = plugin = None

    def setup(self, tb, **kw):
        pass

    def views(self, tb):
        pass

    def _noise(self, tb, noise, env_noise, takes_env_noise=False):
        """A fused rollout's noise argument: explicit noise uploaded into tb.noise; None: the kernel draws the stream."""
        if env_noise is not None and not takes_env_noise:
            raise PGMError(ENV_NOISE_MSG)
        if noise is None:
            return None
        if noise is not tb.noise:
            tb.noise.copy_(noise.to(dtype=F32))
        return tb.noise

    @staticmethod
    def _eval_tail(tb, out):
        return tb.eval_num, int(tb.use_ob_rms), int(tb.raw), tb.gamma, _ptr(out)


class SynthMode(EnvMode):
    """The SynthMO device envs.  run_seeds: the reset tables are stacked per run, task p resets from the block of run
    ``tb.run_of_task[p]`` and every operation goes through its *_runs entry point."""

    def __init__(self, env_name, run_seeds, **other_modes):
        if run_seeds is None:
            return
        self.run_seeds = [int(x) for x in run_seeds]
        if not self.run_seeds:
            raise PGMError('run_seeds=[]: a multi-run batch needs at least one seed')
        for flag, on in other_modes.items():
            if on:
                raise PGMError(f'run_seeds=... with {flag}=...: several runs share one population on the SynthMO '
                               f'device envs only (the reset tables of {flag} have another shape)')
        sp = envspec.make_spec(env_name)
        if sp.get('native') == 'dummy' or sp.get('discrete') or sp.get('user'):
            raise PGMError(f'run_seeds=... with {env_name}: several runs share one population on the SynthMO '
                           f'device envs only (the MO-Dummy / Deep Sea Treasure reset tables are per family)')
        require_runs()
        self.no_step = ('env_step: a multi-run batch (run_seeds=...) has no single-step kernel that takes the reset '
                        'rows per task; the envs are stepped inside rollout()')

    def setup(self, tb, **kw):
        if self.run_seeds is not None:  # every task starts in run 0
            tb.run_of_task = torch.zeros(tb.capacity, dtype=I32, device=tb.dev)

    def _runs(self, tb):
        return ('_runs', (_ptr(tb.run_of_task), len(self.run_seeds))) if self.run_seeds is not None else ('', ())

    def reset(self, tb):
        sfx, runs = self._runs(tb)
        out = torch.empty(tb.P, tb.N, tb.O, dtype=F32, device=tb.dev)
        _call('pgm_env_reset' + sfx, C.byref(tb.dims), C.byref(tb.c_spec), C.byref(tb.c_state), C.byref(tb.c_norm),
              *runs, _ptr(out))
        tb.obs[:, 0].copy_(out)
        tb.masks[:, 0] = 1.0
        tb.bad_masks[:, 0] = 1.0
        return out

    def rollout(self, tb, seed, noise, carry, env_noise):
        sfx, runs = self._runs(tb)
        nz = self._noise(tb, noise, env_noise)
        _call('pgm_rollout' + sfx, C.byref(tb.dims), _ptr(tb.params), C.byref(tb.c_spec), C.byref(tb.c_state),
              C.byref(tb.c_norm), C.byref(tb.c_rb), _ptr(nz), C.c_uint64(seed), int(carry), *runs,
              C.byref(launch_opts()))

    def evaluate(self, tb, mean, var, out):
        sfx, runs = self._runs(tb)
        _call('pgm_eval' + sfx, C.byref(tb.dims), _ptr(tb.params), C.byref(tb.c_spec), _ptr(mean), _ptr(var),
              _ptr(tb.s0_eval), *self._eval_tail(tb, out), *runs, C.byref(launch_opts()))


class HostMode(EnvMode):
    """``tb.host_env`` steps the envs on the host; the device acts, ingests and evaluates with the family's
    rollout_act / env_ingest / eval_act kernels."""
    name = 'host_env'
    overlap = False  # the evaluation is a host episode loop that synchronises every step

    def setup(self, tb, **kw):
        """Pinned host / device staging: the sampled actions (D2H; discrete: int32 indices) and one packed fp64 record
        per step -- raw obs | raw objectives | reward | done, bad_transition as int32 pairs -- so H2D is one copy."""
        he, Pc, N, O, A, K, E = tb.host_env, tb.capacity, tb.N, tb.O, tb.A, tb.K, tb.eval_num
        if tuple(he.dims()) != (O, A, K) or he.N != N:
            raise PGMError(f'host_env has (obs, act, obj) dims {tuple(he.dims())} and {he.N} envs per task; '
                           f'{tb.env_name} with num_processes={N} needs {(O, A, K)} and {N}')
        if getattr(he, 'capacity', he.P) < Pc:
            raise PGMError(f'host_env holds {getattr(he, "capacity", he.P)} tasks, the batch needs {Pc}')
        if E > HOST_EVAL_MAX:
            raise PGMError(f'host-env mode evaluates at most {HOST_EVAL_MAX} episodes per task (eval_num={E})')
        if bool(getattr(he, 'discrete', False)) != tb.discrete:
            raise PGMError(f'host_env.discrete = {getattr(he, "discrete", False)} but {tb.env_name} has '
                           f'{"discrete" if tb.discrete else "continuous"} actions')
        self.no_step = ('env_step: this batch runs on the runtime-dim kernels, which are host-stepped only: the '
                        'environments are stepped inside rollout(), there is no device env to step' if tb.any_dims else
                        'env_step: this batch is in host-env mode (TaskBatch(host_env=...)): the environments are '
                        'stepped on the host inside rollout(), there is no device env to step')
        ashape, adt = ((Pc, N), I32) if tb.discrete else ((Pc, N, A), F32)
        self._h_act = torch.empty(ashape, dtype=adt, pin_memory=True)
        self._d_act = torch.zeros(ashape, dtype=adt, device=tb.dev)
        n = Pc * N * (O + K + 2)
        self._h_tr = torch.zeros(n, dtype=F64, pin_memory=True)
        self._d_tr = torch.zeros(n, dtype=F64, device=tb.dev)
        self._tr_ready = None  # the last H2D copy out of _h_tr (the host waits for it before rewriting the buffer)
        self._h_eobs = torch.zeros(Pc * E * O, dtype=F64, pin_memory=True)
        self._d_eobs = torch.zeros(Pc * E * O, dtype=F64, device=tb.dev)
        self._h_eact = torch.empty(Pc * E * tb.act_width, dtype=adt, pin_memory=True)
        self._d_eact = torch.zeros(Pc * E * tb.act_width, dtype=adt, device=tb.dev)

    def views(self, tb):
        P, N, O, K = tb.P, tb.N, tb.O, tb.K
        n1, n2, n3 = P * N * O, P * N * K, P * N

        def seg(buf):
            flags = buf[n1 + n2 + n3:n1 + n2 + 2 * n3].view(I32).view(2, P, N)
            return (buf[:n1].view(P, N, O), buf[n1:n1 + n2].view(P, N, K), buf[n1 + n2:n1 + n2 + n3].view(P, N),
                    flags[0], flags[1])
        self._tr_len = n1 + n2 + 2 * n3
        self._d_seg = seg(self._d_tr)
        self._h_seg = tuple(v.numpy() for v in seg(self._h_tr))
        tb.host_env.set_active(P)

    def stage(self, t, obs, rew, done, bad, obj):
        """One packed H2D copy of the host transition (t = -1: the reset observation alone); returns the device views."""
        if self._tr_ready is not None:
            self._tr_ready.synchronize()
        ho, hj, hr, hd, hb = self._h_seg
        ho[...] = obs
        if t >= 0:
            hj[...], hr[...], hd[...], hb[...] = obj, rew, done, bad
        n = self._tr_len
        self._d_tr[:n].copy_(self._h_tr[:n], non_blocking=True)
        self._tr_ready = torch.cuda.Event()
        self._tr_ready.record()
        return self._d_seg

    def reset(self, tb):  # one H2D copy of the host envs' reset observations, then the ingest kernel
        tb._ingest(-1, tb.host_env.reset())

    def rollout(self, tb, seed, noise, carry, env_noise):
        """morl/mopg.py:103-135 with the env on the host: per step t the device acts on obs[t], the actions go to the
        host (pinned D2H + the step's one stream synchronise), the host envs step, the transition returns (pinned
        H2D) and the device applies VecNormalize + insert into slot t + 1; then the bootstrap value."""
        P, T, he = tb.P, tb.T, tb.host_env
        if hasattr(he, 'begin_rollout'):  # a host-stepped contract-2 plug-in: this rollout's env noise
            he.begin_rollout(envplug.env_seed(seed), None if env_noise is None else
                             torch.as_tensor(env_noise).detach().cpu().numpy())
        elif env_noise is not None:
            raise PGMError(ENV_NOISE_MSG)
        if noise is None:  # the perf-mode counter stream of `seed`: what the fused rollout draws in-kernel
            tb._draw_noise(seed)
        elif noise is not tb.noise:
            tb.noise.copy_(noise.to(dtype=F32))
        if carry:  # after_update(): slot T -> slot 0 (storage.py:71-75)
            tb.obs[:, 0].copy_(tb.obs[:, T])
            tb.masks[:, 0].copy_(tb.masks[:, T])
            tb.bad_masks[:, 0].copy_(tb.bad_masks[:, T])
        stream = torch.cuda.current_stream()
        prof = tb.host_profile
        h_act = self._h_act[:P]
        a_np = h_act.numpy()
        for t in range(T):
            t0 = time.perf_counter()
            tb._rollout_act(t)
            h_act.copy_(self._d_act[:P], non_blocking=True)
            stream.synchronize()
            t1 = time.perf_counter()
            obs, rew, done, bad, obj = he.step(a_np)
            t2 = time.perf_counter()
            tb._ingest(t, obs, rew, done, bad, obj)
            if prof is not None:
                stream.synchronize()  # (only when timed: the ingest otherwise overlaps nothing the host waits for)
                prof['act'] += t1 - t0
                prof['step'] += t2 - t1
                prof['ingest'] += time.perf_counter() - t2
        tb._rollout_act(T)

    def evaluate(self, tb, mean, var, out):
        """evaluation() (morl/mopg.py:25-46) with the episodes on the host: eval_num episodes per task step together,
        eval_act normalises with the frozen statistics and returns the deterministic actions (discrete: int32 action
        indices [P, E]); an ended episode stops contributing."""
        P, E, O, K, A, he = tb.P, tb.eval_num, tb.O, tb.K, tb.act_width, tb.host_env
        stream = torch.cuda.current_stream()
        h_obs, h_act = self._h_eobs[:P * E * O], self._h_eact[:P * E * A]
        obs_np = h_obs.numpy().reshape(P, E, O)
        act_np = h_act.numpy().reshape((P, E) if tb.discrete else (P, E, A))
        acc = np.zeros((P, E, K))
        disc = 1.0
        alive = np.ones((P, E), dtype=bool)
        obs = he.eval_reset(E)
        d = Dims(P, 1, 0, O, tb.A, K, tb.H, int(tb.layernorm))
        while alive.any():
            obs_np[...] = obs
            self._d_eobs[:P * E * O].copy_(h_obs, non_blocking=True)
            tb._launch(tb.family.eval_act, d, _ptr(tb.params), _ptr(mean), _ptr(var), int(tb.use_ob_rms),
                       _ptr(self._d_eobs), E, _ptr(self._d_eact))
            h_act.copy_(self._d_eact[:P * E * A], non_blocking=True)
            stream.synchronize()
            obs, obj, done = he.eval_step(act_np)
            acc += np.where(alive[..., None], disc * np.asarray(obj, dtype=np.float64), 0.0)
            if not tb.raw:
                disc *= tb.gamma
            alive &= ~np.asarray(done, dtype=bool)
        out.copy_(torch.from_numpy(acc.sum(1) / E))


class DstMode(EnvMode):
    """Deep Sea Treasure stepped inside pgm_rollout_dst / pgm_eval_dst.  max_steps / time_limit_is_bad: the step limit
    and whether it is reported as a time-limit end, as hostenv.DeepSeaTreasureHostVecEnv has them."""
    name = 'device_env'
    no_step = ('env_step: the device Deep Sea Treasure is stepped inside pgm_rollout_dst / pgm_eval_dst; '
               'there is no single-step kernel (pgm_dst_transition evaluates the rule on the host)')
    fused_noise = True

    def setup(self, tb, max_steps, time_limit_is_bad, **kw):
        if (tb.O, tb.A, tb.K) != (3, 4, 2):
            raise PGMError(f'device_env=True with {tb.env_name}: the one discrete-action device env is Deep Sea '
                           f'Treasure (obs 3, 4 actions, 2 objectives)')
        if not 1 <= tb.eval_num <= HOST_EVAL_MAX:
            raise PGMError(f'device_env=True evaluates 1..{HOST_EVAL_MAX} episodes per task in one launch '
                           f'(eval_num={tb.eval_num})')
        require_dst_device()
        self.max_steps = int(max_steps or tb.spec['max_episode_steps'])
        self.time_limit_is_bad = bool(time_limit_is_bad)
        self.c_dst = DstSpec(self.max_steps, int(self.time_limit_is_bad))
        # the constant raw reset observation of (row, col, step) = (0, 0, 0), for env_ingest(-1)
        self._dst_obs0 = torch.zeros(tb.capacity, tb.N, tb.O, dtype=F64, device=tb.dev)

    def reset(self, tb):  # every env at (0, 0, 0); VecNormalize.reset on the constant reset observation
        tb.s.zero_()
        tb._env_ingest(-1, self._dst_obs0)

    def rollout(self, tb, seed, noise, carry, env_noise):
        nz = self._noise(tb, noise, env_noise)
        _call('pgm_rollout_dst', C.byref(tb.dims), _ptr(tb.params), C.byref(self.c_dst), C.byref(tb.c_state),
              C.byref(tb.c_norm), C.byref(tb.c_rb), _ptr(nz), C.c_uint64(seed), int(carry))

    def evaluate(self, tb, mean, var, out):
        _call('pgm_eval_dst', C.byref(tb.dims), _ptr(tb.params), C.byref(self.c_dst), _ptr(mean), _ptr(var),
              *self._eval_tail(tb, out))


class DummyMode(EnvMode):
    """An MO-Dummy env stepped inside pgm_rollout_dummy / pgm_eval_dummy.  max_steps (default 500), bound (5.0),
    time_limit_is_bad (default True: the registration's TimeLimitMask) and R (reset positions per env, default
    envspec.DUMMY_RESETS) are the device env's, as hostenv.DummyMOHostVecEnv has them."""
    name = 'an MO-Dummy env'
    fused_noise = True

    def setup(self, tb, seed, max_steps, time_limit_is_bad, bound, R, **kw):
        env_name, sp, N, E = tb.env_name, tb.spec, tb.N, tb.eval_num
        if not 1 <= E <= HOST_EVAL_MAX:
            raise PGMError(f'{env_name} evaluates 1..{HOST_EVAL_MAX} episodes per task in one launch (eval_num={E})')
        if N > 8:
            raise PGMError(f'{env_name}: num_processes={N} envs per task > 8 unsupported')
        self.max_steps = int(max_steps or sp['max_episode_steps'])
        self.bound = float(sp['bound'] if bound is None else bound)
        self.time_limit_is_bad = True if time_limit_is_bad is None else bool(time_limit_is_bad)
        self.R = int(envspec.DUMMY_RESETS if R is None else R)
        if self.max_steps <= 0 or not self.bound > 0 or self.R < 1:
            raise PGMError(f'{env_name}: max_steps={self.max_steps}, bound={self.bound} and R={self.R} must be '
                           f'positive')
        self.no_step = (f'env_step: {env_name} is stepped inside pgm_rollout_dummy / pgm_eval_dummy; there is '
                        f'no single-step kernel (pgm_dummy_transition evaluates the rule on the host)')
        # per (task, env): resets since env_reset(); the reset positions [N][R][2], [eval_num][R][2]
        tb.z('episode', N, dt=I32)
        self._dummy_train = torch.tensor(envspec.dummy_reset_table(seed, N, self.R), dtype=F64, device=tb.dev)
        self._dummy_eval = torch.tensor(envspec.dummy_reset_table(seed, E, self.R), dtype=F64, device=tb.dev)

    def views(self, tb):
        tlb = int(self.time_limit_is_bad)
        self.c_dummy = DummySpec(self.max_steps, tlb, self.bound, _ptr(self._dummy_train), self.R, tb.N)
        self.c_dummy_eval = DummySpec(self.max_steps, tlb, self.bound, _ptr(self._dummy_eval), self.R, tb.eval_num)

    def reset(self, tb):  # env n of every task at entry (n, 0) of the reset table, at rest; VecNormalize.reset
        tb.s.zero_()
        tb.s[:, :, :2] = self._dummy_train[:, 0]
        tb.elapsed.zero_()
        tb.episode.zero_()
        tb._env_ingest(-1, tb.s)

    def rollout(self, tb, seed, noise, carry, env_noise):
        nz = self._noise(tb, noise, env_noise)
        _call('pgm_rollout_dummy', C.byref(tb.dims), _ptr(tb.params), C.byref(self.c_dummy), C.byref(tb.c_state),
              _ptr(tb.episode), C.byref(tb.c_norm), C.byref(tb.c_rb), _ptr(nz), C.c_uint64(seed), int(carry))

    def evaluate(self, tb, mean, var, out):
        _call('pgm_eval_dummy', C.byref(tb.dims), _ptr(tb.params), C.byref(self.c_dummy_eval), _ptr(mean), _ptr(var),
              *self._eval_tail(tb, out))


class PluginMode(EnvMode):
    """A device env plug-in: env_name is registered with the header's dims, the env stepped inside the fused kernels of
    its library.  R: reset-table entries per env (default envplug.DEFAULT_RESETS).  A contract-2 header's per-step
    uniforms come from the stream of envplug.env_seed(rollout seed); the evaluation's from tb._plug_eval_seed =
    envplug.env_seed(seed): fixed for the batch, so every policy it evaluates meets the same env noise."""
    name = 'env_plugin'
    no_step = ('env_step: an env plug-in is stepped inside pgm_envplug_rollout / pgm_envplug_eval; there '
               'is no single-step kernel (EnvPlugin.transition evaluates the header on the host)')
    fused_noise = True

    def __init__(self, env_name, env_plugin, env_params, host_env, device_env, layernorm, eval_num, num_processes):
        if host_env is not None or device_env:
            raise PGMError('env_plugin=... steps the env inside the plug-in\'s fused kernels: host_env=... and '
                           'device_env=True are other places to step it; give env_plugin alone (the same header on '
                           'the host: host_env=hostenv.PluginHostVecEnv(plugin, ...) without env_plugin)')
        if layernorm:
            raise PGMError('layernorm=True with env_plugin=...: env plug-ins are built for plain towers only')
        if eval_num > HOST_EVAL_MAX or eval_num < 1:
            raise PGMError(f'eval_num={eval_num} with env_plugin=...: a plug-in evaluates 1..{HOST_EVAL_MAX} '
                           f'episodes per task in one launch')
        if num_processes > 8:
            raise PGMError(f'num_processes={num_processes} with env_plugin=...: envs per task > 8 unsupported')
        self.plugin = envplug.as_plugin(env_plugin)
        self._plug_par_np = self.plugin.par_vector(env_params)  # (refuses unknown names, NP == 0)
        try:
            self.plugin.register(env_name)
        except ValueError as e:
            raise PGMError(f'env_plugin=...: {e}') from e

    def setup(self, tb, seed, R, **kw):
        pl, N, dims = self.plugin, tb.N, (tb.O, tb.A, tb.K)
        if pl.dims() != dims or pl.DISCRETE != tb.discrete:
            raise PGMError(f'env_plugin has (obs, act, obj) dims {pl.dims()}, discrete = {pl.DISCRETE}; '
                           f'{tb.env_name} is registered with {dims}, discrete = {tb.discrete}')
        self.R = int(envplug.DEFAULT_RESETS if R is None else R)
        if self.R < 1:
            raise PGMError(f'{tb.env_name}: R={self.R} reset-table entries per env must be at least 1')
        # the plug-in's state words, resets since env_reset(), the reset uniforms
        tb.z('plug_sd', N, pl.SD, dt=F64)
        tb.z('plug_si', N, pl.SI, dt=I32)
        tb.z('episode', N, dt=I32)
        self._plug_train_np = envspec.plugin_reset_table(seed, N, self.R, pl.RW)
        self._plug_train = torch.tensor(self._plug_train_np, dtype=F64, device=tb.dev)
        self._plug_eval = torch.tensor(envspec.plugin_reset_table(seed, tb.eval_num, self.R, pl.RW), dtype=F64,
                                       device=tb.dev)
        self._plug_obs0 = torch.zeros(tb.capacity, N, tb.O, dtype=F64, device=tb.dev)
        self._plug_par = torch.tensor(self._plug_par_np if pl.NP else [0.0], dtype=F64, device=tb.dev)
        tb.env_noise = None  # [T][N][NW] fp64, allocated by the first rollout that is fed its env noise
        tb._plug_eval_seed = envplug.env_seed(seed)

    def reset(self, tb):  # env n of every task at entry (n, 0) of its row: the header's reset on the host
        P, N, pl = tb.P, tb.N, self.plugin
        row = np.broadcast_to(np.arange(N, dtype=np.int32), (P, N)).reshape(-1)
        sd, si, obs = pl.reset(row, np.zeros(P * N, dtype=np.int32), self._plug_train_np, par=self._plug_par_np)
        tb.plug_sd.copy_(torch.from_numpy(sd.reshape(P, N, pl.SD)))
        tb.plug_si.copy_(torch.from_numpy(si.reshape(P, N, pl.SI)))
        self._plug_obs0[:P].copy_(torch.from_numpy(obs.reshape(P, N, tb.O)))
        tb.elapsed.zero_()
        tb.episode.zero_()
        tb._env_ingest(-1, self._plug_obs0)

    def rollout(self, tb, seed, noise, carry, env_noise):
        pl = self.plugin
        nz = self._noise(tb, noise, env_noise, takes_env_noise=pl.NW > 0)
        args = (C.byref(tb.dims), _ptr(tb.params), _ptr(tb.plug_sd), _ptr(tb.plug_si), _ptr(tb.episode),
                _ptr(self._plug_train), self.R, tb.N, C.byref(tb.c_state), C.byref(tb.c_norm), C.byref(tb.c_rb),
                _ptr(nz), C.c_uint64(seed), int(carry))
        if pl.CONTRACT == 1:
            return _call('pgm_envplug_rollout', *args, of=pl)
        ez = None
        if env_noise is not None:
            shape = (tb.T, tb.N, pl.NW)
            if tuple(env_noise.shape) != shape:
                raise PGMError(f'rollout(env_noise=...) of shape {tuple(env_noise.shape)}: this batch steps '
                               f'[T][N][NW] = {shape}')
            if tb.env_noise is None:
                tb.env_noise = torch.zeros(shape, dtype=F64, device=tb.dev)
            tb.env_noise.copy_(torch.as_tensor(env_noise).to(dtype=F64))
            ez = tb.env_noise
        _call('pgm_envplug_rollout_ex', *args, _ptr(self._plug_par), _ptr(ez), C.c_uint64(envplug.env_seed(seed)),
              of=pl)

    def evaluate(self, tb, mean, var, out):
        pl = self.plugin
        args = (C.byref(tb.dims), _ptr(tb.params), _ptr(self._plug_eval), self.R, tb.eval_num, _ptr(mean), _ptr(var),
                *self._eval_tail(tb, out))
        if pl.CONTRACT == 1:
            return _call('pgm_envplug_eval', *args, of=pl)
        _call('pgm_envplug_eval_ex', *args, _ptr(self._plug_par), C.c_uint64(tb._plug_eval_seed), of=pl)


class TaskBatch:
    """HBM state of P tasks sharing env, rollout shape and PPO hyper-parameters.

    ``capacity`` (>= P) sizes every buffer once; ``set_active(P)`` then runs the first P task slots without
    reallocating (the generation loop keeps one TaskBatch for populations of varying size).  The public
    tensors (``params``, ``ob_mean``, ``obs``, ...) are views of the active slots.  Two packed regions make the
    per-iteration snapshot and the per-generation load single copies:
      * ``state``  [3][capacity][L] fp32: params | Adam exp_avg | exp_avg_sq (``params`` = state[0, :P], ...);
      * ``stats64`` flat fp64: the segments of ``STAT_SEGMENTS`` (task weights and every running statistic),
        each [capacity][width] contiguous -- a whole-buffer copy is one iteration's record of every task.
    """
    # (name, width per task: int, or the attribute of the dims it is); the order is the stats64 layout
    STAT_SEGMENTS = (('weights', 'K'), ('ob_mean', 'O'), ('ob_var', 'O'), ('ob_count', 0), ('ret_mean', 0),
                     ('ret_var', 0), ('ret_count', 0), ('obj_mean', 'K'), ('obj_var', 'K'), ('obj_count', 0))
    HOST_EVAL_MAX = HOST_EVAL_MAX

    def __init__(self, env_name, P, num_processes=4, num_steps=2048, seed=0, eval_num=1, gamma=0.995,
                 gae_lambda=0.95, use_gae=True, use_proper_time_limits=True, ob_rms=True, obj_rms=True, raw=True,
                 clip_param=0.2, ppo_epoch=10, num_mini_batch=32, value_loss_coef=0.5, entropy_coef=0.0,
                 max_grad_norm=0.5, adam_eps=1e-5, use_clipped_value_loss=True, device='cuda', capacity=None,
                 layernorm=False, host_env=None, device_env=False, *, max_steps=None, time_limit_is_bad=None,
                 bound=None, R=None, any_dims=False, env_plugin=None, run_seeds=None, env_params=None):
        """device_env: run a discrete-action env on the device (DstMode) instead of on the host; for such an env
        exactly one of host_env and device_env=True is given.  The SynthMO and MO-Dummy envs are device envs already:
        the flag changes nothing there.  max_steps / time_limit_is_bad / bound / R: the device env's settings (DstMode,
        DummyMode, PluginMode).  any_dims=True: run a host-stepped batch of an env envspec knows on the runtime-dim
        kernels (the *_any entry points) instead of the ones compiled for its dims; a registered third-party env
        (envspec.register_env) always runs on them.  env_plugin: a device env plug-in (envplug.EnvPlugin, or the path
        of its header): the batch is a runtime-dim batch on the device envs' schedule (overlapped evaluation included).
        env_params: the runtime parameters of a contract-2 plug-in, a dict name -> float over the header's PAR_NAMES
        (omitted names take the header's default); one set for every task of the batch.  run_seeds: a list of seeds
        makes the batch hold the tasks of several runs (SynthMode, set_runs; SynthMO only); `seed` is then unused."""
        # the env mode: run_seeds refuses the other modes' flags, env_plugin registers env_name; the rest needs the spec
        mode = SynthMode(env_name, run_seeds, host_env=host_env is not None, device_env=bool(device_env),
                         env_plugin=env_plugin is not None)
        if env_plugin is not None:
            mode = PluginMode(env_name, env_plugin, env_params, host_env, device_env, layernorm, eval_num, num_processes)
        elif env_params:
            raise PGMError('env_params=... sets the runtime parameters of env_plugin=...; this batch has no plug-in (a '
                           'host-stepped plug-in takes them itself: hostenv.PluginHostVecEnv(..., env_params=...))')
        self.run_seeds, self.plugin = mode.run_seeds, mode.plugin
        self.spec = sp = envspec.make_spec(env_name)
        self.host_env = host_env
        self.host_profile = None  # a dict {'act', 'step', 'ingest'} of seconds when a caller wants the split timed
        self.env_name = env_name
        self.capacity = Pc = max(P, capacity or P)
        self.P, self.N, self.T = P, num_processes, num_steps
        self.O, self.A, self.K, self.H = sp['obs_dim'], sp['act_dim'], sp['obj_num'], 64
        self.eval_num, self.gamma, self.gae_lambda = eval_num, gamma, gae_lambda
        self.use_gae, self.proper = use_gae, use_proper_time_limits
        self.use_ob_rms, self.use_obj_rms, self.raw = ob_rms, obj_rms, raw
        self.ppo_epoch, self.num_mini_batch = ppo_epoch, num_mini_batch
        self.dev = torch.device(device)
        self.layernorm = bool(layernorm)
        # the runtime-dim kernel family: host-stepped, plain towers, at most HOST_EVAL_MAX evaluation episodes
        self.any_dims = bool(sp.get('user')) or bool(any_dims)
        if self.any_dims:
            what = f'{env_name} runs on the runtime-dim kernels (a registered third-party env, or any_dims=True)'
            if device_env:
                raise PGMError(f'device_env=True: {what}, which step no env on the device; give host_env=...')
            if host_env is None and self.plugin is None:
                raise PGMError(f'{what}, which are host-stepped only: TaskBatch needs host_env=... '
                               f'(hostenv.GymHostVecEnv, --host-env module:callable)')
            if self.layernorm:
                raise PGMError(f'layernorm=True: {what}, which are built for plain towers only')
            if eval_num > HOST_EVAL_MAX:
                raise PGMError(f'eval_num={eval_num}: {what}, which evaluate at most {HOST_EVAL_MAX} episodes '
                               f'per task')
            amin = 2 if sp.get('discrete') else 1
            if not (1 <= self.O <= ANY_MAX_OBS and amin <= self.A <= ANY_MAX_ACT and 1 <= self.K <= ANY_MAX_OBJ):
                raise PGMError(f'{what}, which take obs_dim <= {ANY_MAX_OBS}, {amin} <= act_dim <= {ANY_MAX_ACT} and '
                               f'obj_num <= {ANY_MAX_OBJ}; {env_name} has {(self.O, self.A, self.K)}')
            require_any_dims()
        if self.layernorm and self.O > LN_MAX_OBS:
            raise PGMError(f'layernorm=True with {env_name}: the LayerNorm kernels keep layer 1 LDS-resident and are '
                           f'built for obs_dim <= {LN_MAX_OBS}; obs_dim {self.O} would need a streamed layer-1 '
                           f'LayerNorm kernel, which does not exist')
        # a discrete-action env (spec['discrete']): Categorical head, A = number of actions, one width-1 action per
        # step; such envs run on the host (host_env) or, opted into, on the device (device_env)
        self.discrete = bool(sp.get('discrete', False))
        self.device_env = bool(device_env) and self.discrete  # (a SynthMO env is a device env with or without the flag)
        if self.discrete:
            if host_env is None and not device_env and self.plugin is None:
                raise PGMError(f'{env_name} has discrete actions and no default device environment: TaskBatch needs '
                               f'host_env=... (hostenv.DeepSeaTreasureHostVecEnv, --host-env dst) or device_env=True '
                               f'(--device-env)')
            if host_env is not None and device_env:
                raise PGMError(f'{env_name}: host_env=... and device_env=True are two places to step the same env; '
                               f'give exactly one')
            if self.layernorm:
                raise PGMError(f'layernorm=True with {env_name}: LayerNorm towers with a Categorical head are not built')
            require_categorical()
        self.family = FAMILIES['any' if self.any_dims else 'cat' if self.discrete else 'gauss']
        self.dummy_env = sp.get('native') == 'dummy' and host_env is None
        if sp.get('native') == 'dummy':
            require_dummy_device()  # (the dim sets 6/2/2, 6/2/3 of every Gaussian kernel come with the same bit)
        self.mode = mode = (HostMode() if host_env is not None else DstMode() if self.device_env else
                            DummyMode() if self.dummy_env else mode)
        self.act_width = 1 if self.discrete else self.A
        self._full = {}  # name -> full-capacity tensor whose leading dim is the task slot
        mode.setup(self, seed=seed, max_steps=max_steps, time_limit_is_bad=time_limit_is_bad, bound=bound, R=R)
        self.layout = ParamLayout(self.O, self.A, self.K, self.H, layernorm=self.layernorm, discrete=self.discrete)
        L, O, A, K, N, T, z = self.layout.total, self.O, self.A, self.K, self.N, self.T, self.z
        # spec constants + reset tables (fp64); run_seeds: [num_runs][N][O], [num_runs][eval_num][O], block r run r's
        self._spec_t = {k: torch.tensor(np.ascontiguousarray(sp[k]), dtype=F64, device=self.dev)
                        for k in ('d', 'U', 'c', 'V', 'ebase', 'ecoef', 'act_lo', 'act_hi') if k in sp}
        self.s0_train, self.s0_eval = (
            torch.tensor(envspec.reset_table(O, seed, n) if self.run_seeds is None else
                         np.stack([envspec.reset_table(O, sd, n) for sd in self.run_seeds]), dtype=F64, device=self.dev)
            for n in (N, eval_num))
        # policy + optimiser: one [3][Pc][L] region
        self._state = torch.zeros(3, Pc, L, dtype=F32, device=self.dev)
        z('adam_step', dt=I32)
        z('lr')
        # task weights + running statistics: one flat fp64 region (STAT_SEGMENTS)
        self._seg = []
        off = 0
        for name, wd in self.STAT_SEGMENTS:
            w = getattr(self, wd) if isinstance(wd, str) else 1
            self._seg.append((name, off, w, isinstance(wd, str)))
            off += Pc * w
        self._stats64 = torch.zeros(off, dtype=F64, device=self.dev)
        # env state
        z('s', N, O, dt=F64)
        z('elapsed', N, dt=I32)
        z('obj_acc', N, K, dt=F64)
        z('obj_valid', dt=I32)
        z('ret', N, dt=F64)
        # rollout storage (storage.py:12-30)
        z('obs', T + 1, N, O)
        z('actions', T, N, self.act_width)
        z('logp', T, N)
        z('values', T + 1, N, K)
        z('returns', T + 1, N, K)
        z('rewards', T, N, K)
        z('adv', T, N)
        z('masks', T + 1, N, fill=1.0)
        z('bad_masks', T + 1, N, fill=1.0)
        z('stats', 3)
        z('objs', K, dt=F64)
        # the overlapped evaluation's copy of ob_rms: mean | var of every slot, one copy of the adjacent stats64
        # segments ob_mean, ob_var (STAT_SEGMENTS order)
        self._eval_ob = torch.zeros(2, Pc, O, dtype=F64, device=self.dev)
        self.perms = torch.zeros(ppo_epoch, T * N, dtype=I32, device=self.dev)
        # the rollout's random stream: standard normals [T][N][A], or (discrete) one uniform per (step, env) [T][N]
        self.noise = torch.zeros((T, N) if self.discrete else (T, N, A), dtype=F32, device=self.dev)
        self.hp = PPOHParams(clip_param=clip_param, value_loss_coef=value_loss_coef, entropy_coef=entropy_coef,
                             max_grad_norm=max_grad_norm, adam_eps=adam_eps, beta1=0.9, beta2=0.999,
                             ppo_epoch=ppo_epoch, num_mini_batch=num_mini_batch,
                             use_clipped_value_loss=int(use_clipped_value_loss))
        self.hp_task, self.lam_task = None, None  # device tables of set_task_hparams (None: the shared settings)
        self._eval_stream, self._eval_done = None, None
        self._reset_pending = False  # a pgm_ppo_update_reset queued on the side stream, not yet waited for
        nws = getattr(lib(), self.family.workspace_bytes)(C.byref(Dims(Pc, N, T, O, A, K, self.H, int(self.layernorm))))
        self.update_ws = torch.zeros((nws + 7) // 8, dtype=torch.int64, device=self.dev)
        # sticky OR of every update's exchange-timeout word (workspace word 2P, include/pgm_abi.h): a launch
        # whose spin-wait gave up produced invalid parameters; check_update() turns that into PGMError
        self.update_failed = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.last_fail_word = 0
        self.set_active(P)
        self.reset_stats()

    def __getattr__(self, name):
        """A value its mode holds (max_steps, R, the reset tables, c_dummy, _d_act, ...) under the name it has there."""
        try:
            return self.__dict__['mode'].__dict__[name]
        except KeyError:
            raise AttributeError(f'{type(self).__name__!r} object has no attribute {name!r}') from None

    def z(self, name, *s, dt=F32, fill=0.0):
        """A per-task tensor [capacity, *s]; set_active re-slices its active slots into the attribute ``name``."""
        t = torch.full((self.capacity,) + s, fill, dtype=dt, device=self.dev)
        self._full[name] = t
        return t

    # ------------------------------------------------------------------ the family's kernels
    def _launch(self, name, dims, *args):
        """Entry point `name` of the batch's kernel family: (dims, [head,] args..., stream)."""
        _call(name, C.byref(dims), *((int(self.discrete),) if self.family.head else ()), *args)

    def _env_ingest(self, t, obs, obj=None, rew=None, done=None, bad=None):
        """env_ingest(t) on device buffers: VecNormalize + insert into slot t + 1 (t = -1: the reset observation)."""
        _call(self.family.env_ingest, C.byref(self.dims), C.byref(self.c_state), C.byref(self.c_norm),
              C.byref(self.c_rb), t, _ptr(obs), _ptr(obj), _ptr(rew), _ptr(done), _ptr(bad))

    def _ingest(self, t, obs, rew=None, done=None, bad=None, obj=None):
        """One packed H2D copy of the host transition, then env_ingest(t) (t = -1: the reset observation)."""
        self._env_ingest(t, *self.mode.stage(t, obs, rew, done, bad, obj))

    def _draw_noise(self, seed):
        """The perf-mode counter stream of `seed` into self.noise: normals, or (discrete) uniforms."""
        _call('pgm_uniform_noise' if self.discrete else 'pgm_normal_noise', self.noise.numel(), C.c_uint64(seed),
              _ptr(self.noise))

    def _rollout_act(self, t):
        self._launch(self.family.rollout_act, self.dims, _ptr(self.params), C.byref(self.c_rb), t, _ptr(self.noise),
                     _ptr(self.mode._d_act))

    def set_active(self, P):
        """Run the first P task slots (P <= capacity): re-slices the public views and the kernels' dims."""
        if not 0 < P <= self.capacity:
            raise ValueError(f'active tasks {P} outside [1, capacity {self.capacity}]')
        self.P = P
        for name, t in self._full.items():
            setattr(self, name, t[:P])
        self.params, self.adam_m, self.adam_v = self._state[0, :P], self._state[1, :P], self._state[2, :P]
        for name, off, w, vec in self._seg:
            v = self._stats64[off:off + self.capacity * w]
            setattr(self, name, (v.view(self.capacity, w) if vec else v)[:P])
            if name == 'ob_mean':
                self._ob_src = self._stats64[off:off + 2 * self.capacity * w].view(2, self.capacity, w)
        self._eval_mean, self._eval_var = self._eval_ob[0, :P], self._eval_ob[1, :P]
        self._build_structs()
        self.mode.views(self)

    def set_runs(self, ids):
        """run_of_task of the active tasks: ids[p] in [0, len(run_seeds)) is the run whose reset tables task p uses.
        Checked here (the kernels trust the device copy), then uploaded."""
        if self.run_seeds is None:
            raise PGMError('set_runs: this batch was built without run_seeds=...')
        ids = np.asarray(ids)
        if ids.ndim != 1 or len(ids) != self.P:
            raise PGMError(f'set_runs: {ids.shape} run ids for {self.P} active tasks (one id per task)')
        if len(ids) and (not np.issubdtype(ids.dtype, np.integer) or ids.min() < 0 or ids.max() >= len(self.run_seeds)):
            raise PGMError(f'set_runs: run ids must be integers in [0, {len(self.run_seeds)}), got {ids.tolist()}')
        self.run_of_task[:self.P].copy_(torch.from_numpy(ids.astype(np.int32)))

    def set_task_hparams(self, clip_param=None, value_loss_coef=None, entropy_coef=None, max_grad_norm=None,
                         gae_lambda=None):
        """Per-task PPO settings (the runs of a hyper-parameter grid in one population): each argument is a scalar or a
        length-P array over the active tasks; None keeps the batch's shared value.  Checked here (the kernels trust the
        device tables), then uploaded into ``hp_task`` [capacity][4] / ``lam_task`` [capacity]; from the first call on
        gae() and ppo_update_launch() go through pgm_gae_tasks / pgm_ppo_update_tasks.  A batch that never calls this
        launches what it always launched.  Plain and LayerNorm Gaussian batches on the SynthMO device envs only."""
        for flag, on in (('discrete actions', self.discrete), ('any_dims', self.any_dims),
                         (self.mode.name, self.mode.name is not None)):
            if on:
                raise PGMError(f'set_task_hparams: per-task PPO settings exist for the update kernels of '
                               f'pgm_ppo_update on the SynthMO device envs only; this batch has {flag}')
        given = dict(clip_param=clip_param, value_loss_coef=value_loss_coef, entropy_coef=entropy_coef,
                     max_grad_norm=max_grad_norm, gae_lambda=gae_lambda)
        P = self.P
        rows = {}
        for name, val in given.items():
            if val is None:
                val = self.gae_lambda if name == 'gae_lambda' else getattr(self.hp, name)
            v = check_task_hparam(name, val)
            if v.ndim > 1 or (v.ndim == 1 and len(v) != P):
                raise PGMError(f'set_task_hparams: {name} has shape {v.shape} for {P} active tasks (a scalar or one '
                               f'value per task)')
            rows[name] = np.broadcast_to(v.astype(np.float32), (P,))
        require_tasks()
        if self.hp_task is None:  # every slot starts at the shared values
            shared = [getattr(self.hp, n) for n in TASK_HPARAM_FIELDS]
            self.hp_task = torch.tensor([shared] * self.capacity, dtype=F32, device=self.dev)
            self.lam_task = torch.full((self.capacity,), float(self.gae_lambda), dtype=F32, device=self.dev)
        tab = np.stack([rows[n] for n in TASK_HPARAM_FIELDS], axis=1)
        self.hp_task[:P].copy_(torch.from_numpy(np.ascontiguousarray(tab)))
        self.lam_task[:P].copy_(torch.from_numpy(np.array(rows['gae_lambda'])))

    def set_lr(self, lr):
        """The learning rate of the next update: a scalar for every task, or one value per active task (rounded to
        fp32 exactly as the scalar is)."""
        if np.ndim(lr) == 0:
            self.lr.fill_(float(lr))
            return
        v = np.asarray(lr, dtype=np.float64)
        if v.shape != (self.P,):
            raise PGMError(f'iteration: lr has shape {v.shape} for {self.P} active tasks (a scalar or one value per '
                           f'task)')
        self.lr.copy_(torch.from_numpy(v.astype(np.float32)))

    @property
    def state(self):
        """[3][P][L] view of the active slots (params | exp_avg | exp_avg_sq); strided when P < capacity."""
        return self._state[:, :self.P]

    def stats64_record(self, out):
        """Copy the whole flat fp64 statistics region (weights + every running statistic of every slot) into
        ``out`` (one device copy: an iteration's snapshot record, unpacked on the host by stat_views)."""
        out.copy_(self._stats64)

    def stat_views(self, flat, P=None):
        """Host-side split of a stats64 record (numpy [n]) into {name: [P, width] or [P]} arrays."""
        P = self.P if P is None else P
        out = {}
        for name, off, w, vec in self._seg:
            v = flat[off:off + self.capacity * w]
            out[name] = (v.reshape(self.capacity, w) if vec else v)[:P]
        return out

    def load_stats64(self, host_flat):
        """One H2D copy of a host-built stats64 image (numpy fp64, the stat_views layout)."""
        self._stats64.copy_(torch.from_numpy(np.ascontiguousarray(host_flat, dtype=np.float64)))

    def new_stats64(self):
        """A host stats64 image holding fresh RunningMeanStd values (count 1e-4, mean 0, var 1) and zero weights."""
        flat = np.zeros(self._stats64.numel(), dtype=np.float64)
        v = self.stat_views(flat, self.capacity)
        for var in (v['ob_var'], v['ret_var'], v['obj_var']):
            var[...] = 1.0
        for cnt in (v['ob_count'], v['ret_count'], v['obj_count']):
            cnt[...] = 1e-4
        return flat

    # ------------------------------------------------------------------ structs
    def _build_structs(self):
        self.dims = Dims(self.P, self.N, self.T, self.O, self.A, self.K, self.H, int(self.layernorm))
        st = self._spec_t
        # (a discrete-action env has no SynthMO constants: NULL pointers, and no entry point that reads them is called)
        self.c_spec = EnvSpec(*(_ptr(st.get(k)) for k in ('d', 'U', 'c', 'V', 'ebase', 'ecoef', 'act_lo', 'act_hi')),
                              self.spec.get('max_episode_steps', 0), 0)
        self.c_state = EnvState(_ptr(self.s), _ptr(self.elapsed), _ptr(self.obj_acc), _ptr(self.obj_valid),
                                _ptr(self.ret), _ptr(self.s0_train))
        self.c_norm = NormState(_ptr(self.ob_mean), _ptr(self.ob_var), _ptr(self.ob_count), _ptr(self.ret_mean),
                                _ptr(self.ret_var), _ptr(self.ret_count), _ptr(self.obj_mean), _ptr(self.obj_var),
                                _ptr(self.obj_count), self.gamma, 10.0, 10.0, 1e-8, int(self.use_ob_rms),
                                int(self.use_obj_rms))
        self.c_rb = RolloutBuf(*(_ptr(t) for t in (self.obs, self.actions, self.logp, self.values, self.rewards,
                                                   self.masks, self.bad_masks, self.returns, self.adv)))

    def reset_stats(self):
        """Fresh RunningMeanStd objects: count 1e-4, mean 0, var 1 (running_mean_std.py:5-8)."""
        for mean, var, cnt in ((self.ob_mean, self.ob_var, self.ob_count), (self.ret_mean, self.ret_var, self.ret_count),
                               (self.obj_mean, self.obj_var, self.obj_count)):
            mean.zero_()
            var.fill_(1.0)
            cnt.fill_(1e-4)

    # ------------------------------------------------------------------ kernels
    def env_reset(self):
        """Fresh make_vec_envs + envs.reset() (mopg.py:67-82): obs[:, 0], masks[:, 0] = 1."""
        out = self.mode.reset(self)
        return self.obs[:, 0] if out is None else out

    def env_step(self, action):
        if self.mode.no_step is not None:
            raise PGMError(self.mode.no_step)
        P, N, O, K = self.P, self.N, self.O, self.K
        action = action.to(device=self.dev, dtype=F32).contiguous()
        obs = torch.empty(P, N, O, dtype=F32, device=self.dev)
        rew = torch.empty(P, N, K, dtype=F32, device=self.dev)
        m, b = torch.empty(P, N, dtype=F32, device=self.dev), torch.empty(P, N, dtype=F32, device=self.dev)
        _call('pgm_env_step', C.byref(self.dims), C.byref(self.c_spec), C.byref(self.c_state), C.byref(self.c_norm),
              _ptr(action), _ptr(obs), _ptr(rew), _ptr(m), _ptr(b))
        return obs, rew, m, b

    def act(self, obs, noise=None, deterministic=False):
        if self.any_dims:
            raise PGMError('act: the runtime-dim kernels have no stand-alone Policy.act (pgm_act_forward is compiled '
                           'per dim set); pgm_rollout_act_any acts on the rollout storage inside rollout()')
        P, N = self.P, obs.shape[1]
        obs = obs.to(device=self.dev, dtype=F32).contiguous()
        d = Dims(P, N, self.T, self.O, self.A, self.K, self.H, int(self.layernorm))
        value = torch.empty(P, N, self.K, dtype=F32, device=self.dev)
        logp = torch.empty(P, N, dtype=F32, device=self.dev)
        nz = None if noise is None else noise.to(device=self.dev, dtype=F32).contiguous()
        # discrete: noise is uniforms [N], the action the int32 index [P, N]
        action = torch.empty((P, N) if self.discrete else (P, N, self.A), dtype=I32 if self.discrete else F32,
                             device=self.dev)
        _call('pgm_act_forward_cat' if self.discrete else 'pgm_act_forward', C.byref(d), _ptr(self.params), _ptr(obs),
              _ptr(nz), int(deterministic), _ptr(value), _ptr(action), _ptr(logp))
        return value, action, logp

    def rollout(self, seed, noise=None, carry=True, env_noise=None):
        """noise: the steps' action noise (normals [T][N][A] / uniforms [T][N]); None: the counter stream of `seed`.
        env_noise (a contract-2 plug-in with NW > 0, fused or host-stepped): the steps' uniforms [T][N][NW] in
        [0, 1); None draws the stream of envplug.env_seed(seed)."""
        self.mode.rollout(self, seed, noise, carry, env_noise)

    def gae(self):
        name, lam = ('pgm_gae', self.gae_lambda) if self.lam_task is None else ('pgm_gae_tasks', _ptr(self.lam_task))
        _call(name, C.byref(self.dims), C.byref(self.c_rb), self.gamma, lam, int(self.use_gae), int(self.proper))

    def adv_normalize(self):
        var = self.obj_var if self.use_obj_rms else None
        _call('pgm_adv_normalize', C.byref(self.dims), C.byref(self.c_rb), _ptr(self.weights), _ptr(var))

    def make_perms(self, seed):
        E, n = self.perms.shape
        _call('pgm_randperm', n, E, C.c_uint64(seed), _ptr(self.perms))

    def ppo_update(self, perms=None, defer_flag=False):
        """The update on the current stream.  The exchange-timeout word of this launch is OR-ed into the sticky
        ``update_failed`` flag on the current stream, or (defer_flag) left to ``fold_update_flag`` on a stream that
        runs before the next update's launch (which resets the word)."""
        if self._reset_pending:  # the workspace reset queued on the side stream must land first
            self.wait_eval()
        if perms is not None:
            self.perms.copy_(torch.as_tensor(np.asarray(perms), dtype=I32))
        self.ppo_update_launch()
        if not defer_flag:
            self.fold_update_flag()

    def fold_update_flag(self):
        flag = self.update_ws[2 * self.P:2 * self.P + 1]
        torch.bitwise_or(self.update_failed, flag, out=self.update_failed)  # stream-ordered, no host sync

    def ppo_update_launch(self):
        """The family's update alone on the current stream (pgm_ppo_update: packed rows + the update kernel; the
        others gather from the storage themselves); after set_task_hparams, pgm_ppo_update_tasks."""
        fam, name, hp = self.family, self.family.ppo_update, (C.byref(self.hp),)
        if fam.tasks and self.hp_task is not None:
            name, hp = name + '_tasks', hp + (_ptr(self.hp_task),)
        self._launch(name, self.dims, *hp, _ptr(self.params), _ptr(self.adam_m), _ptr(self.adam_v),
                     _ptr(self.adam_step), _ptr(self.lr), _ptr(self.perms), C.byref(self.c_rb), _ptr(self.stats),
                     _ptr(self.update_ws), *((C.byref(launch_opts()),) if fam.opts else ()))

    def update_variant(self):
        """The update kernel pgm_ppo_update launches for this batch (pgm_ppo_update_variant: the launcher's own rule)."""
        if self.family.variant is not None:  # one kernel, no launch choice
            return self.family.variant
        buf = C.create_string_buffer(128)
        check(lib().pgm_ppo_update_variant(C.byref(self.dims), C.byref(self.hp), C.byref(launch_opts()), buf, 128),
              'pgm_ppo_update_variant')
        return buf.value.decode()

    def take_update_failed(self):
        """True if any PPO update since the last call timed out in a cross-workgroup exchange (its parameters /
        Adam state are invalid); resets the sticky flag.  Synchronises with the stream (after the overlapped
        evaluation, whose stream folds the last update's flag)."""
        self.wait_eval()
        word = int(self.update_failed.item())
        self.last_fail_word = word  # (the OR of the timed-out launches' words: kernels may encode the wait site)
        if word != 0:
            self.update_failed.zero_()
        return word != 0

    def check_update(self):
        """Raise PGMError if any PPO update since the last check timed out (take_update_failed).  Call it once
        per generation or after a timed region, not per update.  Multi-GPU callers share the flag across ranks
        first (MOPGPopulation.run) so that every rank raises together."""
        if self.take_update_failed():
            raise PGMError(f'{UPDATE_TIMEOUT_MSG} (word 0x{self.last_fail_word & (2**64 - 1):x})')

    def evaluate(self, ob_mean=None, ob_var=None, out=None):
        mean = self.ob_mean if ob_mean is None else ob_mean
        var = self.ob_var if ob_var is None else ob_var
        out = self.objs if out is None else out
        self.mode.evaluate(self, mean, var, out)
        return out

    @property
    def eval_stream(self):
        """Side stream of the overlapped evaluation (iteration(..., overlap_eval=True))."""
        if self._eval_stream is None:
            self._eval_stream = torch.cuda.Stream(device=self.dev)
        return self._eval_stream

    def wait_eval(self):
        """Order the current stream after the last overlapped evaluation (its objs are then readable)."""
        if self._eval_done is not None:
            torch.cuda.current_stream().wait_event(self._eval_done)
        self._reset_pending = False

    def iteration(self, j, lr, noise=None, perms=None, carry=True, overlap_eval=False, objs_out=None):
        """One MOPG iteration for every task: rollout, returns, advantages, PPO update, evaluation.

        noise/perms: the reference's RNG draws of iteration j (parity mode); None draws the
        device counter streams keyed by j (perf mode).  lr: a scalar, or one value per active task.

        overlap_eval: the evaluation of this iteration's snapshot (mopg.py:146-155) runs on a side stream,
        concurrently with the NEXT iteration's rollout / returns / advantages (which only read the
        parameters); the next PPO update (which writes them) waits for it.  It normalises with a copy of
        this iteration's ob_rms (the next rollout advances the live one) and writes objs_out (default
        self.objs), readable after wait_eval() or from work queued on eval_stream.

        A mode whose evaluation cannot overlap (HostMode: a host episode loop that synchronises every step) ignores
        overlap_eval: the evaluation runs after the update, with the live ob_rms (not yet advanced by a rollout)."""
        overlap_eval = overlap_eval and self.mode.overlap
        # perf mode: the counter stream of iteration j, drawn by one wide kernel up front (a mode with fused_noise
        # draws the same stream inside its rollout kernel: noise stays None)
        if noise is None and not self.mode.fused_noise:
            self._draw_noise(j)
            noise = self.noise
        perm_ready = None
        if perms is None and overlap_eval:  # the permutations (and lr) only feed the update: set beside the rollout
            side = self.eval_stream  # (behind the previous evaluation, itself behind the previous update)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self.set_lr(lr)
                self.make_perms(j)
                perm_ready = torch.cuda.Event()
                perm_ready.record(side)
        else:
            self.set_lr(lr)
        self.rollout(j, noise=noise, carry=carry)
        self.gae()
        self.adv_normalize()
        if perm_ready is not None:
            # one wait: the side stream ran the previous evaluation (which still reads the parameters) and the
            # workspace reset first
            torch.cuda.current_stream().wait_event(perm_ready)
            self._reset_pending = False
        else:
            if perms is None:
                self.make_perms(j)
            self.wait_eval()  # the previous overlapped evaluation still reads the parameters
        self.ppo_update(perms, defer_flag=overlap_eval)
        if not overlap_eval:
            self.evaluate(out=objs_out)
            return
        if self.P == self.capacity:
            self._eval_ob.copy_(self._ob_src)  # ob_mean | ob_var in one copy
        else:
            self._eval_mean.copy_(self.ob_mean)
            self._eval_var.copy_(self.ob_var)
        ready = torch.cuda.Event()
        ready.record()
        side = self.eval_stream
        side.wait_event(ready)
        with torch.cuda.stream(side):
            # the timeout word of this update, folded off the main stream, then the next update's workspace reset
            # (the next update waits for this stream: perm_ready)
            self.fold_update_flag()
            if self.family.opts:  # (the other families reset their own, smaller workspace: pgm_ppo_update_reset clears
                # the exchange slots of pgm_ppo_update's layout, which they do not have)
                _call('pgm_ppo_update_reset', C.byref(self.dims), _ptr(self.update_ws))
                self._reset_pending = True
            out = self.evaluate(self._eval_mean, self._eval_var, out=objs_out)
            out.record_stream(side)
            self._eval_done = torch.cuda.Event()
            self._eval_done.record(side)

    # ------------------------------------------------------------------ host transfer
    def set_task(self, p, state_dict, opt_state=None, env_params=None, weights=None):
        lay = self.layout
        self.params[p].copy_(torch.from_numpy(lay.flatten(state_dict)))
        m, v, step = lay.adam_from_optimizer_state(opt_state or {})
        self.adam_m[p].copy_(torch.from_numpy(m))
        self.adam_v[p].copy_(torch.from_numpy(v))
        self.adam_step[p] = step
        if weights is not None:
            self.weights[p].copy_(torch.as_tensor(np.asarray(weights, dtype=np.float64)))
        if env_params is not None:
            self.set_env_params(p, env_params)

    def set_env_params(self, p, env_params):
        """Restore ob_rms / ret_rms / obj_rms (mopg.py:70-75); obj_rms may still be scalar-shaped."""
        K = self.K
        ob, rt, oj = env_params.get('ob_rms'), env_params.get('ret_rms'), env_params.get('obj_rms')
        if ob is not None:
            self.ob_mean[p].copy_(torch.as_tensor(np.asarray(ob.mean, np.float64)))
            self.ob_var[p].copy_(torch.as_tensor(np.asarray(ob.var, np.float64)))
            self.ob_count[p] = float(ob.count)
        if rt is not None:
            self.ret_mean[p] = float(np.asarray(rt.mean).reshape(-1)[0])
            self.ret_var[p] = float(np.asarray(rt.var).reshape(-1)[0])
            self.ret_count[p] = float(rt.count)
        if oj is not None:
            self.obj_mean[p].copy_(torch.as_tensor(np.broadcast_to(np.asarray(oj.mean, np.float64), (K,)).copy()))
            self.obj_var[p].copy_(torch.as_tensor(np.broadcast_to(np.asarray(oj.var, np.float64), (K,)).copy()))
            self.obj_count[p] = float(oj.count)

    def get_params(self, p):
        return self.layout.unflatten(self.params[p])
