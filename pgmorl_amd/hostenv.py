"""Host-stepped environments: the vectorised env side of ``TaskBatch(host_env=...)``.

The environments run on the CPU; ``Policy.act``, VecNormalize, the rollout storage, GAE and the PPO update stay on the
device (pgm_rollout_act / pgm_env_ingest / pgm_eval_act, include/pgm_abi.h).  A ``HostVecEnv`` is P tasks x N
environments behind one ``step``: what the reference's per-task ``DummyVecEnv`` of N ``make_env`` thunks returns
(a2c_ppo_acktr/envs.py:84-119, dummy_vec_env.py:45-62), stacked over the tasks, with no normalisation applied -- raw
fp64 observations, the scalar env reward, ``info['obj']`` and the done / bad_transition flags.

* ``SynthHostVecEnv``  SynthMO (envspec.py) in numpy fp64: the stand-in that exercises the whole path without MuJoCo.
* ``DeepSeaTreasureHostVecEnv``  Deep Sea Treasure (``--host-env dst``), the discrete-action grid world of the reference's
                       shipped run, vectorised numpy.
* ``DummyMOHostVecEnv``  MO-Dummy-v0 / MO-Dummy3-v0 (``--host-env dummy``), the reference's MuJoCo-free continuous env,
                       vectorised numpy with the device env's operation order.
* ``PluginHostVecEnv``  a device env plug-in (envplug.EnvPlugin, ``--env-plugin HEADER --host-env plugin``) stepped on
                       the host by the plug-in library's own host functions: the same compiled header on the CPU.
* ``GymHostVecEnv``    any ``make_env(env_name, seed, rank)`` returning gym-style objects (duck-typed: gym itself is
                       never imported here), in the 4-tuple or the 5-tuple step API.
"""
import importlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import envspec

MAX_WORKERS = 16  # cap of GymHostVecEnv's optional thread pool (never sized from the machine's CPU count)


class HostVecEnv:
    """The protocol ``TaskBatch`` drives.  Attributes: ``P`` (active tasks), ``N`` (envs per task), ``obs_dim``,
    ``act_dim``, ``obj_num``.  Every task's env n is seeded ``seed + n`` (each task process of the reference builds
    its own ``make_vec_envs(env_name, seed, N)``, morl/mopg.py:67-69).

    ``discrete = True``: a Discrete(n) action space.  ``act_dim`` is then the number of actions n and ``step`` /
    ``eval_step`` receive the action indices as int32 [P, N] / [P, E] (the policy has the Categorical head)."""
    P = N = obs_dim = act_dim = obj_num = 0
    discrete = False

    def set_active(self, P):
        """Use the first P tasks (P <= the P of construction); followed by ``reset()``."""
        raise NotImplementedError

    def reset(self):
        """Fresh episodes everywhere -> obs f64 [P, N, O]."""
        raise NotImplementedError

    def step(self, actions):
        """actions f32 [P, N, A] (raw policy samples; the env clips) -> (obs f64 [P, N, O], reward f64 [P, N],
        done bool [P, N], bad bool [P, N], obj f64 [P, N, K]).  DummyVecEnv semantics: a done env is reset and obs is
        its reset observation, obj / reward / flags are the terminal step's.  bad: the episode ended at a time
        limit (TimeLimitMask's bad_transition), not in a true terminal state."""
        raise NotImplementedError

    def eval_reset(self, eval_num):
        """eval_num fresh evaluation episodes per task, episode e seeded ``seed + e`` (morl/mopg.py:30-33)
        -> obs f64 [P, E, O]."""
        raise NotImplementedError

    def eval_step(self, actions):
        """actions f32 [P, E, A] -> (obs f64 [P, E, O], obj f64 [P, E, K], done bool [P, E]).  No auto-reset: an
        ended episode's later outputs are masked by the caller."""
        raise NotImplementedError

    def close(self):
        pass

    def dims(self):
        return self.obs_dim, self.act_dim, self.obj_num


class SynthHostVecEnv(HostVecEnv):
    """SynthMO on the host, fp64: a_c = clip(a, lo, hi); s' = tanh(d s + U a_c + c); obj = V s' + ebase - ecoef
    sum(a_c^2); scalar reward 0; done at ``max_episode_steps`` (bad_transition set), then auto-reset to the env's
    reset state.  Constants and reset states are envspec's, so it is the device envs' dynamics exactly."""

    def __init__(self, env_name, P, N, seed=0, max_episode_steps=None):
        sp = envspec.make_spec(env_name)
        if sp.get('user'):
            raise ValueError(f'{env_name} is a registered third-party env with no SynthMO stand-in (use --host-env '
                             f'module:callable)')
        if sp.get('discrete'):
            raise ValueError(f'{env_name} has discrete actions and no SynthMO stand-in (use --host-env dst)')
        if sp.get('native'):
            raise ValueError(f'{env_name} is a native env with no SynthMO stand-in (use --host-env {sp["native"]})')
        self.spec = sp
        self.env_name, self.seed = env_name, seed
        self.capacity = self.P = P
        self.N = N
        self.obs_dim, self.act_dim, self.obj_num = sp['obs_dim'], sp['act_dim'], sp['obj_num']
        self.max_episode_steps = int(max_episode_steps or sp['max_episode_steps'])
        self.s0 = envspec.reset_table(self.obs_dim, seed, N)  # [N, O]: env n of every task
        self.s = self.elapsed = None
        self._es = self._eel = None

    def set_active(self, P):
        if not 0 < P <= self.capacity:
            raise ValueError(f'active tasks {P} outside [1, {self.capacity}]')
        self.P = P
        self.s = self.elapsed = None

    def _dynamics(self, s, actions):
        sp = self.spec
        a_c = np.clip(np.asarray(actions, dtype=np.float64), sp['act_lo'], sp['act_hi'])
        s = np.tanh(sp['d'] * s + np.einsum('oa,pna->pno', sp['U'], a_c) + sp['c'])
        obj = (np.einsum('ko,pno->pnk', sp['V'], s) + sp['ebase']
               - sp['ecoef'] * np.sum(np.square(a_c), axis=-1, keepdims=True))
        return s, obj

    def terminal(self, s, obj):
        """True terminal states [P, N] of the step just taken (none in SynthMO; a subclass may end episodes early)."""
        return np.zeros(s.shape[:2], dtype=bool)

    def reset(self):
        self.s = np.broadcast_to(self.s0, (self.P, self.N, self.obs_dim)).copy()
        self.elapsed = np.zeros((self.P, self.N), dtype=np.int64)
        return self.s.copy()

    def step(self, actions):
        self.s, obj = self._dynamics(self.s, actions)
        self.elapsed += 1
        limit = self.elapsed >= self.max_episode_steps
        term = self.terminal(self.s, obj)
        done = limit | term
        bad = limit & ~term
        if done.any():
            self.s[done] = np.broadcast_to(self.s0, self.s.shape)[done]
            self.elapsed[done] = 0
        return self.s.copy(), np.zeros((self.P, self.N)), done, bad, obj

    def eval_reset(self, eval_num):
        s0 = envspec.reset_table(self.obs_dim, self.seed, eval_num)
        self._es = np.broadcast_to(s0, (self.P, eval_num, self.obs_dim)).copy()
        self._eel = np.zeros((self.P, eval_num), dtype=np.int64)
        return self._es.copy()

    def eval_step(self, actions):
        self._es, obj = self._dynamics(self._es, actions)
        self._eel += 1
        done = (self._eel >= self.max_episode_steps) | self.terminal(self._es, obj)
        return self._es.copy(), obj, done


class DeepSeaTreasureHostVecEnv(HostVecEnv):
    """Deep Sea Treasure (MO-DeepSeaTreasure-v0: obs 3, Discrete(4), 2 objectives), P x N grids in numpy.

    An 11 x 11 grid; cell (r, c) is water if r == 0 or r <= c, otherwise wall; the treasure cells (1,0) = 1,
    (2,1) = 3, (4,3) = 8, (7,6) = 20 can be entered.  An episode starts at (0, 0).  Actions 0 up, 1 down, 2 left,
    3 right; a move into a wall or off the grid leaves the position unchanged.  Every step t += 1; on a treasure cell
    reward = obj_0 = its value and obj_1 = 10 / (t + 1), otherwise all three are 0.  The episode ends on a treasure or
    at t == max_steps.  The raw observation is [r / 10, c / 10, t / max_steps], rounded to fp32 (the env's dtype) and
    widened.  The step limit is reported as a termination (bad = False), as the env itself reports it;
    ``time_limit_is_bad=True`` reports it as a time-limit end instead (tests: both kinds of episode end)."""
    discrete = True
    SIZE = 11
    TREASURES = {(1, 0): 1.0, (2, 1): 3.0, (4, 3): 8.0, (7, 6): 20.0}
    _DR = np.array([-1, 1, 0, 0])
    _DC = np.array([0, 0, -1, 1])

    def __init__(self, env_name='MO-DeepSeaTreasure-v0', P=1, N=1, seed=0, max_steps=None, time_limit_is_bad=False):
        sp = envspec.make_spec(env_name)
        if sp.get('user') or not sp.get('discrete') or (sp['obs_dim'], sp['act_dim'], sp['obj_num']) != (3, 4, 2):
            raise ValueError(f'{env_name} is not a Deep Sea Treasure env (obs 3, 4 actions, 2 objectives)')
        self.env_name, self.seed = env_name, seed  # (the env draws nothing: every seed gives the same episodes)
        self.capacity = self.P = P
        self.N = N
        self.obs_dim, self.act_dim, self.obj_num = sp['obs_dim'], sp['act_dim'], sp['obj_num']
        self.max_steps = int(max_steps or sp['max_episode_steps'])
        self.time_limit_is_bad = bool(time_limit_is_bad)
        n = self.SIZE
        r, c = np.mgrid[0:n, 0:n]
        self.value = np.zeros((n, n))
        for cell, v in self.TREASURES.items():
            self.value[cell] = v
        self.open = (r == 0) | (r <= c) | (self.value > 0)
        self._st = self._est = None  # (row, col, t) int64 [P, N] / [P, E]
        self._edone = None

    def set_active(self, P):
        if not 0 < P <= self.capacity:
            raise ValueError(f'active tasks {P} outside [1, {self.capacity}]')
        self.P = P
        self._st = None

    def _obs(self, st):
        r, c, t = st
        o = np.stack([r / (self.SIZE - 1), c / (self.SIZE - 1), t / self.max_steps], axis=-1)
        return o.astype(np.float32).astype(np.float64)

    def _move(self, st, actions, frozen=None):
        """One step of every env not in ``frozen`` -> (treasure value, fuel objective, found, at the step limit)."""
        r, c, t = st
        a = np.asarray(actions).astype(np.int64)
        a = np.where((a >= 0) & (a < 4), a, 0)
        nr, nc = r + self._DR[a], c + self._DC[a]
        n = self.SIZE
        ok = (nr >= 0) & (nr < n) & (nc >= 0) & (nc < n)
        ok &= self.open[np.clip(nr, 0, n - 1), np.clip(nc, 0, n - 1)]
        if frozen is not None:
            ok &= ~frozen
        r[...] = np.where(ok, nr, r)
        c[...] = np.where(ok, nc, c)
        t += 1 if frozen is None else (~frozen).astype(np.int64)
        val = self.value[r, c]
        found = val > 0
        if frozen is not None:
            val, found = np.where(frozen, 0.0, val), found & ~frozen
        fuel = np.where(found, 10.0 / (t + 1), 0.0)
        return val, fuel, found, t >= self.max_steps

    def reset(self):
        self._st = tuple(np.zeros((self.P, self.N), dtype=np.int64) for _ in range(3))
        return self._obs(self._st)

    def step(self, actions):
        val, fuel, found, limit = self._move(self._st, actions)
        done = found | limit
        bad = limit & ~found if self.time_limit_is_bad else np.zeros_like(done)
        for x in self._st:  # DummyVecEnv auto-reset: the returned observation is the next episode's first
            x[done] = 0
        return self._obs(self._st), val.copy(), done, bad, np.stack([val, fuel], axis=-1)

    def eval_reset(self, eval_num):
        self._est = tuple(np.zeros((self.P, eval_num), dtype=np.int64) for _ in range(3))
        self._edone = np.zeros((self.P, eval_num), dtype=bool)
        return self._obs(self._est)

    def eval_step(self, actions):
        val, fuel, found, limit = self._move(self._est, actions, frozen=self._edone)  # ended episodes stand still
        self._edone = self._edone | found | limit
        return self._obs(self._est), np.stack([val, fuel], axis=-1), self._edone.copy()


class DummyMOHostVecEnv(HostVecEnv):
    """MO-Dummy-v0 / MO-Dummy3-v0 (obs 6, act 2, 2 or 3 objectives; the reference's environments/dummy_mo_env.py:57-148),
    P x N envs in numpy fp64.  The rule of csrc/pgm_dummy.hpp, every operation elementwise in the same order (no dot
    products or norms whose summation order numpy chooses), so that the fp64 outputs are the device's bit for bit:

        ac = clip(a, -1, 1); last = pos; vel = (vel + ac * 0.1) * 0.95; pos = pos + vel; step += 1
        step_distance = sqrt(dx*dx + dy*dy), d = pos - last; step_energy = sqrt(ac0*ac0 + ac1*ac1); totals accumulate
        obj = [step_distance, 1 / (step_energy + 0.1), bound - |pos| (3 objectives)]; reward = obj0 + 0.1 * obj1
        done = step >= max_steps or |pos| > bound; bad = time_limit_is_bad and done and step == max_steps

    The raw observation is [pos, vel, total_distance, total_energy] in fp64.  A done env resets to the next position
    of its row of envspec.dummy_reset_table (episode e of env n: entry (n, e mod R)); evaluation episode e starts at
    entry (e, 0) of the table of eval_num seeds."""

    def __init__(self, env_name='MO-Dummy-v0', P=1, N=1, seed=0, max_steps=None, bound=None, time_limit_is_bad=True,
                 R=None):
        sp = envspec.make_spec(env_name)
        if sp.get('native') != 'dummy':
            raise ValueError(f'{env_name} is not an MO-Dummy env ({envspec.native_env_names()})')
        self.env_name, self.seed = env_name, seed
        self.capacity = self.P = P
        self.N = N
        self.obs_dim, self.act_dim, self.obj_num = sp['obs_dim'], sp['act_dim'], sp['obj_num']
        self.max_steps = int(max_steps or sp['max_episode_steps'])
        self.bound = float(sp['bound'] if bound is None else bound)
        self.time_limit_is_bad = bool(time_limit_is_bad)
        self.R = int(envspec.DUMMY_RESETS if R is None else R)
        self.resets = envspec.dummy_reset_table(seed, N, self.R)  # [N, R, 2]: env n of every task
        self._st = self._est = None  # {'s': f64 [P, N, 6], 'step': i64 [P, N], 'episode': i64 [P, N]}
        self._edone = None

    def set_active(self, P):
        if not 0 < P <= self.capacity:
            raise ValueError(f'active tasks {P} outside [1, {self.capacity}]')
        self.P = P
        self._st = None

    def _fresh(self, pos):
        s = np.zeros(pos.shape[:2] + (6,))
        s[..., :2] = pos
        return {'s': s, 'step': np.zeros(pos.shape[:2], dtype=np.int64),
                'episode': np.zeros(pos.shape[:2], dtype=np.int64)}

    def _move(self, st, actions, frozen=None):
        """One step of every env not in ``frozen`` -> (obj [.., K], reward, done, on the limit step)."""
        s = st['s']
        a = np.asarray(actions, dtype=np.float32).astype(np.float64)
        ac0, ac1 = np.clip(a[..., 0], -1.0, 1.0), np.clip(a[..., 1], -1.0, 1.0)
        lx, ly = s[..., 0], s[..., 1]
        vx = (s[..., 2] + ac0 * 0.1) * 0.95
        vy = (s[..., 3] + ac1 * 0.1) * 0.95
        px, py = lx + vx, ly + vy
        dx, dy = px - lx, py - ly
        dist = np.sqrt(dx * dx + dy * dy)
        energy = np.sqrt(ac0 * ac0 + ac1 * ac1)
        r = np.sqrt(px * px + py * py)
        new = np.stack([px, py, vx, vy, s[..., 4] + dist, s[..., 5] + energy], axis=-1)
        step = st['step'] + 1
        obj = [dist, 1.0 / (energy + 0.1)]
        if self.obj_num == 3:
            obj.append(self.bound - r)
        obj = np.stack(obj, axis=-1)
        reward = obj[..., 0] + 0.1 * obj[..., 1]
        done = (step >= self.max_steps) | (r > self.bound)
        limit = step == self.max_steps
        if frozen is not None:
            new, step = np.where(frozen[..., None], s, new), np.where(frozen, st['step'], step)
            obj, reward = np.where(frozen[..., None], 0.0, obj), np.where(frozen, 0.0, reward)
            done, limit = done & ~frozen, limit & ~frozen
        st['s'], st['step'] = new, step
        return obj, reward, done, limit

    def reset(self):
        self._st = self._fresh(np.broadcast_to(self.resets[:, 0], (self.P, self.N, 2)))
        return self._st['s'].copy()

    def step(self, actions):
        st = self._st
        obj, reward, done, limit = self._move(st, actions)
        bad = done & limit if self.time_limit_is_bad else np.zeros_like(done)
        if done.any():  # DummyVecEnv auto-reset: the returned observation is the next episode's first
            st['episode'] = st['episode'] + done
            n = np.broadcast_to(np.arange(self.N), done.shape)
            pos = self.resets[n, st['episode'] % self.R]
            fresh = np.zeros_like(st['s'])
            fresh[..., :2] = pos
            st['s'] = np.where(done[..., None], fresh, st['s'])
            st['step'] = np.where(done, 0, st['step'])
        return st['s'].copy(), reward, done, bad, obj

    def eval_reset(self, eval_num):
        tab = envspec.dummy_reset_table(self.seed, eval_num, self.R)
        self._est = self._fresh(np.broadcast_to(tab[:, 0], (self.P, eval_num, 2)))
        self._edone = np.zeros((self.P, eval_num), dtype=bool)
        return self._est['s'].copy()

    def eval_step(self, actions):
        obj, _, done, _ = self._move(self._est, actions, frozen=self._edone)  # ended episodes stand still
        self._edone = self._edone | done
        return self._est['s'].copy(), obj, self._edone.copy()


class PluginHostVecEnv(HostVecEnv):
    """A device env plug-in (envplug.EnvPlugin) stepped on the host: ``step``, ``eval_step`` and the resets call the
    plug-in library's pgm_envplug_transition / pgm_envplug_reset, i.e. the compiled header's own functions with the
    forced step limit and the auto-reset.  The reference point of the fused path (for a header without transcendentals
    the two agree bit for bit) and a debugging path for the header's author.  Env n of every task uses row n of
    envspec.plugin_reset_table(seed, N, R, RW); evaluation episode e starts at entry (e, 0) of the eval_num-row
    table.

    A contract-2 header gets what the fused kernels give it: the runtime parameters ``env_params`` (a dict over the
    header's names; omitted names take the default) and, per step, the uniforms of the env-noise stream at the fused
    path's indices -- training word j of (step t, env n): element (t N + n) NW + j of the rollout's env_seed
    (``begin_rollout``, which restarts t); evaluation word j of (episode e, step it): element (e MAX_STEPS + it) NW + j
    of envplug.env_seed(seed)."""

    def __init__(self, plugin, P, N, seed=0, R=None, env_params=None):
        from . import envplug
        self.plugin = pl = envplug.as_plugin(plugin)
        self.par = pl.par_vector(env_params)
        self.seed = seed
        self._env_seed = self._eval_env_seed = envplug.env_seed(seed)
        self._env_noise = None
        self._t = self._et = 0
        self.capacity = self.P = P
        self.N = N
        self.obs_dim, self.act_dim, self.obj_num = pl.O, pl.A, pl.K
        self.discrete = pl.DISCRETE
        self.R = int(envplug.DEFAULT_RESETS if R is None else R)
        self.table = envspec.plugin_reset_table(seed, N, self.R, pl.RW)
        self._st = self._est = self._etable = self._edone = None

    def set_active(self, P):
        if not 0 < P <= self.capacity:
            raise ValueError(f'active tasks {P} outside [1, {self.capacity}]')
        self.P = P
        self._st = None

    def _fresh(self, P, M, table):
        row = np.broadcast_to(np.arange(M, dtype=np.int32), (P, M)).reshape(-1).copy()
        zero = np.zeros(P * M, dtype=np.int32)
        sd, si, obs = self.plugin.reset(row, zero, table, par=self.par)
        return {'sd': sd, 'si': si, 'elapsed': zero.copy(), 'episode': zero.copy(), 'row': row}, obs

    def begin_rollout(self, env_seed, env_noise=None):
        """The env noise of the rollout that starts now: the stream of ``env_seed`` from step 0, or the fed uniforms
        ``env_noise`` [T][N][NW] (what pgm_envplug_rollout_ex takes as env_rnd)."""
        self._env_seed, self._t = int(env_seed), 0
        self._env_noise = None if env_noise is None else np.asarray(env_noise, dtype=np.float64)

    def _train_w(self):
        """[P N][NW]: step t's uniforms of env n, the same for every task; None for a header without them."""
        NW, N = self.plugin.NW, self.N
        if NW == 0:
            return None
        if self._env_noise is not None:
            w = self._env_noise[self._t].reshape(N, NW)
        else:
            w = self.plugin.uniforms(self._env_seed, self._t * N * NW, N * NW).reshape(N, NW)
        return np.broadcast_to(w, (self.P, N, NW)).reshape(-1, NW)

    def _eval_w(self, E):
        NW, L = self.plugin.NW, self.plugin.MAX_STEPS
        if NW == 0:
            return None
        w = np.stack([self.plugin.uniforms(self._eval_env_seed, (e * L + self._et) * NW, NW) for e in range(E)])
        return np.broadcast_to(w, (self.P, E, NW)).reshape(-1, NW)

    def _action(self, actions):
        if self.discrete:
            return np.asarray(actions).astype(np.int32).reshape(-1)
        return np.asarray(actions, dtype=np.float32).reshape(-1, self.act_dim)

    def reset(self):
        self._st, obs = self._fresh(self.P, self.N, self.table)
        self._t = 0
        return obs.reshape(self.P, self.N, self.obs_dim)

    def step(self, actions):
        st, P, N = self._st, self.P, self.N
        o = self.plugin.transition(st['sd'], st['si'], st['elapsed'], st['episode'], st['row'],
                                   self._action(actions), self.table, par=self.par, w=self._train_w())
        self._t += 1
        for k in ('sd', 'si', 'elapsed', 'episode'):
            st[k] = o[k]
        return (o['obs'].reshape(P, N, self.obs_dim), o['reward'].reshape(P, N), o['done'].reshape(P, N).astype(bool),
                o['bad'].reshape(P, N).astype(bool), o['obj'].reshape(P, N, self.obj_num))

    def eval_reset(self, eval_num):
        self._etable = envspec.plugin_reset_table(self.seed, eval_num, self.R, self.plugin.RW)
        self._est, obs = self._fresh(self.P, eval_num, self._etable)
        self._edone = np.zeros(self.P * eval_num, dtype=bool)
        self._eobs = obs
        self._et = 0
        return obs.reshape(self.P, eval_num, self.obs_dim).copy()

    def eval_step(self, actions):
        st, P = self._est, self.P
        E = self._edone.size // P
        act = self._action(actions)
        if self.discrete:  # an ended episode's action is not looked at (and may be anything)
            act = np.where(self._edone, 0, act).astype(np.int32)
        o = self.plugin.transition(st['sd'], st['si'], st['elapsed'], st['episode'], st['row'], act, self._etable,
                                   par=self.par, w=self._eval_w(E))
        self._et += 1
        live = ~self._edone  # ended episodes stand still
        for k in ('sd', 'si', 'elapsed', 'episode'):
            m = live.reshape((-1,) + (1,) * (o[k].ndim - 1))
            st[k] = np.where(m, o[k], st[k])
        done = o['done'].astype(bool) & live
        # (a done episode has been auto-reset by the transition; it is never stepped again, its state is not read)
        self._eobs = np.where((live & ~done)[:, None], o['obs'], self._eobs)
        obj = np.where(live[:, None], o['obj'], 0.0)
        self._edone = self._edone | done
        return (self._eobs.reshape(P, E, self.obs_dim).copy(), obj.reshape(P, E, self.obj_num),
                self._edone.reshape(P, E).copy())


def _reset_obs(r):
    """env.reset(): obs (old API) or (obs, info) (new API)."""
    if isinstance(r, tuple) and len(r) == 2 and isinstance(r[1], dict):
        r = r[0]
    return np.asarray(r, dtype=np.float64).reshape(-1)


def _step_env(env, action):
    """One env.step in either API -> (obs, reward, done, bad, obj)."""
    r = env.step(action)
    if len(r) == 5:  # obs, reward, terminated, truncated, info
        obs, rew, term, trunc, info = r
        done, bad = bool(term) or bool(trunc), bool(trunc) and not bool(term)
    else:  # obs, reward, done, info: TimeLimitMask's key, or gym's own TimeLimit flag
        obs, rew, done, info = r
        done = bool(done)
        bad = 'bad_transition' in info or bool(info.get('TimeLimit.truncated', False))
    return (np.asarray(obs, dtype=np.float64).reshape(-1), float(rew), done, bad,
            np.asarray(info['obj'], dtype=np.float64).reshape(-1))


def is_discrete(space):
    """A gym-style action space with an ``n`` attribute is Discrete(n)."""
    return hasattr(space, 'n')


def probe_dims(env):
    """(obs_dim, act_dim, obj_num) of one gym-style multi-objective env (resets it; may step it once).  For a
    discrete action space act_dim is its number of actions n."""
    obs = _reset_obs(env.reset())
    disc = is_discrete(env.action_space)
    act_dim = int(env.action_space.n) if disc else int(np.prod(env.action_space.shape))
    inner = getattr(env, 'unwrapped', env)
    obj_num = getattr(inner, 'obj_dim', None)
    if obj_num is None:
        obj_num = _step_env(env, 0 if disc else np.zeros(act_dim, dtype=np.float32))[4].size
        env.reset()
    return obs.size, act_dim, int(obj_num)


class GymHostVecEnv(HostVecEnv):
    """P x N env objects from ``make_env(env_name, seed, rank)`` (rank n of every task: the env is expected to be
    seeded ``seed + rank``, as a2c_ppo_acktr/envs.py:47 does), stepped in a host loop or by ``workers`` threads.
    Evaluation episodes run on fresh ``make_env(env_name, seed, eval_id)`` objects, i.e. seeded ``seed + eval_id``."""

    def __init__(self, make_env, env_name, P, N, seed=0, workers=0):
        self.make_env, self.env_name, self.seed = make_env, env_name, seed
        self.capacity = self.P = P
        self.N = N
        self.envs = [[make_env(env_name, seed, n) for n in range(N)] for _ in range(P)]
        self.obs_dim, self.act_dim, self.obj_num = probe_dims(self.envs[0][0])
        self.discrete = is_discrete(self.envs[0][0].action_space)  # then step passes Python ints
        self._eval = []
        workers = min(MAX_WORKERS, int(workers), P * N)
        self._pool = ThreadPoolExecutor(max_workers=workers) if workers > 1 else None

    def _map(self, fn, items):
        return list(self._pool.map(fn, items)) if self._pool is not None else [fn(x) for x in items]

    def set_active(self, P):
        if not 0 < P <= self.capacity:
            raise ValueError(f'active tasks {P} outside [1, {self.capacity}]')
        self.P = P

    def reset(self):
        flat = [e for row in self.envs[:self.P] for e in row]
        obs = self._map(lambda e: _reset_obs(e.reset()), flat)
        return np.stack(obs).reshape(self.P, self.N, self.obs_dim)

    def step(self, actions):
        actions = np.asarray(actions)
        act = (lambda p, n: int(actions[p, n])) if self.discrete else (lambda p, n: actions[p, n])
        jobs = [(self.envs[p][n], act(p, n)) for p in range(self.P) for n in range(self.N)]

        def one(job):
            env, a = job
            obs, rew, done, bad, obj = _step_env(env, a)
            if done:  # DummyVecEnv auto-reset: the returned observation is the next episode's first
                obs = _reset_obs(env.reset())
            return obs, rew, done, bad, obj
        out = self._map(one, jobs)
        P, N = self.P, self.N
        return (np.stack([o[0] for o in out]).reshape(P, N, self.obs_dim),
                np.array([o[1] for o in out], dtype=np.float64).reshape(P, N),
                np.array([o[2] for o in out], dtype=bool).reshape(P, N),
                np.array([o[3] for o in out], dtype=bool).reshape(P, N),
                np.stack([o[4] for o in out]).reshape(P, N, self.obj_num))

    def _close_eval(self):
        for row in self._eval:
            for e in row:
                if hasattr(e, 'close'):
                    e.close()
        self._eval = []

    def eval_reset(self, eval_num):
        self._close_eval()
        self._eval = [[self.make_env(self.env_name, self.seed, e) for e in range(eval_num)] for _ in range(self.P)]
        self._eval_done = np.zeros((self.P, eval_num), dtype=bool)
        obs = [_reset_obs(e.reset()) for row in self._eval for e in row]
        self._eval_obs = np.stack(obs).reshape(self.P, eval_num, self.obs_dim)
        return self._eval_obs.copy()

    def eval_step(self, actions):
        actions = np.asarray(actions)
        E = self._eval_done.shape[1]
        obj = np.zeros((self.P, E, self.obj_num))
        for p in range(self.P):
            for e in range(E):
                if self._eval_done[p, e]:  # an ended episode is not stepped again
                    continue
                a = int(actions[p, e]) if self.discrete else actions[p, e]
                o, _, done, _, ob = _step_env(self._eval[p][e], a)
                self._eval_obs[p, e], obj[p, e], self._eval_done[p, e] = o, ob, done
        return self._eval_obs.copy(), obj, self._eval_done.copy()

    def close(self):
        self._close_eval()
        if self._pool is not None:
            self._pool.shutdown()
            self._pool = None
        for row in self.envs:
            for e in row:
                if hasattr(e, 'close'):
                    e.close()


def resolve(spec):
    """``--host-env SPEC`` -> factory(env_name, P, N, seed) of a HostVecEnv.  ``synth``: SynthHostVecEnv; ``dst``:
    DeepSeaTreasureHostVecEnv; ``dummy``: DummyMOHostVecEnv (the MO-Dummy envs only); ``module:callable``:
    GymHostVecEnv over ``callable(env_name, seed, rank)``.  Raises ValueError for a spec that cannot be imported."""
    if spec == 'synth':
        return SynthHostVecEnv
    if spec == 'dst':
        return DeepSeaTreasureHostVecEnv
    if spec == 'dummy':
        return DummyMOHostVecEnv
    mod, sep, name = str(spec).partition(':')
    if not sep or not mod or not name:
        raise ValueError(f'--host-env {spec!r}: expected "synth", "dst", "dummy" or "module:callable"')
    try:
        fn = getattr(importlib.import_module(mod), name)
    except (ImportError, AttributeError) as e:
        raise ValueError(f'--host-env {spec!r}: cannot import ({e})') from e
    if not callable(fn):
        raise ValueError(f'--host-env {spec!r}: {name} is not callable')
    return lambda env_name, P, N, seed=0: GymHostVecEnv(fn, env_name, P, N, seed)


def register_from_spec(spec, env_name, seed=0):
    """For a ``module:callable`` spec and an env name envspec does not know: build one env, read its dims
    (``probe_dims``, ``is_discrete``), register them (``envspec.register_env``: ValueError for dims outside the
    runtime-dim kernels' range) and close the env.  Returns whether it registered; ``synth`` / ``dst`` / ``dummy`` and
    names envspec knows are left alone, so an unknown name behind those still raises in ``check_spec``."""
    if spec in ('synth', 'dst', 'dummy'):
        return False
    try:
        envspec.make_spec(env_name)
        return False
    except ValueError:
        pass
    mod, sep, name = str(spec).partition(':')
    if not sep or not mod or not name:
        return False  # resolve() words the refusal
    try:
        fn = getattr(importlib.import_module(mod), name)
    except (ImportError, AttributeError) as e:
        raise ValueError(f'--host-env {spec!r}: cannot import ({e})') from e
    env = fn(env_name, seed, 0)
    try:
        O, A, K = probe_dims(env)
        disc = is_discrete(env.action_space)
    finally:
        if hasattr(env, 'close'):
            env.close()
    envspec.register_env(env_name, O, A, K, discrete=disc)
    return True


def check_spec(spec, env_name, seed=0):
    """Refuse, before anything is written or allocated, a --host-env whose env dims are not envspec's for env_name
    (the kernels are compiled for those dims).  Returns the factory."""
    factory = resolve(spec)
    want = envspec.make_spec(env_name)
    if want.get('user') and spec in ('synth', 'dst', 'dummy'):
        raise ValueError(f'--host-env {spec} cannot step the registered third-party env {env_name} (use --host-env '
                         f'module:callable)')
    if spec == 'dummy' and want.get('native') != 'dummy':
        raise ValueError(f'--host-env dummy steps the MO-Dummy envs only ({envspec.native_env_names()}), not {env_name}')
    want = (want['obs_dim'], want['act_dim'], want['obj_num'])
    probe = factory(env_name, 1, 1, seed)
    try:
        got = probe.dims()
    finally:
        probe.close()
    if tuple(got) != want:
        raise ValueError(f'--host-env {spec!r}: {env_name} has (obs, act, obj) dims {tuple(got)}, the kernels of '
                         f'{env_name} are built for {want}')
    return factory
