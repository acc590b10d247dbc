"""numpy fp64 restatements of the contract-2 test env plug-ins of tests/envplug2/*.hpp (include/pgm_envplug.h: runtime
parameters and per-step uniforms), in the shape of tests/envplug_envs.py: vectorised over n envs, every operation
elementwise and in the header's order, so that the fp64 outputs equal the compiled header's bit for bit.  ``reset``,
``observe`` and ``step`` take the parameter vector ``par`` [NP]; ``step`` also takes the step's uniforms ``w`` [n, NW].
``transition`` restates the caller's side (the forced limit, the auto-reset) and ``NumpyPlugin2HostVecEnv`` is the
``HostVecEnv`` over a restatement with the env-noise stream restated from oracle/streams.py.
"""
import os

import numpy as np

from oracle import streams
from pgmorl_amd import envspec
from pgmorl_amd.hostenv import HostVecEnv

from .envplug_envs import INFO_FIELDS, Line, _clip1, _f64

HERE = os.path.dirname(os.path.abspath(__file__))
ENV_SEED_XOR = 0x5EEDE27A0153C0DE  # envplug.ENV_SEED_XOR, restated


def header(name):
    return os.path.join(HERE, 'envplug2', name + '.hpp')


def env_seed(seed):
    return (int(seed) ^ ENV_SEED_XOR) & 0xFFFFFFFFFFFFFFFF


def u53(seed, start, n):
    """Elements start .. start + n - 1 of the env-noise stream: the top 53 bits of oracle.streams.hash_at."""
    h = streams.hash_at(seed, np.arange(start, start + n, dtype=np.uint64))
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


class Slip:
    NAME, ENV = 'slip', 'Slip-v0'
    O, A, K, DISCRETE, SD, SI, RW, MAX_STEPS = 3, 1, 2, False, 2, 0, 1, 12
    CONTRACT, NP, NW = 2, 2, 1
    PAR_NAMES, PAR_DEFAULT = ('slip', 'wind'), (0.2, 0.05)
    BOUND = 1.0

    @staticmethod
    def reset(u, par):
        h = u[:, 0] - 0.5
        return np.stack([h * 0.5, np.zeros(len(u))], axis=-1), np.zeros((len(u), 0), dtype=np.int32)

    @staticmethod
    def observe(sd, si, par):
        return np.stack([sd[:, 0], sd[:, 1], sd[:, 0] * sd[:, 0]], axis=-1)

    @staticmethod
    def step(sd, si, action, par, w):
        a = _f64(action).reshape(len(sd), 1)[:, 0]
        ac = _clip1(a)
        ae = np.where(w[:, 0] < par[0], 0.0, ac)
        m = 0.3 * ae + par[1]
        x = sd[:, 0] + m
        obj = np.stack([1.0 + m, 1.0 - ac * ac], axis=-1)
        reward = obj[:, 0] + 0.5 * obj[:, 1]
        done = np.abs(x) > Slip.BOUND
        margin = np.minimum(np.abs(np.abs(a) - 1.0), np.abs(np.abs(x) - Slip.BOUND))
        return (np.stack([x, m], axis=-1), si, obj, reward, done.astype(np.int32), np.zeros(len(sd), dtype=np.int32),
                margin)


class Gather:
    NAME, ENV = 'gather', 'Gather-v0'
    O, A, K, DISCRETE, SD, SI, RW, MAX_STEPS = 4, 4, 3, True, 0, 3, 1, 10
    CONTRACT, NP, NW = 2, 1, 3
    PAR_NAMES, PAR_DEFAULT = ('p_attack',), (0.1,)

    @staticmethod
    def reset(u, par):
        x = np.where(u[:, 0] < 0.5, 0, 1)
        z = np.zeros_like(x)
        return np.zeros((len(u), 0)), np.stack([x, z, z], axis=-1).astype(np.int32)

    @staticmethod
    def observe(sd, si, par):
        return np.stack([si[:, 0].astype(np.float64) / 2.0, si[:, 1].astype(np.float64) / 2.0,
                         (si[:, 2] & 1).astype(np.float64), ((si[:, 2] >> 1) & 1).astype(np.float64)], axis=-1)

    @staticmethod
    def step(sd, si, action, par, w):
        a = np.asarray(action).astype(np.int32).reshape(len(si))
        x = np.clip(si[:, 0] + (a == 0) - (a == 1), 0, 2)
        y = np.clip(si[:, 1] + (a == 2) - (a == 3), 0, 2)
        moved = (x != si[:, 0]) | (y != si[:, 1])
        carried = si[:, 2].copy()
        enemy = moved & (x == 1) & (y <= 1)
        gold = moved & ~enemy & (x == 2) & (y == 0)
        gem = moved & ~enemy & (x == 2) & (y == 2)
        home = moved & (x == 0) & (y == 0) & (carried != 0)
        attacked = enemy & (w[:, 0] < par[0])
        carried = np.where(gold & ((carried & 1) == 0) & (w[:, 1] < 0.9), carried | 1, carried)
        carried = np.where(gem & ((carried & 2) == 0) & (w[:, 2] < 0.8), carried | 2, carried)
        obj = np.stack([np.where(attacked, -1.0, -0.05), np.where(home, (carried & 1).astype(np.float64), 0.0),
                        np.where(home, ((carried >> 1) & 1).astype(np.float64), 0.0)], axis=-1)
        reward = (obj[:, 0] + obj[:, 1]) + obj[:, 2]
        done = attacked | home
        return (sd, np.stack([x, y, carried], axis=-1).astype(np.int32), obj, reward, done.astype(np.int32),
                np.zeros(len(si), dtype=np.int32), np.full(len(si), np.inf))


class ParMax:
    NAME, ENV = 'parmax', 'ParMax-v0'
    O, A, K, DISCRETE, SD, SI, RW, MAX_STEPS = 2, 1, 3, False, 1, 0, 1, 6
    CONTRACT, NP, NW = 2, 16, 0
    PAR_NAMES = tuple(f'p{i}' for i in range(16))
    PAR_DEFAULT = (0.9, 0.5, 0.1, 1.0, 0.25, 0.5, -0.125, 0.75, -0.5, 1.0, -1.0, 0.5, 0.5, 0.125, 0.25, -0.25)

    @staticmethod
    def reset(u, par):
        return u[:, :1] - 0.5, np.zeros((len(u), 0), dtype=np.int32)

    @staticmethod
    def observe(sd, si, par):
        return np.stack([sd[:, 0], sd[:, 0] * sd[:, 0]], axis=-1)

    @staticmethod
    def step(sd, si, action, par, w):
        p = par
        a = _f64(action).reshape(len(sd), 1)[:, 0]
        ac = _clip1(a)
        x = (p[0] * sd[:, 0] + p[1] * ac) + p[2]
        xx, aa = x * x, ac * ac
        obj = np.stack([((p[3] * x + p[4] * ac) + p[5]) + p[6] * xx,
                        ((p[7] * x + p[8] * ac) + p[9]) + p[10] * aa,
                        (((p[11] * x + p[12] * ac) + p[13]) + p[14] * xx) + p[15]], axis=-1)
        reward = obj[:, 0] + 0.5 * obj[:, 1]
        done = np.abs(x) > 2.0
        margin = np.minimum(np.abs(np.abs(a) - 1.0), np.abs(np.abs(x) - 2.0))
        return x[:, None], si, obj, reward, done.astype(np.int32), np.zeros(len(sd), dtype=np.int32), margin


class NoiseMax:
    NAME, ENV = 'noisemax', 'NoiseMax-v0'
    O, A, K, DISCRETE, SD, SI, RW, MAX_STEPS = 2, 1, 2, False, 1, 0, 1, 8
    CONTRACT, NP, NW = 2, 0, 4
    PAR_NAMES, PAR_DEFAULT = (), ()

    @staticmethod
    def reset(u, par):
        h = u[:, :1] - 0.5
        return h * 0.4, np.zeros((len(u), 0), dtype=np.int32)

    @staticmethod
    def observe(sd, si, par):
        return np.stack([sd[:, 0], sd[:, 0] * sd[:, 0]], axis=-1)

    @staticmethod
    def step(sd, si, action, par, w):
        a = _f64(action).reshape(len(sd), 1)[:, 0]
        ac = _clip1(a)
        x = (sd[:, 0] + 0.2 * ac) + 0.3 * (w[:, 0] - 0.5)
        obj = np.stack([1.0 + w[:, 1] * ac, w[:, 2] - w[:, 3]], axis=-1)
        reward = obj[:, 0] + obj[:, 1]
        done = np.abs(x) > 0.6
        margin = np.minimum(np.abs(np.abs(a) - 1.0), np.abs(np.abs(x) - 0.6))
        return x[:, None], si, obj, reward, done.astype(np.int32), np.zeros(len(sd), dtype=np.int32), margin


class Line2:
    """envplug_envs.Line behind the contract-2 signatures."""
    NAME, ENV = 'line2', 'Line2-v0'
    O, A, K, DISCRETE, SD, SI, RW, MAX_STEPS = (Line.O, Line.A, Line.K, Line.DISCRETE, Line.SD, Line.SI, Line.RW,
                                                Line.MAX_STEPS)
    CONTRACT, NP, NW = 2, 0, 0
    PAR_NAMES, PAR_DEFAULT = (), ()

    @staticmethod
    def reset(u, par):
        return Line.reset(u)

    @staticmethod
    def observe(sd, si, par):
        return Line.observe(sd, si)

    @staticmethod
    def step(sd, si, action, par, w):
        return Line.step(sd, si, action)


ENVS = {e.NAME: e for e in (Slip, Gather, ParMax, NoiseMax, Line2)}


def info(env):
    return {k: int(getattr(env, k)) for k in INFO_FIELDS}


def par_vector(env, env_params=None):
    par = np.array(env.PAR_DEFAULT, dtype=np.float64).reshape(env.NP)
    for k, v in (env_params or {}).items():
        par[env.PAR_NAMES.index(k)] = float(v)
    return par


def reset(env, row, episode, table, par):
    """pgm_envplug_reset_ex: the start states of the entries (row[i], episode[i] mod R) -> (sd, si, obs)."""
    row, episode = np.asarray(row), np.asarray(episode)
    sd, si = env.reset(table[row, episode % table.shape[1]], par)
    return sd, si, env.observe(sd, si, par)


def transition(env, sd, si, elapsed, episode, row, action, table, par, w, margins=None, live=None):
    """pgm_envplug_transition_ex: one step, the forced limit, the auto-reset -> EnvPlugin.transition's dict."""
    sd, si = np.asarray(sd, dtype=np.float64), np.asarray(si, dtype=np.int32)
    elapsed, episode, row = (np.asarray(x, dtype=np.int32) for x in (elapsed, episode, row))
    w = np.zeros((len(elapsed), 0)) if w is None else np.asarray(w, dtype=np.float64).reshape(len(elapsed), env.NW)
    sd, si, obj, reward, done, bad, margin = env.step(sd, si, action, par, w)
    if margins is not None:
        margin = margin if live is None else margin[live]
        margins['env'] = min(margins.get('env', np.inf), float(np.min(margin)) if len(margin) else np.inf)
        if env.NW and env.NP:  # the distance of the first uniform from the first parameter (Slip: w0 < slip)
            d = np.abs(w[:, 0] - par[0])
            d = d if live is None else d[live]
            margins['noise'] = min(margins.get('noise', np.inf), float(np.min(d)) if len(d) else np.inf)
    elapsed = elapsed + 1
    limit = elapsed >= env.MAX_STEPS
    done = np.where(limit, 1, (done != 0).astype(np.int32)).astype(np.int32)
    bad = np.where(limit, 1, (bad != 0).astype(np.int32)).astype(np.int32)
    episode = (episode + done).astype(np.int32)
    fsd, fsi = env.reset(table[row, episode % table.shape[1]], par)
    d = done.astype(bool)
    sd = np.where(d[:, None], fsd, sd)
    si = np.where(d[:, None], fsi, si).astype(np.int32)
    elapsed = np.where(d, 0, elapsed).astype(np.int32)
    return {'sd': sd, 'si': si, 'elapsed': elapsed, 'episode': episode, 'obs': env.observe(sd, si, par), 'obj': obj,
            'reward': reward, 'done': done, 'bad': bad}


class NumpyPlugin2HostVecEnv(HostVecEnv):
    """hostenv.PluginHostVecEnv of a contract-2 header with the numpy restatement in place of the compiled header:
    the same reset tables, parameters and env-noise indices.  ``begin_rollout`` is called by TaskBatch._host_rollout;
    a caller that steps this env itself (the fp64 reference worker) sets ``rollout_seeds``: the env seed of rollout j
    is taken when step t wraps to 0 every ``T`` steps."""

    def __init__(self, env, P, N, seed=0, R=256, env_params=None, margins=None, T=None, rollout_seeds=None):
        self.env, self.seed, self.R = env, seed, R
        self.capacity = self.P = P
        self.N = N
        self.obs_dim, self.act_dim, self.obj_num, self.discrete = env.O, env.A, env.K, env.DISCRETE
        self.table = envspec.plugin_reset_table(seed, N, R, env.RW)
        self.par = par_vector(env, env_params)
        self.margins = margins
        self.T, self.rollout_seeds, self._rollout = T, rollout_seeds, 0
        self._env_seed = self._eval_env_seed = env_seed(seed)
        self._env_noise = None
        self._t = self._et = 0
        self._st = self._est = None

    def set_active(self, P):
        self.P = P
        self._st = None

    def begin_rollout(self, seed, env_noise=None):
        self._env_seed, self._t = int(seed), 0
        self._env_noise = None if env_noise is None else np.asarray(env_noise, dtype=np.float64)

    def _fresh(self, M, table):
        row = np.broadcast_to(np.arange(M, dtype=np.int32), (self.P, M)).reshape(-1).copy()
        zero = np.zeros(self.P * M, dtype=np.int32)
        sd, si, obs = reset(self.env, row, zero, table, self.par)
        return {'sd': sd, 'si': si, 'elapsed': zero.copy(), 'episode': zero.copy(), 'row': row}, obs

    def _act(self, actions):
        if self.discrete:
            return np.asarray(actions).astype(np.int32).reshape(-1)
        return np.asarray(actions, dtype=np.float32).reshape(-1, self.act_dim)

    def reset(self):
        self._st, obs = self._fresh(self.N, self.table)
        self._t = 0
        return obs.reshape(self.P, self.N, self.obs_dim)

    def _train_w(self):
        NW, N = self.env.NW, self.N
        if self.rollout_seeds is not None and self._t % self.T == 0:
            self.begin_rollout(env_seed(self.rollout_seeds[self._rollout]))
            self._rollout += 1
        if NW == 0:
            return None
        if self._env_noise is not None:
            w = self._env_noise[self._t].reshape(N, NW)
        else:
            w = u53(self._env_seed, self._t * N * NW, N * NW).reshape(N, NW)
        return np.broadcast_to(w, (self.P, N, NW)).reshape(-1, NW)

    def step(self, actions):
        st, P, N = self._st, self.P, self.N
        w = self._train_w()
        o = transition(self.env, st['sd'], st['si'], st['elapsed'], st['episode'], st['row'], self._act(actions),
                       self.table, self.par, w, self.margins)
        self._t += 1
        for k in ('sd', 'si', 'elapsed', 'episode'):
            st[k] = o[k]
        return (o['obs'].reshape(P, N, -1), o['reward'].reshape(P, N), o['done'].reshape(P, N).astype(bool),
                o['bad'].reshape(P, N).astype(bool), o['obj'].reshape(P, N, -1))

    def eval_reset(self, eval_num):
        self._etable = envspec.plugin_reset_table(self.seed, eval_num, self.R, self.env.RW)
        self._est, obs = self._fresh(eval_num, self._etable)
        self._edone = np.zeros(self.P * eval_num, dtype=bool)
        self._eobs = obs
        self._et = 0
        return obs.reshape(self.P, eval_num, -1).copy()

    def eval_step(self, actions):
        st, P, env = self._est, self.P, self.env
        E = self._edone.size // P
        live = ~self._edone
        w = None
        if env.NW:
            w = np.stack([u53(self._eval_env_seed, (e * env.MAX_STEPS + self._et) * env.NW, env.NW) for e in range(E)])
            w = np.broadcast_to(w, (P, E, env.NW)).reshape(-1, env.NW)
        o = transition(env, st['sd'], st['si'], st['elapsed'], st['episode'], st['row'], self._act(actions),
                       self._etable, self.par, w, self.margins, live)
        self._et += 1
        for k in ('sd', 'si', 'elapsed', 'episode'):
            m = live.reshape((-1,) + (1,) * (o[k].ndim - 1))
            st[k] = np.where(m, o[k], st[k])
        done = o['done'].astype(bool) & live
        self._eobs = np.where((live & ~done)[:, None], o['obs'], self._eobs)
        obj = np.where(live[:, None], o['obj'], 0.0)
        self._edone = self._edone | done
        return self._eobs.reshape(P, E, -1).copy(), obj.reshape(P, E, -1), self._edone.reshape(P, E).copy()
