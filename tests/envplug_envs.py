"""numpy fp64 restatements of the test env plug-ins of tests/envplug/*.hpp: vectorised over n envs, every operation
elementwise and in the header's order (no dot product or norm whose summation order numpy chooses), so that the fp64
outputs equal the compiled header's bit for bit.  ``transition`` restates the caller's side of the contract
(include/pgm_envplug.h): the forced step limit and the auto-reset from the reset table.  ``NumpyPluginHostVecEnv`` is a
``HostVecEnv`` over a restatement: what the fp64 reference worker steps.

Each ``step`` also reports ``margin``: the smallest distance of the step's inputs from a discontinuity of the rule (the
action clip, the terminal bound), for the seed rule of the tests against the reference.
"""
import os

import numpy as np

from pgmorl_amd import envspec
from pgmorl_amd.hostenv import HostVecEnv

HERE = os.path.dirname(os.path.abspath(__file__))


def header(name):
    return os.path.join(HERE, 'envplug', name + '.hpp')


def _f64(a):
    """The (double) cast of a float action."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _clip1(a):
    return np.where(a < -1.0, -1.0, np.where(a > 1.0, 1.0, a))


class Line:
    NAME, ENV = 'line', 'Line-v0'
    O, A, K, DISCRETE, SD, SI, RW, MAX_STEPS = 5, 1, 2, False, 2, 1, 2, 40
    BOUND = 1.5

    @staticmethod
    def reset(u):
        sd = np.stack([u[:, 0] - 0.5, (u[:, 1] - 0.5) * 0.2], axis=-1)
        return sd, np.zeros((len(u), 1), dtype=np.int32)

    @staticmethod
    def observe(sd, si):
        x, v = sd[:, 0], sd[:, 1]
        return np.stack([x, v, x * x, v * v, si[:, 0].astype(np.float64) / 40.0], axis=-1)

    @staticmethod
    def step(sd, si, action):
        a = _f64(action).reshape(len(sd), 1)[:, 0]
        ac = _clip1(a)
        v = 0.9 * sd[:, 1] + 0.2 * ac
        x = sd[:, 0] + v
        obj = np.stack([1.0 + v, 1.0 - ac * ac], axis=-1)
        reward = obj[:, 0] + 0.5 * obj[:, 1]
        done = np.abs(x) > Line.BOUND
        margin = np.minimum(np.abs(np.abs(a) - 1.0), np.abs(np.abs(x) - Line.BOUND))
        return (np.stack([x, v], axis=-1), si + 1, obj, reward, done.astype(np.int32),
                np.zeros(len(sd), dtype=np.int32), margin)


class Chain:
    NAME, ENV = 'chain', 'Chain-v0'
    O, A, K, DISCRETE, SD, SI, RW, MAX_STEPS = 2, 3, 3, True, 0, 2, 1, 20

    @staticmethod
    def reset(u):
        cell = 2 + (u[:, 0] * 3.0).astype(np.int32)
        return np.zeros((len(u), 0)), np.stack([cell, np.zeros_like(cell)], axis=-1).astype(np.int32)

    @staticmethod
    def observe(sd, si):
        return np.stack([si[:, 0].astype(np.float64) / 6.0, si[:, 1].astype(np.float64) / 20.0], axis=-1)

    @staticmethod
    def step(sd, si, action):
        a = np.asarray(action).astype(np.int32).reshape(len(si))
        i, t = si[:, 0] + a - 1, si[:, 1] + 1
        obj = np.stack([i.astype(np.float64) / 6.0, (6 - i).astype(np.float64) / 6.0,
                        np.where(a == 1, 1.0, 0.0)], axis=-1)
        reward = (obj[:, 0] + obj[:, 1]) + obj[:, 2]
        done = (i <= 0) | (i >= 6)
        return (sd, np.stack([i, t], axis=-1).astype(np.int32), obj, reward, done.astype(np.int32),
                np.zeros(len(si), dtype=np.int32), np.full(len(si), np.inf))


class PlugDummy:
    NAME, ENV = 'plugdummy', 'PlugDummy-v0'
    O, A, K, DISCRETE, SD, SI, RW, MAX_STEPS = 6, 2, 2, False, 6, 1, 2, 500
    BOUND = 5.0

    @staticmethod
    def reset(u):
        sd = np.zeros((len(u), 6))
        sd[:, 0], sd[:, 1] = 2.0 * u[:, 0] - 1.0, 2.0 * u[:, 1] - 1.0
        return sd, np.zeros((len(u), 1), dtype=np.int32)

    @staticmethod
    def observe(sd, si):
        return sd.copy()

    @staticmethod
    def step(sd, si, action):
        a = _f64(action).reshape(len(sd), 2)
        ac0, ac1 = _clip1(a[:, 0]), _clip1(a[:, 1])
        lx, ly = sd[:, 0], sd[:, 1]
        vx, vy = (sd[:, 2] + ac0 * 0.1) * 0.95, (sd[:, 3] + ac1 * 0.1) * 0.95
        px, py = lx + vx, ly + vy
        dx, dy = px - lx, py - ly
        dist = np.sqrt(dx * dx + dy * dy)
        energy = np.sqrt(ac0 * ac0 + ac1 * ac1)
        r = np.sqrt(px * px + py * py)
        new = np.stack([px, py, vx, vy, sd[:, 4] + dist, sd[:, 5] + energy], axis=-1)
        step = si[:, 0] + 1
        obj = np.stack([dist, 1.0 / (energy + 0.1)], axis=-1)
        reward = obj[:, 0] + 0.1 * obj[:, 1]
        done = (step >= 500) | (r > PlugDummy.BOUND)
        bad = done & (step == 500)
        # (the header leaves the state of a done env as it was: the caller resets it)
        keep = done[:, None]
        margin = np.minimum(np.abs(np.abs(a) - 1.0).min(-1), np.abs(r - PlugDummy.BOUND))
        return (np.where(keep, sd, new), np.where(keep, si, step[:, None]).astype(np.int32), obj, reward,
                done.astype(np.int32), bad.astype(np.int32), margin)


class Wide:
    NAME, ENV = 'wide', 'Wide-v0'
    O, A, K, DISCRETE, SD, SI, RW, MAX_STEPS = 32, 8, 3, False, 16, 4, 8, 16

    @staticmethod
    def reset(u):
        c = u[:, np.arange(16) % 8] - 0.5
        sd = np.where(np.arange(16) < 8, c, c * 0.5)
        return sd, np.zeros((len(u), 4), dtype=np.int32)

    @staticmethod
    def observe(sd, si):
        return np.concatenate([sd, sd[:, :15] * sd[:, :15], (si[:, 0].astype(np.float64) / 16.0)[:, None]], axis=-1)

    @staticmethod
    def step(sd, si, action):
        a = _f64(action).reshape(len(sd), 8)
        ac = _clip1(a)
        clipped = (a < -1.0) | (a > 1.0)
        nclip = clipped.sum(-1).astype(np.int32)
        mask = (clipped.astype(np.int32) << np.arange(8, dtype=np.int32)).sum(-1).astype(np.int32)
        new = 0.5 * sd + 0.1 * ac[:, np.arange(16) % 8]
        t = si[:, 0] + 1
        obj = np.stack([1.0 + new[:, 0], 1.0 + new[:, 1], 1.0 + new[:, 2]], axis=-1)
        reward = obj[:, 0] + 0.25 * nclip.astype(np.float64)
        s01 = new[:, 0] + new[:, 1]
        done = s01 > 0.3
        margin = np.minimum(np.abs(np.abs(a) - 1.0).min(-1), np.abs(s01 - 0.3))
        return (new, np.stack([t, si[:, 1] + nclip, mask, t * 2], axis=-1).astype(np.int32), obj, reward,
                done.astype(np.int32), np.zeros(len(sd), dtype=np.int32), margin)


class NoLimit:
    NAME, ENV = 'nolimit', 'NoLimit-v0'
    O, A, K, DISCRETE, SD, SI, RW, MAX_STEPS = 1, 1, 1, False, 1, 0, 1, 7

    @staticmethod
    def reset(u):
        return u[:, :1].copy(), np.zeros((len(u), 0), dtype=np.int32)

    @staticmethod
    def observe(sd, si):
        return sd.copy()

    @staticmethod
    def step(sd, si, action):
        new = sd + 1.0
        z = np.zeros(len(sd), dtype=np.int32)
        return new, si, _f64(action).reshape(len(sd), 1), new[:, 0].copy(), z, z.copy(), np.full(len(sd), np.inf)


ENVS = {e.NAME: e for e in (Line, Chain, PlugDummy, Wide)}
INFO_FIELDS = ('O', 'A', 'K', 'DISCRETE', 'SD', 'SI', 'RW', 'MAX_STEPS')


def info(env):
    return {k: int(getattr(env, k)) for k in INFO_FIELDS}


def reset(env, row, episode, table):
    """pgm_envplug_reset: the start states of the entries (row[i], episode[i] mod R) -> (sd, si, obs)."""
    row, episode = np.asarray(row), np.asarray(episode)
    sd, si = env.reset(table[row, episode % table.shape[1]])
    return sd, si, env.observe(sd, si)


def transition(env, sd, si, elapsed, episode, row, action, table, margins=None, live=None):
    """pgm_envplug_transition: one step, the forced limit, the auto-reset -> the dict EnvPlugin.transition returns."""
    sd, si = np.asarray(sd, dtype=np.float64), np.asarray(si, dtype=np.int32)
    elapsed, episode, row = (np.asarray(x, dtype=np.int32) for x in (elapsed, episode, row))
    sd, si, obj, reward, done, bad, margin = env.step(sd, si, action)
    if margins is not None:  # (live: the evaluation's episodes that still run; an ended one decides nothing)
        margin = margin if live is None else margin[live]
        margins['env'] = min(margins.get('env', np.inf), float(np.min(margin)) if len(margin) else np.inf)
    elapsed = elapsed + 1
    limit = elapsed >= env.MAX_STEPS
    done = np.where(limit, 1, (done != 0).astype(np.int32)).astype(np.int32)
    bad = np.where(limit, 1, (bad != 0).astype(np.int32)).astype(np.int32)
    episode = (episode + done).astype(np.int32)
    fsd, fsi = env.reset(table[row, episode % table.shape[1]])
    d = done.astype(bool)
    sd = np.where(d[:, None], fsd, sd)
    si = np.where(d[:, None], fsi, si).astype(np.int32)
    elapsed = np.where(d, 0, elapsed).astype(np.int32)
    return {'sd': sd, 'si': si, 'elapsed': elapsed, 'episode': episode, 'obs': env.observe(sd, si), 'obj': obj,
            'reward': reward, 'done': done, 'bad': bad}


class NumpyPluginHostVecEnv(HostVecEnv):
    """hostenv.PluginHostVecEnv with the numpy restatement in place of the compiled header (P x N envs, the same
    reset tables); ``margins['env']`` collects the smallest decision margin of every training and (live) evaluation step."""

    def __init__(self, env, P, N, seed=0, R=256, margins=None):
        self.env, self.seed, self.R = env, seed, R
        self.capacity = self.P = P
        self.N = N
        self.obs_dim, self.act_dim, self.obj_num, self.discrete = env.O, env.A, env.K, env.DISCRETE
        self.table = envspec.plugin_reset_table(seed, N, R, env.RW)
        self.margins = margins
        self._st = self._est = None

    def set_active(self, P):
        self.P = P
        self._st = None

    def _fresh(self, M, table):
        row = np.broadcast_to(np.arange(M, dtype=np.int32), (self.P, M)).reshape(-1).copy()
        zero = np.zeros(self.P * M, dtype=np.int32)
        sd, si, obs = reset(self.env, row, zero, table)
        return {'sd': sd, 'si': si, 'elapsed': zero.copy(), 'episode': zero.copy(), 'row': row}, obs

    def _act(self, actions):
        if self.discrete:
            return np.asarray(actions).astype(np.int32).reshape(-1)
        return np.asarray(actions, dtype=np.float32).reshape(-1, self.act_dim)

    def reset(self):
        self._st, obs = self._fresh(self.N, self.table)
        return obs.reshape(self.P, self.N, self.obs_dim)

    def step(self, actions):
        st, P, N = self._st, self.P, self.N
        o = transition(self.env, st['sd'], st['si'], st['elapsed'], st['episode'], st['row'], self._act(actions),
                       self.table, self.margins)
        for k in ('sd', 'si', 'elapsed', 'episode'):
            st[k] = o[k]
        return (o['obs'].reshape(P, N, -1), o['reward'].reshape(P, N), o['done'].reshape(P, N).astype(bool),
                o['bad'].reshape(P, N).astype(bool), o['obj'].reshape(P, N, -1))

    def eval_reset(self, eval_num):
        self._etable = envspec.plugin_reset_table(self.seed, eval_num, self.R, self.env.RW)
        self._est, obs = self._fresh(eval_num, self._etable)
        self._edone = np.zeros(self.P * eval_num, dtype=bool)
        self._eobs = obs
        return obs.reshape(self.P, eval_num, -1).copy()

    def eval_step(self, actions):
        st, P = self._est, self.P
        E = self._edone.size // P
        live = ~self._edone
        o = transition(self.env, st['sd'], st['si'], st['elapsed'], st['episode'], st['row'], self._act(actions),
                       self._etable, self.margins, live)
        for k in ('sd', 'si', 'elapsed', 'episode'):
            m = live.reshape((-1,) + (1,) * (o[k].ndim - 1))
            st[k] = np.where(m, o[k], st[k])
        done = o['done'].astype(bool) & live
        self._eobs = np.where((live & ~done)[:, None], o['obs'], self._eobs)
        obj = np.where(live[:, None], o['obj'], 0.0)
        self._edone = self._edone | done
        return self._eobs.reshape(P, E, -1).copy(), obj.reshape(P, E, -1), self._edone.reshape(P, E).copy()
