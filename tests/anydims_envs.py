"""Two tiny gym-style multi-objective envs with dims no kernel is compiled for (plain numpy, no gym import), for the
runtime-dim kernel family: what a user's ``--host-env tests.anydims_envs:make_env`` looks like.

* ``Tiny-v0``          continuous: 5 observations, 1 action dim, 2 objectives.  A point on a line: v' = 0.9 v + 0.2
                       clip(a, -1, 1), x' = x + v'; obs = [x, v, sin x, cos x, t / LIMIT]; obj = [1 + v', 1 - a_c^2];
                       a TRUE terminal when |x'| > BOUND, a time-limit end (``bad_transition``) at t = LIMIT.
* ``TinyDiscrete-v0``  discrete: 2 observations, 3 actions (left, stay, right), 3 objectives.  A chain of 7 cells;
                       obs = [i / 6, t / LIMIT]; objectives [i / 6, (6 - i) / 6, 1 if stay else 0]; a TRUE terminal at
                       either end of the chain, a time-limit end at t = LIMIT.

Both are deterministic per ``seed + rank``: the start states come from ``numpy.random.RandomState(seed + rank)``, one
draw per episode, and nothing else is random.  A reset that follows a reset with no step in between starts the same
episode again (no draw), so an env that was probed once (hostenv.probe_dims resets it) plays the episodes of one that
was not.
"""
import numpy as np

CONT, DISC = 'Tiny-v0', 'TinyDiscrete-v0'
LIMIT, BOUND = 40, 1.5
DISC_LIMIT = 20


class _Box:
    def __init__(self, n):
        self.shape = (n,)


class _Discrete:
    def __init__(self, n):
        self.n = n


class TinyContEnv:
    obj_dim = 2

    def __init__(self, seed):
        self.action_space = _Box(1)
        self.rng = np.random.RandomState(seed)
        self.x = self.v = 0.0
        self.t = 0
        self.start, self.stepped = None, False
        self.last_x = 0.0  # |x'| of the last step, for the tests' margin from BOUND

    def _obs(self):
        return np.array([self.x, self.v, np.sin(self.x), np.cos(self.x), self.t / LIMIT], dtype=np.float64)

    def reset(self):
        if self.start is None or self.stepped:
            self.start = (self.rng.uniform(-0.5, 0.5, 2) * np.array([1.0, 0.2])).tolist()
        self.x, self.v = self.start
        self.t, self.stepped = 0, False
        return self._obs()

    def step(self, action):
        a = float(np.clip(np.asarray(action, dtype=np.float64).reshape(-1)[0], -1.0, 1.0))
        self.stepped = True
        self.v = 0.9 * self.v + 0.2 * a
        self.x = self.x + self.v
        self.t += 1
        self.last_x = abs(self.x)
        obj = np.array([1.0 + self.v, 1.0 - a * a])
        info = {'obj': obj}
        term = self.last_x > BOUND
        done = term or self.t >= LIMIT
        if done and not term:
            info['bad_transition'] = True
        return self._obs(), float(obj[0] + 0.5 * obj[1]), done, info


class TinyDiscEnv:
    obj_dim = 3
    CELLS = 7

    def __init__(self, seed):
        self.action_space = _Discrete(3)
        self.rng = np.random.RandomState(seed)
        self.i = 3
        self.t = 0
        self.start, self.stepped = None, False

    def _obs(self):
        return np.array([self.i / (self.CELLS - 1), self.t / DISC_LIMIT], dtype=np.float64)

    def reset(self):
        if self.start is None or self.stepped:
            self.start = int(self.rng.randint(2, 5))
        self.i = self.start
        self.t, self.stepped = 0, False
        return self._obs()

    def step(self, action):
        a = int(action)
        self.stepped = True
        self.i += a - 1 if 0 <= a < 3 else 0
        self.t += 1
        n = self.CELLS - 1
        obj = np.array([self.i / n, (n - self.i) / n, 1.0 if a == 1 else 0.0])
        info = {'obj': obj}
        term = self.i <= 0 or self.i >= n
        done = term or self.t >= DISC_LIMIT
        if done and not term:
            info['bad_transition'] = True
        return self._obs(), float(obj.sum()), done, info


def make_env(env_name, seed, rank):
    if env_name == CONT:
        return TinyContEnv(seed + rank)
    if env_name == DISC:
        return TinyDiscEnv(seed + rank)
    raise ValueError(f'tests.anydims_envs.make_env: unknown env {env_name!r} ({CONT}, {DISC})')
