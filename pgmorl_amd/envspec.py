"""SynthMO environment specifications (the build's MuJoCo replacement).

MuJoCo is absent here and on the GPU box, so every MO-* env id of the reference
(environments/__init__.py:3-43) maps to a synthetic env with the same
(obs_dim, act_dim, obj_num, episode length) and an objective of the same form
as the reference env's ``step`` (environments/walker2d.py:16-30 etc.):

    a_c  = clip(a, act_lo, act_hi)
    s'   = tanh(d * s + U @ a_c + c)                      (obs = s')
    obj  = V @ s' + ebase - ecoef * sum(a_c ** 2)         ([K])

Episodes are fixed-length (done only at the time limit, so bad_transition is
always set, a2c_ppo_acktr/envs.py:125-126).  Constants come from splitmix64
(seed 1234) and are pinned by committed fixtures (tests/golden/synth_env_*.npz).
Reset states s0 are drawn per env seed (``args.seed + rank``) from splitmix64.
"""
import numpy as np

_M64 = (1 << 64) - 1


def _splitmix64_stream(seed):
    x = seed & _M64
    while True:
        x = (x + 0x9E3779B97F4A7C15) & _M64
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        yield z ^ (z >> 31)


def _uniforms(seed, n):
    g = _splitmix64_stream(seed)
    return np.array([(next(g) >> 11) * (1.0 / (1 << 53)) for _ in range(n)], dtype=np.float64)


# env id -> (obs_dim, act_dim, obj_num, max_episode_steps, action clip, objective coefficients)
#   obj rows: (velocity-like linear term scale, ebase, ecoef); scale 0 => no state term
_ENVS = {
    # walker2d.py:23-25: speed = v + 1, energy = 4 - sum(a^2) + 1
    'MO-Walker2d-v2': (17, 6, 2, 500, ([-1.0] * 6, [1.0] * 6), [(1.0, 1.0, 0.0), (0.0, 5.0, 1.0)]),
    # half_cheetah.py: run = min(4, v) + 1, energy = 5 - sum(a^2)
    'MO-HalfCheetah-v2': (17, 6, 2, 500, ([-1.0] * 6, [1.0] * 6), [(1.0, 1.0, 0.0), (0.0, 5.0, 1.0)]),
    # hopper.py: run/jump + alive - 2e-4 sum(a^2), clip [2,2,4]
    'MO-Hopper-v2': (11, 3, 2, 500, ([-2.0, -2.0, -4.0], [2.0, 2.0, 4.0]), [(1.5, 1.0, 2e-4), (1.0, 1.0, 2e-4)]),
    # hopper_v3.py: run, jump, energy
    'MO-Hopper-v3': (11, 3, 3, 500, ([-2.0, -2.0, -4.0], [2.0, 2.0, 4.0]),
                     [(1.5, 1.0, 0.0), (1.0, 1.0, 0.0), (0.0, 5.0, 1.0)]),
    # humanoid.py:33-35: run = 1.25 v + 3, energy = 3 - 4 sum(ctrl^2) + 3 (ctrlrange 0.4)
    'MO-Humanoid-v2': (376, 17, 2, 1000, ([-0.4] * 17, [0.4] * 17), [(1.25, 3.0, 0.0), (0.0, 6.0, 4.0)]),
    'MO-Ant-v2': (27, 8, 2, 500, ([-1.0] * 8, [1.0] * 8), [(1.0, 1.0, 0.0), (0.0, 5.0, 0.5)]),
    'MO-Swimmer-v2': (8, 2, 2, 500, ([-1.0] * 2, [1.0] * 2), [(1.0, 0.0, 0.0), (0.0, 0.3, 0.15)]),
}

SPEC_SEED = 1234


def env_names():
    return sorted(_ENVS)


# Discrete-action envs: env id -> (obs_dim, number of actions, obj_num, max_episode_steps).  They have no SynthMO
# stand-in: they are host-stepped (hostenv.DeepSeaTreasureHostVecEnv) or, Deep Sea Treasure with device_env=True,
# stepped inside the fused kernels of csrc/pgm_dst.hip; their policies carry the reference's Categorical head
# (a2c_ppo_acktr/model.py:33-35).
_DISCRETE_ENVS = {
    'MO-DeepSeaTreasure-v0': (3, 4, 2, 50),
}


def discrete_env_names():
    return sorted(_DISCRETE_ENVS)


# Native continuous-action envs: env id -> (obs_dim, act_dim, obj_num, max_episode_steps, bound).  The reference's
# MuJoCo-free test env (environments/dummy_mo_env.py:57-148, registered with max_steps 500 in
# environments/__init__.py:4-16): its real dynamics, not a SynthMO stand-in, stepped inside the fused kernels of
# csrc/pgm_dummy.hip (the default) or on the host (hostenv.DummyMOHostVecEnv); Gaussian head.
_NATIVE_ENVS = {
    'MO-Dummy-v0': (6, 2, 2, 500, 5.0),
    'MO-Dummy3-v0': (6, 2, 3, 500, 5.0),
}
DUMMY_RESETS = 256  # R: reset positions per env seed (dummy_reset_table)
DUMMY_RESET_STREAM = 0xD0330000  # the splitmix64 stream constant of the reset positions (reset_state: 0x5EED0000)


def native_env_names():
    return sorted(_NATIVE_ENVS)


def dummy_reset_table(seed, count, R=DUMMY_RESETS):
    """[count][R][2] fp64 reset positions of the MO-Dummy envs: entry (i, r) = 2 u - 1 with u the splitmix64 uniforms
    of env seed ``seed + i``.  The reference draws np.random.uniform(-1, 1, 2) from numpy's global stream at every
    reset, which is not reproducible per env; this table is a deliberate restatement of that unseeded draw.  A training
    env n starts its episode e at entry (n, e mod R); evaluation episode e starts at entry (e, 0)."""
    if R < 1:
        raise ValueError(f'dummy_reset_table: R = {R} reset positions per env must be at least 1')
    return np.stack([(2.0 * _uniforms(DUMMY_RESET_STREAM + int(seed) + i, 2 * R) - 1.0).reshape(R, 2)
                     for i in range(count)])


PLUGIN_RESET_STREAM = 0xE9F10000  # the splitmix64 stream constant of the env plug-ins' reset uniforms


def plugin_reset_table(seed, count, R, RW):
    """[count][R][RW] fp64 uniforms in [0, 1) for the reset function of a device env plug-in (include/pgm_envplug.h):
    row i holds the splitmix64 uniforms of env seed ``seed + i`` (dummy_reset_table's construction without the
    2 u - 1).  Training env n of every task starts its episode e at entry (n, e mod R); evaluation episode e starts at
    entry (e, 0) of the table of eval_num rows."""
    if R < 1:
        raise ValueError(f'plugin_reset_table: R = {R} reset entries per env must be at least 1')
    if RW < 0:
        raise ValueError(f'plugin_reset_table: RW = {RW} uniforms per entry must not be negative')
    return np.stack([_uniforms(PLUGIN_RESET_STREAM + int(seed) + i, R * RW).reshape(R, RW) for i in range(count)])


# Third-party envs (register_env): env id -> (obs_dim, act_dim or number of actions, obj_num, discrete).  Host-stepped
# only (hostenv.GymHostVecEnv behind ``--host-env module:callable``), on the runtime-dim kernels (the *_any entry points
# of include/pgm_abi.h), whose range these bounds restate.
_USER_ENVS = {}
USER_MAX_OBS, USER_MAX_ACT, USER_MAX_OBJ = 32, 8, 3


def user_env_names():
    return sorted(_USER_ENVS)


def register_env(name, obs_dim, act_dim, obj_num, discrete=False):
    """Make ``make_spec(name)`` know a third-party env: its dims with ``'user': True`` (and ``'discrete'``; act_dim is
    then the number of actions).  ValueError for a name envspec already knows (a second registration with the same
    dims is accepted) and for dims outside the runtime-dim kernels' range."""
    O, A, K, disc = int(obs_dim), int(act_dim), int(obj_num), bool(discrete)
    if name in _ENVS or name in _DISCRETE_ENVS or name in _NATIVE_ENVS:
        raise ValueError(f'register_env: {name!r} is one of envspec\'s own envs')
    if name in _USER_ENVS and _USER_ENVS[name] != (O, A, K, disc):
        raise ValueError(f'register_env: {name!r} is already registered with (obs, act, obj, discrete) = '
                         f'{_USER_ENVS[name]}')
    if not 1 <= O <= USER_MAX_OBS:
        raise ValueError(f'register_env: {name!r} has obs_dim {O}; the runtime-dim kernels take 1 <= obs_dim <= '
                         f'{USER_MAX_OBS}')
    if not (2 if disc else 1) <= A <= USER_MAX_ACT:
        raise ValueError(f'register_env: {name!r} has {A} ' + ('actions' if disc else 'action dims') +
                         f'; the runtime-dim kernels take {"2" if disc else "1"} <= it <= {USER_MAX_ACT}')
    if not 1 <= K <= USER_MAX_OBJ:
        raise ValueError(f'register_env: {name!r} has {K} objectives; the runtime-dim kernels take 1 <= obj_num <= '
                         f'{USER_MAX_OBJ}')
    _USER_ENVS[name] = (O, A, K, disc)


def make_spec(env_name):
    """Constant arrays of one SynthMO env (all fp64); for a discrete-action env the dims alone, with
    ``discrete = True`` and ``act_dim`` the number of actions; for a native env the dims, ``bound``, the action clip
    and ``native`` (no SynthMO arrays); for a registered third-party env the dims with ``user = True``."""
    if env_name in _USER_ENVS:
        O, A, K, disc = _USER_ENVS[env_name]
        sp = {'name': env_name, 'obs_dim': O, 'act_dim': A, 'obj_num': K, 'user': True}
        if disc:
            sp['discrete'] = True
        return sp
    if env_name in _NATIVE_ENVS:
        O, A, K, tmax, bound = _NATIVE_ENVS[env_name]
        return {'name': env_name, 'obs_dim': O, 'act_dim': A, 'obj_num': K, 'max_episode_steps': tmax, 'bound': bound,
                'act_lo': np.full(A, -1.0), 'act_hi': np.full(A, 1.0), 'native': 'dummy'}
    if env_name in _DISCRETE_ENVS:
        O, A, K, tmax = _DISCRETE_ENVS[env_name]
        return {'name': env_name, 'obs_dim': O, 'act_dim': A, 'obj_num': K, 'max_episode_steps': tmax,
                'discrete': True}
    if env_name not in _ENVS:
        raise ValueError(f'unknown env {env_name!r}; known: {env_names() + discrete_env_names() + native_env_names()}')
    O, A, K, tmax, (lo, hi), objrows = _ENVS[env_name]
    u = _uniforms(SPEC_SEED, O + O * A + O + K * O)
    p = 0
    d = (2.0 * u[p:p + O] - 1.0) * 0.9; p += O
    U = ((2.0 * u[p:p + O * A] - 1.0) / np.sqrt(A)).reshape(O, A); p += O * A
    c = (2.0 * u[p:p + O] - 1.0) * 0.1; p += O
    V = np.zeros((K, O))
    for k, (scale, _, _) in enumerate(objrows):
        V[k] = (2.0 * u[p:p + O] - 1.0) * (2.0 * scale / np.sqrt(O))
        p += O
    return {
        'name': env_name, 'obs_dim': O, 'act_dim': A, 'obj_num': K, 'max_episode_steps': tmax,
        'd': d, 'U': U, 'c': c, 'V': V,
        'ebase': np.array([r[1] for r in objrows], dtype=np.float64),
        'ecoef': np.array([r[2] for r in objrows], dtype=np.float64),
        'act_lo': np.array(lo, dtype=np.float64), 'act_hi': np.array(hi, dtype=np.float64),
    }


def reset_state(obs_dim, env_seed):
    """Deterministic reset state of the env seeded ``env_seed`` (never the zero vector)."""
    return 0.5 * (2.0 * _uniforms(0x5EED0000 + int(env_seed), obs_dim) - 1.0)


def reset_table(obs_dim, seed, count):
    """s0 rows for env seeds seed+0 .. seed+count-1 (make_env seeds env rank with seed+rank)."""
    return np.stack([reset_state(obs_dim, seed + r) for r in range(count)])
