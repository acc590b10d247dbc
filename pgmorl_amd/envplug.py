"""Device env plug-ins: a user env stated as one C++ header (include/pgm_envplug.h), compiled into a library of its own
with a fused rollout and evaluation kernel around it (csrc/pgm_envplug.hip, build.build_env).

``EnvPlugin(header)`` builds (or finds) that library, loads it and reads the header's constants;
``TaskBatch(env_name, ..., env_plugin=plugin)`` then trains on the fused path and
``hostenv.PluginHostVecEnv(plugin, ...)`` steps the same compiled header on the host.  libpgm.so is not involved: a
plug-in library exports only the ``pgm_envplug_*`` entry points.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build
from . import envspec
from ._lib import Dims, EnvState, NormState, PGMError, RolloutBuf

PGM_ENVPLUG_ABI = 1
P_, I32, F64 = C.c_void_p, C.c_int32, C.c_double
INFO_FIELDS = ('O', 'A', 'K', 'DISCRETE', 'SD', 'SI', 'RW', 'MAX_STEPS')

SIGS = {
    'pgm_envplug_abi': (C.c_int, []),
    'pgm_envplug_last_error': (C.c_char_p, []),
    'pgm_envplug_info': (C.c_int, [C.POINTER(I32)]),
    # d, params, sd, si, episode, table, R, reset_count, st, ns, rb, stream_in, seed, carry, stream
    'pgm_envplug_rollout': (C.c_int, [C.POINTER(Dims), P_, P_, P_, P_, P_, I32, I32, C.POINTER(EnvState),
                                      C.POINTER(NormState), C.POINTER(RolloutBuf), P_, C.c_uint64, I32, P_]),
    # d, params, table, R, reset_count, ob_mean, ob_var, eval_num, use_ob_rms, raw, gamma, objs_out, stream
    'pgm_envplug_eval': (C.c_int, [C.POINTER(Dims), P_, P_, I32, I32, P_, P_, I32, I32, I32, F64, P_, P_]),
    # n, sd, si, elapsed, episode, row, action, table, R, reset_count, then the nine outputs
    'pgm_envplug_transition': (C.c_int, [I32, P_, P_, P_, P_, P_, P_, P_, I32, I32] + [P_] * 9),
    # n, row, episode, table, R, reset_count, sd_out, si_out, obs_out
    'pgm_envplug_reset': (C.c_int, [I32, P_, P_, P_, I32, I32, P_, P_, P_]),
}

DEFAULT_RESETS = 256  # R: reset-table entries per env row (envspec.plugin_reset_table), as envspec.DUMMY_RESETS


def _np_ptr(a):
    return C.c_void_p(a.ctypes.data)


class EnvPlugin:
    """One built and loaded plug-in library.  Attributes: ``header``, ``lib_path``, ``h`` (the ctypes handle with typed
    prototypes) and the header's constants ``O, A, K, DISCRETE, SD, SI, RW, MAX_STEPS``."""

    def __init__(self, header, force=False, verbose=False):
        self.header = os.path.abspath(os.fspath(header))
        try:
            self.lib_path = _build.build_env(self.header, force=force, verbose=verbose)
        except RuntimeError as e:
            raise PGMError(f'env plug-in {header}: {e}') from e
        self.h = h = C.CDLL(self.lib_path)
        for name, (res, args) in SIGS.items():
            f = getattr(h, name)
            f.restype, f.argtypes = res, args
        if h.pgm_envplug_abi() != PGM_ENVPLUG_ABI:
            raise PGMError(f'{self.lib_path}: plug-in ABI {h.pgm_envplug_abi()} != {PGM_ENVPLUG_ABI}')
        info = (I32 * 8)()
        self.check(h.pgm_envplug_info(info), 'pgm_envplug_info')
        self.info = dict(zip(INFO_FIELDS, (int(v) for v in info)))
        for k, v in self.info.items():
            setattr(self, k, v)
        self.DISCRETE = bool(self.DISCRETE)

    def last_error(self):
        return self.h.pgm_envplug_last_error().decode(errors='replace')

    def check(self, rc, what):
        if rc != 0:
            raise PGMError(f'{what} failed ({rc}): {self.last_error()}')

    def dims(self):
        return self.O, self.A, self.K

    def register(self, env_name):
        """envspec.register_env(env_name, O, A, K, discrete=DISCRETE): ValueError for a name envspec already knows."""
        envspec.register_env(env_name, self.O, self.A, self.K, discrete=self.DISCRETE)
        return env_name

    # ---- the host functions: the compiled header on n items (numpy in, numpy out)
    def reset(self, row, episode, table):
        """Start states of the entries (row[i], episode[i] mod R) of table [rows][R][RW] -> (sd [n, SD], si [n, SI],
        obs [n, O])."""
        row = np.ascontiguousarray(row, dtype=np.int32).reshape(-1)
        episode = np.ascontiguousarray(episode, dtype=np.int32).reshape(-1)
        table = self._table(table)
        n = row.size
        sd, si = np.zeros((n, self.SD)), np.zeros((n, self.SI), dtype=np.int32)
        obs = np.zeros((n, self.O))
        self.check(self.h.pgm_envplug_reset(n, _np_ptr(row), _np_ptr(episode), _np_ptr(table), table.shape[1],
                                            table.shape[0], _np_ptr(sd), _np_ptr(si), _np_ptr(obs)),
                   'pgm_envplug_reset')
        return sd, si, obs

    def transition(self, sd, si, elapsed, episode, row, action, table):
        """One step of n envs with the forced limit and the auto-reset -> dict(sd, si, elapsed, episode, obs, obj,
        reward, done, bad).  action: float32 [n, A], or (DISCRETE) int32 [n]."""
        n = np.asarray(elapsed).size
        sd = np.ascontiguousarray(sd, dtype=np.float64).reshape(n, self.SD)
        si = np.ascontiguousarray(si, dtype=np.int32).reshape(n, self.SI)
        elapsed = np.ascontiguousarray(elapsed, dtype=np.int32).reshape(n)
        episode = np.ascontiguousarray(episode, dtype=np.int32).reshape(n)
        row = np.ascontiguousarray(row, dtype=np.int32).reshape(n)
        if self.DISCRETE:
            action = np.ascontiguousarray(action, dtype=np.int32).reshape(n)
        else:
            action = np.ascontiguousarray(action, dtype=np.float32).reshape(n, self.A)
        table = self._table(table)
        o = {'sd': np.zeros((n, self.SD)), 'si': np.zeros((n, self.SI), dtype=np.int32),
             'elapsed': np.zeros(n, dtype=np.int32), 'episode': np.zeros(n, dtype=np.int32),
             'obs': np.zeros((n, self.O)), 'obj': np.zeros((n, self.K)), 'reward': np.zeros(n),
             'done': np.zeros(n, dtype=np.int32), 'bad': np.zeros(n, dtype=np.int32)}
        self.check(self.h.pgm_envplug_transition(
            n, _np_ptr(sd), _np_ptr(si), _np_ptr(elapsed), _np_ptr(episode), _np_ptr(row), _np_ptr(action),
            _np_ptr(table), table.shape[1], table.shape[0],
            *(_np_ptr(o[k]) for k in ('sd', 'si', 'elapsed', 'episode', 'obs', 'obj', 'reward', 'done', 'bad'))),
            'pgm_envplug_transition')
        return o

    def _table(self, table):
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.ndim != 3 or table.shape[2] != self.RW:
            raise PGMError(f'reset table of shape {table.shape}: this plug-in needs [rows][R][{self.RW}]')
        return table


def as_plugin(x):
    """An EnvPlugin from an EnvPlugin or a header path."""
    return x if isinstance(x, EnvPlugin) else EnvPlugin(x)
