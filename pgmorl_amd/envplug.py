"""Device env plug-ins: a user env stated as one C++ header (include/pgm_envplug.h), compiled into a library of its own
with a fused rollout and evaluation kernel around it (csrc/pgm_envplug.hip, build.build_env).

``EnvPlugin(header)`` builds (or finds) that library, loads it and reads the header's constants;
``TaskBatch(env_name, ..., env_plugin=plugin)`` then trains on the fused path and
``hostenv.PluginHostVecEnv(plugin, ...)`` steps the same compiled header on the host.  libpgm.so is not involved: a
plug-in library exports only the ``pgm_envplug_*`` entry points.

A header under contract 2 (``CONTRACT = 2``) also has ``NP`` runtime parameters (``par_names``, ``par_default``; set per
run with ``TaskBatch(env_params={name: value})`` / ``--env-param NAME=VALUE``) and ``NW`` uniforms per step, drawn from
the env-noise stream ``uniforms(env_seed(seed), ...)``.
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
MAX_NP, MAX_NW = 16, 4
# The env-noise stream of a rollout seeded `seed` (and of the evaluations of a batch seeded `seed`) is the counter
# stream of seed ^ ENV_SEED_XOR, so that it is not the action-noise stream of the same seed.
ENV_SEED_XOR = 0x5EEDE27A0153C0DE


def env_seed(seed):
    return (int(seed) ^ ENV_SEED_XOR) & 0xFFFFFFFFFFFFFFFF


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
    # ---- contract 2
    'pgm_envplug_contract': (C.c_int, []),
    'pgm_envplug_info_ex': (C.c_int, [C.POINTER(I32)]),
    'pgm_envplug_params': (C.c_int, [C.c_char_p, I32, P_]),
    'pgm_envplug_uniforms': (C.c_int, [C.c_uint64, C.c_uint64, C.c_int64, P_]),
    # pgm_envplug_rollout's through carry, then env_par, env_rnd, env_seed, stream
    'pgm_envplug_rollout_ex': (C.c_int, [C.POINTER(Dims), P_, P_, P_, P_, P_, I32, I32, C.POINTER(EnvState),
                                         C.POINTER(NormState), C.POINTER(RolloutBuf), P_, C.c_uint64, I32, P_, P_,
                                         C.c_uint64, P_]),
    # pgm_envplug_eval's through objs_out, then env_par, env_seed, stream
    'pgm_envplug_eval_ex': (C.c_int, [C.POINTER(Dims), P_, P_, I32, I32, P_, P_, I32, I32, I32, F64, P_, P_,
                                      C.c_uint64, P_]),
    # pgm_envplug_transition's inputs, env_par, w, then the nine outputs
    'pgm_envplug_transition_ex': (C.c_int, [I32, P_, P_, P_, P_, P_, P_, P_, I32, I32, P_, P_] + [P_] * 9),
    # pgm_envplug_reset's inputs, env_par, then sd_out, si_out, obs_out
    'pgm_envplug_reset_ex': (C.c_int, [I32, P_, P_, P_, I32, I32, P_, P_, P_, P_]),
}

DEFAULT_RESETS = 256  # R: reset-table entries per env row (envspec.plugin_reset_table), as envspec.DUMMY_RESETS


def _np_ptr(a):
    return C.c_void_p(a.ctypes.data)


class EnvPlugin:
    """One built and loaded plug-in library.  Attributes: ``header``, ``lib_path``, ``h`` (the ctypes handle with typed
    prototypes), the header's constants ``O, A, K, DISCRETE, SD, SI, RW, MAX_STEPS`` and, of contract 2, ``CONTRACT``
    (1 or 2), ``NP``, ``NW``, ``par_names`` (NP strings) and ``par_default`` (fp64 [NP])."""

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
        ex = (I32 * 11)()
        self.check(h.pgm_envplug_info_ex(ex), 'pgm_envplug_info_ex')
        self.CONTRACT, self.NP, self.NW = int(ex[8]), int(ex[9]), int(ex[10])
        names = C.create_string_buffer(64 * MAX_NP)
        self.par_default = np.zeros(self.NP)
        self.check(h.pgm_envplug_params(names, len(names), _np_ptr(self.par_default)), 'pgm_envplug_params')
        self.par_names = [x for x in names.value.decode().split(',') if x]

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

    # ---- contract 2: the runtime parameters and the env-noise stream
    def par_vector(self, env_params=None):
        """fp64 [NP]: ``env_params`` (a dict name -> float over ``par_names``) over the header's defaults.  PGMError for
        an unknown name, for a value that is no finite number and for any env_params of a header with NP == 0."""
        par = self.par_default.copy()
        if not env_params:
            return par
        if self.NP == 0:
            raise PGMError(f'env_params={dict(env_params)!r}: {os.path.basename(self.header)} has no runtime '
                           f'parameters (a CONTRACT = 2 header with NP > 0 declares them)')
        for name, value in dict(env_params).items():
            if name not in self.par_names:
                raise PGMError(f'env_params: {name!r} is not a runtime parameter of {os.path.basename(self.header)} '
                               f'(it has {", ".join(self.par_names)})')
            try:
                v = float(value)
            except (TypeError, ValueError):
                v = float('nan')
            if not np.isfinite(v):
                raise PGMError(f'env_params: {name}={value!r} must be a finite number')
            par[self.par_names.index(name)] = v
        return par

    def _par(self, par):
        par = self.par_default if par is None else np.ascontiguousarray(par, dtype=np.float64).reshape(-1)
        if par.size != self.NP:
            raise PGMError(f'par of {par.size} values: this plug-in has NP = {self.NP} runtime parameters')
        return par

    def uniforms(self, seed, start, n):
        """Elements start .. start + n - 1 of the env-noise stream of ``seed`` (pgm_envplug_uniforms): fp64 in [0, 1)."""
        out = np.zeros(int(n))
        self.check(self.h.pgm_envplug_uniforms(C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint64(int(start)),
                                               int(n), _np_ptr(out)), 'pgm_envplug_uniforms')
        return out

    # ---- the host functions: the compiled header on n items (numpy in, numpy out)
    def reset(self, row, episode, table, par=None):
        """Start states of the entries (row[i], episode[i] mod R) of table [rows][R][RW] -> (sd [n, SD], si [n, SI],
        obs [n, O]).  par: the NP runtime parameters (default: the header's)."""
        row = np.ascontiguousarray(row, dtype=np.int32).reshape(-1)
        episode = np.ascontiguousarray(episode, dtype=np.int32).reshape(-1)
        table = self._table(table)
        n = row.size
        sd, si = np.zeros((n, self.SD)), np.zeros((n, self.SI), dtype=np.int32)
        obs = np.zeros((n, self.O))
        if self.CONTRACT == 1:  # (NP = 0: nothing to pass)
            self.check(self.h.pgm_envplug_reset(n, _np_ptr(row), _np_ptr(episode), _np_ptr(table), table.shape[1],
                                                table.shape[0], _np_ptr(sd), _np_ptr(si), _np_ptr(obs)),
                       'pgm_envplug_reset')
            return sd, si, obs
        par = self._par(par)
        self.check(self.h.pgm_envplug_reset_ex(n, _np_ptr(row), _np_ptr(episode), _np_ptr(table), table.shape[1],
                                               table.shape[0], _np_ptr(par), _np_ptr(sd), _np_ptr(si), _np_ptr(obs)),
                   'pgm_envplug_reset_ex')
        return sd, si, obs

    def transition(self, sd, si, elapsed, episode, row, action, table, par=None, w=None):
        """One step of n envs with the forced limit and the auto-reset -> dict(sd, si, elapsed, episode, obs, obj,
        reward, done, bad).  action: float32 [n, A], or (DISCRETE) int32 [n].  par: the NP runtime parameters (default:
        the header's); w: the step's uniforms [n, NW], required with NW > 0."""
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
        outs = [_np_ptr(o[k]) for k in ('sd', 'si', 'elapsed', 'episode', 'obs', 'obj', 'reward', 'done', 'bad')]
        if self.CONTRACT == 1:  # (NP = NW = 0: nothing to pass)
            self.check(self.h.pgm_envplug_transition(
                n, _np_ptr(sd), _np_ptr(si), _np_ptr(elapsed), _np_ptr(episode), _np_ptr(row), _np_ptr(action),
                _np_ptr(table), table.shape[1], table.shape[0], *outs), 'pgm_envplug_transition')
            return o
        par = self._par(par)
        if self.NW > 0:
            if w is None:
                raise PGMError(f'transition: this plug-in takes NW = {self.NW} uniforms per step: give w [n, {self.NW}]')
            w = np.ascontiguousarray(w, dtype=np.float64).reshape(n, self.NW)
        else:
            w = None
        self.check(self.h.pgm_envplug_transition_ex(
            n, _np_ptr(sd), _np_ptr(si), _np_ptr(elapsed), _np_ptr(episode), _np_ptr(row), _np_ptr(action),
            _np_ptr(table), table.shape[1], table.shape[0], _np_ptr(par), None if w is None else _np_ptr(w), *outs),
            'pgm_envplug_transition_ex')
        return o

    def _table(self, table):
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.ndim != 3 or table.shape[2] != self.RW:
            raise PGMError(f'reset table of shape {table.shape}: this plug-in needs [rows][R][{self.RW}]')
        return table


def as_plugin(x):
    """An EnvPlugin from an EnvPlugin or a header path."""
    return x if isinstance(x, EnvPlugin) else EnvPlugin(x)
