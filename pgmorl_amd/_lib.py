"""ctypes binding of libpgm.so (include/pgm_abi.h).

torch is imported first so that the HIP runtime torch ships (same soname libamdhip64.so.7)
is the one libpgm.so binds to: device pointers and streams are then shared.
There is no fallback: if the library is missing or fails to load, every op raises.
"""
import contextlib
import ctypes as C
import os

import torch  # noqa: F401  (must precede loading libpgm.so)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PGM_LIB') or os.path.join(HERE, 'libpgm.so')
TEST_LIB_PATH = os.path.join(HERE, 'libpgm_test.so')  # -DPGM_TEST_HOOKS build (pgmorl_amd/build.py), tests only

PGM_ABI_VERSION = 5
PGM_ABI_MINOR = 1  # pgm_abi_minor(): the host-stepped environment entry points exist from minor 1
PGM_OK, PGM_E_INVALID_ARG, PGM_E_SHAPE, PGM_E_HIP, PGM_E_UNSUPPORTED = 0, -1, -2, -3, -4
PARAM_TENSORS = ['actor_w1', 'actor_b1', 'actor_w2', 'actor_b2', 'critic_w1', 'critic_b1', 'critic_w2',
                 'critic_b2', 'value_w', 'value_b', 'mean_w', 'mean_b', 'logstd']
# LayerNorm towers (Dims.LN = 1): PGM_PL_* order of pgm_param_layout_ln
PARAM_TENSORS_LN = ['actor_w1', 'actor_g1', 'actor_be1', 'actor_w2', 'actor_g2', 'actor_be2',
                    'critic_w1', 'critic_g1', 'critic_be1', 'critic_w2', 'critic_g2', 'critic_be2',
                    'value_w', 'value_b', 'mean_w', 'mean_b', 'logstd']
# Categorical head (discrete actions): the ten tower / value tensors, then dist.linear (pgm_param_layout_cat)
PARAM_TENSORS_CAT = PARAM_TENSORS[:10] + ['linear_w', 'linear_b']

P_ = C.c_void_p
I32 = C.c_int32
F32 = C.c_float
F64 = C.c_double


class Dims(C.Structure):
    """pgm_dims; LN = 1 selects the LayerNorm towers (0, the default, the plain ones)."""
    _fields_ = [(n, I32) for n in ('P', 'N', 'T', 'O', 'A', 'K', 'H', 'LN')]


class EnvSpec(C.Structure):
    _fields_ = [('d', P_), ('U', P_), ('c', P_), ('V', P_), ('ebase', P_), ('ecoef', P_), ('act_lo', P_),
                ('act_hi', P_), ('max_episode_steps', I32), ('_pad', I32)]


class EnvState(C.Structure):
    _fields_ = [('s', P_), ('elapsed', P_), ('obj_acc', P_), ('obj_acc_valid', P_), ('ret', P_), ('s0', P_)]


class NormState(C.Structure):
    _fields_ = [('ob_mean', P_), ('ob_var', P_), ('ob_count', P_), ('ret_mean', P_), ('ret_var', P_),
                ('ret_count', P_), ('obj_mean', P_), ('obj_var', P_), ('obj_count', P_), ('gamma', F64),
                ('clipob', F64), ('cliprew', F64), ('epsilon', F64), ('use_ob_rms', I32), ('use_obj_rms', I32)]


class RolloutBuf(C.Structure):
    _fields_ = [(n, P_) for n in ('obs', 'actions', 'logp', 'values', 'rewards', 'masks', 'bad_masks',
                                  'returns', 'adv')]


class PPOHParams(C.Structure):
    _fields_ = [('clip_param', F32), ('value_loss_coef', F32), ('entropy_coef', F32), ('max_grad_norm', F32),
                ('adam_eps', F32), ('beta1', F32), ('beta2', F32), ('_pad', F32), ('ppo_epoch', I32),
                ('num_mini_batch', I32), ('use_clipped_value_loss', I32), ('_pad2', I32)]


class DstSpec(C.Structure):
    """pgm_dst_spec: the device Deep Sea Treasure's step limit and how the limit is reported."""
    _fields_ = [('max_steps', I32), ('time_limit_is_bad', I32)]


class DummySpec(C.Structure):
    """pgm_dummy_spec: the MO-Dummy env's step limit, how an end on the limit step is reported, the disc radius and the
    reset table [reset_count][R][2] fp64."""
    _fields_ = [('max_steps', I32), ('time_limit_is_bad', I32), ('bound', F64), ('reset_table', P_), ('R', I32),
                ('reset_count', I32)]


class LaunchOpts(C.Structure):
    """pgm_launch_opts (pgm_abi.h): which kernel family an entry point may launch; all zero = automatic."""
    _fields_ = [(n, I32) for n in ('update_kernel', 'update_split', 'fs_one_per_cu', 'rollout_kernel', 'eval_kernel',
                                   '_pad')]


UPDATE_KERNELS = {'': 0, 'auto': 0, 'fs': 1, 'mfma': 2, 'rowsplit': 2, 'valu': 3}
UPDATE_SPLITS = {'': 0, '0': 1, '1': 2, '2': 3, '3': 3, '4': 4}  # the row-split cap -> PGM_SPLIT_*


def launch_opts(env=None):
    """The launch options of the A/B environment variables (read here, at every call: the library reads none):
    PGM_UPDATE_KERNEL = auto | fs | mfma | valu, PGM_UPDATE_SPLIT = 0 | 1 | 2 | 4 (row-split cap), PGM_FS_DUAL = 0
    (feature-split one workgroup per CU), PGM_ROLLOUT_KERNEL / PGM_EVAL_KERNEL = block."""
    env = os.environ if env is None else env
    k = env.get('PGM_UPDATE_KERNEL', '').strip().lower()
    sp = env.get('PGM_UPDATE_SPLIT', '').strip()
    if k not in UPDATE_KERNELS:
        raise PGMError(f'PGM_UPDATE_KERNEL={k!r}: expected one of {sorted(UPDATE_KERNELS)}')
    if sp not in UPDATE_SPLITS:
        raise PGMError(f'PGM_UPDATE_SPLIT={sp!r}: expected 0, 1, 2 or 4')
    return LaunchOpts(update_kernel=UPDATE_KERNELS[k], update_split=UPDATE_SPLITS[sp],
                      fs_one_per_cu=int(env.get('PGM_FS_DUAL', '').strip() == '0'),
                      rollout_kernel=int(env.get('PGM_ROLLOUT_KERNEL', '').strip().lower().startswith('b')),
                      eval_kernel=int(env.get('PGM_EVAL_KERNEL', '').strip().lower().startswith('b')))


_SIGS = {
    'pgm_abi_version': (C.c_int, []),
    'pgm_last_error': (C.c_char_p, []),
    'pgm_param_layout': (C.c_int, [I32, I32, I32, I32, C.POINTER(I32), C.POINTER(I32)]),
    'pgm_param_layout_ln': (C.c_int, [I32, I32, I32, I32, C.POINTER(I32), C.POINTER(I32)]),
    'pgm_act_forward': (C.c_int, [C.POINTER(Dims), P_, P_, P_, I32, P_, P_, P_, P_]),
    'pgm_env_reset': (C.c_int, [C.POINTER(Dims), C.POINTER(EnvSpec), C.POINTER(EnvState), C.POINTER(NormState),
                                P_, P_]),
    'pgm_env_step': (C.c_int, [C.POINTER(Dims), C.POINTER(EnvSpec), C.POINTER(EnvState), C.POINTER(NormState),
                               P_, P_, P_, P_, P_, P_]),
    'pgm_rollout': (C.c_int, [C.POINTER(Dims), P_, C.POINTER(EnvSpec), C.POINTER(EnvState), C.POINTER(NormState),
                              C.POINTER(RolloutBuf), P_, C.c_uint64, I32, C.POINTER(LaunchOpts), P_]),
    'pgm_gae': (C.c_int, [C.POINTER(Dims), C.POINTER(RolloutBuf), F32, F32, I32, I32, P_]),
    'pgm_adv_normalize': (C.c_int, [C.POINTER(Dims), C.POINTER(RolloutBuf), P_, P_, P_]),
    'pgm_ppo_update': (C.c_int, [C.POINTER(Dims), C.POINTER(PPOHParams), P_, P_, P_, P_, P_, P_,
                                 C.POINTER(RolloutBuf), P_, P_, C.POINTER(LaunchOpts), P_]),
    'pgm_ppo_update_workspace_bytes': (C.c_size_t, [C.POINTER(Dims)]),
    'pgm_ppo_update_variant': (C.c_int, [C.POINTER(Dims), C.c_void_p, C.POINTER(LaunchOpts), C.c_char_p, C.c_int]),
    'pgm_ppo_update_reset': (C.c_int, [C.POINTER(Dims), P_, P_]),
    'pgm_ppo_fs_fragment_map': (C.c_int, [I32, I32, I32, I32, C.POINTER(I32), I32]),
    'pgm_eval': (C.c_int, [C.POINTER(Dims), P_, C.POINTER(EnvSpec), P_, P_, P_, I32, I32, I32, F64, P_,
                           C.POINTER(LaunchOpts), P_]),
    'pgm_randperm': (C.c_int, [I32, I32, C.c_uint64, P_, P_]),
    'pgm_normal_noise': (C.c_int, [C.c_int64, C.c_uint64, P_, P_]),
    # host-stepped environments (ABI minor 1)
    'pgm_abi_minor': (C.c_int, []),
    'pgm_rollout_act': (C.c_int, [C.POINTER(Dims), P_, C.POINTER(RolloutBuf), I32, P_, P_, P_]),
    'pgm_env_ingest': (C.c_int, [C.POINTER(Dims), C.POINTER(EnvState), C.POINTER(NormState), C.POINTER(RolloutBuf),
                                 I32, P_, P_, P_, P_, P_, P_]),
    'pgm_eval_act': (C.c_int, [C.POINTER(Dims), P_, P_, P_, I32, P_, I32, P_, P_]),
    # discrete-action policies (pgm_abi_features() & FEATURE_CATEGORICAL)
    'pgm_abi_features': (C.c_int, []),
    'pgm_abi_feature_mask': (C.c_int, []),
    'pgm_param_layout_cat': (C.c_int, [I32, I32, I32, I32, C.POINTER(I32), C.POINTER(I32)]),
    'pgm_act_forward_cat': (C.c_int, [C.POINTER(Dims), P_, P_, P_, I32, P_, P_, P_, P_]),
    'pgm_rollout_act_cat': (C.c_int, [C.POINTER(Dims), P_, C.POINTER(RolloutBuf), I32, P_, P_, P_]),
    'pgm_eval_act_cat': (C.c_int, [C.POINTER(Dims), P_, P_, P_, I32, P_, I32, P_, P_]),
    'pgm_ppo_update_cat': (C.c_int, [C.POINTER(Dims), C.POINTER(PPOHParams), P_, P_, P_, P_, P_, P_,
                                     C.POINTER(RolloutBuf), P_, P_, P_]),
    'pgm_ppo_update_cat_workspace_bytes': (C.c_size_t, [C.POINTER(Dims)]),
    'pgm_uniform_noise': (C.c_int, [C.c_int64, C.c_uint64, P_, P_]),
    # Deep Sea Treasure on the device (pgm_abi_features() & FEATURE_DST_DEVICE)
    'pgm_rollout_dst': (C.c_int, [C.POINTER(Dims), P_, C.POINTER(DstSpec), C.POINTER(EnvState), C.POINTER(NormState),
                                  C.POINTER(RolloutBuf), P_, C.c_uint64, I32, P_]),
    'pgm_eval_dst': (C.c_int, [C.POINTER(Dims), P_, C.POINTER(DstSpec), P_, P_, I32, I32, I32, F64, P_, P_]),
    'pgm_dst_transition': (C.c_int, [C.POINTER(DstSpec), I32] + [P_] * 12),
    # the MO-Dummy envs on the device (pgm_abi_features() & FEATURE_DUMMY_DEVICE)
    'pgm_rollout_dummy': (C.c_int, [C.POINTER(Dims), P_, C.POINTER(DummySpec), C.POINTER(EnvState), P_,
                                    C.POINTER(NormState), C.POINTER(RolloutBuf), P_, C.c_uint64, I32, P_]),
    'pgm_eval_dummy': (C.c_int, [C.POINTER(Dims), P_, C.POINTER(DummySpec), P_, P_, I32, I32, I32, F64, P_, P_]),
    'pgm_dummy_transition': (C.c_int, [C.POINTER(DummySpec), I32, I32] + [P_] * 12),
    # host-stepped environments of any dims (pgm_abi_feature_mask() & FEATURE_ANY_DIMS); the second argument is the head
    'pgm_rollout_act_any': (C.c_int, [C.POINTER(Dims), I32, P_, C.POINTER(RolloutBuf), I32, P_, P_, P_]),
    'pgm_eval_act_any': (C.c_int, [C.POINTER(Dims), I32, P_, P_, P_, I32, P_, I32, P_, P_]),
    'pgm_env_ingest_any': (C.c_int, [C.POINTER(Dims), C.POINTER(EnvState), C.POINTER(NormState),
                                     C.POINTER(RolloutBuf), I32, P_, P_, P_, P_, P_, P_]),
    'pgm_ppo_update_any': (C.c_int, [C.POINTER(Dims), I32, C.POINTER(PPOHParams), P_, P_, P_, P_, P_, P_,
                                     C.POINTER(RolloutBuf), P_, P_, P_]),
    'pgm_ppo_update_any_workspace_bytes': (C.c_size_t, [C.POINTER(Dims)]),
    # several runs of a sweep in one population (no feature bit: discovered by the symbol pgm_rollout_runs);
    # run_of_task (device int32 [P]) and num_runs sit before obs_out / opts
    'pgm_env_reset_runs': (C.c_int, [C.POINTER(Dims), C.POINTER(EnvSpec), C.POINTER(EnvState), C.POINTER(NormState),
                                     P_, I32, P_, P_]),
    'pgm_rollout_runs': (C.c_int, [C.POINTER(Dims), P_, C.POINTER(EnvSpec), C.POINTER(EnvState), C.POINTER(NormState),
                                   C.POINTER(RolloutBuf), P_, C.c_uint64, I32, P_, I32, C.POINTER(LaunchOpts), P_]),
    'pgm_eval_runs': (C.c_int, [C.POINTER(Dims), P_, C.POINTER(EnvSpec), P_, P_, P_, I32, I32, I32, F64, P_, P_, I32,
                                C.POINTER(LaunchOpts), P_]),
    # per-task PPO settings of a hyper-parameter grid (no feature bit: discovered by the symbol pgm_ppo_update_tasks);
    # hp_task (device pgm_task_hparams [P]) sits after hp, lam_task (device float [P]) in the place of lam
    'pgm_ppo_update_tasks': (C.c_int, [C.POINTER(Dims), C.POINTER(PPOHParams), P_, P_, P_, P_, P_, P_, P_,
                                       C.POINTER(RolloutBuf), P_, P_, C.POINTER(LaunchOpts), P_]),
    'pgm_gae_tasks': (C.c_int, [C.POINTER(Dims), C.POINTER(RolloutBuf), F32, P_, I32, I32, P_]),
    # re-evaluation of a saved Pareto set (no feature bit: discovered by the symbol itself): params, spec, ob_mean,
    # ob_var, starts, E, use_ob_rms, raw, gamma, stochastic, noise_seed, episodes_out, objs_out
    'pgm_eval_episodes': (C.c_int, [C.POINTER(Dims), P_, C.POINTER(EnvSpec), P_, P_, P_, I32, I32, I32, F64, I32,
                                    C.c_uint64, P_, P_, P_]),
    # a dense front from blended members (no feature bit: discovered by the symbol itself): params, M, ob_mean, ob_var,
    # src, alpha, spec, starts, E, use_ob_rms, raw, gamma, episodes_out, objs_out
    'pgm_eval_blend': (C.c_int, [C.POINTER(Dims), P_, I32, P_, P_, P_, P_, C.POINTER(EnvSpec), P_, I32, I32, I32, F64,
                                 P_, P_, P_]),
    # simplex candidates of a three-objective front (no feature bit: discovered by the symbol itself): pgm_eval_blend's
    # arguments with src int32 [Q][3] and w fp64 [Q][3] in the places of src and alpha
    'pgm_eval_blend3': (C.c_int, [C.POINTER(Dims), P_, I32, P_, P_, P_, P_, C.POINTER(EnvSpec), P_, I32, I32, I32, F64,
                                  P_, P_, P_]),
}
RUNS_SYMBOLS = ('pgm_env_reset_runs', 'pgm_rollout_runs', 'pgm_eval_runs')
TASKS_SYMBOLS = ('pgm_ppo_update_tasks', 'pgm_gae_tasks')
EVAL_EPISODES_SYMBOLS = ('pgm_eval_episodes',)
EVAL_BLEND_SYMBOLS = ('pgm_eval_blend',)
EVAL_BLEND3_SYMBOLS = ('pgm_eval_blend3',)
EVAL_EPISODES_MAX = 65536  # episodes per policy in one pgm_eval_episodes call
TASK_HPARAM_FIELDS =('clip_param', 'value_loss_coef', 'entropy_coef', 'max_grad_norm')  # pgm_task_hparams, in order
# the symbols a library of the same ABI version and minor may lack: discovered through pgm_abi_features
FEATURE_CATEGORICAL = 1
FEATURE_DST_DEVICE = 2
FEATURE_DUMMY_DEVICE = 4
FEATURE_ANY_DIMS = 8
# the range of the runtime-dim kernel family (pgm_anydims.hpp)
ANY_MAX_OBS, ANY_MAX_ACT, ANY_MAX_OBJ = 32, 8, 3
_FEATURE_SYMBOLS = {'pgm_abi_features': 0, 'pgm_abi_feature_mask': 0, 'pgm_param_layout_cat': FEATURE_CATEGORICAL,
                    'pgm_act_forward_cat': FEATURE_CATEGORICAL, 'pgm_rollout_act_cat': FEATURE_CATEGORICAL,
                    'pgm_eval_act_cat': FEATURE_CATEGORICAL, 'pgm_ppo_update_cat': FEATURE_CATEGORICAL,
                    'pgm_ppo_update_cat_workspace_bytes': FEATURE_CATEGORICAL,
                    'pgm_uniform_noise': FEATURE_CATEGORICAL, 'pgm_rollout_dst': FEATURE_DST_DEVICE,
                    'pgm_eval_dst': FEATURE_DST_DEVICE, 'pgm_dst_transition': FEATURE_DST_DEVICE,
                    'pgm_rollout_dummy': FEATURE_DUMMY_DEVICE, 'pgm_eval_dummy': FEATURE_DUMMY_DEVICE,
                    'pgm_dummy_transition': FEATURE_DUMMY_DEVICE, 'pgm_rollout_act_any': FEATURE_ANY_DIMS,
                    'pgm_eval_act_any': FEATURE_ANY_DIMS, 'pgm_env_ingest_any': FEATURE_ANY_DIMS,
                    'pgm_ppo_update_any': FEATURE_ANY_DIMS, 'pgm_ppo_update_any_workspace_bytes': FEATURE_ANY_DIMS}

EXPORTS = tuple(_SIGS)

_libs = {}
_active = None


class PGMError(RuntimeError):
    pass


def _load(path):
    if path not in _libs:
        if not os.path.exists(path):
            raise PGMError(f'{path} not built; run `python -m pgmorl_amd.build` (hipcc, gfx950)')
        h = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            if (name in _FEATURE_SYMBOLS or name in RUNS_SYMBOLS or name in TASKS_SYMBOLS or
                    name in EVAL_EPISODES_SYMBOLS or name in EVAL_BLEND_SYMBOLS or
                    name in EVAL_BLEND3_SYMBOLS) and not hasattr(h, name):
                continue  # an older library of this ABI: features() / has_runs() / has_tasks() / has_eval_episodes()
                # / has_eval_blend() / has_eval_blend3() report what is missing
            f = getattr(h, name)
            f.restype, f.argtypes = res, args
        if h.pgm_abi_version() != PGM_ABI_VERSION:
            raise PGMError(f'{path}: ABI {h.pgm_abi_version()} != {PGM_ABI_VERSION}')
        _libs[path] = h
    return _libs[path]


def lib():
    """The loaded libpgm.so (raises if it is missing: there is no CPU fallback); inside test_build(), the test
    build."""
    return _active if _active is not None else _load(LIB_PATH)


@contextlib.contextmanager
def test_build():
    """Route every call of the block through libpgm_test.so, the build with the PGM_TEST_DELAY /
    PGM_TEST_RESIDENT_CUS hooks (tests only; the production library has neither)."""
    global _active
    prev, _active = _active, _load(TEST_LIB_PATH)
    try:
        yield _active
    finally:
        _active = prev


def check(rc, what):
    if rc != PGM_OK:
        msg = lib().pgm_last_error().decode(errors='replace')
        raise PGMError(f'{what} failed ({rc}): {msg}')


def param_layout(O, A, K, H=64):
    """(offsets dict, total) of the flat per-task parameter vector (pgm_param_layout)."""
    offs = (I32 * 13)()
    tot = I32()
    check(lib().pgm_param_layout(O, A, K, H, offs, C.byref(tot)), 'pgm_param_layout')
    return dict(zip(PARAM_TENSORS, list(offs))), tot.value


def features():
    """The bit mask of optional entry-point groups: pgm_abi_feature_mask() (every group), or pgm_abi_features() (the
    groups up to bit 4, its value frozen) from a library without it; a library with neither symbol has none."""
    h = lib()
    if hasattr(h, 'pgm_abi_feature_mask'):
        return int(h.pgm_abi_feature_mask())
    return int(h.pgm_abi_features()) if hasattr(h, 'pgm_abi_features') else 0


def require_categorical():
    if not features() & FEATURE_CATEGORICAL:
        raise PGMError('this libpgm.so has no Categorical-head entry points (pgm_abi_features() & 1 is clear); '
                       'rebuild it with `python -m pgmorl_amd.build`')


def require_dst_device():
    if not features() & FEATURE_DST_DEVICE:
        raise PGMError('this libpgm.so has no device Deep Sea Treasure entry points (pgm_abi_features() & 2 is clear); '
                       'rebuild it with `python -m pgmorl_amd.build`')


def require_dummy_device():
    if not features() & FEATURE_DUMMY_DEVICE:
        raise PGMError('this libpgm.so has no MO-Dummy entry points or dim sets (pgm_abi_features() & 4 is clear); '
                       'rebuild it with `python -m pgmorl_amd.build`')


def require_any_dims():
    if not features() & FEATURE_ANY_DIMS:
        raise PGMError('this libpgm.so has no runtime-dim entry points (pgm_abi_feature_mask() & 8 is clear); '
                       'rebuild it with `python -m pgmorl_amd.build`')


def has_runs():
    """True if the library has the *_runs entry points (several runs in one population): the presence of the symbol
    pgm_rollout_runs, as include/pgm_abi.h documents (there is no feature bit)."""
    return hasattr(lib(), 'pgm_rollout_runs')


def require_runs():
    if not has_runs():
        raise PGMError('this libpgm.so has no pgm_rollout_runs (the per-run reset tables of a batched sweep); '
                       'rebuild it with `python -m pgmorl_amd.build`')


def has_tasks():
    """True if the library has the *_tasks entry points (per-task PPO settings): the presence of the symbol
    pgm_ppo_update_tasks, as include/pgm_abi.h documents (there is no feature bit)."""
    return hasattr(lib(), 'pgm_ppo_update_tasks')


def require_tasks():
    if not has_tasks():
        raise PGMError('this libpgm.so has no pgm_ppo_update_tasks (the per-task PPO settings of a hyper-parameter '
                       'grid); rebuild it with `python -m pgmorl_amd.build`')


def has_eval_episodes():
    """True if the library has pgm_eval_episodes (re-evaluation of a saved Pareto set): the presence of the symbol, as
    include/pgm_abi.h documents (there is no feature bit)."""
    return hasattr(lib(), 'pgm_eval_episodes')


def require_eval_episodes():
    if not has_eval_episodes():
        raise PGMError('this libpgm.so has no pgm_eval_episodes (the re-evaluation of a saved Pareto set); '
                       'rebuild it with `python -m pgmorl_amd.build`')


def has_eval_blend():
    """True if the library has pgm_eval_blend (evaluation of policies blended between two members of a Pareto set):
    the presence of the symbol, as include/pgm_abi.h documents (there is no feature bit)."""
    return hasattr(lib(), 'pgm_eval_blend')


def require_eval_blend():
    if not has_eval_blend():
        raise PGMError('this libpgm.so has no pgm_eval_blend (the evaluation of blended policies); '
                       'rebuild it with `python -m pgmorl_amd.build`')


def has_eval_blend3():
    """True if the library has pgm_eval_blend3 (evaluation of policies blended among three members of a Pareto set):
    the presence of the symbol, as include/pgm_abi.h documents (there is no feature bit)."""
    return hasattr(lib(), 'pgm_eval_blend3')


def require_eval_blend3():
    if not has_eval_blend3():
        raise PGMError('this libpgm.so has no pgm_eval_blend3 (the evaluation of three-member blends); '
                       'rebuild it with `python -m pgmorl_amd.build`')


def param_layout_cat(O, A, K, H=64):
    """(offsets dict, total) of the flat per-task parameter vector of a Categorical-head policy, A = number of
    actions (pgm_param_layout_cat)."""
    require_categorical()
    offs = (I32 * len(PARAM_TENSORS_CAT))()
    tot = I32()
    check(lib().pgm_param_layout_cat(O, A, K, H, offs, C.byref(tot)), 'pgm_param_layout_cat')
    return dict(zip(PARAM_TENSORS_CAT, list(offs))), tot.value


def param_layout_ln(O, A, K, H=64):
    """(offsets dict, total) of the flat per-task parameter vector of LayerNorm towers (pgm_param_layout_ln)."""
    offs = (I32 * len(PARAM_TENSORS_LN))()
    tot = I32()
    check(lib().pgm_param_layout_ln(O, A, K, H, offs, C.byref(tot)), 'pgm_param_layout_ln')
    return dict(zip(PARAM_TENSORS_LN, list(offs))), tot.value
