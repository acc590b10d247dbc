"""CPU-side checks of the *_runs entry points (several runs of a sweep in one population, include/pgm_abi.h) and of
TaskBatch(run_seeds=...): the argument refusals before any device work, the unchanged version pair and feature values,
and the host-side checks of set_runs / run_seeds.  No kernel is launched here."""
import ctypes as C

import numpy as np
import pytest

from pgmorl_amd import _lib
from pgmorl_amd._lib import PGM_E_INVALID_ARG, PGM_E_SHAPE, PGM_E_UNSUPPORTED, PGMError

ONE = C.c_void_p(1)  # a non-NULL pointer nothing dereferences: every refusal below precedes device work


def _structs(null_spec=False, null_rb=False):
    spec = _lib.EnvSpec(*([None if null_spec else ONE] * 8), 20, 0)
    st = _lib.EnvState(ONE, ONE, ONE, ONE, ONE, ONE)
    ns = _lib.NormState(*([ONE] * 9), 0.995, 10.0, 10.0, 1e-8, 1, 1)
    rb = _lib.RolloutBuf(*([None if null_rb else ONE] * 9))
    return spec, st, ns, rb


def _err():
    return _lib.lib().pgm_last_error().decode()


def test_version_pair_and_feature_values_are_unchanged():
    L = _lib.lib()
    assert (L.pgm_abi_version(), L.pgm_abi_minor()) == (5, 1)
    assert L.pgm_abi_features() == 7 and L.pgm_abi_feature_mask() == 15
    assert _lib.has_runs() and all(hasattr(L, s) for s in _lib.RUNS_SYMBOLS)


def _same_refusal(runs_call, base_call, want_rc, want_text, **kw):
    """A bad argument of the existing entry point: the _runs form refuses it with the same status and the same string,
    also when its own run arguments are bad too (the earlier item wins)."""
    rc0 = base_call(**kw)
    msg0 = _err()
    assert rc0 == want_rc and want_text in msg0, (kw, rc0, msg0)
    for runs_kw in (dict(), dict(runs=None), dict(num_runs=0)):
        rc = runs_call(**kw, **runs_kw)
        assert (rc, _err()) == (rc0, msg0), (kw, runs_kw, rc, _err())


def _own_refusals(runs_call, name):
    """Then the run arguments, PGM_E_INVALID_ARG naming the _runs entry point."""
    for runs_kw in (dict(runs=None), dict(num_runs=0), dict(num_runs=-2), dict(runs=None, num_runs=0)):
        assert runs_call(**runs_kw) == PGM_E_INVALID_ARG and name in _err(), runs_kw


def test_rollout_runs_refusals_in_order():
    L = _lib.lib()
    spec, st, ns, rb = _structs()
    ok = _lib.Dims(5, 4, 64, 17, 6, 2, 64)

    def base(d=ok, spec=spec, rb=rb, opts=None, params=ONE):
        return L.pgm_rollout(C.byref(d), params, C.byref(spec), C.byref(st), C.byref(ns), C.byref(rb), None, 0, 0,
                             opts, None)

    def runs(d=ok, spec=spec, rb=rb, opts=None, params=ONE, runs=ONE, num_runs=3):
        return L.pgm_rollout_runs(C.byref(d), params, C.byref(spec), C.byref(st), C.byref(ns), C.byref(rb), None, 0, 0,
                                  runs, num_runs, opts, None)
    # pgm_rollout's checks in its order: dims, struct pointers, LN, launch opts, pointers, T
    _same_refusal(runs, base, PGM_E_SHAPE, 'pgm_rollout', d=_lib.Dims(0, 4, 64, 17, 6, 2, 64))
    _same_refusal(runs, base, PGM_E_UNSUPPORTED, 'hidden size', d=_lib.Dims(5, 4, 64, 17, 6, 2, 32))
    _same_refusal(runs, base, PGM_E_INVALID_ARG, 'pgm_rollout: null pointer in spec/state/norm structs',
                  spec=_structs(null_spec=True)[0])
    _same_refusal(runs, base, PGM_E_UNSUPPORTED, 'pgm_rollout', d=_lib.Dims(5, 4, 64, 376, 17, 2, 64, 1))
    _same_refusal(runs, base, PGM_E_INVALID_ARG, 'pgm_launch_opts', opts=C.byref(_lib.LaunchOpts(rollout_kernel=3)))
    _same_refusal(runs, base, PGM_E_INVALID_ARG, 'pgm_rollout: null pointer', params=None)
    _same_refusal(runs, base, PGM_E_INVALID_ARG, 'pgm_rollout: null pointer', rb=_structs(null_rb=True)[3])
    _same_refusal(runs, base, PGM_E_SHAPE, 'T must be positive', d=_lib.Dims(5, 4, 0, 17, 6, 2, 64))
    # an earlier item wins among the existing checks too: bad opts and a NULL params report the opts
    _same_refusal(runs, base, PGM_E_INVALID_ARG, 'pgm_launch_opts', opts=C.byref(_lib.LaunchOpts(rollout_kernel=3)),
                  params=None)
    _own_refusals(runs, 'pgm_rollout_runs')


def test_eval_runs_refusals_in_order():
    L = _lib.lib()
    spec = _structs()[0]
    ok = _lib.Dims(5, 4, 64, 11, 3, 3, 64)

    def base(d=ok, spec=spec, opts=None, s0=ONE, eval_num=1, out=ONE):
        return L.pgm_eval(C.byref(d), ONE, C.byref(spec), ONE, ONE, s0, eval_num, 1, 1, 0.995, out, opts, None)

    def runs(d=ok, spec=spec, opts=None, s0=ONE, eval_num=1, out=ONE, runs=ONE, num_runs=3):
        return L.pgm_eval_runs(C.byref(d), ONE, C.byref(spec), ONE, ONE, s0, eval_num, 1, 1, 0.995, out, runs,
                               num_runs, opts, None)
    _same_refusal(runs, base, PGM_E_UNSUPPORTED, 'hidden size', d=_lib.Dims(5, 4, 64, 11, 3, 3, 32))
    _same_refusal(runs, base, PGM_E_UNSUPPORTED, 'pgm_eval', d=_lib.Dims(5, 4, 64, 376, 17, 2, 64, 1))
    # (a dim set no kernel is compiled for is found by the dispatch, after every argument check, the run ones included)
    assert runs(d=_lib.Dims(5, 4, 64, 19, 3, 3, 64), runs=None) == PGM_E_INVALID_ARG and 'pgm_eval_runs' in _err()
    assert runs(d=_lib.Dims(5, 4, 64, 19, 3, 3, 64)) == PGM_E_UNSUPPORTED and 'unsupported dims' in _err()
    _same_refusal(runs, base, PGM_E_INVALID_ARG, 'pgm_launch_opts', opts=C.byref(_lib.LaunchOpts(eval_kernel=-1)))
    for kw in (dict(s0=None), dict(eval_num=0), dict(out=None), dict(spec=_structs(null_spec=True)[0])):
        _same_refusal(runs, base, PGM_E_INVALID_ARG, 'pgm_eval: bad arguments', **kw)
    _same_refusal(runs, base, PGM_E_INVALID_ARG, 'pgm_launch_opts', opts=C.byref(_lib.LaunchOpts(eval_kernel=-1)),
                  s0=None)
    _own_refusals(runs, 'pgm_eval_runs')


def test_env_reset_runs_refusals_in_order():
    L = _lib.lib()
    spec, st, ns, _ = _structs()
    ok = _lib.Dims(5, 3, 64, 17, 6, 2, 64)

    def base(d=ok, spec=spec, out=ONE):
        return L.pgm_env_reset(C.byref(d), C.byref(spec), C.byref(st), C.byref(ns), out, None)

    def runs(d=ok, spec=spec, out=ONE, runs=ONE, num_runs=3):
        return L.pgm_env_reset_runs(C.byref(d), C.byref(spec), C.byref(st), C.byref(ns), runs, num_runs, out, None)
    _same_refusal(runs, base, PGM_E_UNSUPPORTED, 'hidden size', d=_lib.Dims(5, 3, 64, 17, 6, 2, 32))
    _same_refusal(runs, base, PGM_E_INVALID_ARG, 'pgm_env_reset: null pointer in spec/state/norm structs',
                  spec=_structs(null_spec=True)[0])
    _same_refusal(runs, base, PGM_E_INVALID_ARG, 'pgm_env_reset: null obs_out', out=None)
    _same_refusal(runs, base, PGM_E_UNSUPPORTED, 'hidden size', d=_lib.Dims(5, 3, 64, 17, 6, 2, 32), out=None)
    _own_refusals(runs, 'pgm_env_reset_runs')


@pytest.mark.parametrize('kw,flag', [(dict(host_env=object()), 'host_env'), (dict(device_env=True), 'device_env'),
                                     (dict(env_plugin='nowhere.hpp'), 'env_plugin')])
def test_run_seeds_refused_with_excluded_flags(kw, flag):
    from pgmorl_amd.runtime import TaskBatch
    with pytest.raises(PGMError, match=flag):
        TaskBatch('MO-Hopper-v2', 2, num_processes=2, num_steps=8, device='cpu', run_seeds=[0, 1], **kw)


@pytest.mark.parametrize('env', ['MO-Dummy-v0', 'MO-Dummy3-v0', 'MO-DeepSeaTreasure-v0'])
def test_run_seeds_refused_with_other_env_families(env):
    from pgmorl_amd.runtime import TaskBatch
    with pytest.raises(PGMError, match='run_seeds'):
        TaskBatch(env, 2, num_processes=2, num_steps=8, device='cpu', run_seeds=[0, 1])
    with pytest.raises(PGMError, match='run_seeds'):
        TaskBatch('MO-Hopper-v2', 2, num_processes=2, num_steps=8, device='cpu', run_seeds=[])


def test_set_runs_range_and_length():
    """The kernels trust the device ids: set_runs checks them on the host.  (A CPU-resident batch: nothing launches.)"""
    from pgmorl_amd import envspec
    from pgmorl_amd.runtime import TaskBatch
    tb = TaskBatch('MO-Hopper-v2', 3, num_processes=2, num_steps=8, eval_num=3, device='cpu', capacity=4,
                   run_seeds=[0, 7, 815117])
    assert tuple(tb.s0_train.shape) == (3, 2, 11) and tuple(tb.s0_eval.shape) == (3, 3, 11)
    np.testing.assert_array_equal(tb.s0_train[2].numpy(), envspec.reset_table(11, 815117, 2))
    np.testing.assert_array_equal(tb.s0_eval[1].numpy(), envspec.reset_table(11, 7, 3))
    tb.set_runs([2, 0, 1])
    assert tb.run_of_task.tolist() == [2, 0, 1, 0] and tb.run_of_task.dtype.is_floating_point is False
    for bad in ([0, 1], [0, 1, 2, 0], [[0, 1, 2]]):
        with pytest.raises(PGMError, match='active tasks'):
            tb.set_runs(bad)
    for bad in ([0, 1, 3], [-1, 0, 0], [0.0, 1.0, 2.0]):
        with pytest.raises(PGMError, match=r'\[0, 3\)'):
            tb.set_runs(bad)
    assert tb.run_of_task.tolist() == [2, 0, 1, 0]  # a refused call uploads nothing
    plain = TaskBatch('MO-Hopper-v2', 3, num_processes=2, num_steps=8, device='cpu')
    assert plain.run_seeds is None and tuple(plain.s0_train.shape) == (2, 11)
    with pytest.raises(PGMError, match='run_seeds'):
        plain.set_runs([0, 0, 0])


def test_population_refuses_run_of_task_without_run_seeds():
    import argparse

    from pgmorl_amd.mopg import MOPGPopulation
    rt = MOPGPopulation(argparse.Namespace(env_name='MO-Hopper-v2'), device='cpu')
    with pytest.raises(PGMError, match='run_seeds'):
        rt._set_runs(None, [0], 1)
    rt = MOPGPopulation(argparse.Namespace(env_name='MO-Hopper-v2'), device='cpu', run_seeds=[3, 4])
    with pytest.raises(PGMError, match='run_of_task is required'):
        rt._set_runs(None, None, 1)
