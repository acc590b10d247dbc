"""The library calls TaskBatch makes, per env mode and kernel family, as literal sequences.

A recording stand-in replaces the loaded library (``_lib._active``; for a plug-in batch also ``plugin.h``): it looks
every symbol up on the real handle, so a missing optional symbol still raises AttributeError, and returns a wrapper
that appends the symbol's name to a list; pgm_env_ingest* and pgm_rollout_act* are recorded with their step argument
(pgm_eval_act* has none: the name alone).  The host-only queries -- pgm_abi_*, *_workspace_bytes, pgm_param_layout*,
pgm_last_error and a plug-in's info / reset / transition / uniform functions -- launch nothing: they are forwarded and
not recorded.  Without a device every other symbol is recorded and answers PGM_OK uncalled; on the device it is recorded
and called.  The expected sequences below are the kernel sequence of each combination written out by hand, not generated
from the code under test."""
import re

import numpy as np
import pytest
import torch

from pgmorl_amd import _lib, runtime
from pgmorl_amd._lib import PGMError
from pgmorl_amd.hostenv import DeepSeaTreasureHostVecEnv, SynthHostVecEnv
from pgmorl_amd.runtime import TaskBatch

from .test_envplug2 import plugins  # noqa: F401 (fixture: the test headers' libraries, built and loaded once)

HOST_ONLY = re.compile(r'pgm_abi_|pgm_\w*workspace_bytes$|pgm_param_layout|pgm_last_error$|'
                       r'pgm_envplug_(abi|info|params|last_error|reset|transition|uniforms)')
SYNTH, DST, DUMMY = 'MO-Hopper-v2', 'MO-DeepSeaTreasure-v0', 'MO-Dummy-v0'


class Recorder:
    def __init__(self, real, calls, launch):
        self._real, self._calls, self._launch = real, calls, launch

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if HOST_ONLY.match(name):
            return fn

        def call(*args):
            what = name
            if name.startswith('pgm_env_ingest'):  # (dims, state, norm, rb, t, ...)
                what += f'({int(args[4])})'
            elif name.startswith('pgm_rollout_act'):  # (dims, [head,] params, rb, t, ...)
                what += f'({int(args[4 if name.endswith("_any") else 3])})'
            self._calls.append(what)
            return fn(*args) if self._launch else _lib.PGM_OK
        return call


def _record(monkeypatch, launch, plugin=None):
    calls = []
    monkeypatch.setattr(_lib, '_active', Recorder(_lib.lib(), calls, launch))
    if plugin is not None:
        monkeypatch.setattr(plugin, 'h', Recorder(plugin.h, calls, launch))
    if not launch:
        monkeypatch.setattr(runtime, '_stream', lambda: None)
    return calls


def _take(calls):
    got = list(calls)
    del calls[:]
    return got


# ------------------------------------------------------------------------------------------------ 1. without a device
ITER = ['pgm_normal_noise', 'pgm_rollout', 'pgm_gae', 'pgm_adv_normalize', 'pgm_randperm', 'pgm_ppo_update',
        'pgm_eval']
FUSED = ['pgm_gae', 'pgm_adv_normalize', 'pgm_randperm']  # between a fused rollout and the update
TINY = dict(num_processes=2, num_steps=8, ppo_epoch=1, num_mini_batch=2, device='cpu')


def _reset_and_iterate(tb, calls):
    tb.env_reset()
    reset = _take(calls)
    tb.iteration(0, 3e-4, overlap_eval=False)
    return reset, _take(calls)


@pytest.mark.parametrize('layernorm', [False, True], ids=['plain', 'layernorm'])
def test_synthmo(monkeypatch, layernorm):
    calls = _record(monkeypatch, False)
    tb = TaskBatch(SYNTH, 2, layernorm=layernorm, **TINY)
    assert not calls, 'the constructor launches nothing'
    assert _reset_and_iterate(tb, calls) == (['pgm_env_reset'], ITER)


def test_synthmo_runs(monkeypatch):
    calls = _record(monkeypatch, False)
    tb = TaskBatch(SYNTH, 2, run_seeds=[0, 1], **TINY)
    assert _reset_and_iterate(tb, calls) == (
        ['pgm_env_reset_runs'],
        ['pgm_normal_noise', 'pgm_rollout_runs', 'pgm_gae', 'pgm_adv_normalize', 'pgm_randperm', 'pgm_ppo_update',
         'pgm_eval_runs'])
    with pytest.raises(PGMError, match='a multi-run batch'):
        tb.env_step(torch.zeros(2, 2, 3))


def test_synthmo_task_hparams(monkeypatch):
    calls = _record(monkeypatch, False)
    tb = TaskBatch(SYNTH, 2, **TINY)
    tb.set_task_hparams(clip_param=[0.1, 0.3])
    assert _reset_and_iterate(tb, calls) == (
        ['pgm_env_reset'],
        ['pgm_normal_noise', 'pgm_rollout', 'pgm_gae_tasks', 'pgm_adv_normalize', 'pgm_randperm',
         'pgm_ppo_update_tasks', 'pgm_eval'])


def test_dst_device(monkeypatch):
    calls = _record(monkeypatch, False)
    tb = TaskBatch(DST, 2, device_env=True, **TINY)
    assert _reset_and_iterate(tb, calls) == (
        ['pgm_env_ingest(-1)'], ['pgm_rollout_dst'] + FUSED + ['pgm_ppo_update_cat', 'pgm_eval_dst'])
    assert tb.update_variant() == 'ppo_update_cat_kernel (one workgroup per tower)' and not calls
    with pytest.raises(PGMError, match='pgm_dst_transition'):
        tb.env_step(torch.zeros(2, 2, 1))


def test_dummy_device(monkeypatch):
    calls = _record(monkeypatch, False)
    tb = TaskBatch(DUMMY, 2, **TINY)
    assert _reset_and_iterate(tb, calls) == (
        ['pgm_env_ingest(-1)'], ['pgm_rollout_dummy'] + FUSED + ['pgm_ppo_update', 'pgm_eval_dummy'])
    with pytest.raises(PGMError, match='pgm_dummy_transition'):
        tb.env_step(torch.zeros(2, 2, 2))


@pytest.mark.parametrize('name,env_name,ex', [('line', 'DispatchLine-v0', ''), ('slip', 'DispatchSlip-v0', '_ex')],
                         ids=['contract1', 'contract2'])
def test_plugin(monkeypatch, plugins, name, env_name, ex):  # noqa: F811
    pl = plugins[name]
    assert pl.CONTRACT == (2 if ex else 1)  # envplug_envs.py's 'line', envplug2_envs.py's 'slip'
    calls = _record(monkeypatch, False, pl)
    tb = TaskBatch(env_name, 2, env_plugin=pl, **TINY)
    assert _reset_and_iterate(tb, calls) == (
        ['pgm_env_ingest_any(-1)'],
        ['pgm_envplug_rollout' + ex] + FUSED + ['pgm_ppo_update_any', 'pgm_envplug_eval' + ex])
    assert tb.update_variant() == 'ppo_update_any_kernel' and not calls
    with pytest.raises(PGMError, match='EnvPlugin.transition evaluates the header on the host'):
        tb.env_step(torch.zeros(2, 2, 1))


# ------------------------------------------------------------------------------------------------ 2. on the device
def _host_case(case):
    P, N, T = 2, 2, 8
    if case == 'cat':
        return TaskBatch(DST, P, num_processes=N, num_steps=T, ppo_epoch=1, num_mini_batch=2,
                         host_env=DeepSeaTreasureHostVecEnv(DST, P, N, max_steps=6))
    return TaskBatch(SYNTH, P, num_processes=N, num_steps=T, ppo_epoch=1, num_mini_batch=2, any_dims=case == 'any',
                     host_env=SynthHostVecEnv(SYNTH, P, N, max_episode_steps=6))


@pytest.mark.gpu
@pytest.mark.parametrize('case,sfx,draw,refusal', [('gauss', '', 'pgm_normal_noise', 'host-env mode'),
                                                   ('cat', '_cat', 'pgm_uniform_noise', 'host-env mode'),
                                                   ('any', '_any', 'pgm_normal_noise', 'runtime-dim kernels')])
def test_host_stepped(gpu, monkeypatch, case, sfx, draw, refusal):
    calls = _record(monkeypatch, True)
    tb = _host_case(case)
    T = tb.T
    assert not calls, 'the constructor launches nothing'
    tb.env_reset()
    ingest = 'pgm_env_ingest_any' if case == 'any' else 'pgm_env_ingest'  # (one ingest kernel for both heads)
    assert _take(calls) == [f'{ingest}(-1)']
    tb.rollout(0)
    want = [draw]
    for t in range(T):
        want += [f'pgm_rollout_act{sfx}({t})', f'{ingest}({t})']
    assert _take(calls) == want + [f'pgm_rollout_act{sfx}({T})']
    steps = []
    real = tb.host_env.eval_step
    monkeypatch.setattr(tb.host_env, 'eval_step', lambda a: (steps.append(1), real(a))[1])
    tb.evaluate()
    torch.cuda.synchronize()
    assert steps and _take(calls) == [f'pgm_eval_act{sfx}'] * len(steps)
    assert np.isfinite(tb.objs.cpu().numpy()).all()
    with pytest.raises(PGMError, match=refusal):
        tb.env_step(torch.zeros(2, 2, 1))
    tb.check_update()


@pytest.mark.gpu
@pytest.mark.parametrize('env,kw,want', [
    (SYNTH, {}, ['pgm_normal_noise', 'pgm_randperm', 'pgm_rollout', 'pgm_gae', 'pgm_adv_normalize', 'pgm_ppo_update',
                 'pgm_ppo_update_reset', 'pgm_eval']),
    (DST, {'device_env': True}, ['pgm_randperm', 'pgm_rollout_dst', 'pgm_gae', 'pgm_adv_normalize',
                                 'pgm_ppo_update_cat', 'pgm_eval_dst'])], ids=['synthmo', 'dst'])
def test_overlapped_iterations(gpu, monkeypatch, env, kw, want):
    calls = _record(monkeypatch, True)
    tb = TaskBatch(env, 2, num_processes=2, num_steps=16, ppo_epoch=1, num_mini_batch=2, **kw)
    tb.weights.fill_(0.5)
    tb.env_reset()
    _take(calls)
    for j in range(2):
        tb.iteration(j, 3e-4, overlap_eval=True)
        assert _take(calls) == want, f'iteration {j}'
    tb.check_update()
    assert np.isfinite(tb.objs.cpu().numpy()).all()
