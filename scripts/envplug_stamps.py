"""Diagnostic: per-phase cycle shares of the plug-in rollout kernel (plugdummy.hpp, built with -DPGM_STAMPS) beside the
built-in rollout_dummy_kernel's (libpgm_stamps.so), same tasks, same session.

    python -m pgmorl_amd.build --stamps          # libpgm_stamps.so, where the sources are built
    PGM_LIB=pgmorl_amd/libpgm_stamps.so python scripts/envplug_stamps.py [--tasks 40] [--out FILE]

Phases of both kernels (PGM_STAMP ids): 0 loop top + the random draw one step ahead, 1 policy_forward, 2 store_values +
sampling + the env transition + the hand-off barrier, 3 norm_stats, 4 vecnorm_emit.  Cycles are s_memtime ticks of
thread 0's wave of workgroup 1, summed over the timed rollouts.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pgmorl_amd import _lib, build, envspec  # noqa: E402
from pgmorl_amd.envplug import SIGS, EnvPlugin  # noqa: E402
from pgmorl_amd.policy import new_policy  # noqa: E402
from pgmorl_amd.runtime import TaskBatch  # noqa: E402

N, T = 4, 2048
PHASES = ('draw', 'policy_forward', 'sample+transition', 'norm_stats', 'vecnorm_emit')


def _batch(env, tasks, **kw):
    tb = TaskBatch(env, tasks, num_processes=N, num_steps=T, **kw)
    spec = envspec.make_spec(env)
    torch.manual_seed(0)
    for p in range(tasks):
        tb.set_task(p, new_policy(spec['obs_dim'], spec['act_dim'], spec['obj_num']).state_dict(),
                    weights=np.ones(spec['obj_num']) / spec['obj_num'])
    tb.env_reset()
    return tb


def _read(h, name, reset=1):
    buf = (C.c_ulonglong * 64)()
    assert getattr(h, f'pgm_debug_stamps_{name}')(buf, reset) == 0
    return [int(buf[i]) for i in range(len(PHASES))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tasks', type=int, default=40)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    L = _lib.lib()
    assert hasattr(L, 'pgm_debug_stamps_dummy'), 'run with PGM_LIB=pgmorl_amd/libpgm_stamps.so'
    hdr = os.path.join(ROOT, 'tests', 'envplug', 'plugdummy.hpp')
    plugin = EnvPlugin(hdr)
    plugin.lib_path = build.build_env(hdr, stamps=True)
    hs = C.CDLL(plugin.lib_path)
    for name, (res, args) in SIGS.items():
        f = getattr(hs, name)
        f.restype, f.argtypes = res, args
    plugin.h = hs
    tp = _batch(plugin.register('PlugDummy-v0'), a.tasks, env_plugin=plugin)
    td = _batch('MO-Dummy-v0', a.tasks)
    assert hs.pgm_debug_stamp_block_envplug(1) == 0 and L.pgm_debug_stamp_block_dummy(1) == 0
    out = {}
    for j in range(3 + a.reps):
        if j == 3:
            torch.cuda.synchronize()
            _read(hs, 'envplug')
            _read(L, 'dummy')
        tp.rollout(j, noise=None, carry=j > 0)
        td.rollout(j, noise=None, carry=j > 0)
    torch.cuda.synchronize()
    for key, cyc in (('plugin', _read(hs, 'envplug')), ('builtin', _read(L, 'dummy'))):
        tot = sum(cyc)
        out[key] = {'cycles_per_step': {ph: c / (a.reps * T) for ph, c in zip(PHASES, cyc)},
                    'share': {ph: c / tot for ph, c in zip(PHASES, cyc)}, 'total_per_step': tot / (a.reps * T)}
    out['plugin_minus_builtin_cycles_per_step'] = {
        ph: out['plugin']['cycles_per_step'][ph] - out['builtin']['cycles_per_step'][ph] for ph in PHASES}
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, 'w') as fp:
            json.dump(out, fp, indent=1)


if __name__ == '__main__':
    main()
