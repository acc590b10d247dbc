"""Contract 2 of the device env plug-ins: what it costs in the fused rollout, in one session.

    python scripts/envplug2_rollout.py [--parent-lib PATH] [--warmup 3] [--reps 9] [--out profiles/envplug2_rollout.json]

N = 4 envs, T = 2048 steps, device RNG, P = 6 and 40 tasks, HIP-event timing on the launch stream, warm-up runs first,
then the median and the min-max of the timed ones (the protocol of scripts/envplug_iteration.py).
  * ``--parent-lib``: a plug-in library of tests/envplug/plugdummy.hpp built from the parent commit's csrc/ and
    include/ (build.py's flags).  Its pgm_envplug_rollout and this tree's, on two batches with the same policies,
    interleaved: a contract-1 header is meant to cost what it cost (DESIGN.md 28 tables equal register counts).
    ``branch_outside_parent_spread`` says whether the medians differ by more than the parent's own min-max spread.
  * tests/envplug2/plugdummy2.hpp (plugdummy.hpp under CONTRACT = 2: NP 2, NW 1, the word scaling a small
    disturbance of the action) against plugdummy.hpp, interleaved: the parameters, the hash of one word per
    (step, env) drawn a step ahead, and the ctx.  The difference is reported as measured; ``exceeds_session_spread``
    says whether it is more than the larger min-max spread of the two.
Nothing is asserted but finiteness.  DESIGN.md quotes the file.
"""
import argparse
import copy
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pgmorl_amd import envplug, envspec  # noqa: E402
from pgmorl_amd.envplug import EnvPlugin  # noqa: E402
from pgmorl_amd.policy import new_policy  # noqa: E402
from pgmorl_amd.runtime import TaskBatch  # noqa: E402

N, T = 4, 2048


def _batch(env, tasks, **kw):
    tb = TaskBatch(env, tasks, num_processes=N, num_steps=T, **kw)
    spec = envspec.make_spec(env)
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    for p in range(tasks):
        pol = new_policy(spec['obs_dim'], spec['act_dim'], spec['obj_num'])
        tb.set_task(p, pol.state_dict(), weights=rng.dirichlet(np.ones(spec['obj_num'])))
    tb.env_reset()
    return tb


def _timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    return s, e


def _summary(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms)), 'all_ms': list(ms)}


def _pair(ta, tb, warmup, reps):
    """Rollouts of two batches interleaved -> their summaries."""
    ev = []
    for j in range(warmup + reps):
        ev.append((_timed(lambda: ta.rollout(j, noise=None, carry=j > 0)),
                   _timed(lambda: tb.rollout(j, noise=None, carry=j > 0))))
    torch.cuda.synchronize()
    assert torch.isfinite(ta.rewards).all() and torch.isfinite(tb.rewards).all()
    return [_summary([s.elapsed_time(e) for s, e in (x[i] for x in ev[warmup:])]) for i in range(2)]


def parent_plugin(plugin, path):
    """The same header's library built from the parent commit: the contract-1 entry points alone."""
    old = copy.copy(plugin)
    old.lib_path = os.path.abspath(path)
    old.h = h = C.CDLL(old.lib_path)
    for name in ('pgm_envplug_last_error', 'pgm_envplug_rollout', 'pgm_envplug_eval', 'pgm_envplug_transition',
                 'pgm_envplug_reset'):
        f = getattr(h, name)
        f.restype, f.argtypes = envplug.SIGS[name]
    assert not hasattr(h, 'pgm_envplug_rollout_ex'), 'the parent library has no _ex entry point'
    return old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=os.path.join('profiles', 'envplug2_rollout.json'))
    a = ap.parse_args()
    res = {'N': N, 'T': T, 'rng': 'device', 'device': torch.cuda.get_device_name(0), 'warmup': a.warmup, 'reps': a.reps}
    lines = []
    one = EnvPlugin(os.path.join(ROOT, 'tests', 'envplug', 'plugdummy.hpp'))
    two = EnvPlugin(os.path.join(ROOT, 'tests', 'envplug2', 'plugdummy2.hpp'))
    one.register('PlugDummy-v0')
    two.register('PlugDummy2-v0')
    assert (one.CONTRACT, two.CONTRACT, two.NP, two.NW) == (1, 2, 2, 1)
    for tasks in (6, 40):
        if a.parent_lib:
            old = parent_plugin(one, a.parent_lib)
            parent, branch = _pair(_batch('PlugDummy-v0', tasks, env_plugin=old),
                                   _batch('PlugDummy-v0', tasks, env_plugin=one), a.warmup, a.reps)
            spread = parent['max_ms'] - parent['min_ms']
            d = {'parent_rollout': parent, 'branch_rollout': branch, 'parent_spread_ms': spread,
                 'branch_minus_parent_ms': branch['median_ms'] - parent['median_ms'],
                 'branch_outside_parent_spread': abs(branch['median_ms'] - parent['median_ms']) > spread}
            res[f'plugdummy_parent_vs_branch_P{tasks}'] = d
            lines.append({'pair': 'plugdummy.hpp parent vs branch', 'P': tasks, 'parent_ms': parent['median_ms'],
                          'branch_ms': branch['median_ms'], **{k: v for k, v in d.items() if not isinstance(v, dict)}})
        c1, c2 = _pair(_batch('PlugDummy-v0', tasks, env_plugin=one),
                       _batch('PlugDummy2-v0', tasks, env_plugin=two, env_params={'gust': 0.01, 'lift': 0.001}),
                       a.warmup, a.reps)
        spread = max(c1['max_ms'] - c1['min_ms'], c2['max_ms'] - c2['min_ms'])
        d = {'contract1_rollout': c1, 'contract2_rollout': c2, 'session_spread_ms': spread,
             'contract2_minus_contract1_ms': c2['median_ms'] - c1['median_ms'],
             'contract2_over_contract1': c2['median_ms'] / c1['median_ms'],
             'contract2_minus_contract1_ns_per_step': 1e6 * (c2['median_ms'] - c1['median_ms']) / T,
             'exceeds_session_spread': c2['median_ms'] - c1['median_ms'] > spread}
        res[f'plugdummy2_vs_plugdummy_P{tasks}'] = d
        lines.append({'pair': 'plugdummy2.hpp (contract 2) vs plugdummy.hpp', 'P': tasks,
                      'contract1_ms': c1['median_ms'], 'contract2_ms': c2['median_ms'],
                      **{k: v for k, v in d.items() if not isinstance(v, dict)}})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(res, fp, indent=1)
    for ln in lines:
        print(json.dumps(ln))


if __name__ == '__main__':
    main()
