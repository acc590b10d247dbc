"""Device env plug-ins: the fused rollout and evaluation of a plug-in library against the host-stepped path of the same
compiled header, in one session.

    python scripts/envplug_iteration.py [--warmup 3] [--reps 9] [--host-runs 3] [--out profiles/envplug_iteration.json]

tests/envplug/line.hpp (Gaussian, 5/1/2) and tests/envplug/chain.hpp (Categorical, 2/3/3) at P = 6 and P = 40 tasks,
N = 4 envs, T = 2048 steps, 10 epochs x 32 minibatches, device RNG.  The protocol of scripts/dummy_device_iteration.py:
  * fused (TaskBatch(env_plugin=...)): pgm_envplug_rollout, the runtime-dim update (pgm_ppo_update_any),
    pgm_envplug_eval and the whole iteration (TaskBatch.iteration, in-order schedule), HIP-event timing on the launch
    stream, warm-up runs first, then the median and the min-max of the timed ones;
  * host-stepped (TaskBatch(host_env=PluginHostVecEnv(plugin))): rollout and evaluation by wall time with a final
    synchronise, one warm-up, then ``--host-runs`` runs: the fastest and all of them;
  * the same env in both forms: tests/envplug/plugdummy.hpp against the built-in MO-Dummy-v0 (pgm_rollout_dummy /
    pgm_eval_dummy) at the same P in the same session, interleaved.  How far the plug-in form lies from the built-in
    one is reported, not fixed in advance; ``plugin_slower_than_spread`` says whether the plug-in's median is more
    than the session's own min-max spread (the larger of the two kernels') above the built-in's.
Acceptance (asserted): at both P, for both headers, the fused rollout's median is below the host-stepped rollout's
fastest run.  No absolute time is fixed.  DESIGN.md quotes the file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pgmorl_amd import envspec  # noqa: E402
from pgmorl_amd.envplug import EnvPlugin  # noqa: E402
from pgmorl_amd.hostenv import PluginHostVecEnv  # noqa: E402
from pgmorl_amd.policy import new_policy  # noqa: E402
from pgmorl_amd.runtime import TaskBatch  # noqa: E402

N, T, E, M = 4, 2048, 10, 32
HEADERS = {'line': 'Line-v0', 'chain': 'Chain-v0'}


def _header(name):
    return os.path.join(ROOT, 'tests', 'envplug', name + '.hpp')


def _batch(env, tasks, **kw):
    tb = TaskBatch(env, tasks, num_processes=N, num_steps=T, ppo_epoch=E, num_mini_batch=M, **kw)
    spec = envspec.make_spec(env)
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    for p in range(tasks):
        pol = new_policy(spec['obs_dim'], spec['act_dim'], spec['obj_num'], discrete=bool(spec.get('discrete')))
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


def measure_fused(env, plugin, tasks, warmup, reps):
    tb = _batch(env, tasks, env_plugin=plugin)
    assert tb.plugin is plugin and tb.host_env is None
    ev = []
    for j in range(warmup + reps):
        tb.lr.fill_(3e-4)
        r = _timed(lambda: tb.rollout(j, noise=None, carry=j > 0))
        tb.gae()
        tb.adv_normalize()
        tb.make_perms(j)
        u = _timed(tb.ppo_update)
        v = _timed(tb.evaluate)
        ev.append((r, u, v))
    torch.cuda.synchronize()
    its = [_timed(lambda: tb.iteration(warmup + reps + j, 3e-4, carry=True)) for j in range(warmup + reps)]
    torch.cuda.synchronize()
    tb.check_update()
    assert torch.isfinite(tb.params).all() and torch.isfinite(tb.objs).all()
    cols = [[s.elapsed_time(e) for s, e in (x[i] for x in ev[warmup:])] for i in range(3)]
    return {'rollout': _summary(cols[0]), 'update': _summary(cols[1]), 'eval': _summary(cols[2]),
            'iteration': _summary([s.elapsed_time(e) for s, e in its[warmup:]]), 'update_kernel': tb.update_variant(),
            'episodes_per_env_last_rollouts': float(tb.episode.double().mean())}


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def measure_host(env, plugin, tasks, runs):
    tb = _batch(env, tasks, host_env=PluginHostVecEnv(plugin, tasks, N))
    roll, evl = [], []
    for j in range(1 + runs):  # the first run warms up: first launches, pinned buffers
        r = _wall(lambda: tb.rollout(j, noise=None, carry=j > 0))
        v = _wall(tb.evaluate)
        if j:
            roll.append(r)
            evl.append(v)
    return {'rollout': _summary(roll), 'eval': _summary(evl)}


def measure_dummy_pair(plugin, tasks, warmup, reps):
    """plugdummy.hpp and the built-in MO-Dummy-v0, rollout and evaluation interleaved in one session."""
    tp = _batch(plugin.register('PlugDummy-v0'), tasks, env_plugin=plugin)
    td = _batch('MO-Dummy-v0', tasks)
    ev = []
    for j in range(warmup + reps):
        ev.append((_timed(lambda: tp.rollout(j, noise=None, carry=j > 0)),
                   _timed(lambda: td.rollout(j, noise=None, carry=j > 0)),
                   _timed(tp.evaluate), _timed(td.evaluate)))
    torch.cuda.synchronize()
    cols = [_summary([s.elapsed_time(e) for s, e in (x[i] for x in ev[warmup:])]) for i in range(4)]
    spread = max(cols[0]['max_ms'] - cols[0]['min_ms'], cols[1]['max_ms'] - cols[1]['min_ms'])
    return {'plugin_rollout': cols[0], 'builtin_rollout': cols[1], 'plugin_eval': cols[2], 'builtin_eval': cols[3],
            'rollout_plugin_over_builtin': cols[0]['median_ms'] / cols[1]['median_ms'],
            'session_spread_ms': spread,
            'plugin_slower_than_spread': cols[0]['median_ms'] - cols[1]['median_ms'] > spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--host-runs', type=int, default=3)
    ap.add_argument('--out', default=os.path.join('profiles', 'envplug_iteration.json'))
    a = ap.parse_args()
    res = {'N': N, 'T': T, 'ppo_epoch': E, 'num_mini_batch': M, 'rng': 'device',
           'device': torch.cuda.get_device_name(0), 'warmup': a.warmup, 'reps': a.reps, 'host_runs': a.host_runs}
    ok = True
    lines = []
    for name, env in HEADERS.items():
        plugin = EnvPlugin(_header(name))
        plugin.register(env)
        for tasks in (6, 40):
            f = measure_fused(env, plugin, tasks, a.warmup, a.reps)
            h = measure_host(env, plugin, tasks, a.host_runs)
            faster = f['rollout']['median_ms'] < h['rollout']['min_ms']
            ok = ok and faster
            r = {'fused': f, 'host_stepped': h,
                 'rollout_ratio_host_fastest_over_fused_median': h['rollout']['min_ms'] / f['rollout']['median_ms'],
                 'eval_ratio_host_fastest_over_fused_median': h['eval']['min_ms'] / f['eval']['median_ms'],
                 'fused_us_per_step': 1e3 * f['rollout']['median_ms'] / T,
                 'host_us_per_step': 1e3 * h['rollout']['min_ms'] / T,
                 'fused_iteration_ms': f['iteration']['median_ms'],
                 'host_rollout_update_eval_ms': h['rollout']['min_ms'] + f['update']['median_ms'] + h['eval']['min_ms'],
                 'fused_rollout_below_host_fastest': faster}
            res[f'{name}_P{tasks}'] = r
            lines.append({'header': name, 'P': tasks, **{k: v for k, v in r.items() if not isinstance(v, dict)},
                          'fused_rollout_ms': f['rollout']['median_ms'], 'host_rollout_ms': h['rollout']['min_ms'],
                          'fused_eval_ms': f['eval']['median_ms'], 'host_eval_ms': h['eval']['min_ms'],
                          'update_ms': f['update']['median_ms'], 'update_kernel': f['update_kernel']})
    dummy = EnvPlugin(_header('plugdummy'))
    for tasks in (6, 40):
        d = measure_dummy_pair(dummy, tasks, a.warmup, a.reps)
        res[f'plugdummy_vs_builtin_P{tasks}'] = d
        lines.append({'pair': 'plugdummy vs MO-Dummy-v0', 'P': tasks, 'plugin_rollout_ms': d['plugin_rollout']['median_ms'],
                      'builtin_rollout_ms': d['builtin_rollout']['median_ms'],
                      'plugin_eval_ms': d['plugin_eval']['median_ms'], 'builtin_eval_ms': d['builtin_eval']['median_ms'],
                      **{k: v for k, v in d.items() if not isinstance(v, dict)}})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(res, fp, indent=1)
    for ln in lines:
        print(json.dumps(ln))
    assert ok, 'a fused plug-in rollout is not faster than the host-stepped one'


if __name__ == '__main__':
    main()
