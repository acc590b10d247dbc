"""Deep Sea Treasure: the fused device rollout and evaluation against the host-stepped path, in one session.

    python scripts/dst_device_iteration.py [--warmup 3] [--reps 9] [--host-runs 3] [--out profiles/dst_device_iteration.json]

MO-DeepSeaTreasure-v0 at P = 6 and P = 40 tasks, N = 4 envs, T = 2048 steps, 10 epochs x 32 minibatches, device RNG.
  * fused (TaskBatch(device_env=True)): pgm_rollout_dst and pgm_eval_dst, HIP-event timing on the launch stream,
    warm-up runs first, then the median and the min-max of the timed ones;
  * host-stepped (TaskBatch(host_env=DeepSeaTreasureHostVecEnv)): rollout and evaluation by wall time with a final
    synchronise (the path synchronises every step, so events would time the same thing), one warm-up, then
    ``--host-runs`` runs: the fastest and all of them;
  * the update (ppo_update_cat_kernel; the same kernel on both paths), HIP events;
  * for scale, the block-form LayerNorm rollout (rollout_kernel<LNTowers>, MO-Walker2d-v2, P = 40) in the same session.
Acceptance (asserted): at both P the fused rollout's median is below the host-stepped rollout's fastest run.  The file
also records the ratio, the per-step time and the resulting iteration time (rollout + update + evaluation; the
returns / advantage kernels are common to both paths and left out).  DESIGN.md quotes the file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pgmorl_amd import envspec  # noqa: E402
from pgmorl_amd.hostenv import DeepSeaTreasureHostVecEnv  # noqa: E402
from pgmorl_amd.policy import new_policy  # noqa: E402
from pgmorl_amd.runtime import TaskBatch  # noqa: E402

ENV, LN_ENV, N, T, E, M = 'MO-DeepSeaTreasure-v0', 'MO-Walker2d-v2', 4, 2048, 10, 32


def _batch(env, tasks, **kw):
    spec = envspec.make_spec(env)
    tb = TaskBatch(env, tasks, num_processes=N, num_steps=T, ppo_epoch=E, num_mini_batch=M, **kw)
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    for p in range(tasks):
        pol = new_policy(spec['obs_dim'], spec['act_dim'], spec['obj_num'], discrete=bool(spec.get('discrete')),
                         layernorm=bool(kw.get('layernorm')))
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


def measure_fused(tasks, warmup, reps):
    tb = _batch(ENV, tasks, device_env=True)
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
    tb.check_update()
    assert torch.isfinite(tb.params).all() and torch.isfinite(tb.objs).all()
    cols = [[s.elapsed_time(e) for s, e in (x[i] for x in ev[warmup:])] for i in range(3)]
    return {'rollout': _summary(cols[0]), 'update': _summary(cols[1]), 'eval': _summary(cols[2]),
            'update_kernel': tb.update_variant()}


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def measure_host(tasks, runs):
    tb = _batch(ENV, tasks, host_env=DeepSeaTreasureHostVecEnv(ENV, tasks, N))
    roll, evl = [], []
    for j in range(1 + runs):  # the first run warms up: first launches, pinned buffers
        r = _wall(lambda: tb.rollout(j, noise=None, carry=j > 0))
        v = _wall(tb.evaluate)
        if j:
            roll.append(r)
            evl.append(v)
    return {'rollout': _summary(roll), 'eval': _summary(evl)}


def measure_ln_block(warmup, reps):
    tb = _batch(LN_ENV, 40, layernorm=True)
    ev = [_timed(lambda: tb.rollout(j, noise=None, carry=j > 0)) for j in range(warmup + reps)]
    torch.cuda.synchronize()
    return _summary([s.elapsed_time(e) for s, e in ev[warmup:]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--host-runs', type=int, default=3)
    ap.add_argument('--out', default=os.path.join('profiles', 'dst_device_iteration.json'))
    a = ap.parse_args()
    res = {'env': ENV, 'N': N, 'T': T, 'ppo_epoch': E, 'num_mini_batch': M, 'rng': 'device',
           'device': torch.cuda.get_device_name(0), 'warmup': a.warmup, 'reps': a.reps, 'host_runs': a.host_runs}
    ok = True
    for tasks in (6, 40):
        f, h = measure_fused(tasks, a.warmup, a.reps), measure_host(tasks, a.host_runs)
        upd = f['update']['median_ms']
        fused_it = f['rollout']['median_ms'] + upd + f['eval']['median_ms']
        host_it = h['rollout']['min_ms'] + upd + h['eval']['min_ms']
        faster = f['rollout']['median_ms'] < h['rollout']['min_ms']
        ok = ok and faster
        res[f'P{tasks}'] = {
            'fused': f, 'host_stepped': h,
            'rollout_ratio_host_fastest_over_fused_median': h['rollout']['min_ms'] / f['rollout']['median_ms'],
            'eval_ratio_host_fastest_over_fused_median': h['eval']['min_ms'] / f['eval']['median_ms'],
            'fused_us_per_step': 1e3 * f['rollout']['median_ms'] / T,
            'host_us_per_step': 1e3 * h['rollout']['min_ms'] / T,
            'fused_iteration_ms': fused_it, 'host_iteration_ms': host_it, 'iteration_ratio': host_it / fused_it,
            'fused_rollout_below_host_fastest': faster}
    res['ln_block_rollout_walker_P40'] = measure_ln_block(a.warmup, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        json.dump(res, fp, indent=1)
    for tasks in (6, 40):
        r = res[f'P{tasks}']
        print(json.dumps({'P': tasks, **{k: v for k, v in r.items() if not isinstance(v, dict)},
                          'fused_rollout_ms': r['fused']['rollout']['median_ms'],
                          'host_rollout_ms': r['host_stepped']['rollout']['min_ms'],
                          'fused_eval_ms': r['fused']['eval']['median_ms'],
                          'host_eval_ms': r['host_stepped']['eval']['min_ms'],
                          'update_ms': r['fused']['update']['median_ms']}))
    print(json.dumps({'ln_block_rollout_walker_P40': {k: v for k, v in res['ln_block_rollout_walker_P40'].items()
                                                      if k != 'all_ms'}}))
    assert ok, 'the fused rollout is not faster than the host-stepped one'


if __name__ == '__main__':
    main()
