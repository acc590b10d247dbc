"""MO-Dummy-v0: the fused device rollout and evaluation against the host-stepped path, in one session.

    python scripts/dummy_device_iteration.py [--warmup 3] [--reps 9] [--host-runs 3] [--out profiles/dummy_device_iteration.json]

MO-Dummy-v0 at P = 6 and P = 40 tasks, N = 4 envs, T = 2048 steps, 10 epochs x 32 minibatches, device RNG.  The method
of scripts/dst_device_iteration.py:
  * fused (the default TaskBatch of this env): pgm_rollout_dummy, the update with its variant name, pgm_eval_dummy and
    the whole iteration (TaskBatch.iteration, in-order schedule), HIP-event timing on the launch stream, warm-up runs
    first, then the median and the min-max of the timed ones;
  * host-stepped (TaskBatch(host_env=DummyMOHostVecEnv)): rollout and evaluation by wall time with a final synchronise
    (the path synchronises every step, so events would time the same thing), one warm-up, then ``--host-runs`` runs:
    the fastest and all of them.  Its device half is the existing pgm_rollout_act / pgm_env_ingest / pgm_eval_act;
  * the nearest existing kernel, the block-form Swimmer rollout (rollout_kernel<PlainTowers, 8, 2, 2>,
    PGM_ROLLOUT_KERNEL=block, MO-Swimmer-v2) at the same P in the same session.
Acceptance (asserted): at both P the fused rollout's median is below the host-stepped rollout's fastest run.  No
absolute time is fixed.  DESIGN.md quotes the file.
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
from pgmorl_amd.hostenv import DummyMOHostVecEnv  # noqa: E402
from pgmorl_amd.policy import new_policy  # noqa: E402
from pgmorl_amd.runtime import TaskBatch  # noqa: E402

ENV, SWIMMER, N, T, E, M = 'MO-Dummy-v0', 'MO-Swimmer-v2', 4, 2048, 10, 32


def _batch(env, tasks, **kw):
    spec = envspec.make_spec(env)
    tb = TaskBatch(env, tasks, num_processes=N, num_steps=T, ppo_epoch=E, num_mini_batch=M, **kw)
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


def measure_fused(tasks, warmup, reps):
    tb = _batch(ENV, tasks)
    assert tb.dummy_env
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


def measure_host(tasks, runs):
    tb = _batch(ENV, tasks, host_env=DummyMOHostVecEnv(ENV, tasks, N))
    roll, evl = [], []
    for j in range(1 + runs):  # the first run warms up: first launches, pinned buffers
        r = _wall(lambda: tb.rollout(j, noise=None, carry=j > 0))
        v = _wall(tb.evaluate)
        if j:
            roll.append(r)
            evl.append(v)
    return {'rollout': _summary(roll), 'eval': _summary(evl)}


def measure_swimmer_block(tasks, warmup, reps):
    prev = os.environ.get('PGM_ROLLOUT_KERNEL')
    os.environ['PGM_ROLLOUT_KERNEL'] = 'block'  # (read at every call by _lib.launch_opts)
    try:
        tb = _batch(SWIMMER, tasks)
        ev = [_timed(lambda: tb.rollout(j, noise=None, carry=j > 0)) for j in range(warmup + reps)]
        torch.cuda.synchronize()
    finally:
        if prev is None:
            del os.environ['PGM_ROLLOUT_KERNEL']
        else:
            os.environ['PGM_ROLLOUT_KERNEL'] = prev
    return _summary([s.elapsed_time(e) for s, e in ev[warmup:]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--host-runs', type=int, default=3)
    ap.add_argument('--out', default=os.path.join('profiles', 'dummy_device_iteration.json'))
    a = ap.parse_args()
    res = {'env': ENV, 'N': N, 'T': T, 'ppo_epoch': E, 'num_mini_batch': M, 'rng': 'device',
           'device': torch.cuda.get_device_name(0), 'warmup': a.warmup, 'reps': a.reps, 'host_runs': a.host_runs}
    ok = True
    for tasks in (6, 40):
        f, h = measure_fused(tasks, a.warmup, a.reps), measure_host(tasks, a.host_runs)
        sw = measure_swimmer_block(tasks, a.warmup, a.reps)
        upd = f['update']['median_ms']
        host_it = h['rollout']['min_ms'] + upd + h['eval']['min_ms']
        faster = f['rollout']['median_ms'] < h['rollout']['min_ms']
        ok = ok and faster
        res[f'P{tasks}'] = {
            'fused': f, 'host_stepped': h, 'swimmer_block_rollout': sw,
            'rollout_ratio_host_fastest_over_fused_median': h['rollout']['min_ms'] / f['rollout']['median_ms'],
            'eval_ratio_host_fastest_over_fused_median': h['eval']['min_ms'] / f['eval']['median_ms'],
            'fused_us_per_step': 1e3 * f['rollout']['median_ms'] / T,
            'host_us_per_step': 1e3 * h['rollout']['min_ms'] / T,
            'fused_iteration_ms': f['iteration']['median_ms'], 'host_rollout_update_eval_ms': host_it,
            'rollout_over_swimmer_block': f['rollout']['median_ms'] / sw['median_ms'],
            'fused_rollout_below_host_fastest': faster}
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
                          'update_ms': r['fused']['update']['median_ms'], 'update_kernel': r['fused']['update_kernel'],
                          'swimmer_block_rollout_ms': r['swimmer_block_rollout']['median_ms']}))
    assert ok, 'the fused rollout is not faster than the host-stepped one'


if __name__ == '__main__':
    main()
