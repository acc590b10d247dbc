"""PPO-update time of the Categorical-head kernel against the nearest plain one, and the per-step cost of the
host-env seam with a discrete-action env.

    python scripts/cat_iteration.py [--warmup 3] [--reps 9] [--out profiles/cat_iteration.json]

Update: MO-DeepSeaTreasure-v0 (3/4/2, ppo_update_cat_kernel) against MO-Swimmer-v2 (8/2/2) forced to the comparable
split, one workgroup per tower (PGM_UPDATE_KERNEL=mfma PGM_UPDATE_SPLIT=1: ppo_update_mfma_kernel MODE 1), both at
P = 40 tasks, N = 4 envs, T = 2048 steps, 10 epochs x 32 minibatches.  Swimmer has the nearest dims (9,472 against
8,960 multiply-adds per row) and the same one-workgroup-per-tower structure.  HIP-event timing on the launch stream,
warm-up iterations first, medians of the timed ones; each update runs on the storage of one rollout of its own env.
Seam: one T = 512 rollout at P = 6 and P = 40 with TaskBatch.host_profile, i.e. the host-side time per step of
pgm_rollout_act_cat + the action copy (act), DeepSeaTreasureHostVecEnv.step (step) and the transition copy +
pgm_env_ingest (ingest).  Nothing here gates; DESIGN.md quotes the file.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pgmorl_amd import envspec  # noqa: E402
from pgmorl_amd.hostenv import DeepSeaTreasureHostVecEnv  # noqa: E402
from pgmorl_amd.policy import new_policy  # noqa: E402
from pgmorl_amd.runtime import TaskBatch  # noqa: E402

CAT_ENV, PLAIN_ENV, P, N, T, E, M = 'MO-DeepSeaTreasure-v0', 'MO-Swimmer-v2', 40, 4, 2048, 10, 32
PLAIN_OPTS = {'PGM_UPDATE_KERNEL': 'mfma', 'PGM_UPDATE_SPLIT': '1'}


def _batch(env, tasks, steps, **kw):
    spec = envspec.make_spec(env)
    disc = bool(spec.get('discrete', False))
    he = DeepSeaTreasureHostVecEnv(env, tasks, N) if disc else None
    tb = TaskBatch(env, tasks, num_processes=N, num_steps=steps, ppo_epoch=E, num_mini_batch=M, host_env=he, **kw)
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    for p in range(tasks):
        pol = new_policy(spec['obs_dim'], spec['act_dim'], spec['obj_num'], discrete=disc)
        tb.set_task(p, pol.state_dict(), weights=rng.dirichlet(np.ones(spec['obj_num'])))
    tb.env_reset()
    return tb


def measure_update(env, warmup, reps):
    tb = _batch(env, P, T)
    plain = not tb.discrete
    if plain:
        os.environ.update(PLAIN_OPTS)
    try:
        variant = tb.update_variant()
        tb.rollout(0, noise=None, carry=False)
        tb.gae()
        tb.adv_normalize()
        ev = []
        for j in range(warmup + reps):
            tb.lr.fill_(3e-4)
            tb.make_perms(j)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            tb.ppo_update()
            e.record()
            ev.append((s, e))
        torch.cuda.synchronize()
        tb.check_update()
    finally:
        for k in PLAIN_OPTS:
            os.environ.pop(k, None)
    ms = [s.elapsed_time(e) for s, e in ev[warmup:]]
    assert torch.isfinite(tb.params).all()
    return {'update_ms': float(np.median(ms)), 'update_kernel': variant, 'update_ms_all': ms}


def measure_seam(tasks, steps=512):
    tb = _batch(CAT_ENV, tasks, steps)
    tb.rollout(0, noise=None, carry=False)  # warm-up: first launches, pinned buffers
    tb.host_profile = {'act': 0.0, 'step': 0.0, 'ingest': 0.0}
    tb.rollout(1, noise=None, carry=True)
    torch.cuda.synchronize()
    return {k: 1e6 * v / steps for k, v in tb.host_profile.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=os.path.join('profiles', 'cat_iteration.json'))
    a = ap.parse_args()
    cat = measure_update(CAT_ENV, a.warmup, a.reps)
    plain = measure_update(PLAIN_ENV, a.warmup, a.reps)
    res = {'P': P, 'N': N, 'T': T, 'ppo_epoch': E, 'num_mini_batch': M, 'rng': 'device',
           'device': torch.cuda.get_device_name(0), 'warmup': a.warmup, 'reps': a.reps,
           'update_cat_env': CAT_ENV, 'update_plain_env': PLAIN_ENV,
           'update_cat_ms': cat['update_ms'], 'update_plain_ms': plain['update_ms'],
           'update_ratio': cat['update_ms'] / plain['update_ms'],
           'update_cat_kernel': cat['update_kernel'], 'update_plain_kernel': plain['update_kernel'],
           'seam_us_per_step': {f'P{p}': measure_seam(p) for p in (6, 40)},
           'samples': {'cat': cat, 'plain': plain}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != 'samples'}))


if __name__ == '__main__':
    main()
