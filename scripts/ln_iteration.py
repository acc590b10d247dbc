"""Rollout and PPO-update time of the LayerNorm towers against the plain ones on the headline shape.

    python scripts/ln_iteration.py [--warmup 3] [--reps 9] [--out profiles/ln_iteration.json]

MO-Walker2d-v2, P = 40 tasks, N = 4 envs, T = 2048 steps, 10 epochs x 32 minibatches, device RNG.  HIP-event timing
on the launch stream, warm-up iterations first, medians of the timed ones.  Four numbers:
  * the rollout with layernorm=False (lane kernel) and layernorm=True (rollout_ln_kernel);
  * the update with layernorm=False forced to the comparable split, one workgroup per tower
    (PGM_UPDATE_KERNEL=mfma PGM_UPDATE_SPLIT=1), and with layernorm=True (ppo_update_ln_kernel);
and the two LayerNorm / plain ratios.  Nothing here gates; DESIGN.md quotes the file.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pgmorl_amd import envspec  # noqa: E402
from pgmorl_amd.policy import new_policy  # noqa: E402
from pgmorl_amd.runtime import TaskBatch  # noqa: E402

ENV, P, N, T, E, M = 'MO-Walker2d-v2', 40, 4, 2048, 10, 32
PLAIN_OPTS = {'PGM_UPDATE_KERNEL': 'mfma', 'PGM_UPDATE_SPLIT': '1'}


def _timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    return s, e


def measure(layernorm, warmup, reps):
    spec = envspec.make_spec(ENV)
    tb = TaskBatch(ENV, P, num_processes=N, num_steps=T, ppo_epoch=E, num_mini_batch=M, layernorm=layernorm)
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    for p in range(P):
        pol = new_policy(spec['obs_dim'], spec['act_dim'], spec['obj_num'], layernorm=layernorm)
        w = rng.dirichlet(np.ones(spec['obj_num']))
        tb.set_task(p, pol.state_dict(), weights=w)
    tb.env_reset()
    if not layernorm:
        os.environ.update(PLAIN_OPTS)
    try:
        variant = tb.update_variant()
        ev = []
        for j in range(warmup + reps):
            tb.lr.fill_(3e-4)
            r = _timed(lambda: tb.rollout(j, noise=None, carry=j > 0))
            tb.gae()
            tb.adv_normalize()
            tb.make_perms(j)
            u = _timed(tb.ppo_update)
            ev.append((r, u))
        torch.cuda.synchronize()
        tb.check_update()
    finally:
        for k in PLAIN_OPTS:
            os.environ.pop(k, None)
    roll = [s.elapsed_time(e) for (s, e), _ in ev[warmup:]]
    upd = [s.elapsed_time(e) for _, (s, e) in ev[warmup:]]
    assert torch.isfinite(tb.params).all()
    return {'rollout_ms': float(np.median(roll)), 'update_ms': float(np.median(upd)), 'update_kernel': variant,
            'rollout_ms_all': roll, 'update_ms_all': upd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=os.path.join('profiles', 'ln_iteration.json'))
    a = ap.parse_args()
    plain = measure(False, a.warmup, a.reps)
    ln = measure(True, a.warmup, a.reps)
    res = {'env': ENV, 'P': P, 'N': N, 'T': T, 'ppo_epoch': E, 'num_mini_batch': M, 'rng': 'device',
           'device': torch.cuda.get_device_name(0), 'warmup': a.warmup, 'reps': a.reps,
           'rollout_plain_ms': plain['rollout_ms'], 'rollout_ln_ms': ln['rollout_ms'],
           'update_plain_ms': plain['update_ms'], 'update_ln_ms': ln['update_ms'],
           'rollout_ratio': ln['rollout_ms'] / plain['rollout_ms'],
           'update_ratio': ln['update_ms'] / plain['update_ms'],
           'update_plain_kernel': plain['update_kernel'], 'update_ln_kernel': ln['update_kernel'],
           'samples': {'plain': plain, 'layernorm': ln}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != 'samples'}))


if __name__ == '__main__':
    main()
