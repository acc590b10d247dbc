"""Per-step cost of the host-stepped rollout (TaskBatch(host_env=...)) beside the fused rollout and the PPO update.

    python scripts/hostenv_step.py [--warmup 3] [--reps 9] [--out profiles/hostenv_step.json]

MO-Walker2d-v2, N = 4 envs, T = 2048 steps, 10 epochs x 32 minibatches, device RNG, P = 6 tasks (the reference
scripts' --num-tasks 6) and P = 40, environments = SynthHostVecEnv (SynthMO in numpy: a cheap host env, so what is
measured is the seam, not a physics engine).  Warm-up iterations first, medians of the timed ones.  Per P:
  * the host-stepped rollout's wall time per step, and its split (timed in iterations of their own, with one extra
    synchronise after the ingest so that the third part is complete):
      act     pgm_rollout_act launch + pinned D2H of the actions + the stream synchronise
      step    host_env.step
      ingest  packing + pinned H2D of the transition + pgm_env_ingest
  * from the same batch shape on the device envs: the fused pgm_rollout per step and the PPO update (HIP events).
Nothing here gates; DESIGN.md quotes the file.
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
from pgmorl_amd.hostenv import SynthHostVecEnv  # noqa: E402
from pgmorl_amd.policy import new_policy  # noqa: E402
from pgmorl_amd.runtime import TaskBatch  # noqa: E402

ENV, N, T, E, M = 'MO-Walker2d-v2', 4, 2048, 10, 32


def _batch(P, host):
    spec = envspec.make_spec(ENV)
    he = SynthHostVecEnv(ENV, P, N, seed=0) if host else None
    tb = TaskBatch(ENV, P, num_processes=N, num_steps=T, ppo_epoch=E, num_mini_batch=M, host_env=he)
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    for p in range(P):
        pol = new_policy(spec['obs_dim'], spec['act_dim'], spec['obj_num'])
        tb.set_task(p, pol.state_dict(), weights=rng.dirichlet(np.ones(spec['obj_num'])))
    tb.env_reset()
    return tb


def _update(tb, j):
    tb.lr.fill_(3e-4)
    tb.gae()
    tb.adv_normalize()
    tb.make_perms(j)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    tb.ppo_update()
    e.record()
    return s, e


def measure_host(P, warmup, reps):
    tb = _batch(P, True)
    wall, split = [], []
    for j in range(warmup + 2 * reps):
        profiled = j >= warmup + reps
        tb.host_profile = {'act': 0.0, 'step': 0.0, 'ingest': 0.0} if profiled else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tb.rollout(j, noise=None, carry=j > 0)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if profiled:
            split.append({k: v / T * 1e6 for k, v in tb.host_profile.items()})
        elif j >= warmup:
            wall.append(dt / T * 1e6)
        _update(tb, j)
    torch.cuda.synchronize()
    tb.check_update()
    assert torch.isfinite(tb.params).all()
    out = {'rollout_us_per_step': float(np.median(wall)), 'rollout_us_per_step_all': wall}
    for k in ('act', 'step', 'ingest'):
        out[f'{k}_us_per_step'] = float(np.median([s[k] for s in split]))
    return out


def measure_fused(P, warmup, reps):
    tb = _batch(P, False)
    ev = []
    for j in range(warmup + reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        tb.rollout(j, noise=None, carry=j > 0)
        e.record()
        ev.append(((s, e), _update(tb, j)))
    torch.cuda.synchronize()
    tb.check_update()
    roll = [s.elapsed_time(e) for (s, e), _ in ev[warmup:]]
    upd = [s.elapsed_time(e) for _, (s, e) in ev[warmup:]]
    return {'fused_rollout_us_per_step': float(np.median(roll)) / T * 1e3, 'fused_rollout_ms': float(np.median(roll)),
            'update_ms': float(np.median(upd)), 'update_kernel': tb.update_variant()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--tasks', type=int, nargs='+', default=[6, 40])
    ap.add_argument('--out', default=os.path.join('profiles', 'hostenv_step.json'))
    a = ap.parse_args()
    res = {'env': ENV, 'N': N, 'T': T, 'ppo_epoch': E, 'num_mini_batch': M, 'rng': 'device', 'host_env': 'synth',
           'device': torch.cuda.get_device_name(0), 'warmup': a.warmup, 'reps': a.reps, 'tasks': {}}
    for P in a.tasks:
        r = measure_host(P, a.warmup, a.reps)
        r.update(measure_fused(P, a.warmup, a.reps))
        r['host_rollout_ms'] = r['rollout_us_per_step'] * T / 1e3
        res['tasks'][str(P)] = r
        print(json.dumps({'P': P, **{k: v for k, v in r.items() if not k.endswith('_all')}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
