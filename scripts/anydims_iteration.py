"""What the runtime-dim kernel family (the *_any entry points) costs inside a host-stepped iteration.

    python scripts/anydims_iteration.py [--warmup 3] [--reps 9] [--tasks 6 40] [--out profiles/anydims_iteration.json]

At MO-Walker2d-v2 dims (17/6/2) behind SynthHostVecEnv, N = 4 envs, T = 2048 steps, 10 epochs x 32 minibatches, P = 6
and P = 40 tasks, one session, warm-up iterations first, medians with min-max of the timed ones:

  * the host-stepped iteration (rollout, returns, advantages, update; wall time with a final synchronise) with the
    kernels compiled for 17/6/2 and with the runtime-dim family forced (TaskBatch(any_dims=True));
  * the update alone, HIP events on the launch stream;
  * the split of the rollout per step: act, host step, ingest (TaskBatch.host_profile, one extra rollout).

At 32/8/3 Gaussian (every maximum, no padding), P = 40: the update alone, on synthetic storage.

The claim under test: the runtime-dim update is a small share of a host-stepped iteration.  Nothing here gates;
DESIGN.md quotes the file.
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
from pgmorl_amd.hostenv import HostVecEnv, SynthHostVecEnv  # noqa: E402
from pgmorl_amd.policy import new_policy  # noqa: E402
from pgmorl_amd.runtime import TaskBatch  # noqa: E402

ENV, N, T, E, M = 'MO-Walker2d-v2', 4, 2048, 10, 32


def _stat(xs):
    return {'median': float(np.median(xs)), 'min': float(np.min(xs)), 'max': float(np.max(xs))}


def _fill(tb, spec):
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    for p in range(tb.P):
        pol = new_policy(spec['obs_dim'], spec['act_dim'], spec['obj_num'], discrete=bool(spec.get('discrete')))
        tb.set_task(p, pol.state_dict(), weights=rng.dirichlet(np.ones(spec['obj_num'])))


def measure_iteration(P, any_dims, warmup, reps, steps):
    spec = envspec.make_spec(ENV)
    tb = TaskBatch(ENV, P, num_processes=N, num_steps=steps, ppo_epoch=E, num_mini_batch=M,
                   host_env=SynthHostVecEnv(ENV, P, N), any_dims=any_dims)
    _fill(tb, spec)
    tb.env_reset()
    wall, upd, roll = [], [], []
    for j in range(warmup + reps):
        tb.lr.fill_(3e-4)
        tb._draw_noise(j)
        tb.make_perms(j)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tb.rollout(j, noise=tb.noise, carry=j > 0)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        tb.gae()
        tb.adv_normalize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        tb.ppo_update()
        e.record()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        wall.append(1e3 * (t2 - t0))
        roll.append(1e3 * (t1 - t0))
        upd.append(s.elapsed_time(e))
    tb.check_update()
    assert torch.isfinite(tb.params).all()
    tb.host_profile = {'act': 0.0, 'step': 0.0, 'ingest': 0.0}
    tb.rollout(warmup + reps, noise=tb.noise, carry=True)
    torch.cuda.synchronize()
    split = {k: 1e6 * v / steps for k, v in tb.host_profile.items()}
    w, u = wall[warmup:], upd[warmup:]
    return {'update_kernel': tb.update_variant(), 'iteration_ms': _stat(w), 'rollout_ms': _stat(roll[warmup:]),
            'update_ms': _stat(u), 'update_share': float(np.median(u) / np.median(w)), 'us_per_step': split}


class _NoEnv(HostVecEnv):
    """Dims only: the 32/8/3 update runs on synthetic storage, no env is stepped."""

    def __init__(self, dims, P, n):
        self.obs_dim, self.act_dim, self.obj_num = dims
        self.capacity, self.P, self.N = P, P, n

    def set_active(self, P):
        self.P = P


def measure_update_max(P, warmup, reps, steps):
    dims = (32, 8, 3)
    name = 'AnyMax-32-8-3'
    envspec.register_env(name, *dims)
    spec = envspec.make_spec(name)
    tb = TaskBatch(name, P, num_processes=N, num_steps=steps, ppo_epoch=E, num_mini_batch=M,
                   host_env=_NoEnv(dims, P, N))
    _fill(tb, spec)
    g = torch.Generator(device='cpu').manual_seed(0)
    for buf, scale in ((tb.obs, 1.0), (tb.actions, 1.0), (tb.values, 0.5), (tb.returns, 0.5), (tb.adv, 1.0)):
        buf.copy_(torch.randn(buf.shape, generator=g) * scale)
    tb.logp.fill_(-8.0 * 0.9189385)  # the log-prob of the mean action at logstd 0
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
    assert torch.isfinite(tb.params).all()
    return {'update_kernel': tb.update_variant(), 'update_ms': _stat([s.elapsed_time(e) for s, e in ev[warmup:]])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--tasks', type=int, nargs='+', default=[6, 40])
    ap.add_argument('--steps', type=int, default=T)
    ap.add_argument('--out', default=os.path.join('profiles', 'anydims_iteration.json'))
    a = ap.parse_args()
    res = {'env': ENV, 'N': N, 'T': a.steps, 'ppo_epoch': E, 'num_mini_batch': M, 'rng': 'device',
           'device': torch.cuda.get_device_name(0), 'warmup': a.warmup, 'reps': a.reps, 'walker': {}}
    for P in a.tasks:
        res['walker'][f'P{P}'] = {'compiled': measure_iteration(P, False, a.warmup, a.reps, a.steps),
                                  'any_dims': measure_iteration(P, True, a.warmup, a.reps, a.steps)}
        print(json.dumps({f'P{P}': res['walker'][f'P{P}']}), flush=True)
    res['max_dims_32_8_3'] = {f'P{max(a.tasks)}': measure_update_max(max(a.tasks), a.warmup, a.reps, a.steps)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res['max_dims_32_8_3']))


if __name__ == '__main__':
    main()
