"""Bit-for-bit comparison of the one-workgroup-per-task policy kernels between two builds of libpgm.so.

    python scripts/policy_refactor_equal.py --parent /path/to/parent/libpgm.so \
        [--out profiles/policy_refactor_equal.json]

The same seeded inputs go through both libraries (the parent's from --parent, this tree's from pgmorl_amd/):
  * pgm_act_forward sampled and deterministic -- plain towers on 8/2/2, 11/3/2, 11/3/3, 17/6/2, 27/8/2 and 376/17/2,
    LayerNorm towers on the five small ones, pgm_act_forward_cat on 3/4/2 -- at P = 3, N in {1, 3, 8};
  * block-form pgm_rollout (carry 0 then 1, explicit noise and the counter stream, a time limit that resets inside T)
    and pgm_eval (eval_num 1 / 3, raw 0 / 1, episodes cut to 12 steps): every storage array, the env state and the
    running statistics -- plain and LayerNorm on 11/3/2, 11/3/3 and 17/6/2, plain on 376/17/2;
  * pgm_env_ingest(-1, 0), pgm_rollout_act(0, T - 1, T) and pgm_eval_act (E 1 / 8, use_ob 0 / 1) for plain
    (17/6/2, 11/3/3), LayerNorm (11/3/2, 11/3/3) and Categorical policies at N in {1, 3, 8}.
Prints and writes the array count and max |d|; exits 1 unless every array is identical.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pgmorl_amd import _lib, envspec  # noqa: E402
from pgmorl_amd._lib import Dims  # noqa: E402
from pgmorl_amd.hostenv import DeepSeaTreasureHostVecEnv, SynthHostVecEnv  # noqa: E402
from pgmorl_amd.policy import new_policy  # noqa: E402
from pgmorl_amd.runtime import TaskBatch  # noqa: E402

P = 3
# 8/2/2, 11/3/2, 11/3/3 (the one dim set with three objectives), 17/6/2, 27/8/2, 376/17/2 (streamed layer 1)
PLAIN = ['MO-Swimmer-v2', 'MO-Hopper-v2', 'MO-Hopper-v3', 'MO-Walker2d-v2', 'MO-Ant-v2', 'MO-Humanoid-v2']
DST = 'MO-DeepSeaTreasure-v0'
STORAGE = ('obs', 'actions', 'logp', 'values', 'rewards', 'masks', 'bad_masks')
STATE = ('s', 'elapsed', 'obj_acc', 'obj_valid', 'ret', '_stats64')


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _batch(env, N, T, ln=False, host=False, **kw):
    spec = envspec.make_spec(env)
    disc = bool(spec.get('discrete', False))
    he = None
    if host:
        he = DeepSeaTreasureHostVecEnv(env, P, N) if disc else SynthHostVecEnv(env, P, N, seed=0)
    tb = TaskBatch(env, P, num_processes=N, num_steps=T, ppo_epoch=1, num_mini_batch=1, layernorm=ln, host_env=he, **kw)
    torch.manual_seed(3)
    rng = np.random.RandomState(3)
    for p in range(P):
        pol = new_policy(spec['obs_dim'], spec['act_dim'], spec['obj_num'], layernorm=ln, discrete=disc)
        tb.set_task(p, pol.state_dict(), weights=rng.dirichlet(np.ones(spec['obj_num'])))
    return tb


def _snap(out, tag, tb, names):
    for n in names:
        out[f'{tag}/{n}'] = getattr(tb, n).detach().cpu().numpy().copy()


def collect_act(out):
    g = torch.Generator().manual_seed(5)
    for env, ln in [(e, False) for e in PLAIN] + [(e, True) for e in PLAIN[:5]] + [(DST, False)]:
        tb = _batch(env, 8, 2, ln=ln, host=env == DST)
        for N in (1, 3, 8):
            obs = torch.randn(P, N, tb.O, generator=g)
            noise = torch.rand(N, generator=g) if tb.discrete else torch.randn(N, tb.A, generator=g)
            for det in (False, True):
                v, a, lp = tb.act(obs, None if det else noise, deterministic=det)
                for n, x in (('value', v), ('action', a), ('logp', lp)):
                    out[f'act/{env}/ln{int(ln)}/N{N}/det{int(det)}/{n}'] = x.cpu().numpy()


def collect_block(out):
    os.environ['PGM_ROLLOUT_KERNEL'] = os.environ['PGM_EVAL_KERNEL'] = 'block'
    try:
        g = torch.Generator().manual_seed(6)
        for env, N, T, lns in (('MO-Hopper-v2', 3, 5, (False, True)), ('MO-Walker2d-v2', 8, 3, (False, True)),
                               ('MO-Hopper-v3', 3, 2, (False, True)), ('MO-Humanoid-v2', 2, 2, (False,))):
            for ln in lns:
                for explicit in (True, False):
                    tag = f'block/{env}/ln{int(ln)}/{"noise" if explicit else "counter"}'
                    tb = _batch(env, N, T, ln=ln, eval_num=3)
                    tb.c_spec.max_episode_steps = 2  # an auto-reset inside every T here
                    tb.env_reset()
                    for carry in (0, 1):
                        nz = torch.randn(T, N, tb.A, generator=g) if explicit else None
                        tb.rollout(11 + carry, noise=nz, carry=bool(carry))
                        _snap(out, f'{tag}/carry{carry}', tb, STORAGE + STATE)
                    tb.c_spec.max_episode_steps = 12  # evaluation episodes cut short
                    for en in (1, 3):
                        for raw in (0, 1):
                            tb.eval_num, tb.raw = en, bool(raw)
                            out[f'{tag}/eval{en}/raw{raw}'] = tb.evaluate().cpu().numpy().copy()
    finally:
        os.environ.pop('PGM_ROLLOUT_KERNEL')
        os.environ.pop('PGM_EVAL_KERNEL')


def collect_seam(out):
    T = 3
    lib = _lib.lib()
    for env, ln in (('MO-Walker2d-v2', False), ('MO-Hopper-v3', False), ('MO-Hopper-v2', True), ('MO-Hopper-v3', True),
                    (DST, False)):
        for N in (1, 3, 8):
            rng = np.random.RandomState(100 + N)
            g = torch.Generator().manual_seed(8)
            tag = f'seam/{env}/ln{int(ln)}/N{N}'
            tb = _batch(env, N, T, ln=ln, host=True)
            O, K = tb.O, tb.K
            tb._ingest(-1, rng.randn(P, N, O))
            _snap(out, f'{tag}/ingest-1', tb, ('obs', 'masks', 'bad_masks', 'obj_acc', 'obj_valid', 'ret', '_stats64'))
            tb.obs[:, 1:].copy_(torch.randn(P, T, N, O, generator=g))
            tb.noise.copy_(torch.rand(T, N, generator=g) if tb.discrete else torch.randn(T, N, tb.A, generator=g))
            for t in (0, T - 1, T):
                tb._rollout_act(t)
                _snap(out, f'{tag}/act{t}', tb, ('values', 'actions', 'logp'))
                _snap(out, f'{tag}/act{t}', tb.mode, ('_d_act',))
            done = rng.rand(P, N) < 0.4
            tb._ingest(0, rng.randn(P, N, O), rng.randn(P, N), done, done & (rng.rand(P, N) < 0.5), rng.randn(P, N, K))
            _snap(out, f'{tag}/ingest0', tb, ('obs', 'rewards', 'masks', 'bad_masks', 'obj_acc', 'obj_valid', 'ret',
                                               '_stats64'))
            d = Dims(P, 1, 0, O, tb.A, K, tb.H, int(ln))
            for E in (1, 8):
                raw = torch.tensor(rng.randn(P, E, O), device=tb.dev)
                for use_ob in (0, 1):
                    if tb.discrete:
                        ea, fn = torch.zeros(P, E, dtype=torch.int32, device=tb.dev), lib.pgm_eval_act_cat
                    else:
                        ea, fn = torch.zeros(P, E, tb.A, device=tb.dev), lib.pgm_eval_act
                    _lib.check(fn(C.byref(d), _ptr(tb.params), _ptr(tb.ob_mean), _ptr(tb.ob_var), use_ob, _ptr(raw), E,
                                  _ptr(ea), _stream()), 'pgm_eval_act')
                    out[f'{tag}/eval_act/E{E}/ob{use_ob}'] = ea.cpu().numpy()


def collect(path):
    _lib._active = _lib._load(path)
    out = {}
    collect_act(out)
    collect_block(out)
    collect_seam(out)
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True, help="the parent commit's libpgm.so")
    ap.add_argument('--out', default=os.path.join('profiles', 'policy_refactor_equal.json'))
    a = ap.parse_args()
    ref, new = collect(os.path.abspath(a.parent)), collect(_lib.LIB_PATH)
    assert ref.keys() == new.keys()
    differing, worst = {}, 0.0
    for k, x in ref.items():
        y = new[k]
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            dmax = float('inf')
            if x.shape == y.shape:
                dmax = float(np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64))))
            differing[k] = dmax
            worst = max(worst, dmax)
    groups = {}
    for k in ref:
        groups[k.split('/')[0]] = groups.get(k.split('/')[0], 0) + 1
    res = {'device': torch.cuda.get_device_name(0), 'arrays': len(ref), 'arrays_by_group': groups,
           'elements': int(sum(x.size for x in ref.values())), 'nonfinite_elements': int(sum(
               (~np.isfinite(x.astype(np.float64))).sum() for x in ref.values())),
           'max_abs_diff': worst, 'differing': differing}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    sys.exit(1 if differing else 0)


if __name__ == '__main__':
    main()
