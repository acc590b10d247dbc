"""The measurement of DESIGN.md §27 (re-evaluating a saved Pareto set): evaluate_policies at E = 64 on the front of one
finished MO-Walker2d-v2 run (the reference launcher's flags), against the same result obtained with what existed
before pgm_eval_episodes: E launches of pgm_eval with eval_num = 1 over the same policies, one per start state.

    python scripts/eval_set.py --out profiles/eval_set.json [--save-dir DIR] [--episodes 64]

Without --save-dir the run is made first (seed 0, a temporary directory).  Each side: 3 warm-ups, then 9 timed
repetitions ending in a synchronise, median (min-max).  Wall times include the upload of the policies and the download
of the result on both sides; the kernel's own time is taken with HIP events around pgm_eval_episodes on resident
buffers.
"""
import argparse
import contextlib
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sweep_compare import FLAGS  # noqa: E402 (the launcher's MO-Walker2d-v2 flags)

WARM, TIMED = 3, 9


def spread(v):
    return {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}


def timed(fn):
    import torch
    out, ms = None, []
    for i in range(WARM + TIMED):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i >= WARM:
            ms.append(1e3 * (time.perf_counter() - t0))
    return out, spread(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--save-dir', default=None)
    ap.add_argument('--episodes', type=int, default=64)
    o = ap.parse_args()
    import numpy as np
    import torch

    from pgmorl_amd import _lib, envspec, evaluate
    from pgmorl_amd.run import main as run_main
    tmp = None
    save_dir = o.save_dir
    if save_dir is None:
        tmp = save_dir = tempfile.mkdtemp(prefix='eval_set_run_')
        t0, prev = time.perf_counter(), torch.get_default_dtype()
        try:
            with open(os.devnull, 'w') as null, contextlib.redirect_stdout(null):
                run_main([*FLAGS, '--seed', '0', '--save-dir', save_dir])
        finally:
            torch.set_default_dtype(prev)  # (the command sets float64, as the reference's does)
        print(f'run finished in {time.perf_counter() - t0:.1f} s', flush=True)
    try:
        args, params, ob_mean, ob_var, stored = evaluate.load_pareto_set(save_dir)
    finally:
        if tmp is not None:
            shutil.rmtree(tmp, ignore_errors=True)
    E, M = o.episodes, params.shape[0]
    sp = envspec.make_spec(args.env_name)
    O, A, K, tmax = sp['obs_dim'], sp['act_dim'], sp['obj_num'], sp['max_episode_steps']
    kw = dict(gamma=args.gamma, raw=args.raw, use_ob_rms=args.ob_rms, layernorm=args.layernorm)

    # ---- the new way: one call
    new, new_ms = timed(lambda: evaluate.evaluate_policies(args.env_name, params, ob_mean, ob_var, E, args.seed, **kw))

    # ---- resident buffers for the two device-only timings
    dev = torch.device('cuda')
    f64 = dict(dtype=torch.float64, device=dev)
    st = {k: torch.tensor(np.ascontiguousarray(sp[k]), **f64) for k in evaluate.SPEC_KEYS}
    c_spec = _lib.EnvSpec(*(C.c_void_p(st[k].data_ptr()) for k in evaluate.SPEC_KEYS), tmax, 0)
    starts = torch.tensor(envspec.reset_table(O, args.seed, E), **f64)
    d = _lib.Dims(M, 1, 1, O, A, K, 64, int(args.layernorm))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    opts = _lib.LaunchOpts()
    L = _lib.lib()

    def events(fn):
        ms = []
        for i in range(WARM + TIMED):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= WARM:
                ms.append(a.elapsed_time(b))
        return spread(ms)

    prm_d, mean_d, var_d = params.to(dev), ob_mean.to(dev), ob_var.to(dev)
    ep_d, objs_d = torch.empty(M, E, K, **f64), torch.empty(M, K, **f64)

    def new_launch():
        _lib.check(L.pgm_eval_episodes(C.byref(d), p(prm_d), C.byref(c_spec), p(mean_d), p(var_d), p(starts), E,
                                       int(args.ob_rms), int(args.raw), args.gamma, 0, 0, p(ep_d), p(objs_d), stream()),
                   'pgm_eval_episodes')
    kernel_ms = events(new_launch)

    # ---- the way before: E launches of pgm_eval (eval_num = 1, start row e), result [E][M][K]
    old_d = torch.empty(E, M, K, **f64)

    def old_launches(prm, mean, var):
        for e in range(E):
            s0 = C.c_void_p(starts.data_ptr() + e * O * 8)
            _lib.check(L.pgm_eval(C.byref(d), p(prm), C.byref(c_spec), p(mean), p(var), s0, 1, int(args.ob_rms),
                                  int(args.raw), args.gamma, p(old_d[e]), C.byref(opts), stream()), 'pgm_eval')

    def old_way():
        old_launches(params.to(dev), ob_mean.to(dev), ob_var.to(dev))
        return old_d.cpu().numpy().transpose(1, 0, 2)
    old, old_ms = timed(old_way)
    old_kernel_ms = events(lambda: old_launches(prm_d, mean_d, var_d))

    steps = M * E * tmax
    result = {
        'device': torch.cuda.get_device_name(0), 'env': args.env_name, 'flags': FLAGS, 'M': int(M), 'E': int(E),
        'episode_steps': int(tmax), 'env_steps': int(steps),
        'evaluate_policies_wall_ms': new_ms, 'pgm_eval_episodes_kernel_ms': kernel_ms,
        'env_steps_per_s_kernel': round(steps / (kernel_ms['median'] * 1e-3)),
        'pgm_eval_x_E_wall_ms': old_ms, 'pgm_eval_x_E_launches_ms': old_kernel_ms,
        'wall_ratio': round(old_ms['median'] / new_ms['median'], 3),
        'device_ratio': round(old_kernel_ms['median'] / kernel_ms['median'], 3),
        'max_abs_difference': float(np.abs(new - old).max()),
        'summary': evaluate.summarise(new, stored, args.seed, 0, False),
    }
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, 'w') as fp:
        json.dump(result, fp, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == '__main__':
    main()
