"""The measurement of DESIGN.md §29 (a dense Pareto front from blended policies): evaluate_candidates (one
pgm_eval_blend per slice, the blend formed in the kernel's weight load) on the front of one finished MO-Walker2d-v2 run
(the reference launcher's flags), against the same result obtained with what existed before pgm_eval_blend: blend() on
the host in bounded slices, upload of the materialised candidates, evaluate_policies (pgm_eval_episodes).

    python scripts/interpolate_set.py --out profiles/interpolate_set.json [--save-dir DIR] [--points 15]
                                      [--neighbours 2] [--episodes 1 8]

Without --save-dir the run is made first (seed 0, a temporary directory).  Each side and E: 3 warm-ups, then 9 timed
repetitions ending in a synchronise, median (min-max).  Wall times include every upload and the download of the result
on both sides; the device times are HIP events around the entry points on resident buffers.
"""
import argparse
import contextlib
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eval_set import TIMED, WARM, spread, timed  # noqa: E402 (the protocol of §27)
from sweep_compare import FLAGS  # noqa: E402 (the launcher's MO-Walker2d-v2 flags)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--save-dir', default=None)
    ap.add_argument('--points', type=int, default=15)
    ap.add_argument('--neighbours', type=int, default=2)
    ap.add_argument('--episodes', type=int, nargs='+', default=[1, 8])
    o = ap.parse_args()
    import numpy as np
    import torch

    from pgmorl_amd import _lib, envspec, evaluate, interpolate
    from pgmorl_amd.run import main as run_main
    tmp = None
    save_dir = o.save_dir
    if save_dir is None:
        tmp = save_dir = tempfile.mkdtemp(prefix='interpolate_set_run_')
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
    M = params.shape[0]
    pairs = interpolate.neighbour_pairs(stored, o.neighbours)
    table = interpolate.candidate_table(M, pairs, o.points)
    src, alpha = table
    Q = len(src)
    sp = envspec.make_spec(args.env_name)
    O, A, K, tmax = sp['obs_dim'], sp['act_dim'], sp['obj_num'], sp['max_episode_steps']
    kw = dict(gamma=args.gamma, raw=args.raw, use_ob_rms=args.ob_rms, layernorm=args.layernorm)
    SLICE = interpolate.FALLBACK_CHUNK
    resident = torch.cuda.get_device_properties(0).multi_processor_count * 4 * 2  # waves: CUs x SIMDs x 2
    print(f'M = {M}, {len(pairs)} pairs, Q = {Q} candidates', flush=True)

    dev = torch.device('cuda')
    f64 = dict(dtype=torch.float64, device=dev)
    st = {k: torch.tensor(np.ascontiguousarray(sp[k]), **f64) for k in evaluate.SPEC_KEYS}
    c_spec = _lib.EnvSpec(*(C.c_void_p(st[k].data_ptr()) for k in evaluate.SPEC_KEYS), tmax, 0)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
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

    # resident buffers of the device-only timings: the members and the table; the materialised candidates
    prm_d, mean_d, var_d = params.to(dev), ob_mean.to(dev), ob_var.to(dev)
    src_d, alpha_d = torch.from_numpy(src).to(dev), torch.from_numpy(alpha).to(dev)
    mat = [interpolate.blend(params, ob_mean, ob_var, (src[lo:lo + SLICE], alpha[lo:lo + SLICE]))
           for lo in range(0, Q, SLICE)]
    upload_bytes = sum(sum(t.numel() * t.element_size() for t in m) for m in mat)
    mat_d = [torch.cat([m[i] for m in mat]).to(dev) for i in range(3)]
    del mat

    result = {'device': torch.cuda.get_device_name(0), 'env': args.env_name, 'flags': FLAGS, 'M': int(M),
              'neighbours': o.neighbours, 'points': o.points, 'pairs': len(pairs), 'Q': int(Q),
              'episode_steps': int(tmax), 'param_floats': int(params.shape[1]),
              'blend_upload_bytes': int(sum(t.numel() * t.element_size() for t in (params, ob_mean, ob_var)) +
                                        src.nbytes + alpha.nbytes),
              'materialised_upload_bytes': int(upload_bytes), 'episodes': {}}
    for E in o.episodes:
        starts = torch.tensor(envspec.reset_table(O, args.seed, E), **f64)

        # ---- (a) the new way: the members uploaded once, one pgm_eval_blend per slice of the table
        def blend_way():
            return interpolate.evaluate_candidates(args.env_name, params, ob_mean, ob_var, table, E, args.seed,
                                                   return_objs=True, **kw)
        (new, new_objs), new_ms = timed(blend_way)

        # ---- (b) the way before: blend() on the host in slices, upload, evaluate_policies
        def materialise_way():
            out = np.empty((Q, E, K))
            for lo in range(0, Q, SLICE):
                bp, bm, bv = interpolate.blend(params, ob_mean, ob_var, (src[lo:lo + SLICE], alpha[lo:lo + SLICE]))
                out[lo:lo + SLICE] = evaluate.evaluate_policies(args.env_name, bp, bm, bv, E, args.seed, chunk=SLICE,
                                                                **kw)
            return out
        old, old_ms = timed(materialise_way)

        ep_d, objs_d = torch.empty(Q, E, K, **f64), torch.empty(Q, K, **f64)
        d = _lib.Dims(Q, 1, 0, O, A, K, 64, 0)

        def blend_launch():
            _lib.check(L.pgm_eval_blend(C.byref(d), p(prm_d), M, p(mean_d), p(var_d), p(src_d), p(alpha_d),
                                        C.byref(c_spec), p(starts), E, int(args.ob_rms), int(args.raw), args.gamma,
                                        p(ep_d), p(objs_d), stream()), 'pgm_eval_blend')

        def episodes_launch():
            _lib.check(L.pgm_eval_episodes(C.byref(d), p(mat_d[0]), C.byref(c_spec), p(mat_d[1]), p(mat_d[2]),
                                           p(starts), E, int(args.ob_rms), int(args.raw), args.gamma, 0, 0, p(ep_d),
                                           p(objs_d), stream()), 'pgm_eval_episodes')
        blend_dev, episodes_dev = events(blend_launch), events(episodes_launch)

        steps = Q * E * tmax
        an = interpolate.analyse(table, new_objs, M, o.points)
        result['episodes'][str(E)] = {
            'env_steps': int(steps),
            'evaluate_candidates_wall_ms': new_ms, 'materialise_evaluate_policies_wall_ms': old_ms,
            'wall_ratio': round(old_ms['median'] / new_ms['median'], 3),
            'pgm_eval_blend_device_ms': blend_dev, 'pgm_eval_episodes_device_ms': episodes_dev,
            'device_ratio': round(episodes_dev['median'] / blend_dev['median'], 3),
            # two waves per SIMD are resident (the kernel's launch bound): the grid runs in `rounds` rounds of tmax steps
            'blend_resident_waves': resident, 'blend_rounds': -(-Q * E // resident),
            'blend_us_per_step_of_a_wave': round(1e3 * blend_dev['median'] / -(-Q * E // resident) / tmax, 4),
            'env_steps_per_s_blend_device': round(steps / (blend_dev['median'] * 1e-3)),
            'env_steps_per_s_episodes_device': round(steps / (episodes_dev['median'] * 1e-3)),
            'max_abs_difference': float(np.abs(new - old).max()),
            'summary': interpolate.summarise(an, stored, o.neighbours, E, args.seed, args.seed),
        }
        print(json.dumps({E: result['episodes'][str(E)]}, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, 'w') as fp:
        json.dump(result, fp, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == '__main__':
    main()
