"""The measurement of DESIGN.md §30 (simplex blends for three-objective fronts): evaluate_candidates3 (one
pgm_eval_blend3 per slice, the three-member blend formed in the kernel's weight load) on the front of one finished
MO-Hopper-v3 run (the reference launcher's flags), against the same numbers obtained with what existed before
pgm_eval_blend3: the three-member blend on the host in bounded slices, upload of the materialised candidates,
evaluate_policies (pgm_eval_episodes).  Beside it pgm_eval_blend on the pair rows alone (time per step of a wave of the
two kernels), and hypervolume and sparsity of the stored, the re-measured, the pair-dense and the simplex-dense front.

    python scripts/interpolate_simplex.py --out profiles/interpolate_simplex.json [--save-dir DIR] [--points 5]
                                          [--neighbours 4] [--episodes 1 8] [--b-candidates 20480]

Without --save-dir the run is made first (seed 0, a temporary directory).  Each side and E: 3 warm-ups, then 9 timed
repetitions ending in a synchronise, median (min-max).  Wall times include every upload and the download of the result
on both sides; the device times are HIP events around the entry points on resident buffers.  The run's archive holds
some 10^4 members and the table some 3 10^5 candidates of 41 kB each, which the host side can neither hold nor blend in
a reasonable time: the two sides are compared on an evenly strided subset of --b-candidates candidates (both sides are
linear in the number of candidates), and the new side is also timed on the whole table.
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

# the launcher's MO-Hopper-v3 flags
FLAGS = ['--env-name', 'MO-Hopper-v3', '--obj-num', '3', '--num-env-steps', '8000000', '--warmup-iter', '200',
         '--update-iter', '40', '--min-weight', '0.0', '--max-weight', '1.0', '--delta-weight', '0.25', '--eval-num', '1',
         '--pbuffer-num', '20', '--pbuffer-size', '2', '--selection-method', 'prediction-guided',
         '--num-weight-candidates', '7', '--num-tasks', '15', '--sparsity', '1000000.0', '--obj-rms', '--ob-rms', '--raw',
         '--rng', 'device']


def host_blend3(np, params, ob_mean, ob_var, src, w):
    """The definition, restated for the side that has no blend3: (wa A + wb B) + wc C in fp64, parameters rounded to
    fp32 once."""
    def mix(x):
        a, b, c = (x[src[:, i]].astype(np.float64) for i in range(3))
        return (w[:, 0, None] * a + w[:, 1, None] * b) + w[:, 2, None] * c
    return mix(params).astype(np.float32), mix(ob_mean), mix(ob_var)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--save-dir', default=None)
    ap.add_argument('--points', type=int, default=5)
    ap.add_argument('--neighbours', type=int, default=4)
    ap.add_argument('--episodes', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--b-candidates', type=int, default=20480, help='candidates of the subset side (b) is measured on')
    o = ap.parse_args()
    import numpy as np
    import torch

    from pgmorl_amd import _lib, envspec, evaluate, interpolate
    from pgmorl_amd.pareto import compute_sparsity
    from pgmorl_amd.run import main as run_main
    tmp = None
    save_dir = o.save_dir
    run_s = None
    if save_dir is None:
        tmp = save_dir = tempfile.mkdtemp(prefix='interpolate_simplex_run_')
        t0, prev = time.perf_counter(), torch.get_default_dtype()
        try:
            with open(os.devnull, 'w') as null, contextlib.redirect_stdout(null):
                run_main([*FLAGS, '--seed', '0', '--save-dir', save_dir])
        finally:
            torch.set_default_dtype(prev)  # (the command sets float64, as the reference's does)
        run_s = time.perf_counter() - t0
        print(f'run finished in {run_s:.1f} s', flush=True)
    try:
        args, params, ob_mean, ob_var, stored = evaluate.load_pareto_set(save_dir)
    finally:
        if tmp is not None:
            shutil.rmtree(tmp, ignore_errors=True)
    M = params.shape[0]
    pairs = interpolate.neighbour_pairs(stored, o.neighbours)
    triangles = interpolate.neighbour_triangles(stored, o.neighbours, pairs)
    table3 = interpolate.candidate_table3(M, pairs, triangles, o.points)
    table2 = interpolate.candidate_table(M, pairs, o.points)
    src, w = table3
    Q, Q2 = len(src), len(table2[0])
    inside = len({m for t in triangles for m in t})
    sp = envspec.make_spec(args.env_name)
    O, A, K, tmax = sp['obs_dim'], sp['act_dim'], sp['obj_num'], sp['max_episode_steps']
    kw = dict(gamma=args.gamma, raw=args.raw, use_ob_rms=args.ob_rms, layernorm=args.layernorm)
    SLICE = interpolate.FALLBACK_CHUNK
    resident = torch.cuda.get_device_properties(0).multi_processor_count * 4 * 2  # waves: CUs x SIMDs x 2
    print(f'M = {M}, {len(pairs)} pairs, {len(triangles)} triangles ({inside} members inside one), Q = {Q} candidates '
          f'({Q2} of them members and pair rows)', flush=True)

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

    def per_step(ms, waves):
        """us per step of a wave: two waves per SIMD are resident (the launch bound), so the grid runs in rounds"""
        return round(1e3 * ms / -(-waves // resident) / tmax, 4)

    # side (b) materialises 41 kB per candidate on the host: it is measured on an evenly strided subset of the table
    # (members, pair rows and triangle rows in the table's proportions), on which side (a) is measured as well
    Qb = min(Q, o.b_candidates)
    sub = np.arange(Q)[::max(1, Q // Qb)][:Qb]
    src_b, w_b = np.ascontiguousarray(src[sub]), np.ascontiguousarray(w[sub])
    table_b = (src_b, w_b)

    # resident buffers of the device-only timings: the members and the tables; the materialised subset
    prm_n, mean_n, var_n = params.numpy(), ob_mean.numpy(), ob_var.numpy()
    prm_d, mean_d, var_d = params.to(dev), ob_mean.to(dev), ob_var.to(dev)
    src_d, w_d = torch.from_numpy(src).to(dev), torch.from_numpy(w).to(dev)
    srcb_d, wb_d = torch.from_numpy(src_b).to(dev), torch.from_numpy(w_b).to(dev)
    src2_d, alpha2_d = torch.from_numpy(table2[0]).to(dev), torch.from_numpy(table2[1]).to(dev)
    mat = [host_blend3(np, prm_n, mean_n, var_n, src_b[lo:lo + SLICE], w_b[lo:lo + SLICE]) for lo in range(0, Qb, SLICE)]
    upload_bytes = sum(sum(t.nbytes for t in m) for m in mat)
    mat_d = [torch.from_numpy(np.concatenate([m[i] for m in mat])).to(dev) for i in range(3)]
    del mat
    hv = interpolate._hypervolume3  # (the native 3-D hypervolume, as the command with --simplex)

    def front_of(means, n):
        idx = interpolate.get_ep_indices(means[:n])
        return {'hypervolume': float(hv(means[idx])), 'sparsity': float(compute_sparsity(means[idx])), 'size': len(idx)}

    members_bytes = int(sum(t.numel() * t.element_size() for t in (params, ob_mean, ob_var)))
    result = {'device': torch.cuda.get_device_name(0), 'env': args.env_name, 'flags': FLAGS, 'run_seconds': run_s,
              'M': int(M), 'neighbours': o.neighbours, 'points': o.points, 'pairs': len(pairs),
              'triangles': len(triangles), 'members_inside_a_triangle': inside, 'Q': int(Q), 'Q_pair_rows': int(Q2),
              'Q_subset': int(Qb), 'episode_steps': int(tmax), 'param_floats': int(params.shape[1]),
              'blend3_upload_bytes': members_bytes + src.nbytes + w.nbytes,
              'subset_blend3_upload_bytes': members_bytes + src_b.nbytes + w_b.nbytes,
              'subset_materialised_upload_bytes': int(upload_bytes), 'episodes': {}}
    for E in o.episodes:
        starts = torch.tensor(envspec.reset_table(O, args.seed, E), **f64)

        # ---- (a) the new way: the members uploaded once, one pgm_eval_blend3 per slice of the table
        def blend3_way(table=table3):
            return interpolate.evaluate_candidates3(args.env_name, params, ob_mean, ob_var, table, E, args.seed,
                                                    return_objs=True, **kw)
        (_, new_objs), full_ms = timed(blend3_way)
        (new, _), new_ms = timed(lambda: blend3_way(table_b))

        # ---- (b) the way before: the blend on the host in slices, upload, evaluate_policies
        def materialise_way():
            out = np.empty((Qb, E, K))
            for lo in range(0, Qb, SLICE):
                bp, bm, bv = host_blend3(np, prm_n, mean_n, var_n, src_b[lo:lo + SLICE], w_b[lo:lo + SLICE])
                out[lo:lo + SLICE] = evaluate.evaluate_policies(args.env_name, torch.from_numpy(bp),
                                                                torch.from_numpy(bm), torch.from_numpy(bv), E,
                                                                args.seed, chunk=SLICE, **kw)
            return out
        old, old_ms = timed(materialise_way)

        ep_d, objs_d = torch.empty(Q, E, K, **f64), torch.empty(Q, K, **f64)
        dims = lambda n: _lib.Dims(n, 1, 0, O, A, K, 64, 0)  # noqa: E731
        d, d2, db = dims(Q), dims(Q2), dims(Qb)
        common = (C.byref(c_spec), p(starts), E, int(args.ob_rms), int(args.raw), args.gamma, p(ep_d), p(objs_d))

        def blend3_launch(dd=d, s_=src_d, w_=w_d):  # the whole simplex table
            _lib.check(L.pgm_eval_blend3(C.byref(dd), p(prm_d), M, p(mean_d), p(var_d), p(s_), p(w_), *common,
                                         stream()), 'pgm_eval_blend3')

        def blend_pair_rows_launch():  # the member and pair rows through the two-member kernel
            _lib.check(L.pgm_eval_blend(C.byref(d2), p(prm_d), M, p(mean_d), p(var_d), p(src2_d), p(alpha2_d), *common,
                                        stream()), 'pgm_eval_blend')

        def episodes_launch():
            _lib.check(L.pgm_eval_episodes(C.byref(db), p(mat_d[0]), C.byref(c_spec), p(mat_d[1]), p(mat_d[2]),
                                           p(starts), E, int(args.ob_rms), int(args.raw), args.gamma, 0, 0, p(ep_d),
                                           p(objs_d), stream()), 'pgm_eval_episodes')
        blend3_dev = events(blend3_launch)
        blend3_sub_dev = events(lambda: blend3_launch(db, srcb_d, wb_d))
        episodes_dev = events(episodes_launch)
        blend3_pairs_dev = events(lambda: blend3_launch(d2))  # (the table's first Q2 rows are the member and pair rows)
        pair_rows3 = ep_d[:Q2].cpu().numpy()
        blend_pairs_dev = events(blend_pair_rows_launch)
        pair_rows2 = ep_d[:Q2].cpu().numpy()

        t0 = time.perf_counter()
        an = interpolate.analyse3(table3, new_objs, M, o.points, len(pairs), len(triangles))
        summary = dict(interpolate.summarise(an, stored, o.neighbours, E, args.seed, args.seed, hv), simplex=True,
                       num_triangles=an['num_triangles'], num_filled=an['num_filled'])
        pair_dense = front_of(new_objs, Q2)
        analysis_s = time.perf_counter() - t0
        result['episodes'][str(E)] = {
            'env_steps': int(Q * E * tmax), 'subset_env_steps': int(Qb * E * tmax),
            'evaluate_candidates3_wall_ms': full_ms,
            'subset': {'evaluate_candidates3_wall_ms': new_ms, 'materialise_evaluate_policies_wall_ms': old_ms,
                       'wall_ratio': round(old_ms['median'] / new_ms['median'], 3),
                       'pgm_eval_blend3_device_ms': blend3_sub_dev, 'pgm_eval_episodes_device_ms': episodes_dev,
                       'device_ratio': round(episodes_dev['median'] / blend3_sub_dev['median'], 3),
                       'max_abs_difference': float(np.abs(new - old).max())},
            'pgm_eval_blend3_device_ms': blend3_dev,
            'resident_waves': resident, 'blend3_rounds': -(-Q * E // resident),
            'blend3_us_per_step_of_a_wave': per_step(blend3_dev['median'], Q * E),
            'env_steps_per_s_blend3_device': round(Q * E * tmax / (blend3_dev['median'] * 1e-3)),
            'env_steps_per_s_episodes_device': round(Qb * E * tmax / (episodes_dev['median'] * 1e-3)),
            'pair_rows': {'waves': Q2 * E, 'rounds': -(-Q2 * E // resident),
                          'pgm_eval_blend3_device_ms': blend3_pairs_dev, 'pgm_eval_blend_device_ms': blend_pairs_dev,
                          'blend3_us_per_step_of_a_wave': per_step(blend3_pairs_dev['median'], Q2 * E),
                          'blend_us_per_step_of_a_wave': per_step(blend_pairs_dev['median'], Q2 * E),
                          'bit_equal': bool(np.array_equal(pair_rows3, pair_rows2))},
            'fronts': {'stored': dict(summary['stored'], size=int(M)),
                       'remeasured': dict(summary['members'], size=int(M)), 'pair_dense': pair_dense,
                       'simplex_dense': dict(summary['dense'], size=summary['dense_front_size'])},
            'analysis_seconds': round(analysis_s, 1),
            'summary': summary,
        }
        print(json.dumps({E: result['episodes'][str(E)]}, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, 'w') as fp:
        json.dump(result, fp, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == '__main__':
    main()
