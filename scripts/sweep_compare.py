"""Wall time of a batched sweep (morl.run_many: all runs in one device population) against the same runs as solo
morl.run calls one after another in the same process.

    python scripts/sweep_compare.py --out profiles/sweep_compare.json [--configs pgmorl6 all30] [--reps 3]

Configs are the reference launcher's MO-Walker2d-v2 flags (scripts/walker2d-v2.py: 5e6 steps, 6 tasks, warm-up 80,
update 20, device RNG): pgmorl6 = six seeds x prediction-guided, all30 = six seeds x the five methods.  The two sides
alternate: one warm-up of each first, then --reps repetitions each; medians and the spread (min, max) are reported
with the split into MOPG time and generation-boundary time from the timing records.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLAGS = ['--env-name', 'MO-Walker2d-v2', '--num-env-steps', '5000000', '--warmup-iter', '80', '--update-iter', '20',
         '--min-weight', '0.0', '--max-weight', '1.0', '--delta-weight', '0.2', '--eval-num', '1', '--pbuffer-num', '100',
         '--pbuffer-size', '2', '--num-weight-candidates', '7', '--num-tasks', '6', '--sparsity', '1.0', '--obj-rms',
         '--ob-rms', '--raw', '--rng', 'device']
CONFIGS = {'pgmorl6': ['--pgmorl'], 'all30': ['--pgmorl', '--ra', '--random', '--pfa', '--moead']}


def args_for(root, methods, steps):
    from pgmorl_amd import sweep
    from pgmorl_amd.run import get_parser, merge_argv
    flags = list(FLAGS)
    if steps:
        flags[flags.index('--num-env-steps') + 1] = str(steps)
    _, _, runs = sweep.plan([*methods, '--num-seeds', '6', '--save-dir', root, '--', *flags])
    return [get_parser().parse_args(merge_argv(argv)) for _, _, argv in runs]


def solo_side(root, methods, steps):
    from pgmorl_amd import morl
    t0 = time.perf_counter()
    rl = host = 0.0
    variant = None
    for a in args_for(root, methods, steps):
        from pgmorl_amd.mopg import MOPGPopulation
        rt = MOPGPopulation(a, device='cuda', rng='device')
        ep = morl.run(a, device='cuda', rng='device', log=None, runtime=rt)
        rl += ep.timing['rl_s']
        host += ep.timing['host_s']
        variant = rt.tb.update_variant()
    return {'wall_s': time.perf_counter() - t0, 'rl_s': rl, 'boundary_s': host, 'update': variant}


def sweep_side(root, methods, steps, max_tasks=None):
    from pgmorl_amd import morl
    from pgmorl_amd.mopg import MOPGPopulation
    info, rts = {}, []

    def make(a, run_seeds):
        rts.append(MOPGPopulation(a, device='cuda', rng='device', run_seeds=run_seeds))
        return rts[-1]
    t0 = time.perf_counter()
    morl.run_many(args_for(root, methods, steps), device='cuda', rng='device', log=None, runtime=make, info=info,
                  max_tasks=max_tasks)
    return {'wall_s': time.perf_counter() - t0, 'rl_s': info['rl_s'], 'boundary_s': sum(info['boundary_s']),
            'update': rts[-1].tb.update_variant(), 'chunks': info['chunks'],
            'tasks_per_generation': sorted({g['tasks'] for g in info['generations']})}


def summarise(rows):
    out = {}
    for k in ('wall_s', 'rl_s', 'boundary_s'):
        v = [r[k] for r in rows]
        out[k] = {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
    out.update({k: rows[-1][k] for k in rows[-1] if k not in out})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--configs', nargs='+', default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--max-tasks', type=int, nargs='+', default=[],
                    help='also time the sweep side alone with these --max-tasks caps (chunked sweeps)')
    ap.add_argument('--sweep-only', action='store_true', help='skip the solo / sweep comparison (with --max-tasks)')
    ap.add_argument('--steps', type=int, default=0, help='--num-env-steps of every run (default: the launcher\'s 5e6)')
    o = ap.parse_args()
    import torch
    torch.set_default_dtype(torch.float64)
    result = {'device': torch.cuda.get_device_name(0), 'flags': FLAGS, 'steps': o.steps or 5000000, 'reps': o.reps,
              'configs': {}}
    for name in o.configs:
        methods = CONFIGS[name]
        rows = {'solo': [], 'sweep': []}
        for rep in range(-1, o.reps if not o.sweep_only else -1):  # rep -1: the warm-up of each side, not recorded
            for side, fn in (('solo', solo_side), ('sweep', sweep_side)):
                root = tempfile.mkdtemp(prefix=f'sweep_compare_{side}_')
                try:
                    r = fn(root, methods, o.steps)
                finally:
                    shutil.rmtree(root, ignore_errors=True)
                print(f'{name} rep {rep} {side}: wall {r["wall_s"]:.2f} s, MOPG {r["rl_s"]:.2f} s, boundary '
                      f'{r["boundary_s"]:.2f} s', flush=True)
                if rep >= 0:
                    rows[side].append(r)
        c = {'runs': 6 * len(methods)}
        if not o.sweep_only:
            c.update({side: summarise(v) for side, v in rows.items()})
            c['wall_ratio_solo_over_sweep'] = round(c['solo']['wall_s']['median'] / c['sweep']['wall_s']['median'], 3)
            c['mopg_ratio_solo_over_sweep'] = round(c['solo']['rl_s']['median'] / c['sweep']['rl_s']['median'], 3)
        for cap in o.max_tasks:  # the sweep side alone, chunked: one warm-up, then --reps repetitions
            capped = []
            for rep in range(-1, o.reps):
                root = tempfile.mkdtemp(prefix='sweep_compare_capped_')
                try:
                    r = sweep_side(root, methods, o.steps, max_tasks=cap)
                finally:
                    shutil.rmtree(root, ignore_errors=True)
                print(f'{name} --max-tasks {cap} rep {rep}: wall {r["wall_s"]:.2f} s, MOPG {r["rl_s"]:.2f} s', flush=True)
                if rep >= 0:
                    capped.append(r)
            c[f'sweep_max_tasks_{cap}'] = summarise(capped)
        result['configs'][name] = c
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as fp:  # (after every config: a later one may be cut short)
            json.dump(result, fp, indent=1)
    print(json.dumps(result['configs'], indent=1))


if __name__ == '__main__':
    main()
