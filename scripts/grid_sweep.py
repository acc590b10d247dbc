"""The two measurements of DESIGN.md §26 (hyper-parameter grids): what the per-task table costs an update launch, and
what a grid sweep gains over one sweep per grid point.

    python scripts/grid_sweep.py --out profiles/grid_sweep.json [--parts table grid] [--reps 2]

table: pgm_ppo_update_tasks with a uniform table against pgm_ppo_update, interleaved in one session, on
MO-Walker2d-v2 with T 2048, N 4, 10 epochs x 32 minibatches at P = 40 (the feature-split kernel, NS 6) and P = 180 (the
MODE 0 kernel a 30-run chunk gets), and with --layernorm at P = 40 (the LayerNorm kernel, whose TASKS twin has the
largest scratch growth of the resource table): 3 warm-up and 9 timed launches of each, HIP events around the whole entry
point (the row packing included), median (min-max) in ms.  The state is restored before every launch, so every launch does
the same work.
grid: MO-Walker2d-v2 with the reference launcher's flags, three learning rates x two seeds x prediction-guided, as one
grid sweep (6 runs, 36 tasks in one population) and as three of the sweeps without --grid one after the other (2 runs,
12 tasks each); the sides alternate, one warm-up of each, then --reps repetitions; wall, MOPG and boundary seconds.
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

from sweep_compare import FLAGS  # noqa: E402 (the launcher's MO-Walker2d-v2 flags)

LRS = ['1e-4', '3e-4', '1e-3']


def spread(v):
    return {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}


# ------------------------------------------------------------------------------------------------ the table's cost
def table_cost(P, layernorm=False, warm=3, timed=9):
    import numpy as np
    import torch

    from pgmorl_amd import envspec
    from pgmorl_amd.policy import new_policy
    from pgmorl_amd.runtime import TaskBatch
    env = 'MO-Walker2d-v2'
    spec = envspec.make_spec(env)
    tb = TaskBatch(env, P, num_processes=4, num_steps=2048, ppo_epoch=10, num_mini_batch=32, layernorm=layernorm)
    torch.manual_seed(0)
    w = np.linspace(0, 1, P)
    for p in range(P):
        pol = new_policy(spec['obs_dim'], spec['act_dim'], spec['obj_num'], layernorm=layernorm)
        tb.set_task(p, pol.state_dict(), {}, None, [w[p], 1 - w[p]])
    tb.env_reset()
    tb.iteration(0, 3e-4, carry=False)  # real storage, advantages and permutations; then the launches below
    tb.make_perms(1)
    state0, step0 = tb.state.clone(), tb.adam_step.clone()
    variant = tb.update_variant()
    hp = tb.hp
    times = {'plain': [], 'tasks': []}
    outs = {}
    for i in range(warm + timed):
        for side in ('plain', 'tasks'):
            tb.state.copy_(state0)
            tb.adam_step.copy_(step0)
            if side == 'tasks':
                tb.set_task_hparams(clip_param=hp.clip_param, value_loss_coef=hp.value_loss_coef,
                                    entropy_coef=hp.entropy_coef, max_grad_norm=hp.max_grad_norm)
            else:
                tb.hp_task = None
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            tb.ppo_update_launch()
            b.record()
            torch.cuda.synchronize()
            tb.fold_update_flag()
            if i >= warm:
                times[side].append(a.elapsed_time(b))
            outs[side] = tb.state.clone()
    tb.check_update()
    r = {'P': P, 'layernorm': layernorm, 'update': variant, 'plain_ms': spread(times['plain']),
         'tasks_ms': spread(times['tasks']), 'bit_equal': bool(torch.equal(outs['plain'], outs['tasks']))}
    m, lo, hi = r['tasks_ms']['median'], r['plain_ms']['min'], r['plain_ms']['max']
    r['tasks_median_inside_plain_spread'] = bool(lo <= m <= hi)
    r['tasks_median_over_plain_median'] = round(m / r['plain_ms']['median'], 4)
    return r


# ------------------------------------------------------------------------------------------------ what a grid gains
def _run_sweep(root, own):
    """One sweep through the command line's own plan (no files besides the runs' trees) -> its timing."""
    from pgmorl_amd import morl, sweep
    from pgmorl_amd.mopg import MOPGPopulation
    from pgmorl_amd.run import get_parser, merge_argv
    opts, base, runs = sweep.plan([*own, '--save-dir', root, '--', *FLAGS])
    args_list = [get_parser().parse_args(merge_argv(argv)) for _, _, argv in runs]
    info, rts = {}, []

    def make(a, run_seeds, run_hparams=None):
        rts.append(MOPGPopulation(a, device='cuda', rng='device', run_seeds=run_seeds, run_hparams=run_hparams))
        return rts[-1]
    morl.run_many(args_list, device='cuda', rng='device', log=None, runtime=make, info=info, vary=opts.vary)
    return {'rl_s': info['rl_s'], 'boundary_s': sum(info['boundary_s']), 'update': rts[-1].tb.update_variant(),
            'tasks_per_generation': sorted({g['tasks'] for g in info['generations']}), 'runs': len(runs)}


def grid_side(root):
    t0 = time.perf_counter()
    r = _run_sweep(root, ['--pgmorl', '--num-seeds', '2', '--grid', 'lr', *LRS])
    r['wall_s'] = time.perf_counter() - t0
    return r


def three_sweeps(root):
    """Today's way: one sweep per learning rate (--lr after the dashes), one after the other."""
    from pgmorl_amd import morl, sweep
    from pgmorl_amd.mopg import MOPGPopulation
    from pgmorl_amd.run import get_parser, merge_argv
    t0 = time.perf_counter()
    out = {'rl_s': 0.0, 'boundary_s': 0.0, 'runs': 0}
    for lr in LRS:
        opts, base, runs = sweep.plan(['--pgmorl', '--num-seeds', '2', '--save-dir', os.path.join(root, lr), '--',
                                       *FLAGS, '--lr', lr])
        args_list = [get_parser().parse_args(merge_argv(argv)) for _, _, argv in runs]
        info, rts = {}, []

        def make(a, run_seeds):
            rts.append(MOPGPopulation(a, device='cuda', rng='device', run_seeds=run_seeds))
            return rts[-1]
        morl.run_many(args_list, device='cuda', rng='device', log=None, runtime=make, info=info)
        out['rl_s'] += info['rl_s']
        out['boundary_s'] += sum(info['boundary_s'])
        out['runs'] += len(runs)
        out['update'] = rts[-1].tb.update_variant()
        out['tasks_per_generation'] = sorted({g['tasks'] for g in info['generations']})
    out['wall_s'] = time.perf_counter() - t0
    return out


def summarise(rows):
    out = {k: spread([r[k] for r in rows]) for k in ('wall_s', 'rl_s', 'boundary_s')}
    out.update({k: rows[-1][k] for k in rows[-1] if k not in out})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--parts', nargs='+', default=['table', 'grid'], choices=['table', 'grid'])
    ap.add_argument('--reps', type=int, default=2)
    o = ap.parse_args()
    import torch
    torch.set_default_dtype(torch.float64)
    result = {}
    if os.path.exists(o.out):
        with open(o.out) as fp:
            result = json.load(fp)
    result['device'] = torch.cuda.get_device_name(0)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as fp:
            json.dump(result, fp, indent=1)
    if 'table' in o.parts:
        result['table'] = []
        for P, ln in ((40, False), (180, False), (40, True)):
            r = table_cost(P, ln)
            print(json.dumps(r), flush=True)
            result['table'].append(r)
            save()
    if 'grid' in o.parts:
        rows = {'three_sweeps': [], 'grid': []}
        for rep in range(-1, o.reps):  # rep -1: the warm-up of each side, not recorded
            for side, fn in (('three_sweeps', three_sweeps), ('grid', grid_side)):
                root = tempfile.mkdtemp(prefix=f'grid_sweep_{side}_')
                try:
                    r = fn(root)
                finally:
                    shutil.rmtree(root, ignore_errors=True)
                print(f'rep {rep} {side}: wall {r["wall_s"]:.2f} s, MOPG {r["rl_s"]:.2f} s, boundary '
                      f'{r["boundary_s"]:.2f} s ({r["update"]}, {r["tasks_per_generation"]} tasks)', flush=True)
                if rep >= 0:
                    rows[side].append(r)
        g = {side: summarise(v) for side, v in rows.items()}
        g['flags'], g['lrs'], g['reps'] = FLAGS, LRS, o.reps
        g['wall_ratio'] = round(g['three_sweeps']['wall_s']['median'] / g['grid']['wall_s']['median'], 3)
        g['mopg_ratio'] = round(g['three_sweeps']['rl_s']['median'] / g['grid']['rl_s']['median'], 3)
        result['grid'] = g
        save()
    print(json.dumps(result, indent=1))


if __name__ == '__main__':
    main()
