"""A sweep in the shape of the reference launchers (scripts/walker2d-v2.py and its siblings: --num-seeds runs for each
selected method, every run --num-tasks tasks), with all runs sharing ONE device population (morl.run_many):

    python -m pgmorl_amd.sweep [--pgmorl] [--ra] [--pfa] [--moead] [--random] [--num-seeds 6] [--seeds S ...] \
           [--grid FLAG V1 [V2 ...]]... --save-dir ROOT [--max-tasks M] \
           -- <any pgmorl_amd.run flag except --seed / --selection-method / --save-dir>

Run i of method m writes ROOT/<m>/<i>/ (m in pgmorl, ra, pfa, moead, random) with the args.txt, log.txt, generation
directories, final/ and timing.json of a solo ``python -m pgmorl_amd.run``; ROOT/sweep_timing.json holds the sweep's
wall time, its MOPG time, the per-run boundary times, the chunking and the tasks per generation.  The default seeds are
the launcher's own draw: random.seed(1000), one randint(0, 1000000) per seed index, shared by the methods of that index.

--grid FLAG V1 [V2 ...] (repeatable; FLAG one of lr, lr-decay-ratio, gae-lambda, clip-param, value-loss-coef,
entropy-coef, max-grad-norm) adds a hyper-parameter grid: the runs are the cartesian product of the grids, the seeds
and the methods, all in the same population (the settings are per task on the device), and a run lands in
ROOT/<m>/<point>/<i>/ with <point> the grids' flag=value joined by commas in the order given, e.g.
lr=0.0003,clip-param=0.1.  The runs are ordered grid point outermost, then seed index, then method.
"""
import argparse
import itertools
import json
import math
import os
import random
import sys

# launcher flag -> (--selection-method, directory), in the launchers' own order inside one seed index
METHODS = (('pgmorl', 'prediction-guided'), ('ra', 'ra'), ('random', 'random'), ('pfa', 'pfa'), ('moead', 'moead'))
OWN_FLAGS = ('--seed', '--selection-method', '--save-dir')  # set per run by the sweep
# --grid flags that are refused with a reason of their own (the others outside morl.GRID_FIELDS are unknown)
NOT_PER_TASK = {'gamma': 'gamma also enters the rollout\'s return normalisation and the evaluation discount, which are '
                         'not per task',
                **{k: f'{k} is a shape of the shared rollout storage and update launch'
                   for k in ('num-steps', 'num-processes', 'ppo-epoch', 'num-mini-batch')}}


def default_seeds(n):
    """The launchers' draw (scripts/*.py: random.seed(1000), then one randint per seed index), on a generator of its
    own."""
    g = random.Random(1000)
    return [g.randint(0, 1000000) for _ in range(n)]


def get_parser():
    ap = argparse.ArgumentParser(description='PG-MORL sweep on one MI355X: many seeds and selection methods in one '
                                             'population', usage=__doc__)
    for flag, _ in METHODS:
        ap.add_argument(f'--{flag}', action='store_true', default=False)
    ap.add_argument('--num-seeds', type=int, default=6)
    ap.add_argument('--seeds', type=int, nargs='+', default=None, help='the seeds themselves (overrides --num-seeds)')
    ap.add_argument('--save-dir', required=True, metavar='ROOT')
    ap.add_argument('--max-tasks', type=int, default=None,
                    help='most tasks of one launch; more runs are processed in consecutive chunks')
    ap.add_argument('--grid', action='append', nargs='+', default=None, metavar=('FLAG', 'V'),
                    help='a hyper-parameter grid: FLAG V1 [V2 ...]; repeatable, the runs are the cartesian product')
    return ap


def _full_flag(given):
    """The run flag argparse reads `given` as: itself, or the one flag it is an unambiguous prefix of (else None)."""
    from .run import get_parser as run_parser
    known = list(run_parser()._option_string_actions)
    if given in known:
        return given
    hits = [k for k in known if k.startswith(given)]
    return hits[0] if len(hits) == 1 else None


def grid_points(grids, rest):
    """[(field, flag, [value text, ...])] of the --grid options, after every refusal (PGMError naming the flag)."""
    from ._lib import PGMError
    from .morl import GRID_FIELDS
    from .runtime import TASK_FIELDS, check_task_hparam
    out = []
    for g in grids or []:
        flag = g[0].replace('_', '-')
        field = flag.replace('-', '_')
        if flag in NOT_PER_TASK:
            raise PGMError(f'--grid {flag}: {NOT_PER_TASK[flag]}; the runs of one population share it '
                           f'(grids: {", ".join(k.replace("_", "-") for k in GRID_FIELDS)})')
        if field not in GRID_FIELDS:
            raise PGMError(f'--grid {flag}: unknown grid flag (one of '
                           f'{", ".join(k.replace("_", "-") for k in GRID_FIELDS)})')
        if any(field == f for f, _, _ in out):
            raise PGMError(f'--grid {flag} given twice: one value list per flag')
        for a in rest:
            given = a.split('=')[0]
            if given.startswith('--') and len(given) > 2 and _full_flag(given) == f'--{flag}':
                raise PGMError(f'--grid {flag} and {given} after "--": the grid sets --{flag} of every run itself')
        texts = list(g[1:])
        if not texts:
            raise PGMError(f'--grid {flag}: no values')
        vals = []
        for t in texts:
            try:
                v = float(t)
            except ValueError:
                raise PGMError(f'--grid {flag}: {t!r} is not a number') from None
            if field in TASK_FIELDS:
                check_task_hparam(field, v, f'--grid {flag}')
            elif not math.isfinite(v):
                raise PGMError(f'--grid {flag}: {t} must be finite')
            if v in vals:
                raise PGMError(f'--grid {flag}: the value {t} is listed twice')
            vals.append(v)
        out.append((field, flag, vals))
    return out


def plan(argv):
    """(sweep options, run argv, [(method dir, seed index, run argv of that run)]) after every refusal; touches neither
    the file system nor the device.  With --grid the first element of a triple is <method>/<point>, and opts.vary names
    the fields the runs differ in (morl.run_many's vary; () without a grid)."""
    from ._lib import PGMError
    from . import envspec
    from .run import get_parser as run_parser, merge_argv
    argv = list(argv)
    own, rest = (argv[:argv.index('--')], argv[argv.index('--') + 1:]) if '--' in argv else (argv, [])
    opts = get_parser().parse_args(own)
    for a in rest:
        flag = a.split('=')[0]
        own_flag = [f for f in OWN_FLAGS if flag.startswith('--') and len(flag) > 2 and f.startswith(flag)]
        if own_flag:  # (argparse also takes an unambiguous prefix, --see 3)
            raise PGMError(f'{own_flag[0]} after "--": the sweep sets --seed, --selection-method and --save-dir of '
                           f'every run itself (--seeds, the method flags, --save-dir ROOT)')
    grids = grid_points(opts.grid, rest)
    opts.vary = tuple(field for field, _, _ in grids)
    methods = [(flag, m) for flag, m in METHODS if getattr(opts, flag)]
    if not methods:
        raise PGMError('no selection method: pass at least one of --pgmorl --ra --pfa --moead --random')
    seeds = list(opts.seeds) if opts.seeds is not None else default_seeds(opts.num_seeds)
    if not seeds:
        raise PGMError('no seeds: --num-seeds must be at least 1')
    base = run_parser().parse_args(merge_argv(rest))
    if base.host_env is not None:
        raise PGMError('--host-env in a sweep: the runs share one population on the SynthMO device envs only '
                       '(host-stepped sweeps are not built)')
    if base.device_env:
        raise PGMError('--device-env in a sweep: the runs share one population on the SynthMO device envs only '
                       '(the device Deep Sea Treasure has no per-run reset table)')
    if base.env_plugin is not None:
        raise PGMError('--env-plugin in a sweep: the runs share one population on the SynthMO device envs only '
                       '(plug-in reset tables are per family)')
    if base.env_name in envspec.native_env_names() or base.env_name in envspec.discrete_env_names():
        raise PGMError(f'--env-name {base.env_name} in a sweep: the MO-Dummy and Deep Sea Treasure envs have reset '
                       f'tables of their own shape; sweeps run the SynthMO device envs only')
    spec = envspec.make_spec(base.env_name)  # (ValueError from envspec for a name it does not know)
    ws = int(os.environ.get('WORLD_SIZE', '1') or 1)
    if ws > 1:
        raise PGMError(f'WORLD_SIZE={ws}: a sweep runs on one rank (multi-GPU sweeps are not built)')
    if any(m == 'pfa' for _, m in methods) and base.obj_num > 2:
        raise PGMError('--pfa with three objectives: pfa needs 2 objectives (morl/morl.py:141-143)')
    if base.layernorm:
        from .runtime import LN_MAX_OBS
        if spec['obs_dim'] > LN_MAX_OBS:
            raise PGMError(f'--layernorm with {base.env_name}: the LayerNorm kernels are built for obs_dim <= '
                           f'{LN_MAX_OBS}')
    if opts.max_tasks is not None:
        from .morl import tasks_per_run
        if opts.max_tasks < tasks_per_run(base):
            raise PGMError(f'--max-tasks {opts.max_tasks} is below the {tasks_per_run(base)} tasks of one run')
    runs = []
    for point in itertools.product(*[vals for _, _, vals in grids]):
        # (no grid: one empty point, the directories and argv of a sweep without --grid)
        name = ','.join(f'{gflag}={v!r}' for (_, gflag, _), v in zip(grids, point))
        pargv = [x for (_, gflag, _), v in zip(grids, point) for x in (f'--{gflag}', repr(v))]
        for i, seed in enumerate(seeds):
            for flag, m in methods:
                top = os.path.join(flag, name) if grids else flag
                d = os.path.join(opts.save_dir, top, str(i))
                runs.append((top, i, rest + pargv + ['--seed', str(seed), '--selection-method', m, '--save-dir', d]))
    return opts, base, runs


class _RunLog:
    """One run's log.txt, with the lines also on stdout behind the run's directory."""

    def __init__(self, path, tag):
        self.f, self.tag = open(path, 'w'), tag

    def __call__(self, *m):
        line = ' '.join(str(x) for x in m) + '\n'
        self.f.write(line)
        sys.stdout.write(f'[{self.tag}] {line}')
        sys.stdout.flush()


def main(argv=None):
    import torch
    from .run import get_parser as run_parser, merge_argv
    argv = sys.argv[1:] if argv is None else argv
    opts, base, runs = plan(argv)
    torch.set_default_dtype(torch.float64)
    from .morl import check_sweep_args, run_many, sweep_chunks
    from .mopg import MOPGPopulation
    args_list = [run_parser().parse_args(merge_argv(rargv)) for _, _, rargv in runs]
    # run_many's own refusals, before ROOT is made (it checks again)
    check_sweep_args(args_list, opts.vary)
    sweep_chunks(args_list, opts.max_tasks, lambda P: MOPGPopulation.update_fits(args_list[0], P, base.device))
    logs = []
    for a, (flag, i, rargv) in zip(args_list, runs):
        os.makedirs(a.save_dir, exist_ok=True)
        with open(os.path.join(a.save_dir, 'args.txt'), 'w') as fp:
            fp.write(str(merge_argv(rargv)))
        logs.append(_RunLog(os.path.join(a.save_dir, 'log.txt'), f'{flag}/{i}'))
    info = {}
    try:
        run_many(args_list, device=base.device, rng=base.rng, log=logs, max_tasks=opts.max_tasks, info=info,
                 vary=opts.vary)
    finally:
        for lg in logs:
            lg.f.close()
    info['dirs'] = [os.path.join(flag, str(i)) for flag, i, _ in runs]
    info['seeds'] = [a.seed for a in args_list]
    info['methods'] = [a.selection_method for a in args_list]
    with open(os.path.join(opts.save_dir, 'sweep_timing.json'), 'w') as fp:
        json.dump(info, fp, indent=1)
    print(f"[sweep] {len(runs)} runs in {len(info['chunks'])} chunk(s): wall {info['wall_s']:.2f} s, MOPG "
          f"{info['rl_s']:.2f} s, boundaries {sum(info['boundary_s']):.2f} s")


if __name__ == '__main__':
    main()
