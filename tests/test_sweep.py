"""The batched sweep on the host: the command line of ``python -m pgmorl_amd.sweep`` (seeds, directory layout, every
refusal before ROOT exists), run_many's argument check, its chunking, and the isolation of the runs' host random streams
(with a stand-in runtime: no GPU here)."""
import filecmp
import os
import types

import numpy as np
import pytest
import torch

from pgmorl_amd import morl, sweep
from pgmorl_amd._lib import PGMError
from pgmorl_amd.layout import ParamLayout
from pgmorl_amd.run import get_parser, merge_argv
from pgmorl_amd.sample import DeviceSnapshot, RunningMeanStd, Sample

TINY = ['--env-name', 'MO-Hopper-v2', '--num-steps', '8', '--num-processes', '2', '--ppo-epoch', '1', '--num-mini-batch',
        '2', '--num-env-steps', str(8 * 2 * 6), '--warmup-iter', '2', '--update-iter', '2', '--delta-weight', '0.5',
        '--num-tasks', '4', '--rl-log-interval', '1']


def test_default_seeds_are_the_launchers_draw():
    import random
    state = random.getstate()
    assert sweep.default_seeds(6) == [815117, 449815, 702363, 797306, 103955, 412728]
    assert random.getstate() == state  # drawn on a private generator
    assert sweep.default_seeds(2) == [815117, 449815]


def test_plan_lays_the_runs_out_like_the_launchers(tmp_path):
    root = tmp_path / 'ROOT'
    opts, base, runs = sweep.plan(['--pgmorl', '--random', '--ra', '--num-seeds', '2', '--save-dir', str(root), '--',
                                   *TINY])
    assert [(m, i) for m, i, _ in runs] == [('pgmorl', 0), ('ra', 0), ('random', 0), ('pgmorl', 1), ('ra', 1),
                                           ('random', 1)]
    parsed = [get_parser().parse_args(merge_argv(argv)) for _, _, argv in runs]
    assert [a.seed for a in parsed] == [815117] * 3 + [449815] * 3  # one seed per index, shared by its methods
    assert [a.selection_method for a in parsed] == ['prediction-guided', 'ra', 'random'] * 2
    assert [a.save_dir for a in parsed] == [os.path.join(str(root), m, str(i)) for m, i, _ in runs]
    assert all(a.num_steps == 8 and a.gamma == 0.995 and a.ob_rms for a in parsed)  # run's own defaults merged
    morl.check_sweep_args(parsed)
    _, _, runs = sweep.plan(['--moead', '--pfa', '--seeds', '3', '11', '5', '--save-dir', str(root), '--', *TINY])
    assert [(m, i) for m, i, _ in runs] == [('pfa', 0), ('moead', 0), ('pfa', 1), ('moead', 1), ('pfa', 2), ('moead', 2)]
    assert not root.exists()


@pytest.mark.parametrize('own,rest,match', [
    (['--pgmorl'], ['--host-env', 'synth'], '--host-env'),
    (['--pgmorl'], ['--device-env'], '--device-env'),
    (['--pgmorl'], ['--env-plugin', 'some.hpp'], '--env-plugin'),
    (['--pgmorl'], ['--env-name', 'MO-Dummy-v0'], 'MO-Dummy-v0'),
    (['--pgmorl'], ['--env-name', 'MO-Dummy3-v0', '--obj-num', '3'], 'MO-Dummy3-v0'),
    (['--pgmorl'], ['--env-name', 'MO-DeepSeaTreasure-v0'], 'MO-DeepSeaTreasure-v0'),
    (['--pfa', '--pgmorl'], ['--env-name', 'MO-Hopper-v3', '--obj-num', '3'], 'pfa'),
    (['--pgmorl'], ['--seed', '3'], '--seed'),
    (['--pgmorl'], ['--selection-method', 'ra'], '--selection-method'),
    (['--pgmorl'], ['--see', '3'], '--seed'),  # argparse would take the prefix
    (['--pgmorl'], ['--save-d=x'], '--save-dir'),
    (['--pgmorl'], ['--save-dir', 'x'], '--save-dir'),
    ([], [], 'selection method'),
    (['--pgmorl', '--max-tasks', '2'], TINY, '--max-tasks'),
    (['--pgmorl', '--layernorm-is-not-a-sweep-flag'], [], None),
])
def test_sweep_refusals_leave_root_absent(tmp_path, own, rest, match):
    root = tmp_path / 'ROOT'
    argv = [*own, '--save-dir', str(root), '--', *rest]
    if match is None:
        with pytest.raises(SystemExit):
            sweep.main(argv)
    else:
        with pytest.raises(PGMError, match=match):
            sweep.main(argv)
    assert not root.exists()


def test_sweep_refuses_more_than_one_rank(tmp_path, monkeypatch):
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(PGMError, match='WORLD_SIZE=2'):
        sweep.main(['--pgmorl', '--save-dir', str(tmp_path / 'ROOT'), '--', *TINY])
    assert not (tmp_path / 'ROOT').exists()


def _args(save_dir, seed, method, extra=()):
    return get_parser().parse_args(merge_argv([*TINY, *extra, '--seed', str(seed), '--selection-method', method,
                                               '--save-dir', str(save_dir)]))


def test_run_many_names_the_differing_field(tmp_path):
    a = _args(tmp_path / 'a', 1, 'ra')
    for extra, field in ((['--gamma', '0.99'], 'gamma'), (['--num-tasks', '5'], 'num_tasks'),
                         (['--env-name', 'MO-Walker2d-v2'], 'env_name'), (['--layernorm'], 'layernorm')):
        with pytest.raises(ValueError, match=f"'{field}'"):
            morl.run_many([a, _args(tmp_path / 'b', 2, 'random', extra)], device='cpu')
    with pytest.raises(ValueError, match='save_dir'):
        morl.run_many([a, _args(tmp_path / 'a', 2, 'random')], device='cpu')
    assert not (tmp_path / 'a').exists() and not (tmp_path / 'b').exists()  # refused before anything is created


def test_sweep_chunks():
    a = [_args('x', s, 'ra') for s in range(5)]  # 4 tasks per run (--num-tasks 4 >= the 3-weight grid)
    assert morl.tasks_per_run(a[0]) == 4
    assert morl.sweep_chunks(a) == [[0, 1, 2, 3, 4]]
    assert morl.sweep_chunks(a, max_tasks=9) == [[0, 1], [2, 3], [4]]
    assert morl.sweep_chunks(a, max_tasks=4) == [[0], [1], [2], [3], [4]]
    assert morl.sweep_chunks(a, fits=lambda P: P <= 12) == [[0, 1, 2], [3, 4]]
    assert morl.sweep_chunks(a, max_tasks=8, fits=lambda P: P <= 12) == [[0, 1], [2, 3], [4]]
    assert morl.sweep_chunks(a, fits=lambda P: False) == [[0], [1], [2], [3], [4]]  # one run is what a solo run tries
    with pytest.raises(ValueError, match='max-tasks'):
        morl.sweep_chunks(a, max_tasks=3)


def test_update_task_limit_is_the_launchers_rule():
    """MOPGPopulation.update_fits restates a limit the library owns (pgm_ppo_update_variant never refuses a P).  The
    restatement is tied to the text of include/pgm_abi.h and to the launchers' own refusals, so that a changed limit
    fails here instead of drifting."""
    import re

    from pgmorl_amd.mopg import MOPGPopulation as M
    from pgmorl_amd.runtime import LN_MAX_OBS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = ' '.join(open(os.path.join(root, 'include', 'pgm_abi.h')).read().split())
    doc = header[header.index('PPO.update minibatch loop'):header.index('int pgm_ppo_update(')]
    doc = doc.replace(' * ', ' ')
    m = re.search(r'obs_dim > (\d+) \(Humanoid\): layer 1 streamed from L2, needs (\d+)P <= CU count', doc)
    assert m and (int(m.group(1)), int(m.group(2))) == (M.UPDATE_RESIDENT_MAX_OBS, M.UPDATE_WORKGROUPS_PER_TASK)
    m = re.search(r'd->LN = 1: ppo_update_ln_kernel, one workgroup per tower .*? needs (\d+)P <= CU count', doc)
    assert m and int(m.group(1)) == M.UPDATE_WORKGROUPS_PER_TASK
    assert LN_MAX_OBS == M.UPDATE_RESIDENT_MAX_OBS
    csrc = os.path.join(root, 'pgmorl_amd', 'csrc')
    wide = open(os.path.join(csrc, 'pgm_ppo_wide.hip')).read()
    assert f'{M.UPDATE_WORKGROUPS_PER_TASK} * d->P > cus' in wide and 'the wide update needs 2P <= CUs' in wide
    assert 'needs 2 P = %d <= %d' in ' '.join(open(os.path.join(csrc, 'pgm_ppo_ln.hip')).read().split()).replace('" "', '')
    for cus in (256, 255, 304, 1):
        for ln, O in ((True, 11), (False, 376), (True, 17)):
            lim = M.update_task_limit(ln, O, cus)
            assert 2 * lim <= cus < 2 * (lim + 1)
        assert M.update_task_limit(False, 17, cus) == float('inf') and M.update_task_limit(False, 32, cus) == float('inf')
    a = _args('x', 0, 'ra', ['--layernorm'])
    assert M.update_fits(a, 10 ** 6, device='cpu')  # no device to ask: nothing is refused (the launch itself would)


class StandIn:
    """A runtime with the run / evaluate_samples / materialize / _batch / device surface morl.run documents.  An
    offspring's objectives are a fixed function of (run seed, task weights, iteration); its parameters are the elite's
    plus that function.  It draws from no random stream."""

    def __init__(self, args, run_seeds=None):
        self.args, self.device = args, torch.device('cpu')
        self.run_seeds = run_seeds
        self.layout = ParamLayout(11, 3, 2)
        self.calls = []

    def _batch(self, P):
        return types.SimpleNamespace(layout=self.layout)

    def _seed(self, run_of_task, p):
        return self.args.seed if self.run_seeds is None else self.run_seeds[int(run_of_task[p])]

    @staticmethod
    def _objs(seed, w, j):
        w = np.asarray(w, dtype=np.float64)
        ph = 0.37 * seed + 0.11 * j
        return np.array([10.0 * w[0] + np.sin(ph) + 0.05 * j, 10.0 * w[1] + np.cos(1.3 * ph) + 0.07 * j])

    def evaluate_samples(self, samples, weights_batch, run_of_task=None):
        assert (run_of_task is None) == (self.run_seeds is None)
        return np.stack([self._objs(self._seed(run_of_task, p), w, -1) for p, w in enumerate(weights_batch)])

    def run(self, task_batch, iteration, num_updates, start_time=None, log=print, run_of_task=None):
        assert (run_of_task is None) == (self.run_seeds is None)
        a = self.args
        total = int(a.num_env_steps) // a.num_steps // a.num_processes
        its = range(iteration, min(iteration + num_updates, total))
        self.calls.append(len(task_batch))
        out = []
        for p, t in enumerate(task_batch):
            seed, w = self._seed(run_of_task, p), t.scalarization.weights.numpy()
            offs = []
            for j in its:
                objs = self._objs(seed, w, j)
                snap = t.sample.snapshot
                new = DeviceSnapshot(self.layout, snap.params + float(objs.sum()) * 1e-3, snap.adam_m, snap.adam_v,
                                     snap.adam_step + 1)
                ep = {'ob_rms': RunningMeanStd(shape=(11,)), 'ret_rms': RunningMeanStd(shape=()),
                      'obj_rms': RunningMeanStd(shape=())}
                ep['obj_rms'].mean = np.float64(objs[0])
                offs.append(Sample.from_snapshot(new, ep, objs=objs))
            out.append(offs)
        for j in its:
            for lg, n in ([(log, len(task_batch))] if callable(log) else
                          [(lg, int(np.sum(np.asarray(run_of_task) == r))) for r, lg in enumerate(log)]):
                lg(f'[RL] Updates {j + 1} (x{n} tasks)')
        return out

    def materialize(self, samples, dst=0):
        return 0


TEXT_FILES = ('ep/objs.txt', 'population/objs.txt', 'population/optgraph.txt', 'elites/elites.txt',
              'elites/weights.txt', 'elites/offsprings.txt')


def _same_text_trees(sweep_dir, solo_dir, method):
    gens = sorted(d for d in os.listdir(solo_dir) if d.isdigit())
    assert gens == ['2', '4', '6'] and sorted(d for d in os.listdir(sweep_dir) if d.isdigit()) == gens
    names = [f'{g}/{f}' for g in gens for f in TEXT_FILES] + ['final/objs.txt', 'final/env_params.txt']
    if method == 'prediction-guided':
        names += [f'{g}/elites/predictions.txt' for g in gens]
    for n in names:
        assert filecmp.cmp(os.path.join(sweep_dir, n), os.path.join(solo_dir, n), shallow=False), n
    assert sorted(os.listdir(os.path.join(sweep_dir, 'final'))) == sorted(os.listdir(os.path.join(solo_dir, 'final')))


@pytest.fixture
def float64_default():
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)  # as pgmorl_amd.run / pgmorl_amd.sweep set it
    yield
    torch.set_default_dtype(prev)


RUNS = [(3, 'random'), (3, 'prediction-guided'), (11, 'random'), (11, 'prediction-guided')]


@pytest.mark.parametrize('max_tasks', [None, 8])
def test_run_many_gives_every_run_the_draws_it_sees_alone(tmp_path, float64_default, max_tasks):
    """Seeds (3, 11) x (random, prediction-guided) in one run_many against each run alone: the warm-up policy draws
    (torch), random_selection and the prediction-guided candidates (numpy) come out of the process-global streams, so a
    draw leaked from one run into another changes a text file."""
    solo_logs = {}
    for s, m in RUNS:
        a = _args(tmp_path / 'solo' / f'{m}_{s}', s, m)
        np.random.seed(12345)  # (whatever the streams hold before: run() seeds them)
        lines = []
        morl.run(a, device='cpu', log=lines.append, runtime=StandIn(a))
        solo_logs[(s, m)] = [x for x in lines if not str(x).startswith('[timing]')]
    args_list = [_args(tmp_path / 'sweep' / f'{m}_{s}', s, m) for s, m in RUNS]
    logs = [[] for _ in RUNS]
    made, info = [], {}

    def make(a, run_seeds):
        made.append(StandIn(a, run_seeds))
        return made[-1]
    eps = morl.run_many(args_list, device='cpu', log=[lg.append for lg in logs], runtime=make, max_tasks=max_tasks,
                        info=info)
    if max_tasks is None:
        assert info['chunks'] == [[0, 1, 2, 3]] and [rt.run_seeds for rt in made] == [[3, 3, 11, 11]]
        assert made[0].calls == [12, 16, 16]  # one runtime call per generation: 3 warm-up tasks, then 4, per run
    else:
        assert info['chunks'] == [[0, 1], [2, 3]] and [rt.run_seeds for rt in made] == [[3, 3], [11, 11]]
        assert made[0].calls == [6, 8, 8]
    assert len(info['boundary_s']) == 4 and info['rl_s'] >= 0 and info['wall_s'] > 0
    for a, lines, ep, (s, m) in zip(args_list, logs, eps, RUNS):
        _same_text_trees(a.save_dir, str(tmp_path / 'solo' / f'{m}_{s}'), m)
        assert [x for x in lines if not str(x).startswith('[timing]')] == solo_logs[(s, m)]
        assert os.path.exists(os.path.join(a.save_dir, 'timing.json')) and ep.timing['train_env_steps'] > 0
    # not vacuous: the two seeds, and the two methods of one seed, end in different archives
    f = [open(os.path.join(a.save_dir, '6', 'elites', 'weights.txt')).read() for a in args_list]
    assert f[0] != f[2] and f[0] != f[1]
