"""CPU-side checks of the hyper-parameter grids: the mixed-row inputs of the GPU tests from the oracle
alone, the refusal order of pgm_ppo_update_tasks / pgm_gae_tasks, TaskBatch.set_task_hparams, the per-run learning
rate, ``sweep --grid`` (layout, order, every refusal with ROOT absent) and run_many(vary=...) on a stand-in runtime.
No kernel is launched here."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest

from pgmorl_amd import _lib, morl, sweep
from pgmorl_amd._lib import PGM_E_INVALID_ARG, PGM_E_SHAPE, PGM_E_UNSUPPORTED, PGMError
from pgmorl_amd.mopg import MOPGPopulation, linear_lr

from . import grid_inputs as gi
from .test_sweep import TINY, StandIn, _args, float64_default  # noqa: F401 (fixture)

ONE = C.c_void_p(1)  # a non-NULL pointer nothing dereferences: every refusal below precedes device work


def _err():
    return _lib.lib().pgm_last_error().decode()


# ------------------------------------------------------------------------------------------------ inputs
@pytest.mark.parametrize('name', list(gi.CASES))
def test_mixed_inputs_meet_the_conditions_at_the_recorded_seeds(name):
    _, results, worst = gi.mixed_case(name)  # asserts conditions + same_decisions of every task under its own row
    assert len(results) == gi.P == 4
    margins = [v for k, v in worst.items() if k.startswith('margin')]
    print(name, 'seed', gi.SEEDS[name], 'smallest margin', min(margins))
    assert min(margins) >= 1e-4
    if name != 'hopper_ln':  # the first seed tried is the recorded one
        assert gi.SEEDS[name] == 11


def test_layernorm_case_fails_at_seed_11():
    """Why the LayerNorm case sits at seed 12: at 11 task 3 (row f) is 8.07e-5 from the max tie at step 2."""
    _, _, bad, _ = gi.evaluate('hopper_ln', 11)
    assert bad and all('task 3' in b and 'max tie' in b for b in bad), bad
    assert gi.SEEDS['hopper_ln'] == 12


@pytest.mark.parametrize('name', gi.SWAP_CHECKED)
def test_mixed_inputs_discriminate_between_the_rows(name):
    """Task p's data under any other task's settings leaves the parameter band by >= 10x: a kernel that read the wrong
    table entry (or the launch's shared values) fails the GPU comparison on every task."""
    f = gi.swap_factors(name)
    assert len(f) == 12
    print(name, 'smallest factor', min(f.values()), 'at', min(f, key=f.get))
    assert min(f.values()) >= 10.0, f


# ------------------------------------------------------------------------------------------------ ABI
def test_version_features_and_symbols():
    L = _lib.lib()
    assert (L.pgm_abi_version(), L.pgm_abi_minor()) == (5, 1)
    assert L.pgm_abi_features() == 7 and L.pgm_abi_feature_mask() == 15
    assert _lib.has_tasks() and all(hasattr(L, s) for s in _lib.TASKS_SYMBOLS)
    assert C.sizeof(C.c_float) * len(_lib.TASK_HPARAM_FIELDS) == 16
    assert _lib.TASK_HPARAM_FIELDS == tuple(n for n, _ in _lib.PPOHParams._fields_[:4])  # hp's first four, in order


def test_ppo_update_tasks_refusals_in_order():
    L = _lib.lib()
    ok = _lib.Dims(4, 4, 64, 11, 3, 2, 64)
    hp = _lib.PPOHParams(0.2, 0.5, 0.0, 0.5, 1e-5, 0.9, 0.999, 0.0, 2, 2, 1, 0)
    rb = _lib.RolloutBuf(*([ONE] * 9))

    def base(d=ok, hp=hp, rb=rb, opts=None, params=ONE, lr=ONE):
        return L.pgm_ppo_update(C.byref(d), C.byref(hp) if hp is not None else None, params, ONE, ONE, ONE, lr, ONE,
                                C.byref(rb), ONE, ONE, opts, None)

    def tasks(d=ok, hp=hp, rb=rb, opts=None, params=ONE, lr=ONE, tab=ONE):
        return L.pgm_ppo_update_tasks(C.byref(d), C.byref(hp) if hp is not None else None, tab, params, ONE, ONE, ONE,
                                      lr, ONE, C.byref(rb), ONE, ONE, opts, None)

    def same(want_rc, want_text, **kw):
        rc0 = base(**kw)
        msg0 = _err()
        assert rc0 == want_rc and want_text in msg0, (kw, rc0, msg0)
        for tab in (ONE, None):  # the earlier item wins, also when the table is missing too
            assert (tasks(tab=tab, **kw), _err()) == (rc0, msg0), (kw, tab, _err())
    # pgm_ppo_update's checks in its order: dims, hidden size, LN, launch opts, NULL pointers, shapes
    same(PGM_E_SHAPE, 'pgm_ppo_update', d=_lib.Dims(0, 4, 64, 11, 3, 2, 64))
    same(PGM_E_UNSUPPORTED, 'hidden size', d=_lib.Dims(4, 4, 64, 11, 3, 2, 32))
    same(PGM_E_UNSUPPORTED, 'pgm_ppo_update', d=_lib.Dims(4, 4, 64, 376, 17, 2, 64, 1))
    same(PGM_E_INVALID_ARG, 'pgm_launch_opts', opts=C.byref(_lib.LaunchOpts(update_kernel=9)))
    same(PGM_E_INVALID_ARG, 'pgm_ppo_update: null pointer', params=None)
    same(PGM_E_INVALID_ARG, 'pgm_ppo_update: null pointer', hp=None)
    same(PGM_E_INVALID_ARG, 'pgm_ppo_update: null pointer', lr=None)
    same(PGM_E_INVALID_ARG, 'pgm_ppo_update: null pointer', rb=_lib.RolloutBuf(*([None] * 9)))
    same(PGM_E_SHAPE, 'num_mini_batch', hp=_lib.PPOHParams(0.2, 0.5, 0.0, 0.5, 1e-5, 0.9, 0.999, 0.0, 2, 0, 1, 0))
    same(PGM_E_SHAPE, 'num_mini_batch', hp=_lib.PPOHParams(0.2, 0.5, 0.0, 0.5, 1e-5, 0.9, 0.999, 0.0, 0, 2, 1, 0))
    same(PGM_E_SHAPE, 'num_mini_batch', d=_lib.Dims(4, 1, 1, 11, 3, 2, 64))  # T N < num_mini_batch
    same(PGM_E_INVALID_ARG, 'pgm_launch_opts', opts=C.byref(_lib.LaunchOpts(update_kernel=9)), params=None)
    # then its own: the NULL table, naming the _tasks entry point, for every tower type and obs_dim family
    for d in (ok, _lib.Dims(4, 4, 64, 11, 3, 2, 64, 1), _lib.Dims(4, 8, 32, 376, 17, 2, 64)):
        assert tasks(d=d, tab=None) == PGM_E_INVALID_ARG and 'pgm_ppo_update_tasks' in _err(), _err()


def test_gae_tasks_refusals_in_order():
    L = _lib.lib()
    ok = _lib.Dims(4, 4, 64, 11, 3, 2, 64)
    rb = _lib.RolloutBuf(*([ONE] * 9))

    def base(d=ok, rb=rb):
        return L.pgm_gae(C.byref(d) if d is not None else None, C.byref(rb), 0.99, 0.95, 1, 1, None)

    def tasks(d=ok, rb=rb, tab=ONE):
        return L.pgm_gae_tasks(C.byref(d) if d is not None else None, C.byref(rb), 0.99, tab, 1, 1, None)
    for want_rc, text, kw in ((PGM_E_INVALID_ARG, 'pgm_gae: null pointer', dict(d=None)),
                              (PGM_E_INVALID_ARG, 'pgm_gae: null pointer', dict(rb=_lib.RolloutBuf(*([None] * 9)))),
                              (PGM_E_SHAPE, 'pgm_gae: bad dims', dict(d=_lib.Dims(0, 4, 64, 11, 3, 2, 64))),
                              (PGM_E_SHAPE, 'N*K <= 64', dict(d=_lib.Dims(4, 33, 64, 11, 3, 2, 64)))):
        rc0 = base(**kw)
        msg0 = _err()
        assert rc0 == want_rc and text in msg0, (kw, rc0, msg0)
        for tab in (ONE, None):
            assert (tasks(tab=tab, **kw), _err()) == (rc0, msg0), (kw, tab)
    assert tasks(tab=None) == PGM_E_INVALID_ARG and 'pgm_gae_tasks' in _err()


# ------------------------------------------------------------------------------------------------ set_task_hparams
def _cpu_batch(P=3, **kw):
    from pgmorl_amd.runtime import TaskBatch
    return TaskBatch('MO-Hopper-v2', P, num_processes=2, num_steps=8, device='cpu', **kw)


def test_set_task_hparams_tables_and_value_checks():
    tb = _cpu_batch(3, capacity=4, clip_param=0.3, gae_lambda=0.9)
    assert tb.hp_task is None and tb.lam_task is None  # never called: the shared settings, the existing entry points
    tb.set_task_hparams(clip_param=[0.1, 0.2, 0.3], entropy_coef=0.01, gae_lambda=[0.0, 0.5, 1.0])
    assert tuple(tb.hp_task.shape) == (4, 4) and tuple(tb.lam_task.shape) == (4,)  # sized for the capacity
    f32 = np.float32
    want = np.array([[0.1, 0.5, 0.01, 0.5], [0.2, 0.5, 0.01, 0.5], [0.3, 0.5, 0.01, 0.5], [0.3, 0.5, 0.0, 0.5]], f32)
    np.testing.assert_array_equal(tb.hp_task.numpy(), want)  # None = the batch's shared value; spare slot: shared
    np.testing.assert_array_equal(tb.lam_task.numpy(), np.array([0.0, 0.5, 1.0, 0.9], f32))
    assert tb.hp_task.data_ptr() % 16 == 0
    before = tb.hp_task.clone(), tb.lam_task.clone()
    for kw, match in ((dict(clip_param=0.0), 'clip_param'), (dict(clip_param=[0.1, -0.2, 0.1]), 'clip_param'),
                      (dict(max_grad_norm=0.0), 'max_grad_norm'), (dict(gae_lambda=1.5), 'gae_lambda'),
                      (dict(gae_lambda=[0.5, -0.1, 0.5]), 'gae_lambda'), (dict(entropy_coef=float('nan')), 'finite'),
                      (dict(value_loss_coef=[0.5, float('inf'), 0.5]), 'finite'),
                      (dict(clip_param=[0.1, 0.2]), 'active tasks'), (dict(clip_param=[[0.1, 0.2, 0.3]]), 'active tasks'),
                      (dict(value_loss_coef='x'), 'value_loss_coef')):
        with pytest.raises(PGMError, match=match):
            tb.set_task_hparams(**kw)
    assert all((a == b).all() for a, b in zip(before, (tb.hp_task, tb.lam_task)))  # a refused call uploads nothing
    tb.set_task_hparams(value_loss_coef=-0.5, entropy_coef=-1.0, gae_lambda=0.0)  # signs of the coefficients are free


def test_iteration_lr_scalar_or_per_task():
    tb = _cpu_batch(3, capacity=4)
    tb.set_lr(3e-4)
    assert tb.lr.tolist() == [float(np.float32(3e-4))] * 3
    lrs = [1e-4, 3e-4 - 3e-4 * (7 / 12.0), 1e-3]
    tb.set_lr(np.asarray(lrs))
    assert tb.lr.tolist() == [float(np.float32(x)) for x in lrs]
    for bad in ([1e-4, 3e-4], [[1e-4, 3e-4, 1e-3]]):
        with pytest.raises(PGMError, match='active tasks'):
            tb.set_lr(bad)


def test_set_task_hparams_refused_on_other_batch_kinds():
    from pgmorl_amd.runtime import TaskBatch
    for env, kw, flag in (('MO-Dummy-v0', {}, 'MO-Dummy'), ('MO-DeepSeaTreasure-v0', dict(device_env=True), 'discrete')):
        tb = TaskBatch(env, 2, num_processes=2, num_steps=8, device='cpu', **kw)
        with pytest.raises(PGMError, match=flag):
            tb.set_task_hparams(clip_param=0.1)
    # the kinds that need a host env or a compiled header to exist: the flags set_task_hparams looks at, on a plain batch
    from pgmorl_amd.runtime import DstMode, HostMode, PluginMode
    for attr, val, flag in (('any_dims', True, 'any_dims'), ('mode', PluginMode, 'env_plugin'),
                            ('mode', DstMode, 'device_env'), ('mode', HostMode, 'host_env'),
                            ('discrete', True, 'discrete')):
        tb = _cpu_batch(2)
        setattr(tb, attr, val)
        with pytest.raises(PGMError, match=flag):
            tb.set_task_hparams(clip_param=0.1)
        assert tb.hp_task is None


# ------------------------------------------------------------------------------------------------ per-run lr
@pytest.mark.parametrize('decay,ratio', [(True, 1.0), (False, 1.0), (True, 0.5)])
def test_per_run_lr_is_the_solo_expression_rounded_to_fp32(decay, ratio):
    a = argparse.Namespace(env_name='MO-Hopper-v2', lr=3e-4, lr_decay_ratio=ratio, use_linear_lr_decay=decay,
                           gae_lambda=0.95, clip_param=0.2, value_loss_coef=0.5, entropy_coef=0.0, max_grad_norm=0.5)
    runs = [dict(lr=1e-4), dict(lr=3e-4), dict(lr=1e-3, lr_decay_ratio=0.25), {}]
    rt = MOPGPopulation(a, device='cpu', run_seeds=[0, 1, 2, 3], run_hparams=runs)
    total = 611
    rot = [3, 0, 0, 2, 1, 2]
    for j in (0, total // 2, total - 1):
        got = rt.task_lr(rot, j, total)
        assert got.dtype == np.float32 and got.shape == (6,)
        for p, r in enumerate(rot):
            lr0, rr = runs[r].get('lr', a.lr), runs[r].get('lr_decay_ratio', ratio)
            solo = linear_lr(j, total, lr0, rr) if decay else lr0  # MOPGPopulation.run's expression, Python floats
            assert got[p] == np.float32(solo), (j, p)
            # what a solo run uploads: lr.fill_(float(lr)) rounds the same double to fp32
            import torch
            assert float(torch.zeros(1, dtype=torch.float32).fill_(float(solo))[0]) == float(got[p])
    tab = rt.task_hparams(rot)
    assert tab['clip_param'] == [0.2] * 6 and set(tab) == {'gae_lambda', 'clip_param', 'value_loss_coef',
                                                           'entropy_coef', 'max_grad_norm'}


def test_run_hparams_are_checked():
    a = argparse.Namespace(env_name='MO-Hopper-v2')
    for runs, match in (([dict(clip_param=0.0), {}], 'clip_param'), ([dict(gamma=0.9), {}], 'gamma'),
                        ([dict(lr=float('nan')), {}], 'lr'), ([{}], 'one dict per run')):
        with pytest.raises(PGMError, match=match):
            MOPGPopulation(a, device='cpu', run_seeds=[0, 1], run_hparams=runs)
    with pytest.raises(PGMError, match='one dict per run'):
        MOPGPopulation(a, device='cpu', run_hparams=[{}])


# ------------------------------------------------------------------------------------------------ plan() with grids
def test_plan_without_a_grid_is_unchanged(tmp_path):
    root = tmp_path / 'ROOT'
    opts, base, runs = sweep.plan(['--pgmorl', '--ra', '--num-seeds', '2', '--save-dir', str(root), '--', *TINY])
    want = []
    for i, seed in enumerate((815117, 449815)):
        for flag, m in (('pgmorl', 'prediction-guided'), ('ra', 'ra')):
            want.append((flag, i, TINY + ['--seed', str(seed), '--selection-method', m, '--save-dir',
                                          os.path.join(str(root), flag, str(i))]))
    assert runs == want and opts.vary == () and opts.grid is None
    assert not root.exists()


def test_plan_with_grids_layout_and_order(tmp_path):
    root = tmp_path / 'ROOT'
    opts, base, runs = sweep.plan(['--pgmorl', '--ra', '--num-seeds', '2', '--grid', 'lr', '1e-4', '3e-4', '1e-3',
                                   '--grid', 'clip-param', '0.1', '0.2', '--save-dir', str(root), '--', *TINY])
    assert opts.vary == ('lr', 'clip_param')
    points = [f'lr={a},clip-param={b}' for a in ('0.0001', '0.0003', '0.001') for b in ('0.1', '0.2')]
    # grid point outermost, then seed index, then method; the first element is <method>/<point>
    want = [(f'{m}/{pt}', i) for pt in points for i in (0, 1) for m in ('pgmorl', 'ra')]
    assert [(top, i) for top, i, _ in runs] == want
    from pgmorl_amd.run import get_parser, merge_argv
    parsed = [get_parser().parse_args(merge_argv(argv)) for _, _, argv in runs]
    assert [a.save_dir for a in parsed] == [os.path.join(str(root), top, str(i)) for top, i, _ in runs]
    assert [(a.lr, a.clip_param) for a in parsed] == [(x, y) for x in (1e-4, 3e-4, 1e-3) for y in (0.1, 0.2)
                                                      for _ in range(4)]
    assert [a.seed for a in parsed] == [815117, 815117, 449815, 449815] * 6
    assert all(a.use_linear_lr_decay and a.num_steps == 8 for a in parsed)  # run's defaults still merged
    morl.check_sweep_args(parsed, opts.vary)
    with pytest.raises(ValueError, match="'clip_param'"):
        morl.check_sweep_args(parsed, ('lr',))
    # the field's name with underscores is the same flag; one grid of one value is a grid
    _, _, r1 = sweep.plan(['--pgmorl', '--seeds', '5', '--grid', 'gae_lambda', '0.9', '--save-dir', str(root), '--',
                           *TINY])
    assert [(t, i) for t, i, _ in r1] == [('pgmorl/gae-lambda=0.9', 0)]
    assert not root.exists()


@pytest.mark.parametrize('own,rest,match', [
    (['--grid', 'gamma', '0.99', '0.995'], [], r'--grid gamma.*return normalisation'),
    (['--grid', 'num-steps', '8', '16'], [], r'--grid num-steps.*shape'),
    (['--grid', 'num-processes', '2'], [], r'--grid num-processes.*shape'),
    (['--grid', 'ppo-epoch', '2'], [], r'--grid ppo-epoch.*shape'),
    (['--grid', 'num-mini-batch', '2'], [], r'--grid num-mini-batch.*shape'),
    (['--grid', 'adam-eps', '1e-5'], [], r'--grid adam-eps: unknown'),
    (['--grid', 'seed', '1', '2'], [], r'--grid seed: unknown'),
    (['--grid', 'lr', '1e-4'], ['--lr', '3e-4'], r'--grid lr and --lr after'),
    (['--grid', 'clip-param', '0.1'], ['--clip-p', '0.3'], r'--grid clip-param and --clip-p after'),
    (['--grid', 'lr', '1e-4', '--grid', 'lr', '3e-4'], [], r'--grid lr given twice'),
    (['--grid', 'lr'], [], r'--grid lr: no values'),
    (['--grid', 'lr', '1e-3', '0.001'], [], r'--grid lr: the value 0.001 is listed twice'),
    (['--grid', 'lr', 'fast'], [], r"--grid lr: 'fast' is not a number"),
    (['--grid', 'lr', 'inf'], [], r'--grid lr: inf must be finite'),
    (['--grid', 'clip-param', '0.1', '0'], [], r'--grid clip-param.*> 0'),
    (['--grid', 'max-grad-norm', '-1'], [], r'--grid max-grad-norm.*> 0'),
    (['--grid', 'gae-lambda', '0.9', '1.1'], [], r'--grid gae-lambda.*\[0, 1\]'),
    (['--grid', 'entropy-coef', 'nan'], [], r'--grid entropy-coef.*finite'),
])
def test_grid_refusals_leave_root_absent(tmp_path, own, rest, match):
    root = tmp_path / 'ROOT'
    with pytest.raises(PGMError, match=match):
        sweep.main(['--pgmorl', *own, '--save-dir', str(root), '--', *TINY, *rest])
    assert not root.exists()


def test_lr_after_the_dashes_is_not_the_decay_ratio_grid(tmp_path):
    """--lr is a flag of its own, not a prefix of --lr-decay-ratio: both may be given."""
    _, _, runs = sweep.plan(['--pgmorl', '--seeds', '5', '--grid', 'lr-decay-ratio', '0.5', '1', '--save-dir',
                             str(tmp_path / 'ROOT'), '--', *TINY, '--lr', '1e-3'])
    assert [t for t, _, _ in runs] == ['pgmorl/lr-decay-ratio=0.5', 'pgmorl/lr-decay-ratio=1.0']


# ------------------------------------------------------------------------------------------------ run_many(vary=...)
class GridStandIn(StandIn):
    """StandIn that records the per-task tables a MOPGPopulation would upload, expanded through run_of_task."""

    def __init__(self, args, run_seeds, run_hparams=None):
        super().__init__(args, run_seeds)
        self.run_hparams = run_hparams
        self.tables = []

    def run(self, task_batch, iteration, num_updates, start_time=None, log=print, run_of_task=None):
        total = int(self.args.num_env_steps) // self.args.num_steps // self.args.num_processes
        self.tables.append((list(run_of_task), MOPGPopulation.task_hparams(self, run_of_task),
                            MOPGPopulation.task_lr(self, run_of_task, iteration, total)))
        return super().run(task_batch, iteration, num_updates, start_time, log, run_of_task)

    run_lr = MOPGPopulation.run_lr


def test_run_many_vary(tmp_path, float64_default):
    lrs = (3e-4, 1e-3, 1e-4)
    args_list = [_args(tmp_path / f'r{i}', 3, 'random', ['--lr', repr(lr), '--clip-param', repr(cp)])
                 for i, (lr, cp) in enumerate(zip(lrs, (0.2, 0.1, 0.3)))]
    # without vary the refusal and its message are what they were
    with pytest.raises(ValueError, match=r"run 1 differs from run 0 in 'clip_param' .*seed, selection_method, save_dir only"):
        morl.run_many(args_list, device='cpu')
    with pytest.raises(ValueError, match="'lr'"):
        morl.run_many(args_list, device='cpu', vary=('clip_param',))
    with pytest.raises(ValueError, match="vary='gamma'"):
        morl.run_many(args_list, device='cpu', vary=('lr', 'gamma'))
    with pytest.raises(ValueError, match="vary='num_steps'"):
        morl.run_many(args_list, device='cpu', vary=('num_steps',))
    assert not any((tmp_path / f'r{i}').exists() for i in range(3))
    made, info = [], {}

    def make(a, run_seeds, run_hparams=None):
        made.append(GridStandIn(a, run_seeds, run_hparams))
        return made[-1]
    # 4 tasks per run, at most 8 per launch: runs (0, 1) and (2) -- the tables follow the chunk's own run indices
    morl.run_many(args_list, device='cpu', runtime=make, max_tasks=8, info=info, vary=('lr', 'clip_param'))
    assert info['chunks'] == [[0, 1], [2]]
    assert [rt.run_hparams for rt in made] == [[dict(lr=3e-4, clip_param=0.2), dict(lr=1e-3, clip_param=0.1)],
                                               [dict(lr=1e-4, clip_param=0.3)]]
    total = int(args_list[0].num_env_steps) // 8 // 2
    for rt, runs in zip(made, ([0, 1], [2])):
        assert rt.calls == [3 * len(runs), 4 * len(runs), 4 * len(runs)]
        for (rot, tab, lr), it in zip(rt.tables, (0, 2, 4)):
            n = len(rot) // len(runs)
            assert rot == [r for r in range(len(runs)) for _ in range(n)]  # task order = run order
            assert tab['clip_param'] == [args_list[runs[r]].clip_param for r in rot]
            assert tab['max_grad_norm'] == [0.5] * len(rot) and tab['gae_lambda'] == [0.95] * len(rot)
            want = [np.float32(linear_lr(it, total, args_list[runs[r]].lr, 1.0)) for r in rot]
            assert lr.tolist() == [float(x) for x in want]
    # vary=() passes no run_hparams: a two-argument factory still works
    same = [_args(tmp_path / f's{i}', 3, m) for i, m in enumerate(('random', 'ra'))]
    morl.run_many(same, device='cpu', runtime=lambda a, run_seeds: StandIn(a, run_seeds))
