"""Per-task PPO settings on the device: pgm_ppo_update_tasks on each of the eight update kernels and
pgm_gae_tasks against the entry points they extend (bit for bit) and against the fp64 oracle, then a 2 x 2
hyper-parameter grid through run_many(vary=...) and ``python -m pgmorl_amd.sweep --grid`` against the solo runs.

The mixed inputs are tests/grid_inputs.py's (four tasks under rows a, c, d, f of branch_inputs.ROWS, seeds and
discrimination checked from the oracle alone, tests/test_grid.py); the kernels are forced and asserted with the knobs of
tests/test_gpu_update_branches.py, whose bands are used unchanged.  Every forced placement takes P = 4 on a device of
>= 64 CUs (the widest grid is the 16-row tiles': 16 x 4 x ceil(4 / 8) = 64 workgroups), so no case is split in two.
"""
import ctypes as C
import filecmp
import functools
import os

import numpy as np
import pytest
import torch

from oracle import ppo as oppo
from pgmorl_amd import _lib
from pgmorl_amd._lib import Dims, RolloutBuf
from pgmorl_amd.runtime import TaskBatch

from . import branch_inputs as bi
from . import grid_inputs as gi
from .test_gpu_kernels import _close, _random_storage
from .test_gpu_returns import FLAGS, GAMMA, LAM, PAD, SENTINEL, _dev, _ptr, _stream
from .test_gpu_runs import LOOP_ENV, _Env, _files, _log_text, _loop_args
from .test_gpu_update_branches import KERNELS

pytestmark = pytest.mark.gpu

# kernel -> (its uniform-table case of branch_inputs.oracle_case, its mixed cases of grid_inputs)
CASES = {k: (('hopper2', False), ('hopper',)) for k in ('fs', 'mfma4', 'mfma2', 'mfma1', 'mfma0', 'valu')}
CASES['fs'] = (('hopper2', False), ('hopper', 'walker'))
CASES['wide'] = CASES['wide1'] = CASES['wide2'] = (('humanoid32', False), ('humanoid',))
CASES['ln'] = (('hopper2', True), ('hopper_ln',))
MIXED = [(k, c) for k, (_, cs) in CASES.items() for c in cs]
ARRAYS = ('params', 'adam_m', 'adam_v', 'adam_step', 'stats')
TABLE_SENTINEL, ROW_SENTINEL = -4321.0, -123.0


def _knobs(kernel):
    knob, split, _, _ = KERNELS[kernel]
    env = {}
    for name, val in (('PGM_UPDATE_KERNEL', knob), ('PGM_UPDATE_SPLIT', split)):
        if val is not None:
            env[name] = val
    return env


class _Knobs(_Env):
    """The kernel's launch knobs in the environment, the other one removed."""

    def __init__(self, kernel):
        super().__init__(_knobs(kernel))

    def __enter__(self):
        self.gone = {k: os.environ.pop(k) for k in ('PGM_UPDATE_KERNEL', 'PGM_UPDATE_SPLIT')
                     if k in os.environ and k not in self.env}
        super().__enter__()

    def __exit__(self, *exc):
        super().__exit__(*exc)
        os.environ.update(self.gone)


def _variant_ok(kernel, got):
    variant = KERNELS[kernel][2]
    assert got.startswith(variant) if variant.endswith('(') else got == variant, got


def _launch(kernel, shape, ln, hp, pols, data, perms, table=None, capacity=None):
    """One update of the P tasks under the shared hp (table=None: pgm_ppo_update) or with a per-task table (a dict of
    set_task_hparams' arguments: pgm_ppo_update_tasks) -> {array: CPU tensor}, plus the spare slot with capacity."""
    env, P, T, N, E, M = shape
    with _Knobs(kernel):
        tb = TaskBatch(env, P, num_processes=N, num_steps=T, ppo_epoch=E, num_mini_batch=M, layernorm=ln,
                       clip_param=hp['clip_param'], value_loss_coef=hp['value_loss_coef'],
                       entropy_coef=hp['entropy_coef'], max_grad_norm=hp['max_grad_norm'],
                       use_clipped_value_loss=hp['use_clipped_value_loss'], capacity=capacity)
        tb.hp.adam_eps, tb.hp.beta1, tb.hp.beta2 = hp['adam_eps'], hp['beta1'], hp['beta2']
        _variant_ok(kernel, tb.update_variant())
        for p, pol in enumerate(pols):
            tb.set_task(p, pol.state_dict())
        obs, actions, logp, values, returns, adv = data
        for dst, src in ((tb.obs, torch.from_numpy(obs)), (tb.actions, actions), (tb.logp, logp), (tb.values, values),
                         (tb.returns, returns), (tb.adv, adv)):
            dst.copy_(src)
        tb.lr.fill_(bi.LR)
        if table is not None:
            tb.set_task_hparams(**table)
            assert tb.hp_task is not None and tuple(tb.hp_task.shape) == (tb.capacity, 4)
        if capacity is not None:  # a sentinel in the spare table entry and in every spare state row
            assert tb.capacity == P + 1
            tb.hp_task[P] = TABLE_SENTINEL
            tb._state[:, P] = ROW_SENTINEL
            tb._full['adam_step'][P] = 77
            tb._full['stats'][P] = ROW_SENTINEL
        tb.ppo_update(torch.stack(perms).numpy())
        assert int(tb.update_ws[2 * P]) == 0, 'workspace word 2P: an exchange timed out'
        tb.check_update()
        out = {k: getattr(tb, k).cpu().clone() for k in ARRAYS}
        out['layout'] = tb.layout
        if capacity is not None:
            out['spare'] = {'table': tb.hp_task[P].cpu(), 'state': tb._state[:, P].cpu(),
                            'adam_step': int(tb._full['adam_step'][P]), 'stats': tb._full['stats'][P].cpu()}
    return out


def _uniform_table(hp):
    return {k: hp[k] for k in ('clip_param', 'value_loss_coef', 'entropy_coef', 'max_grad_norm')}


def _mixed_table():
    return {k: [gi.hp_of(p)[k] for p in range(gi.P)] for k in ('clip_param', 'value_loss_coef', 'entropy_coef',
                                                               'max_grad_norm')}


# ------------------------------------------------------------------------------------------------ 1. uniform table
@pytest.mark.parametrize('kernel', list(CASES))
def test_uniform_table_equals_the_plain_entry_point(gpu, kernel):
    (shape_name, ln), _ = CASES[kernel]
    (args, spec, pols, data, perms), _, _ = bi.oracle_case(shape_name, ln, 'a')
    hp, shape = bi.hparams('a'), bi.SHAPES[shape_name]
    plain = _launch(kernel, shape, ln, hp, pols, data, perms)
    tasks = _launch(kernel, shape, ln, hp, pols, data, perms, table=_uniform_table(hp))
    for k in ARRAYS:
        assert torch.equal(plain[k], tasks[k]), f'{kernel}: {k} differs between pgm_ppo_update and the uniform table'
    assert int(plain['adam_step'][0]) == shape[4] * shape[5]


# ------------------------------------------------------------------------------------------------ 2.-4. mixed table
@functools.lru_cache(maxsize=None)
def _mixed_tasks_launch(kernel, case):
    """The one pgm_ppo_update_tasks launch of a mixed case (capacity P + 1, sentinels in the spare slot), shared by the
    comparisons below.  The shared hp of the launch is row a's with the four per-task fields set to values no row has,
    so a kernel that read them from hp instead of the table fails every comparison."""
    (args, spec, pols, data, perms), results, _ = gi.mixed_case(case)
    hp = dict(bi.hparams('a'), clip_param=0.37, value_loss_coef=0.91, entropy_coef=0.23, max_grad_norm=3.3)
    return _launch(kernel, gi.shape_of(case), gi.CASES[case][5], hp, pols, data, perms, table=_mixed_table(),
                   capacity=gi.P + 1)


@pytest.mark.parametrize('kernel,case', MIXED)
def test_mixed_table_equals_one_plain_launch_per_row(gpu, kernel, case):
    (args, spec, pols, data, perms), _, _ = gi.mixed_case(case)
    got = _mixed_tasks_launch(kernel, case)
    for p in range(gi.P):
        plain = _launch(kernel, gi.shape_of(case), gi.CASES[case][5], gi.hp_of(p), pols, data, perms)
        for k in ARRAYS:
            assert torch.equal(got[k][p], plain[k][p]), \
                f'{kernel} {case}: {k} of task {p} (row {gi.ROWS[p]}) differs from the plain launch under that row'
    # not vacuous: under row a's settings the other tasks end elsewhere (the last plain launch is row f's)
    assert not torch.equal(got['params'][0], plain['params'][0])


@pytest.mark.parametrize('kernel,case', MIXED)
def test_mixed_table_against_the_oracle(gpu, kernel, case):
    (args, spec, pols, data, perms), results, _ = gi.mixed_case(case)
    got = _mixed_tasks_launch(kernel, case)
    lay = got['layout']
    _, _, _, _, E, M = gi.shape_of(case)
    params, am, av = got['params'].numpy(), got['adam_m'].numpy(), got['adam_v'].numpy()
    what = f'{kernel} {case}'
    for p, (pol, agent, st, _) in enumerate(results):  # results[p]: bi.run_oracle(pols[p], hparams(row_p), ...)
        ref = lay.flatten(pol.state_dict(), dtype=np.float64)
        m_ref, v_ref, step = lay.adam_from_optimizer_state(agent.optimizer.state_dict()['state'])
        for name, g, r, atol, rtol in (('params', params[p], ref, 2e-6, 1e-5), ('exp_avg', am[p], m_ref, 1e-7, 1e-3),
                                       ('exp_avg_sq', av[p], v_ref, 1e-10, 1e-3),
                                       ('loss stats', got['stats'][p].numpy(), st, 1e-5, 1e-4)):
            err = np.abs(np.asarray(g, np.float64) - r)
            print(f'{what} task {p} row {gi.ROWS[p]}: {name} max abs err {err.max():.3e}, '
                  f'{(err / (atol + rtol * np.abs(r))).max():.3f} of the band')
        assert int(got['adam_step'][p]) == step == E * M
        _close(params[p], ref, 2e-6, 1e-5, f'{what} task {p}: params')
        _close(am[p], m_ref, 1e-7, 1e-3, f'{what} task {p}: exp_avg')
        _close(av[p], v_ref, 1e-10, 1e-3, f'{what} task {p}: exp_avg_sq')
        _close(got['stats'][p], st, 1e-5, 1e-4, f'{what} task {p}: loss stats')
        if kernel == 'ln' and gi.ROWS[p] == 'f':  # the entropy term's own gradient: the logstd slice of exp_avg
            o, A = lay.offsets['logstd'], spec['act_dim']
            assert np.abs(am[p][o:o + A]).min() > 0
            _close(am[p][o:o + A], m_ref[o:o + A], 1e-7, 1e-3, f'{what} task {p}: exp_avg logstd')


@pytest.mark.parametrize('kernel,case', MIXED)
def test_spare_slot_is_untouched(gpu, kernel, case):
    """capacity P + 1: neither the spare table entry is written nor the spare task's rows (its entry holds a value
    that would turn every parameter it touched into something else)."""
    spare = _mixed_tasks_launch(kernel, case)['spare']
    assert (spare['table'] == TABLE_SENTINEL).all()
    assert (spare['state'] == ROW_SENTINEL).all() and (spare['stats'] == ROW_SENTINEL).all()
    assert spare['adam_step'] == 77


# ------------------------------------------------------------------------------------------------ 5. pgm_gae_tasks
LAMS = (0.0, 0.9, 0.95, 1.0)


def _gae_call(gpu, storage, use_gae, proper, lam_task=None):
    """pgm_gae (lam_task None) or pgm_gae_tasks on [P][T][N][K] storage -> (returns [P][T+1][N][K] pre-filled with
    the sentinel, the sentinel words behind it)."""
    rew, val, masks, bad = storage
    P, T, N, K = rew.shape
    flat = torch.full((P * (T + 1) * N * K + PAD,), SENTINEL, device=gpu)
    t = [_dev(x, gpu) for x in (rew, val, masks, bad)]
    rb = RolloutBuf(values=_ptr(t[1]), rewards=_ptr(t[0]), masks=_ptr(t[2]), bad_masks=_ptr(t[3]), returns=_ptr(flat))
    d = Dims(P, N, T, 11, 3, K, 64, 0)
    if lam_task is None:
        rc = _lib.lib().pgm_gae(C.byref(d), C.byref(rb), GAMMA, LAM, int(use_gae), int(proper), _stream())
        _lib.check(rc, 'pgm_gae')
    else:
        tab = torch.full((P + 1,), float('nan'), device=gpu)  # the entry behind the table is never read
        tab[:P] = torch.tensor(lam_task, dtype=torch.float32)
        rc = _lib.lib().pgm_gae_tasks(C.byref(d), C.byref(rb), GAMMA, _ptr(tab), int(use_gae), int(proper), _stream())
        _lib.check(rc, 'pgm_gae_tasks')
    out = flat.cpu().numpy()
    return out[:-PAD].reshape(P, T + 1, N, K), out[-PAD:]


def _check_gae_tasks(gpu, storage, use_gae, proper, what):
    rew, val, masks, bad = storage
    P, T = rew.shape[0], rew.shape[1]
    assert P == len(LAMS)
    got, tail = _gae_call(gpu, storage, use_gae, proper, LAMS)
    for p, lam in enumerate(LAMS):
        r, v = torch.from_numpy(rew[p]).double(), torch.from_numpy(val[p]).double()
        m = torch.from_numpy(masks[p]).double().unsqueeze(-1)
        b = torch.from_numpy(bad[p]).double().unsqueeze(-1)
        ret = torch.zeros(T + 1, rew.shape[2], rew.shape[3], dtype=torch.float64)
        oppo.compute_returns_inplace(r, v.clone(), m, b, ret, v[-1], use_gae, GAMMA, lam, proper)
        _close(got[p, :T], ret.numpy()[:T], 1e-5, 1e-5, f'returns {what} task {p} lam {lam}')
    if use_gae:
        assert (got[:, T] == SENTINEL).all(), 'GAE wrote returns[T]'
    else:
        np.testing.assert_array_equal(got[:, T], val[:, T])
    assert (tail == SENTINEL).all(), 'pgm_gae_tasks wrote past the returns'
    # every entry equal to LAM: pgm_gae's result bit for bit
    same, _ = _gae_call(gpu, storage, use_gae, proper, (LAM,) * P)
    plain, _ = _gae_call(gpu, storage, use_gae, proper)
    assert np.array_equal(same, plain), f'{what}: a uniform table differs from pgm_gae'
    if use_gae and T > 1:  # not vacuous: lambda matters under GAE (and only there)
        assert not np.array_equal(got[0, :T], plain[0, :T])


@pytest.mark.parametrize('use_gae,proper', FLAGS)
@pytest.mark.parametrize('N,K,T', [(4, 2, 1), (21, 3, 17), (4, 3, 2048)])
def test_gae_tasks_lane_and_chunk_edges(gpu, use_gae, proper, N, K, T):
    _check_gae_tasks(gpu, _random_storage(4, T, N, K, seed=T + N), use_gae, proper, f'N={N} K={K} T={T}')


@pytest.mark.parametrize('use_gae,proper', FLAGS)
def test_gae_tasks_mask_patterns(gpu, use_gae, proper):
    """tests/test_gpu_returns.py's mask patterns (done at every step; time-limit cuts; dones on chunk boundaries) on four
    tasks, each with its own lambda."""
    P, N, K, T = 4, 4, 3, 2048
    rew, val, masks, bad = _random_storage(P, T, N, K, seed=21)
    chunk = -(-T // (1024 // (N * K)))
    assert chunk == 25
    masks[:, :, 0] = 0.0
    bad[:, :, 0] = 1.0
    masks[:, :, 1], bad[:, :, 1] = 1.0, 1.0
    bad[:, [1, T], 1] = 0.0
    masks[:, 1, 1] = 0.0
    masks[:, :, 2], bad[:, :, 2] = 1.0, 1.0
    masks[:, [chunk, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1, 40 * chunk, 81 * chunk, T - 1], 2] = 0.0
    bad[:, 40 * chunk, 2] = 0.0
    _check_gae_tasks(gpu, (rew, val, masks, bad), use_gae, proper, 'mask patterns')


# ------------------------------------------------------------------------------------------------ 6. end to end
GRID = [(3e-4, 0.2), (3e-4, 0.1), (1e-3, 0.2), (1e-3, 0.1)]  # lr outermost, as --grid lr ... --grid clip-param ...
GRID_SEED, GRID_METHOD = 5, 'prediction-guided'


def _grid_args(save_dir, lr, clip):
    return _loop_args(save_dir, GRID_SEED, GRID_METHOD, extra=('--lr', repr(lr), '--clip-param', repr(clip)))


@pytest.fixture(scope='module')
def solo_grid_trees(gpu, tmp_path_factory):
    """The four solo morl.run trees, one per grid point (one workgroup per task in the update), computed once."""
    from pgmorl_amd.mopg import MOPGPopulation
    from pgmorl_amd.morl import run
    root = tmp_path_factory.mktemp('solo_grid')
    out = {}
    with _Env(LOOP_ENV):
        for lr, clip in GRID:
            a = _grid_args(root / f'{lr}_{clip}', lr, clip)
            rt = MOPGPopulation(a, device='cuda', rng='host')
            lines = []
            run(a, device='cuda', rng='host', log=lines.append, runtime=rt)
            out[(lr, clip)] = (a.save_dir, _log_text(lines), rt.tb.update_variant())
    return out


def _assert_tree(save_dir, solo_dir, what, skip=('timing.json',)):
    names = _files(solo_dir)
    assert [n for n in _files(save_dir) if n not in ('args.txt', 'log.txt')] == names, what
    assert any(n.endswith('EP_policy_0.pt') for n in names)
    for n in names:
        if n not in skip:
            assert filecmp.cmp(os.path.join(save_dir, n), os.path.join(solo_dir, n), shallow=False), (what, n)


def test_grid_run_many_trees_equal_the_solo_runs(gpu, tmp_path, solo_grid_trees):
    from pgmorl_amd.mopg import MOPGPopulation
    from pgmorl_amd.morl import run_many
    args_list = [_grid_args(tmp_path / f'{lr}_{clip}', lr, clip) for lr, clip in GRID]
    logs = [[] for _ in args_list]
    rts, info = [], {}

    def make(a, run_seeds, run_hparams=None):
        rts.append(MOPGPopulation(a, device='cuda', rng='host', run_seeds=run_seeds, run_hparams=run_hparams))
        return rts[-1]
    with _Env(LOOP_ENV):
        run_many(args_list, device='cuda', rng='host', log=[lg.append for lg in logs], runtime=make, info=info,
                 vary=('lr', 'clip_param'))
        variants = [rt.tb.update_variant() for rt in rts]
    assert info['chunks'] == [[0, 1, 2, 3]] and info['generations'][0]['tasks'] == 3 * len(GRID)
    assert rts[0].tb.hp_task is not None and rts[0].tb.lam_task is not None  # the _tasks entry points ran
    assert rts[0].run_hparams == [dict(lr=lr, clip_param=clip) for lr, clip in GRID]
    for a, lines, point in zip(args_list, logs, GRID):
        solo_dir, solo_log, solo_variant = solo_grid_trees[point]
        assert variants == [solo_variant], (variants, solo_variant)
        _assert_tree(a.save_dir, solo_dir, point)
        assert _log_text(lines) == solo_log, point
    # not vacuous: the learning rates end in different archives, and so do the two clip_params of at least one of them
    # (four iterations of one epoch x two minibatches: at the smaller lr the ratio may stay inside both clip ranges)
    f = [open(os.path.join(a.save_dir, 'final', 'objs.txt')).read() for a in args_list]
    assert f[0] != f[2] and f[1] != f[3] and (f[0] != f[1] or f[2] != f[3])


def test_grid_sweep_command_line(gpu, tmp_path, solo_grid_trees):
    import json

    from pgmorl_amd import sweep
    a = _grid_args('unused', 3e-4, 0.2)
    root = tmp_path / 'root'
    prev = torch.get_default_dtype()
    try:
        with _Env(LOOP_ENV):
            sweep.main(['--pgmorl', '--seeds', str(GRID_SEED), '--grid', 'lr', '3e-4', '1e-3', '--grid', 'clip-param',
                        '0.2', '0.1', '--save-dir', str(root), '--', '--env-name', a.env_name, '--obj-num', '2',
                        '--num-steps', str(a.num_steps), '--num-processes', str(a.num_processes), '--ppo-epoch', '1',
                        '--num-mini-batch', '2', '--num-env-steps', str(a.num_env_steps), '--warmup-iter', '2',
                        '--update-iter', '1', '--delta-weight', '0.5', '--rl-log-interval', '1', '--rng', 'host',
                        '--pbuffer-num', str(a.pbuffer_num)])
    finally:
        torch.set_default_dtype(prev)
    dirs = [f'pgmorl/lr={lr!r},clip-param={clip!r}/0' for lr, clip in GRID]
    assert sorted(os.listdir(root / 'pgmorl')) == sorted(d.split('/')[1] for d in dirs)
    st = json.load(open(root / 'sweep_timing.json'))
    assert st['runs'] == 4 and st['dirs'] == dirs and st['chunks'] == [[0, 1, 2, 3]]
    for d, point in zip(dirs, GRID):
        solo_dir, solo_log, _ = solo_grid_trees[point]
        _assert_tree(str(root / d), solo_dir, point)
        assert f"'--lr', '{point[0]!r}', '--clip-param', '{point[1]!r}'" in open(root / d / 'args.txt').read()
        # (the command line sets torch's default dtype to float64, as pgmorl_amd.run does: its log prints the same
        # fp64 tensors without the dtype suffix the fixture's runs print)
        log = open(root / d / 'log.txt').read().rstrip('\n')
        assert _log_text(log.split('\n')) == solo_log.replace(', dtype=torch.float64', ''), point
