"""Several runs of a sweep in one device population: pgm_env_reset_runs / pgm_rollout_runs / pgm_eval_runs against
the existing entry points (bit for bit) and the CPU oracle (the bands of tests/test_gpu_kernels.py), and morl.run_many /
``python -m pgmorl_amd.sweep`` against solo morl.run trees (byte for byte).

Shapes: P = 5 tasks with run_of_task = [0, 1, 1, 0, 2] (non-contiguous, non-monotone, the last run used once), run
seeds (0, 7, 815117), T = 64 with the episode limit cut to 20 steps (every env auto-resets three times and every
evaluation episode is 20 steps), N in {1, 3, 4} (lane kernel N = 1, 4; N = 3 is the block kernel's) and, for Humanoid,
N in {1, 2, 4} (the wide kernel; N >= 2 takes its half-block env index) plus 3 (block); eval_num 1 (N = 1) or 3."""
import filecmp
import os
import re

import numpy as np
import pytest
import torch

from oracle import ppo as oppo
from oracle.mopg import evaluation as oracle_evaluation
from oracle.policy import make_policy
from oracle.vecenv import RunningMeanStd, VecNormalizedSynth
from pgmorl_amd import envspec
from pgmorl_amd.runtime import TaskBatch

from .helpers import perturb, small_args
from .test_gpu_kernels import _close, _oracle_rollout, _teacher_forced_check

pytestmark = pytest.mark.gpu

SEEDS = (0, 7, 815117)
RUNS = [0, 1, 1, 0, 2]
T, STEPS = 64, 20
# (env, layernorm): dims 17/6/2, 11/3/3, 376/17/2 and LayerNorm 11/3/2
FAMILIES = [('MO-Walker2d-v2', False), ('MO-Hopper-v3', False), ('MO-Humanoid-v2', False), ('MO-Hopper-v2', True)]
CASES = [(env, ln, N, kernel) for env, ln in FAMILIES for N in ((1, 2, 4, 3) if 'Humanoid' in env else (1, 3, 4))
         for kernel in (('auto',) if ln else ('auto', 'block'))]  # (LayerNorm: one kernel family, opts ignored)
FIELDS = ('obs', 'actions', 'logp', 'values', 'rewards', 'masks', 'bad_masks', 's', 'elapsed', 'obj_acc', 'obj_valid',
          'ret', 'weights', 'ob_mean', 'ob_var', 'ob_count', 'ret_mean', 'ret_var', 'ret_count', 'obj_mean', 'obj_var',
          'obj_count')


def _policies(env, ln, P, seed=3):
    spec = envspec.make_spec(env)
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed + 100)
    pols = []
    for _ in range(P):
        pol = make_policy(spec['obs_dim'], spec['act_dim'], spec['obj_num'], layernorm=ln)
        with torch.no_grad():
            for prm in pol.parameters():
                prm.copy_(prm.float().double())
        pols.append(perturb(pol, 0.05, gen))
    return spec, pols


def _batch(env, ln, pols, N, eval_num, stats=None, **kw):
    tb = TaskBatch(env, len(pols), num_processes=N, num_steps=T, eval_num=eval_num, layernorm=ln, **kw)
    tb.c_spec.max_episode_steps = STEPS
    for p, pol in enumerate(pols):
        tb.set_task(p, pol.state_dict())
        if stats is not None:
            tb.set_env_params(p, {'ob_rms': stats[p]})
    return tb


def _snap(tb):
    return {k: getattr(tb, k).clone() for k in FIELDS}


def _sequence(tb, noise):
    """env_reset, two rollouts (carry 0 then 1; noise [2][T][N][A] fed, or None: the counter streams of seeds 5, 6) and
    one evaluation: every buffer, state word and statistic after each."""
    out = {}
    tb.env_reset()
    out['reset'] = _snap(tb)
    for r in range(2):
        tb.rollout(5 + r, noise=None if noise is None else noise[r], carry=r > 0)
        out[f'rollout{r}'] = _snap(tb)
    out['eval'] = {'objs': tb.evaluate().clone()}
    torch.cuda.synchronize()
    return out


def _assert_equal(got, want, rows, what):
    for stage, fields in want.items():
        for k, v in fields.items():
            g = got[stage][k][rows]
            assert g.dtype == v.dtype and torch.equal(g, v), f'{what}: {stage}.{k} differs'


def _noise(spec, N, seed=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, T, N, spec['act_dim'], generator=g).cuda()


def _kernels(monkeypatch, kernel):
    if kernel == 'block':
        monkeypatch.setenv('PGM_ROLLOUT_KERNEL', 'block')
        monkeypatch.setenv('PGM_EVAL_KERNEL', 'block')


def _stats(spec, P, seed=2):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(P):
        r = RunningMeanStd(shape=(spec['obs_dim'],))
        r.update(rng.randn(50, spec['obs_dim']) * 0.3 + 0.1)
        out.append(r)
    return out


@pytest.mark.parametrize('env,ln,N,kernel', CASES)
def test_r1_one_run_equals_the_existing_entry_points(gpu, monkeypatch, env, ln, N, kernel):
    _kernels(monkeypatch, kernel)
    P, E = 3, 1 if N == 1 else 3
    spec, pols = _policies(env, ln, P)
    noise = _noise(spec, N)
    want = _sequence(_batch(env, ln, pols, N, E, seed=7), noise)
    tb = _batch(env, ln, pols, N, E, run_seeds=[7])
    tb.set_runs([0] * P)
    _assert_equal(_sequence(tb, noise), want, slice(None), 'num_runs = 1')


@pytest.mark.parametrize('env,ln,N,kernel', CASES)
def test_r2_grouped_launch_equals_one_launch_per_run(gpu, monkeypatch, env, ln, N, kernel):
    _kernels(monkeypatch, kernel)
    P, E = len(RUNS), 1 if N == 1 else 3
    spec, pols = _policies(env, ln, P)
    stats = _stats(spec, P)
    for noise in (_noise(spec, N), None):
        tb = _batch(env, ln, pols, N, E, stats=stats, run_seeds=SEEDS)
        tb.set_runs(RUNS)
        got = _sequence(tb, noise)
        for r, seed in enumerate(SEEDS):
            rows = [p for p, x in enumerate(RUNS) if x == r]
            solo = _batch(env, ln, [pols[p] for p in rows], N, E, stats=[stats[p] for p in rows], seed=seed)
            _assert_equal(got, _sequence(solo, noise), rows, f'run {r} (seed {seed}), noise fed: {noise is not None}')


@pytest.mark.parametrize('env,ln,N', [('MO-Walker2d-v2', False, 4), ('MO-Humanoid-v2', False, 2),
                                      ('MO-Hopper-v2', True, 3)])
def test_r2_spare_slot_keeps_its_sentinel(gpu, env, ln, N):
    """capacity P + 1: the launches cover the active slots only and read run ids of the active slots only."""
    P = len(RUNS)
    spec, pols = _policies(env, ln, P)
    noise = _noise(spec, N)
    tb = _batch(env, ln, pols, N, 3, run_seeds=SEEDS, capacity=P + 1)
    tb.set_runs(RUNS)
    sent = {}
    for k, full in tb._full.items():
        full[P] = 1 if full.dtype == torch.int32 else -123.0
        sent[k] = full[P].clone()
    tb.run_of_task[P] = 2 ** 30  # never read: task slot P is not launched
    got = _sequence(tb, noise)
    for k, v in sent.items():
        assert torch.equal(tb._full[k][P], v), f'spare slot: {k} was written'
    ref = _batch(env, ln, pols, N, 3, run_seeds=SEEDS)
    ref.set_runs(RUNS)
    _assert_equal(got, _sequence(ref, noise), slice(None), 'capacity P + 1')


@pytest.mark.parametrize('env,ln,N', [('MO-Walker2d-v2', False, 4), ('MO-Hopper-v3', False, 3),
                                      ('MO-Humanoid-v2', False, 4), ('MO-Hopper-v2', True, 4)])
def test_r3_the_run_id_matters(gpu, env, ln, N):
    """Tasks 0, 1 and 3 get identical parameters and statistics: 0 and 3 (run 0) are bit-equal, 0 and 1 (runs 0, 1)
    differ from the first reset on and in the evaluation objectives."""
    spec, pols = _policies(env, ln, len(RUNS))
    pols = [pols[0], pols[0], pols[2], pols[0], pols[4]]
    stats = _stats(spec, 1) * len(RUNS)
    tb = _batch(env, ln, pols, N, 3, stats=stats, run_seeds=SEEDS)
    tb.set_runs(RUNS)
    got = _sequence(tb, _noise(spec, N))
    for stage, fields in got.items():
        for k, v in fields.items():
            assert torch.equal(v[0], v[3]), f'same run, same task: {stage}.{k} differs'
    assert not torch.equal(got['reset']['obs'][0, 0], got['reset']['obs'][1, 0])
    assert not torch.equal(got['reset']['s'][0], got['reset']['s'][1])
    assert not torch.equal(got['rollout1']['obs'][0], got['rollout1']['obs'][1])
    assert not torch.equal(got['eval']['objs'][0], got['eval']['objs'][1])


@pytest.mark.parametrize('env,ln,N', [('MO-Walker2d-v2', False, 4), ('MO-Hopper-v3', False, 3),
                                      ('MO-Humanoid-v2', False, 4), ('MO-Hopper-v2', True, 4)])
def test_r4_grouped_launch_against_the_oracle(gpu, env, ln, N):
    """One grouped rollout and one grouped evaluation against the oracle stepped with each task's own run seed, in the
    bands of tests/test_gpu_kernels.py (Humanoid: its teacher-forced check and the 1e-3 + 2e-4 |ref| evaluation band)."""
    P, E = len(RUNS), 3
    spec, pols = _policies(env, ln, P)
    spec = dict(spec, max_episode_steps=STEPS)
    wide = spec['obs_dim'] > 48
    noise = torch.randn(T, N, spec['act_dim'], generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    tb = _batch(env, ln, pols, N, E, run_seeds=SEEDS)
    tb.set_runs(RUNS)
    tb.env_reset()
    tb.rollout(0, noise=noise.float().cuda(), carry=False)
    for p, r in enumerate(RUNS):
        s0 = envspec.reset_table(spec['obs_dim'], SEEDS[r], N)
        if wide:
            _teacher_forced_check(tb, p, pols[p], spec, s0, noise)
            continue
        envs = VecNormalizedSynth(spec, s0, 0.995)
        ro = oppo.RolloutStorage(T, N, spec['obs_dim'], spec['act_dim'], spec['obj_num'])
        ro.obs[0].copy_(torch.from_numpy(envs.reset()).double())
        _oracle_rollout(pols[p], envs, ro, noise.float().double())
        _close(tb.obs[p].cpu(), ro.obs, 5e-5, 1e-4, f'obs task {p}')
        _close(tb.actions[p].cpu(), ro.actions, 5e-5, 1e-4, f'actions task {p}')
        _close(tb.logp[p].cpu(), ro.action_log_probs[..., 0], 2e-4, 1e-4, f'logp task {p}')
        _close(tb.values[p].cpu(), ro.value_preds, 5e-5, 1e-4, f'values task {p}')
        _close(tb.rewards[p].cpu(), ro.rewards, 5e-5, 1e-4, f'rewards task {p}')
        np.testing.assert_array_equal(tb.masks[p].cpu().numpy(), ro.masks[..., 0].numpy())
        np.testing.assert_array_equal(tb.bad_masks[p].cpu().numpy(), ro.bad_masks[..., 0].numpy())
        assert float(ro.masks.sum()) == (T + 1) * N - 3 * N  # three auto-resets per env
        _close(tb.obj_var[p].cpu(), envs.obj_rms.var, 0, 1e-6, f'obj_rms.var task {p}')
    stats = _stats(spec, P)
    ev = _batch(env, ln, pols, N, E, stats=stats, run_seeds=SEEDS, raw=False)
    ev.set_runs(RUNS)
    objs = ev.evaluate().cpu().numpy()
    args = small_args(env, eval_num=E, raw=False)
    for p, r in enumerate(RUNS):
        ref = oracle_evaluation(args, spec, envspec.reset_table(spec['obs_dim'], SEEDS[r], E), pols[p], stats[p])
        atol, rtol = (1e-3, 2e-4) if wide else (1e-4, 1e-5)
        _close(objs[p], ref, atol, rtol, f'evaluation task {p} (run {r})')


# ------------------------------------------------------------------------------------------------ the whole loop (R5, R6)
LOOP_RUNS = [(0, 'prediction-guided'), (0, 'random'), (5, 'prediction-guided'), (5, 'random')]
LOOP_ENV = {'PGM_UPDATE_KERNEL': 'mfma', 'PGM_UPDATE_SPLIT': '0'}  # one workgroup per task: sums independent of P


def _loop_args(save_dir, seed, method, env='MO-Hopper-v2', K=2, extra=()):
    from pgmorl_amd.run import get_parser, merge_argv
    Tl, Nl = 32, 2
    argv = ['--env-name', env, '--obj-num', str(K), '--num-steps', str(Tl), '--num-processes', str(Nl), '--ppo-epoch',
            '1', '--num-mini-batch', '2', '--num-env-steps', str(Tl * Nl * 4), '--warmup-iter', '2', '--update-iter',
            '1', '--delta-weight', '0.5', '--rl-log-interval', '1', '--rng', 'host', '--pbuffer-num',
            '100' if K == 2 else '5', *extra, '--seed', str(seed), '--selection-method', method, '--save-dir',
            str(save_dir)]
    return get_parser().parse_args(merge_argv(argv))


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _log_text(lines):
    """The log without its time / FPS figures."""
    text = '\n'.join(str(x) for x in lines)
    text = re.sub(r'FPS \d+, time [\d.]+ seconds', 'FPS #, time # seconds', text)
    return re.sub(r'\[timing\].*', '[timing]', text)


def _sweep(root, max_tasks=None, rng='host'):
    from pgmorl_amd.mopg import MOPGPopulation
    from pgmorl_amd.morl import run_many
    args_list = [_loop_args(root / f'{m}_{s}', s, m) for s, m in LOOP_RUNS]
    logs = [[] for _ in args_list]
    rts, info = [], {}

    def make(a, run_seeds):
        rts.append(MOPGPopulation(a, device='cuda', rng=rng, run_seeds=run_seeds))
        return rts[-1]
    eps = run_many(args_list, device='cuda', rng=rng, log=[lg.append for lg in logs], runtime=make,
                   max_tasks=max_tasks, info=info)
    return args_list, logs, [rt.tb.update_variant() for rt in rts], info, eps


@pytest.fixture(scope='module')
def solo_trees(gpu, tmp_path_factory):
    """The four solo morl.run trees (one workgroup per task in the update), computed once."""
    from pgmorl_amd.mopg import MOPGPopulation
    from pgmorl_amd.morl import run
    root = tmp_path_factory.mktemp('solo')
    out = {}
    with _Env(LOOP_ENV):
        for s, m in LOOP_RUNS:
            a = _loop_args(root / f'{m}_{s}', s, m)
            rt = MOPGPopulation(a, device='cuda', rng='host')
            lines = []
            run(a, device='cuda', rng='host', log=lines.append, runtime=rt)
            out[(s, m)] = (a.save_dir, _log_text(lines), rt.tb.update_variant())
    return out


def _files(d):
    return sorted(os.path.relpath(os.path.join(b, f), d) for b, _, fs in os.walk(d) for f in fs)


def _assert_trees(args_list, logs, variants, solo_trees):
    assert len(set(variants)) == 1
    for a, lines, (s, m) in zip(args_list, logs, LOOP_RUNS):
        solo_dir, solo_log, solo_variant = solo_trees[(s, m)]
        assert variants[0] == solo_variant, (variants, solo_variant)
        names = _files(solo_dir)
        assert _files(a.save_dir) == names and any(n.endswith('EP_policy_0.pt') for n in names)
        for n in names:
            if n != 'timing.json':
                assert filecmp.cmp(os.path.join(a.save_dir, n), os.path.join(solo_dir, n), shallow=False), (s, m, n)
        assert _log_text(lines) == solo_log, (s, m)


def test_r5_sweep_trees_equal_the_solo_runs(gpu, tmp_path, solo_trees):
    with _Env(LOOP_ENV):
        args_list, logs, variants, info, eps = _sweep(tmp_path)
    assert info['chunks'] == [[0, 1, 2, 3]] and info['generations'][0]['tasks'] == 3 * len(LOOP_RUNS)
    assert all(any('[RL] Updates' in str(x) and '(x3 tasks' in str(x) for x in lg) for lg in logs)
    _assert_trees(args_list, logs, variants, solo_trees)


def test_r6_chunked_sweep_trees_are_unchanged(gpu, tmp_path, solo_trees):
    with _Env(LOOP_ENV):
        args_list, logs, variants, info, eps = _sweep(tmp_path, max_tasks=12)  # 6 tasks per run: two runs per chunk
    assert info['chunks'] == [[0, 1], [2, 3]]
    assert max(g['tasks'] for g in info['generations']) <= 12
    _assert_trees(args_list, logs, variants, solo_trees)


def test_r5_sweep_with_default_launch_options(gpu, tmp_path):
    args_list, logs, variants, info, eps = _sweep(tmp_path, rng='device')
    for a, ep in zip(args_list, eps):
        final = np.loadtxt(os.path.join(a.save_dir, 'final', 'objs.txt'), delimiter=',', ndmin=2)
        assert final.shape == (len(ep.sample_batch), 2) and len(final) >= 1 and np.isfinite(final).all()
        assert os.path.exists(os.path.join(a.save_dir, 'timing.json'))


@pytest.mark.parametrize('env,K,extra', [('MO-Hopper-v3', 3, []), ('MO-Hopper-v2', 2, ['--layernorm'])])
def test_r5_sweep_command_line(gpu, tmp_path, env, K, extra):
    import json

    from pgmorl_amd import sweep
    a = _loop_args('unused', 0, 'ra', env=env, K=K)
    root = tmp_path / 'root'
    prev = torch.get_default_dtype()
    try:
        sweep.main(['--pgmorl', '--seeds', '815117', '--save-dir', str(root), '--', '--env-name', env, '--obj-num', str(K),
                    '--num-steps', str(a.num_steps), '--num-processes', str(a.num_processes), '--ppo-epoch', '1',
                    '--num-mini-batch', '2', '--num-env-steps', str(a.num_env_steps), '--warmup-iter', '2',
                    '--update-iter', '1', '--delta-weight', '0.5', '--pbuffer-num', str(a.pbuffer_num), *extra])
    finally:
        torch.set_default_dtype(prev)
    d = root / 'pgmorl' / '0'
    for f in ('args.txt', 'log.txt', 'timing.json', 'final/objs.txt', 'final/EP_policy_0.pt', '2/ep/objs.txt',
              '4/elites/predictions.txt'):
        assert os.path.exists(d / f), f
    final = np.loadtxt(d / 'final' / 'objs.txt', delimiter=',', ndmin=2)
    assert final.shape[1] == K and np.isfinite(final).all()
    assert "'--seed', '815117'" in open(d / 'args.txt').read()
    st = json.load(open(root / 'sweep_timing.json'))
    assert st['runs'] == 1 and st['dirs'] == ['pgmorl/0'] and st['wall_s'] > 0 and len(st['boundary_s']) == 1
