"""Contract 2 of the device env plug-ins on the GPU (runtime parameters, per-step uniforms): the fused kernels behind
pgm_envplug_rollout_ex / pgm_envplug_eval_ex against the host-stepped path of the same compiled header on the same
device, bit for bit; the parameters and the env noise take effect and do not depend on the task; line2.hpp equals
line.hpp; spare task rows stay untouched; two MOPG iterations of slip.hpp against the fp64 reference; the CLI.

Bit equality between the fused and the host-stepped path is a fair demand here for the reasons tests/test_gpu_envplug.py
gives, plus two: the parameters are the same fp64 words on both sides, and the uniforms are integer hashes
(tests/test_envplug2.py: pgm_envplug_uniforms equals the restatement from oracle/streams.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import ppo as oppo
from pgmorl_amd import build, envplug
from pgmorl_amd.envplug import EnvPlugin
from pgmorl_amd.hostenv import PluginHostVecEnv
from pgmorl_amd.runtime import TaskBatch

from . import anydims_ref as ar
from . import envplug2_envs as p2
from . import envplug2_ref as r2
from . import envplug_envs as pe
from . import envplug_ref as er
from .test_envplug2 import OTHER
from .test_gpu_envplug import (ENVSTATE, SENTINEL, STATE, STORED, _assert_env_state, _assert_equal, _load, _snapshot)
from .test_gpu_kernels import _close

pytestmark = pytest.mark.gpu

P, T, R = r2.P, r2.T, r2.R
ALL = (p2.Slip, p2.Gather, p2.ParMax, p2.NoiseMax, p2.Line2)
PARAMS = {'slip': r2.COND['slip']['env_params'], 'gather': r2.COND['gather']['env_params'], 'parmax': OTHER['parmax'],
          'noisemax': None, 'line2': None}
EVERY = STORED + STATE + ENVSTATE


@pytest.fixture(scope='module')
def plugins():
    hs = [p2.header(e.NAME) for e in ALL] + [pe.header('line')]
    build.build_envs(hs)
    d = {e.NAME: EnvPlugin(p2.header(e.NAME)) for e in ALL}
    d['line'] = EnvPlugin(pe.header('line'))
    return d


def _fused(pl, env, pols, N, T=T, env_params=None, **kw):
    kw.setdefault('R', R)
    return _load(TaskBatch(r2.register(env), len(pols), num_processes=N, num_steps=T, env_plugin=pl,
                           env_params=env_params, **kw), pols)


def _hosted(pl, env, pols, N, T=T, env_params=None, **kw):
    he = PluginHostVecEnv(pl, kw.get('capacity') or len(pols), N, seed=kw.get('seed', 0), R=kw.pop('R', R),
                          env_params=env_params)
    return _load(TaskBatch(r2.register(env), len(pols), num_processes=N, num_steps=T, host_env=he, **kw), pols)


# ------------------------------------------------------------------------------------------------ G1, G2. fused = hosted
@pytest.mark.parametrize('N', [1, 3, 8])
@pytest.mark.parametrize('env', [p2.Slip, p2.Gather, p2.ParMax, p2.NoiseMax], ids=lambda e: e.NAME)
def test_fused_rollout_equals_host_stepped(gpu, plugins, env, N):
    """Two batches with the same policies, parameters and fed action noise, one host-stepped (the compiled header on
    the CPU with PluginHostVecEnv's stream), one fused: rollout 0 draws the env noise of env_seed(0) in the kernel,
    rollout 1 (carried) is fed uploaded uniforms, rollout 2 (carried) draws env_seed(2); R = 3 so the table wraps.
    Every stored field, running statistic and env-state word is torch.equal.

    So that no case passes vacuously the first rollout of slip and gather, read on the host-stepped side, holds a true
    terminal, a forced limit, two auto-resets and env-noise words on both sides of the first parameter.  Parameters
    and seeds: tests/envplug2_ref.py COND (slip: slip 0.3, wind 0.125; gather: p_attack 0.5; policy seed 0, noise
    seed 4), picked on the CPU, where the fp64 reference counts (terminals, limits, resets, below, above)
    slip N=1: 5, 5, 10, 19, 21; N=3: 31, 7, 38, 54, 66; N=8: 79, 28, 107, 115, 205;
    gather N=1: 5, 9, 14, 22, 18; N=3: 50, 16, 66, 62, 58; N=8: 95, 51, 146, 170, 150."""
    pl = plugins[env.NAME]
    c = r2.COND.get(env.NAME, dict(pol_seed=0, noise_seed=4))
    pols = r2.policies(env, P, c['pol_seed'])
    noise = r2.noise(env, N, 3, c['noise_seed'])
    fed = torch.rand(T, N, env.NW, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    th = _hosted(pl, env, pols, N, env_params=PARAMS[env.NAME])
    tf = _fused(pl, env, pols, N, env_params=PARAMS[env.NAME])
    assert tf.plugin is pl and tf.host_env is None and th.plugin is None and pl.CONTRACT == 2
    th.env_reset()
    tf.env_reset()
    _assert_equal(_snapshot(th), _snapshot(tf), 'after env_reset')
    _assert_env_state(tf, th.host_env, 'after env_reset')
    for r in range(3):
        en = fed if (r == 1 and env.NW) else None
        th.rollout(r, noise=noise[r], carry=r > 0, env_noise=en)
        tf.rollout(r, noise=noise[r], carry=r > 0, env_noise=en)
        h, d = _snapshot(th), _snapshot(tf)
        _assert_equal(h, d, f'(rollout {r})')
        _assert_env_state(tf, th.host_env, f'(rollout {r})')
        if r == 0 and env.NAME in r2.COND:
            w0 = pl.uniforms(envplug.env_seed(0), 0, T * N * env.NW).reshape(T, N, env.NW)[..., 0]
            got = r2.count(h['masks'][:, 1:].numpy(), h['bad_masks'][:, 1:].numpy(), w0, th.host_env.par[0])
            print(f'{env.NAME} N={N}: host-stepped first rollout {got}; the fp64 reference {r2.COUNTS[env.NAME, N]}')
            assert r2.meets(got), got
    assert float(tf.values.abs().sum()) > 0 and float(tf.logp.abs().sum()) > 0 and int(tf.episode.max()) >= R


# ------------------------------------------------------------------------------------------------ G3. the parameters
@pytest.mark.parametrize('env', [p2.Slip, p2.ParMax], ids=lambda e: e.NAME)
def test_parameters_take_effect(gpu, plugins, env):
    """Two batches that differ only in env_params give other rewards; no env_params equals the defaults passed
    explicitly, bitwise."""
    pl, N = plugins[env.NAME], 3
    pols = r2.policies(env, P, 0)
    noise = r2.noise(env, N, 1, 5)[0]
    dflt = dict(zip(env.PAR_NAMES, env.PAR_DEFAULT))
    snaps = []
    for params in (None, dflt, OTHER[env.NAME], dict(dflt, **{env.PAR_NAMES[-1]: dflt[env.PAR_NAMES[-1]] + 0.25})):
        tb = _fused(pl, env, pols, N, env_params=params)
        tb.env_reset()
        tb.rollout(0, noise=noise, carry=False)
        tb.evaluate()
        snaps.append(_snapshot(tb, EVERY + ('objs',)))
    _assert_equal(snaps[0], snaps[1], '(defaults vs the defaults passed explicitly)')
    for other in snaps[2:]:
        assert not torch.equal(snaps[0]['rewards'], other['rewards']), 'other parameters, the same rewards'
        assert not torch.equal(snaps[0]['objs'], other['objs']), 'other parameters, the same evaluation'


# ------------------------------------------------------------------------------------------------ G4. the noise
@pytest.mark.parametrize('env', [p2.Slip, p2.Gather, p2.NoiseMax], ids=lambda e: e.NAME)
def test_env_noise_takes_effect_and_ignores_the_task(gpu, plugins, env):
    """Tasks 0 and 2 hold the same policy: their rows are identical in every field (the env noise of (t, n) is not the
    task's).  The same fed action noise under another rollout seed gives other env noise: other rewards."""
    pl, N = plugins[env.NAME], 3
    pols = r2.policies(env, 2, 3)
    pols = [pols[0], pols[1], pols[0]]
    noise = r2.noise(env, N, 1, 6)[0]
    ta, tb = (_fused(pl, env, pols, N, env_params=PARAMS[env.NAME]) for _ in range(2))
    ta.env_reset()
    tb.env_reset()
    ta.rollout(0, noise=noise, carry=False)
    tb.rollout(1, noise=noise, carry=False)
    for name in EVERY:
        x = getattr(ta, name)
        assert torch.equal(x[0], x[2]), f'{name}: tasks with one policy differ'
    assert not torch.equal(ta.rewards[0], ta.rewards[1]) or not torch.equal(ta.actions[0], ta.actions[1])
    assert not torch.equal(ta.rewards, tb.rewards), 'another rollout seed, the same env noise'
    ta.evaluate()
    assert torch.equal(ta.objs[0], ta.objs[2])


# ------------------------------------------------------------------------------------------------ G5. the twin
@pytest.mark.parametrize('N', [1, 3, 8])
def test_line2_equals_line(gpu, plugins, N):
    """line.hpp restated under CONTRACT = 2 (NP = NW = 0) through the _ex entry points equals line.hpp through the
    old ones on every field, rollout (two, the second carried, one with in-kernel action noise) and evaluation."""
    pols = r2.policies(p2.Line2, P, 0)
    kw = dict(eval_num=N, raw=False, gamma=0.99)
    ta = _fused(plugins['line2'], p2.Line2, pols, N, **kw)
    tb = _load(TaskBatch(er.register(pe.Line), P, num_processes=N, num_steps=T, env_plugin=plugins['line'], R=R, **kw),
               pols)
    assert ta.plugin.CONTRACT == 2 and tb.plugin.CONTRACT == 1
    ta.env_reset()
    tb.env_reset()
    noise = r2.noise(p2.Line2, N, 1, 9)[0]
    for r, z in enumerate((noise, None)):
        ta.rollout(r, noise=z, carry=r > 0)
        tb.rollout(r, noise=z, carry=r > 0)
        _assert_equal(_snapshot(ta, EVERY), _snapshot(tb, EVERY), f'(rollout {r})')
    assert int(ta.episode.max()) > 0
    ta.objs.fill_(SENTINEL)
    tb.objs.fill_(SENTINEL)
    got_a, got_b = ta.evaluate().cpu().clone(), tb.evaluate().cpu().clone()
    assert torch.equal(got_a, got_b) and (got_a != SENTINEL).all() and np.isfinite(got_a.numpy()).all()


# ------------------------------------------------------------------------------------------------ G6. evaluation
@pytest.mark.parametrize('raw', [0, 1])
@pytest.mark.parametrize('E', [1, 3, 8])
@pytest.mark.parametrize('env', [p2.Slip, p2.NoiseMax, p2.ParMax], ids=lambda e: e.NAME)
def test_eval_ex_equals_host_evaluate(gpu, plugins, env, E, raw):
    """pgm_envplug_eval_ex and the host-stepped evaluation (pgm_eval_act_any + the compiled header on the CPU, the
    stream of env_seed(batch seed) at (e MAX_STEPS + it) NW + j) at rel 1e-12, the band of
    test_gpu_envplug.test_eval_equals_host_evaluate; a second launch is bit-equal."""
    pl = plugins[env.NAME]
    pols = r2.policies(env, P, 2)
    kw = dict(eval_num=E, raw=bool(raw), ob_rms=True, gamma=0.995, seed=3, env_params=PARAMS[env.NAME])
    th, tf = _hosted(pl, env, pols, 1, T=8, **kw), _fused(pl, env, pols, 1, T=8, **kw)
    rng = np.random.RandomState(3)
    mean = torch.tensor(rng.randn(P, env.O) * 0.2, device=gpu)
    var = torch.tensor(rng.rand(P, env.O) + 0.5, device=gpu)
    tf.objs.fill_(SENTINEL)
    got_h = th.evaluate(mean, var).cpu().numpy().copy()
    got_f = tf.evaluate(mean, var).cpu().numpy().copy()
    print(f'{env.NAME} E={E}: max rel err {np.abs(got_f / got_h - 1).max():.3e}')
    assert np.isfinite(got_f).all() and (got_f != SENTINEL).all()
    _close(got_f, got_h, 0, 1e-12, 'pgm_envplug_eval_ex vs _host_evaluate')
    tf.objs.fill_(SENTINEL)
    assert np.array_equal(tf.evaluate(mean, var).cpu().numpy(), got_f), 'two launches with one env_seed'


def test_eval_env_seed_changes_slips_objectives(gpu, plugins):
    env, pl, E = p2.Slip, plugins['slip'], 8
    pols = r2.policies(env, P, 2)
    tf = _fused(pl, env, pols, 1, T=8, eval_num=E, env_params={'slip': 0.5}, ob_rms=False)
    a = tf.evaluate().cpu().clone()
    assert tf._plug_eval_seed == envplug.env_seed(0)
    tf._plug_eval_seed = envplug.env_seed(1)
    b = tf.evaluate().cpu().clone()
    tf._plug_eval_seed = envplug.env_seed(0)
    c = tf.evaluate().cpu().clone()
    assert torch.equal(a, c) and not torch.equal(a, b), (a, b)


# ------------------------------------------------------------------------------------------------ G7. sentinels
def test_spare_slot_stays_untouched(gpu, plugins):
    """Capacity P + 1 with P active: task row P of every buffer (plug_sd, plug_si, episode among them), returns and
    adv keep their sentinel through two rollouts and an evaluation; the active rows equal a batch of capacity P; the
    parameter vector and the reset tables are read only."""
    env, N = p2.Slip, 3
    pl = plugins[env.NAME]
    pols = r2.policies(env, P, 0)
    tb = _fused(pl, env, pols, N, capacity=P + 1, env_params=PARAMS['slip'])
    tc = _fused(pl, env, pols, N, env_params=PARAMS['slip'])
    tb.env_reset()
    tc.env_reset()
    full = dict(tb._full)
    assert all(k in full for k in ENVSTATE)
    for name, t in full.items():
        t[P].fill_(int(SENTINEL) if t.dtype == torch.int32 else SENTINEL)
    for name in ('returns', 'adv'):
        full[name].fill_(SENTINEL)
    tb._state[:, P].fill_(SENTINEL)
    cap = tb.capacity
    for name, off, w, vec in tb._seg:
        tb._stats64[off:off + cap * w].view(cap, w)[P].fill_(SENTINEL)
    before = {k: v.cpu().clone() for k, v in full.items()}
    state, stats = tb._state.cpu().clone(), tb._stats64.cpu().clone()
    consts = [x.cpu().clone() for x in (tb.mode._plug_train, tb.mode._plug_eval, tb.mode._plug_par)]
    noise = r2.noise(env, N, 1, 1)[0]
    fed = torch.rand(T, N, env.NW, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    for t in (tb, tc):
        t.rollout(0, noise=noise, carry=False, env_noise=fed)
        t.rollout(1, noise=None, carry=True)
        t.evaluate()
    torch.cuda.synchronize()
    _assert_equal(_snapshot(tb, EVERY + ('objs',)), _snapshot(tc, EVERY + ('objs',)), '(capacity P + 1 vs P)')
    assert int(tb.episode.max()) > 0, 'the rollout ran'
    for name, t in full.items():
        assert torch.equal(t[P].cpu(), before[name][P]), f'task row P of {name} was written'
    for name in ('returns', 'adv'):
        assert torch.equal(full[name].cpu(), before[name]), f'{name} was written'
    assert torch.equal(tb._state.cpu(), state), 'parameters / Adam moments were written'
    for x, y in zip((tb.mode._plug_train, tb.mode._plug_eval, tb.mode._plug_par), consts):
        assert torch.equal(x.cpu(), y)
    assert torch.equal(tb.env_noise.cpu(), fed), 'the fed env noise was written'
    for name, off, w, vec in tb._seg:
        assert torch.equal(tb._stats64[off:off + cap * w].view(cap, w)[P].cpu(),
                           stats[off:off + cap * w].view(cap, w)[P]), f'task row P of {name} was written'


# ------------------------------------------------------------------------------------------------ G8. end to end
def test_mopg_iterations_of_slip_against_the_reference(gpu, plugins):
    """Two MOPG iterations of slip.hpp through TaskBatch(env_plugin=..., env_params=...) against the reference worker
    stepping the numpy restatement with the same parameters and env-noise indices, at the bands of
    test_gpu_envplug.test_mopg_iterations_against_the_reference."""
    env, c = p2.Slip, r2.MOPG
    Pm, Tm, N, E, M, iters = (c[k] for k in ('P', 'T', 'N', 'E', 'M', 'iters'))
    name, args, pols, w, refs, bad, margins = r2.mopg_case(env, r2.MOPG_SEED)
    assert not bad, bad
    tb = TaskBatch(name, Pm, num_processes=N, num_steps=Tm, ppo_epoch=E, num_mini_batch=M, env_plugin=plugins['slip'],
                   R=c['R'], env_params=c['env_params'])
    for p, pol in enumerate(pols):
        tb.set_task(p, pol.state_dict(), {}, None, w[p])
    tb.env_reset()
    fn = ar.gauss_noise_fn(Tm, N, env.A, E)
    total = int(args.num_env_steps) // Tm // N
    objs_out = torch.zeros(iters, Pm, env.K, dtype=torch.float64, device=gpu)
    for j in range(iters):
        rnd, perms = fn(j)
        tb.iteration(j, oppo.linear_lr(j, total, args.lr), noise=rnd, perms=torch.stack(perms).numpy(), carry=j > 0,
                     objs_out=objs_out[j])
        objs, params = objs_out[j].cpu().numpy().copy(), tb.params.cpu().numpy().copy()
        acts, rets = tb.actions.cpu(), tb.returns.cpu()
        masks, bads = tb.masks.cpu(), tb.bad_masks.cpu()
        if j == 0:
            assert int(((masks == 0) & (bads == 1)).sum()) > 0, 'a true terminal (masks 0, bad_masks 1) in the storage'
        for p in range(Pm):
            pol, ref_objs, st = refs[p][j]
            _close(acts[p], st['actions'], 5e-5, 1e-4, f'actions iter {j}')
            assert torch.equal(masks[p].double(), st['masks'][..., 0]) and torch.equal(bads[p].double(), st['bad_masks'][..., 0])
            _close(rets[p][:Tm], st['returns'][:Tm], 1e-5, 1e-5, f'returns iter {j}')
            _close(params[p], tb.layout.flatten(pol.state_dict(), dtype=np.float64), 2e-5, 1e-4, f'params iter {j}')
            print(f'slip task {p} iter {j}: objs {objs[p]} (reference {ref_objs})')
            _close(objs[p], ref_objs, *er.OBJ_BAND, f'eval objs iter {j}')
    tb.check_update()


def _cli(tmp, extra=()):
    from pgmorl_amd.run import main
    Tc, N = 32, 2
    argv = ['--env-name', 'Slip-v0-cli', '--obj-num', '2', '--num-steps', str(Tc), '--num-processes', str(N),
            '--ppo-epoch', '1', '--num-mini-batch', '2', '--num-env-steps', str(Tc * N * 4), '--warmup-iter', '2',
            '--update-iter', '1', '--delta-weight', '0.5', '--selection-method', 'prediction-guided', '--save-dir',
            str(tmp), '--rl-log-interval', '1', '--rng', 'host', '--pbuffer-num', '100', '--env-plugin',
            os.path.relpath(p2.header('slip')), '--env-param', 'slip=0.3'] + list(extra)
    prev = torch.get_default_dtype()
    try:
        main(argv)
    finally:
        torch.set_default_dtype(prev)
    return np.loadtxt(tmp / 'final' / 'objs.txt', delimiter=',', ndmin=2)


def test_cli_env_param(gpu, tmp_path, capsys):
    """pgmorl_amd.run --env-plugin slip.hpp --env-param slip=0.3 at a tiny budget: args.txt records the flag, and the
    same run with "--host-env plugin" writes the same final objectives; another value writes others."""
    final = _cli(tmp_path / 'fused')
    args_txt = open(tmp_path / 'fused' / 'args.txt').read()
    assert "'--env-param', 'slip=0.3'" in args_txt, args_txt
    assert final.shape[1] == 2 and np.isfinite(final).all()
    hosted = _cli(tmp_path / 'hosted', ('--host-env', 'plugin'))
    assert np.array_equal(final, hosted), (final, hosted)
    other = _cli(tmp_path / 'other', ('--env-param', 'wind=0.125'))
    capsys.readouterr()
    assert "'--env-param', 'wind=0.125'" in open(tmp_path / 'other' / 'args.txt').read()
    assert other.shape != final.shape or not np.array_equal(final, other)
