"""Device env plug-ins on the GPU: the fused rollout and evaluation kernels of a plug-in library
(csrc/pgm_envplug.hip) against the host-stepped path of the same compiled header on the same device, bit for bit;
plugdummy.hpp against the built-in MO-Dummy kernels; the evaluation against the host-stepped one; two MOPG iterations
against the fp64 reference; the CLI.

Bit equality between the fused and the host-stepped path is a fair demand for the four test headers (no
transcendental): both run the same device functions -- policy_forward (on zero-padded images in the runtime-dim
kernels: the chain ends with fma(0, 0, acc) = acc), the Gaussian / Categorical arithmetic, norm_stats, vecnorm_emit --
and both evaluate the same header with correctly rounded fp64 operations (tests/test_envplug.py: the host function
equals the numpy restatement bit for bit)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import ppo as oppo
from pgmorl_amd import _lib, build, envspec
from pgmorl_amd.envplug import EnvPlugin
from pgmorl_amd.hostenv import PluginHostVecEnv
from pgmorl_amd.runtime import TaskBatch

from . import anydims_ref as ar
from . import cat_inputs as ci
from . import envplug_envs as pe
from . import envplug_ref as er
from .test_gpu_kernels import _close

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
P, T, R = 3, 64, 3
STORED = ('obs', 'actions', 'logp', 'values', 'rewards', 'masks', 'bad_masks')
STATE = ('ob_mean', 'ob_var', 'ob_count', 'ret_mean', 'ret_var', 'ret_count', 'obj_mean', 'obj_var', 'obj_count',
         'obj_acc', 'ret', 'obj_valid')
ENVSTATE = ('plug_sd', 'plug_si', 'elapsed', 'episode')
ALL = (pe.Line, pe.Chain, pe.PlugDummy, pe.Wide)


@pytest.fixture(scope='module')
def plugins():
    build.build_envs([pe.header(e.NAME) for e in ALL])
    return {e.NAME: EnvPlugin(pe.header(e.NAME)) for e in ALL}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _load(tb, pols):
    for p, pol in enumerate(pols):
        tb.set_task(p, pol.state_dict())
    return tb


def _policies(env, n, seed):
    return ar.make_policies(envspec.make_spec(er.register(env)), n, seed)


def _fused(pl, env, pols, N, T=T, **kw):
    kw.setdefault('R', R)
    return _load(TaskBatch(er.register(env), len(pols), num_processes=N, num_steps=T, env_plugin=pl, **kw), pols)


def _hosted(pl, env, pols, N, T=T, **kw):
    he = PluginHostVecEnv(pl, kw.get('capacity') or len(pols), N, seed=kw.get('seed', 0), R=kw.pop('R', R))
    return _load(TaskBatch(er.register(env), len(pols), num_processes=N, num_steps=T, host_env=he, **kw), pols)


def _snapshot(tb, names=STORED + STATE):
    return {k: getattr(tb, k).cpu().clone() for k in names}


def _assert_equal(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), f'{k} differs {what}: ' \
            f'{int((a[k] != b[k]).sum())} of {a[k].numel()} elements'


def _assert_env_state(tf, he, what):
    """The device-side state words, step and episode counters are the host env's."""
    st, n = he._st, tf.P * tf.N
    assert np.array_equal(tf.plug_sd.cpu().numpy().reshape(n, -1).view(np.int64), st['sd'][:n].view(np.int64)), what
    assert np.array_equal(tf.plug_si.cpu().numpy().reshape(n, -1), st['si'][:n]), f'si {what}'
    assert np.array_equal(tf.elapsed.cpu().numpy().reshape(n), st['elapsed'][:n]), f'elapsed {what}'
    assert np.array_equal(tf.episode.cpu().numpy().reshape(n), st['episode'][:n]), f'episode {what}'


def _noise(env, N, rounds, seed, T=T):
    g = torch.Generator().manual_seed(seed)
    if env.DISCRETE:
        return torch.rand(rounds, T, N, generator=g, dtype=torch.float32)
    return torch.randn(rounds, T, N, env.A, generator=g, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ G1. fused = host-stepped
@pytest.mark.parametrize('N', [1, 3, 8])
@pytest.mark.parametrize('env', ALL, ids=lambda e: e.NAME)
def test_fused_rollout_equals_host_stepped(gpu, plugins, env, N):
    """Two batches with the same policies and the same fed noise / uniforms, one host-stepped (the compiled header on
    the CPU, the runtime-dim act and ingest kernels), one fused: two rollouts of T = 64 steps (the second carried),
    R = 3 so the reset table wraps.  No float field differs: every stored field, the bootstrap values, every running
    statistic and count, obj_acc, ret, obj_acc_valid; the device-side env state is the host env's."""
    pl = plugins[env.NAME]
    pols = _policies(env, P, 0)
    noise = _noise(env, N, 2, 4)
    th, tf = _hosted(pl, env, pols, N), _fused(pl, env, pols, N)
    assert tf.plugin is pl and tf.any_dims and tf.host_env is None and not hasattr(tf, '_h_act') and th.plugin is None
    th.env_reset()
    tf.env_reset()
    _assert_equal(_snapshot(th), _snapshot(tf), 'after env_reset')
    _assert_env_state(tf, th.host_env, 'after env_reset')
    ends = bads = 0
    for r in range(2):
        th.rollout(r, noise=noise[r], carry=r > 0)
        tf.rollout(r, noise=noise[r], carry=r > 0)
        h, d = _snapshot(th), _snapshot(tf)
        _assert_equal(h, d, f'(rollout {r})')
        _assert_env_state(tf, th.host_env, f'(rollout {r})')
        ends += int((h['masks'][:, 1:] == 0).sum())
        bads += int((h['bad_masks'][:, 1:] == 0).sum())
    assert float(tf.values.abs().sum()) > 0 and float(tf.logp.abs().sum()) > 0
    print(f'{env.NAME} N={N}: {ends} episode ends, {bads} of them by the limit, episode max {int(tf.episode.max())}')
    if env.MAX_STEPS < T:
        assert ends > 0 and int(tf.episode.max()) >= R, 'episodes end; the table wraps'
    if env in (pe.Chain, pe.Wide):
        assert bads > 0, 'episodes ended by the forced limit (bad_masks 0) occur'


@pytest.mark.parametrize('env', [pe.Line, pe.Chain], ids=lambda e: e.NAME)
def test_in_kernel_draws_are_the_counter_streams(gpu, plugins, env):
    """rollout(seed, noise=None) draws pgm_normal_noise's element (t N + n) A + a / pgm_uniform_noise's element
    t N + n of the stream of `seed` in the kernel: equal in every stored field, statistic and env state, over two
    carried rollouts, to the rollout fed that stream."""
    pl, N = plugins[env.NAME], 3
    pols = _policies(env, P, 1)
    ta, tb = _fused(pl, env, pols, N), _fused(pl, env, pols, N)
    ta.env_reset()
    tb.env_reset()
    fn, what = ((_lib.lib().pgm_uniform_noise, 'pgm_uniform_noise') if env.DISCRETE
                else (_lib.lib().pgm_normal_noise, 'pgm_normal_noise'))
    for r, seed in enumerate((7, 1 << 40)):
        ta.rollout(seed, noise=None, carry=r > 0)
        z = torch.full((T, N) if env.DISCRETE else (T, N, env.A), SENTINEL, device=gpu)
        _lib.check(fn(z.numel(), C.c_uint64(seed), _ptr(z), _stream()), what)
        tb.rollout(seed + 1, noise=z, carry=r > 0)  # (the seed is not read when a stream is given)
        _assert_equal(_snapshot(ta, STORED + STATE + ENVSTATE), _snapshot(tb, STORED + STATE + ENVSTATE),
                      f'(rollout {r})')
    assert float(ta.actions.std()) > 0.3


def test_spare_slot_stays_untouched(gpu, plugins):
    """Capacity P + 1 with P active: task row P of every buffer, returns and adv keep their sentinel through two
    rollouts and an evaluation, and the active rows equal a batch of capacity P."""
    env, N = pe.Line, 3
    pl = plugins[env.NAME]
    pols = _policies(env, P, 0)
    tb, tc = _fused(pl, env, pols, N, capacity=P + 1), _fused(pl, env, pols, N)
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
    tb._eval_ob[:, P].fill_(SENTINEL)
    before = {k: v.cpu().clone() for k, v in full.items()}
    state, stats, evob = tb._state.cpu().clone(), tb._stats64.cpu().clone(), tb._eval_ob.cpu().clone()
    tables = tb.mode._plug_train.cpu().clone(), tb.mode._plug_eval.cpu().clone()
    noise = _noise(env, N, 1, 1)[0]
    for t in (tb, tc):
        t.rollout(0, noise=noise, carry=False)
        t.rollout(1, noise=None, carry=True)
        t.evaluate()
    torch.cuda.synchronize()
    _assert_equal(_snapshot(tb, STORED + STATE + ENVSTATE + ('objs',)), _snapshot(tc, STORED + STATE + ENVSTATE + ('objs',)),
                  '(capacity P + 1 vs P)')
    assert int(tb.episode.max()) > 0, 'the rollout ran'
    for name, t in full.items():
        assert torch.equal(t[P].cpu(), before[name][P]), f'task row P of {name} was written'
    for name in ('returns', 'adv'):
        assert torch.equal(full[name].cpu(), before[name]), f'{name} was written'
    assert torch.equal(tb._state.cpu(), state), 'parameters / Adam moments were written'
    assert torch.equal(tb._eval_ob.cpu(), evob)
    assert torch.equal(tb.mode._plug_train.cpu(), tables[0]) and torch.equal(tb.mode._plug_eval.cpu(), tables[1])
    for name, off, w, vec in tb._seg:
        assert torch.equal(tb._stats64[off:off + cap * w].view(cap, w)[P].cpu(),
                           stats[off:off + cap * w].view(cap, w)[P]), f'task row P of {name} was written'


# ------------------------------------------------------------------------------------------------ G2. plug-in = built-in
def _dummy_policies(seed):
    """Task 0 as initialised; tasks 1, 2 with an fc_mean bias of +-4: they run at the clip and leave the disc of
    radius 5 within a few steps, so true terminals occur inside T = 64."""
    pols = _policies(pe.PlugDummy, P, seed)
    for p, sign in ((1, (1.0, -1.0)), (2, (-1.0, 1.0))):
        with torch.no_grad():
            pols[p].dist.fc_mean.bias.copy_(torch.tensor(sign, dtype=torch.float64) * 4.0)
    return pols


@pytest.mark.parametrize('N', [3, 8])
def test_plugdummy_equals_the_builtin_dummy(gpu, plugins, N):
    """plugdummy.hpp's fused rollout and evaluation equal pgm_rollout_dummy / pgm_eval_dummy (MO-Dummy-v0, K = 2) in
    every stored field, statistic, env state word and objective.  Both kernels get reset tables built from ONE uniform
    array (the built-in's positions are 2 u - 1 formed on the host, the plug-in forms 2 u - 1 in its reset)."""
    pl = plugins['plugdummy']
    pols = _dummy_policies(0)
    kw = dict(eval_num=N, raw=False, gamma=0.99)
    tp = _fused(pl, pe.PlugDummy, pols, N, **kw)
    td = _load(TaskBatch('MO-Dummy-v0', P, num_processes=N, num_steps=T, R=R, **kw), pols)
    assert td.dummy_env and td.mode.max_steps == 500 and td.mode.bound == 5.0 and td.mode.time_limit_is_bad
    u_train, u_eval = tp.mode._plug_train.clone(), tp.mode._plug_eval.clone()
    td.mode._dummy_train.copy_(2.0 * u_train - 1.0)
    td.mode._dummy_eval.copy_(2.0 * u_eval - 1.0)
    tp.env_reset()
    td.env_reset()
    noise = _noise(pe.PlugDummy, N, 2, 9)
    for r in range(2):
        tp.rollout(r, noise=noise[r], carry=r > 0)
        td.rollout(r, noise=noise[r], carry=r > 0)
        _assert_equal(_snapshot(tp), _snapshot(td), f'(rollout {r})')
        assert torch.equal(tp.plug_sd.cpu(), td.s.cpu()) and torch.equal(tp.elapsed.cpu(), td.elapsed.cpu())
        assert torch.equal(tp.plug_si.cpu()[..., 0], td.elapsed.cpu()) and torch.equal(tp.episode.cpu(), td.episode.cpu())
    m, b = tp.masks.cpu()[:, 1:], tp.bad_masks.cpu()[:, 1:]
    assert int(((m == 0) & (b == 1)).sum()) > 0 and int(tp.episode.max()) >= R, 'true terminals; the table wraps'
    tp.objs.fill_(SENTINEL)
    td.objs.fill_(SENTINEL)
    for use_ob in (True, False):
        tp.use_ob_rms = td.use_ob_rms = use_ob
        got_p, got_d = tp.evaluate().cpu().clone(), td.evaluate().cpu().clone()
        assert torch.equal(got_p, got_d) and np.isfinite(got_p.numpy()).all() and (got_p != SENTINEL).all()


# ------------------------------------------------------------------------------------------------ G3. evaluation
@pytest.mark.parametrize('raw', [0, 1])
@pytest.mark.parametrize('use_ob', [0, 1])
@pytest.mark.parametrize('E', [1, 8])
@pytest.mark.parametrize('env', [pe.Line, pe.PlugDummy, pe.Wide], ids=lambda e: e.NAME)
def test_eval_equals_host_evaluate(gpu, plugins, env, E, use_ob, raw):
    """The fused evaluation and the host-stepped one (pgm_eval_act_any + the compiled header on the CPU) run the same
    fp32 forward on the same fp64 observations: objectives at rel 1e-12, the bound of
    test_eval_dummy_equals_host_evaluate_unsaturated."""
    pl = plugins[env.NAME]
    pols = _policies(env, P, 2)
    kw = dict(eval_num=E, raw=bool(raw), ob_rms=bool(use_ob), gamma=0.995, seed=3)
    th, tf = _hosted(pl, env, pols, 1, T=8, **kw), _fused(pl, env, pols, 1, T=8, **kw)
    rng = np.random.RandomState(3)
    mean = torch.tensor(rng.randn(P, env.O) * 0.2, device=gpu)
    var = torch.tensor(rng.rand(P, env.O) + 0.5, device=gpu)
    tf.objs.fill_(SENTINEL)
    got_h = th.evaluate(mean, var).cpu().numpy().copy()
    got_f = tf.evaluate(mean, var).cpu().numpy().copy()
    print(f'{env.NAME} E={E}: max rel err {np.abs(got_f / got_h - 1).max():.3e}')
    assert np.isfinite(got_f).all() and (got_f != SENTINEL).all()
    _close(got_f, got_h, 0, 1e-12, 'pgm_envplug_eval vs _host_evaluate')


@pytest.mark.parametrize('use_ob', [0, 1])
@pytest.mark.parametrize('E', [1, 8])
def test_eval_chain_under_the_logit_margin_rule(gpu, plugins, E, use_ob):
    """chain.hpp (Categorical: the lowest-index argmax) at the first seed at which, from the reference alone, the top
    two logits of every evaluated row are >= MARGIN apart and the fp32 arm runs the same episodes: the fused
    evaluation equals the reference's objectives (exact sums of sixths) at rel 1e-12, and the host-stepped one."""
    env, pl = pe.Chain, plugins['chain']
    seed, (pols, rms, want, bad, margins) = er.chain_eval_seed(E, use_ob)
    assert not bad, (seed, bad)
    kw = dict(eval_num=E, raw=True, ob_rms=bool(use_ob), seed=0)
    th, tf = _hosted(pl, env, pols, 1, T=8, **kw), _fused(pl, env, pols, 1, T=8, **kw)
    mean = torch.tensor(np.stack([r.mean for r in rms]), device=gpu)
    var = torch.tensor(np.stack([r.var for r in rms]), device=gpu)
    got_h = th.evaluate(mean, var).cpu().numpy().copy()
    got_f = tf.evaluate(mean, var).cpu().numpy().copy()
    print(f'seed {seed}, logit margin {margins["logit"]:.3g}: fused {got_f[0]}, reference {want[0]}')
    _close(got_f, want, 0, 1e-12, 'pgm_envplug_eval vs the reference')
    _close(got_f, got_h, 0, 1e-12, 'pgm_envplug_eval vs _host_evaluate')


def test_eval_episode_ended_by_the_forced_limit(gpu, plugins):
    """A 'stay' policy on the chain never reaches an end of it: every evaluation episode ends by the forced limit after
    exactly MAX_STEPS = 20 steps, so objective 2 (one per 'stay') is 20 and objectives 0 + 1 sum to 20."""
    env, pl, E = pe.Chain, plugins['chain'], 8
    pols = _policies(env, P, 0)
    for pol in pols:
        with torch.no_grad():
            pol.dist.linear.bias.copy_(torch.tensor([-5.0, 5.0, -5.0], dtype=torch.float64))
    kw = dict(eval_num=E, raw=True, ob_rms=False)
    th, tf = _hosted(pl, env, pols, 1, T=8, **kw), _fused(pl, env, pols, 1, T=8, **kw)
    got_f, got_h = tf.evaluate().cpu().numpy().copy(), th.evaluate().cpu().numpy().copy()
    assert np.array_equal(got_f[:, 2], np.full(P, 20.0)), got_f
    _close(got_f[:, 0] + got_f[:, 1], np.full(P, 20.0), 0, 1e-12, 'objectives 0 + 1 over 20 steps')
    _close(got_f, got_h, 0, 1e-12, 'pgm_envplug_eval vs _host_evaluate')


# ------------------------------------------------------------------------------------------------ G4. the reference
@pytest.mark.parametrize('env', [pe.Line, pe.Chain], ids=lambda e: e.NAME)
def test_mopg_iterations_against_the_reference(gpu, plugins, env):
    """Two MOPG iterations through TaskBatch(env_plugin=...) against the reference worker stepping the numpy
    restatement, at test_mopg_iterations_end_to_end's tolerances; overlap_eval is bitwise equal to in-order."""
    c = er.MOPG
    Pm, Tm, N, E, M, iters = (c[k] for k in ('P', 'T', 'N', 'E', 'M', 'iters'))
    seed = er.MOPG_SEEDS[env.NAME]
    name, args, pols, w, refs, bad, margins = er.mopg_case(env, seed)
    assert not bad, bad
    pl = plugins[env.NAME]
    batches = []
    for overlap in (False, True):
        tb = TaskBatch(name, Pm, num_processes=N, num_steps=Tm, ppo_epoch=E, num_mini_batch=M, env_plugin=pl, R=c['R'])
        for p, pol in enumerate(pols):
            tb.set_task(p, pol.state_dict(), {}, None, w[p])
        tb.env_reset()
        batches.append((tb, overlap, torch.zeros(iters, Pm, env.K, dtype=torch.float64, device=gpu)))
    fn = ci.mopg_noise_fn(Tm, N, E) if env.DISCRETE else ar.gauss_noise_fn(Tm, N, env.A, E)
    total = int(args.num_env_steps) // Tm // N
    for j in range(iters):
        rnd, perms = fn(j)
        for tb, overlap, objs_out in batches:
            tb.iteration(j, oppo.linear_lr(j, total, args.lr), noise=rnd, perms=torch.stack(perms).numpy(), carry=j > 0,
                         overlap_eval=overlap, objs_out=objs_out[j])
        tb = batches[0][0]
        objs, params = batches[0][2][j].cpu().numpy().copy(), tb.params.cpu().numpy().copy()
        acts, rets = tb.actions.cpu(), tb.returns.cpu()
        masks, bads = tb.masks.cpu(), tb.bad_masks.cpu()
        if j == 0:
            assert int(((masks == 0) & (bads == 1)).sum()) > 0, 'a true terminal (masks 0, bad_masks 1) in the storage'
        for p in range(Pm):
            pol, ref_objs, st = refs[p][j]
            if env.DISCRETE:
                assert torch.equal(acts[p].double(), st['actions']), f'task {p} iteration {j}: rollout actions'
            else:
                _close(acts[p], st['actions'], 5e-5, 1e-4, f'actions iter {j}')  # band of test_rollout
            assert torch.equal(masks[p].double(), st['masks'][..., 0]) and torch.equal(bads[p].double(), st['bad_masks'][..., 0])
            _close(rets[p][:Tm], st['returns'][:Tm], 1e-5, 1e-5, f'returns iter {j}')  # band of test_gae
            _close(params[p], tb.layout.flatten(pol.state_dict(), dtype=np.float64), 2e-5, 1e-4, f'params iter {j}')
            print(f'{env.NAME} task {p} iter {j}: objs {objs[p]} (reference {ref_objs})')
            _close(objs[p], ref_objs, *er.OBJ_BAND, f'eval objs iter {j}')
    (ta, _, oa), (tb, _, ob) = batches
    tb.wait_eval()
    torch.cuda.synchronize()
    ta.check_update()
    tb.check_update()
    assert torch.equal(oa.cpu(), ob.cpu()), 'overlap_eval objectives differ from in-order'
    _assert_equal(_snapshot(ta, STORED + STATE + ENVSTATE + ('params', 'adam_m', 'adam_v')),
                  _snapshot(tb, STORED + STATE + ENVSTATE + ('params', 'adam_m', 'adam_v')), '(overlap vs in-order)')


# ------------------------------------------------------------------------------------------------ G5. the CLI
def _cli(tmp, env, rng, extra=()):
    from pgmorl_amd.run import main
    Tc, N = 32, 2
    argv = ['--env-name', env.ENV + '-cli', '--obj-num', str(env.K), '--num-steps', str(Tc), '--num-processes', str(N),
            '--ppo-epoch', '1', '--num-mini-batch', '2', '--num-env-steps', str(Tc * N * 4), '--warmup-iter', '2',
            '--update-iter', '1', '--delta-weight', '0.5', '--selection-method', 'prediction-guided', '--save-dir',
            str(tmp), '--rl-log-interval', '1', '--rng', rng, '--pbuffer-num', '100', '--env-plugin',
            os.path.relpath(pe.header(env.NAME))] + list(extra)
    prev = torch.get_default_dtype()
    try:
        main(argv)
    finally:
        torch.set_default_dtype(prev)
    return np.loadtxt(tmp / 'final' / 'objs.txt', delimiter=',', ndmin=2)


@pytest.mark.parametrize('rng', ['host', 'device'])
@pytest.mark.parametrize('env', [pe.Line, pe.Chain], ids=lambda e: e.NAME)
def test_cli_env_plugin(gpu, tmp_path, capsys, env, rng):
    """pgmorl_amd.run --env-plugin tests/envplug/<header> --env-name <a name envspec does not know> at a tiny budget:
    the results tree is written; in --rng host mode "--host-env plugin" (the same header stepped on the host) writes
    the same final objectives."""
    final = _cli(tmp_path / 'fused', env, rng)
    capsys.readouterr()
    assert env.ENV + '-cli' in envspec.user_env_names()
    for it in ('2', '3', '4'):
        for f in ('ep/objs.txt', 'population/objs.txt', 'elites/elites.txt', 'elites/offsprings.txt'):
            assert os.path.exists(tmp_path / 'fused' / it / f), f'{it}/{f}'
    for f in ('args.txt', 'log.txt', 'final/objs.txt', 'final/EP_policy_0.pt'):
        assert os.path.exists(tmp_path / 'fused' / f), f
    assert final.shape[1] == env.K and np.isfinite(final).all()
    if rng == 'host':
        hosted = _cli(tmp_path / 'hosted', env, rng, ('--host-env', 'plugin'))
        capsys.readouterr()
        assert np.array_equal(final, hosted), (final, hosted)
