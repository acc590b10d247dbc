"""The one-workgroup-per-task policy kernels are instantiations of one body per job (act, host-env act, host-env
evaluation act, fused rollout) over a Towers and a Head type.  What that makes true by construction is
pinned here, bit for bit, so that a later edit to one instantiation cannot drift from the others:

  * TaskBatch.act(obs[:, 0], noise[0]) is slot 0 of pgm_rollout_act(0) on a host-env batch and, for the Gaussian
    families, of the block-form fused rollout;
  * act(..., deterministic=True) gives the actions of pgm_eval_act with use_ob_rms = 0 on the same rows widened to
    fp64.

Plain Walker, plain Swimmer, LayerNorm Hopper-v2 and Categorical Deep Sea Treasure; P = 3, N in {1, 3, 8} (one row
per wave pair, an uneven split, all rows), T = 2, random policies, explicit noise / uniforms."""
import ctypes as C

import numpy as np
import pytest
import torch

from pgmorl_amd import _lib, envspec
from pgmorl_amd._lib import Dims
from pgmorl_amd.hostenv import DeepSeaTreasureHostVecEnv, SynthHostVecEnv
from pgmorl_amd.policy import new_policy
from pgmorl_amd.runtime import TaskBatch

pytestmark = pytest.mark.gpu

P, T = 3, 2
CASES = {'walker': ('MO-Walker2d-v2', False), 'swimmer': ('MO-Swimmer-v2', False), 'hopper-ln': ('MO-Hopper-v2', True),
         'dst-cat': ('MO-DeepSeaTreasure-v0', False)}
GAUSSIAN = [c for c in CASES if c != 'dst-cat']
NS = (1, 3, 8)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _batch(case, N, host):
    env, ln = CASES[case]
    spec = envspec.make_spec(env)
    disc = bool(spec.get('discrete', False))
    he = None
    if host:
        he = DeepSeaTreasureHostVecEnv(env, P, N) if disc else SynthHostVecEnv(env, P, N, seed=0)
    tb = TaskBatch(env, P, num_processes=N, num_steps=T, ppo_epoch=1, num_mini_batch=1, layernorm=ln, host_env=he)
    torch.manual_seed(7)
    rng = np.random.RandomState(7)
    for p in range(P):
        pol = new_policy(spec['obs_dim'], spec['act_dim'], spec['obj_num'], layernorm=ln, discrete=disc)
        tb.set_task(p, pol.state_dict(), weights=rng.dirichlet(np.ones(spec['obj_num'])))
    tb.env_reset()
    return tb


def _noise(tb):
    g = torch.Generator().manual_seed(13)
    return torch.rand(T, tb.N, generator=g) if tb.discrete else torch.randn(T, tb.N, tb.A, generator=g)


@pytest.fixture(scope='module', params=[(c, n) for c in CASES for n in NS], ids=lambda cn: f'{cn[0]}-{cn[1]}')
def host_case(gpu, request):
    """One host-env batch per (case, N): act() sampled and deterministic on the rows of slot 0, slot 0 as
    pgm_rollout_act(0) wrote it, and pgm_eval_act on the same rows.  CPU tensors, shared by the two tests below."""
    case, N = request.param
    tb = _batch(case, N, host=True)
    noise = _noise(tb)
    tb.noise.copy_(noise)
    rows = tb.obs[:, 0].clone()
    tb._rollout_act(0)
    out = {'slot': (tb.values[:, 0], tb.actions[:, 0], tb.logp[:, 0]), 'action_out': tb.mode._d_act[:P],
           'act': tb.act(rows, noise[0]), 'det': tb.act(rows, deterministic=True)}
    d = Dims(P, 1, 0, tb.O, tb.A, tb.K, tb.H, int(tb.layernorm))
    if tb.discrete:
        ea = torch.zeros(P, N, dtype=torch.int32, device=tb.dev)
        fn, what = _lib.lib().pgm_eval_act_cat, 'pgm_eval_act_cat'
    else:
        ea, fn, what = torch.zeros(P, N, tb.A, device=tb.dev), _lib.lib().pgm_eval_act, 'pgm_eval_act'
    raw = rows.double().contiguous()
    _lib.check(fn(C.byref(d), _ptr(tb.params), _ptr(None), _ptr(None), 0, _ptr(raw), N, _ptr(ea), _stream()), what)
    out['eval_act'] = ea
    return {k: tuple(x.cpu() for x in v) if isinstance(v, tuple) else v.cpu() for k, v in out.items()}


def test_act_is_rollout_act_slot0(host_case):
    r = host_case
    (v, a, lp), (sv, sa, slp) = r['act'], r['slot']
    assert torch.equal(v, sv), 'values'
    assert torch.equal(lp, slp), 'log-probs'
    assert torch.equal(a, r['action_out']), 'action_out'
    # the rollout storage holds the action as fp32: the index of a discrete action, exact
    assert torch.equal(a.float().reshape(sa.shape), sa), 'stored actions'


def test_deterministic_act_is_eval_act(host_case):
    r = host_case
    assert torch.equal(r['det'][1], r['eval_act'])


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('case', GAUSSIAN)
def test_act_is_block_rollout_slot0(gpu, monkeypatch, case, N):
    monkeypatch.setenv('PGM_ROLLOUT_KERNEL', 'block')  # the plain family's workgroup-per-task kernel
    tb = _batch(case, N, host=False)
    noise = _noise(tb)
    rows = tb.obs[:, 0].clone()
    tb.rollout(0, noise=noise, carry=False)
    v, a, lp = tb.act(rows, noise[0])
    assert torch.equal(tb.obs[:, 0], rows)
    assert torch.equal(v, tb.values[:, 0]), 'values'
    assert torch.equal(a, tb.actions[:, 0]), 'actions'
    assert torch.equal(lp, tb.logp[:, 0]), 'log-probs'
