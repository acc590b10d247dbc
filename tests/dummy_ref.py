"""The fp64 reference of the MO-Dummy envs (MO-Dummy-v0 / MO-Dummy3-v0).  TEST INFRASTRUCTURE ONLY.

The Gaussian ``oracle.policy.Policy`` over ``hostenv.DummyMOHostVecEnv`` through ``RefVecNormalize`` of
tests/cat_ref.py: the rollout (morl/mopg.py:103-135), the evaluation (morl/mopg.py:25-46) and the MOPG iterations of
oracle.mopg.mopg_worker, plus the ctypes wrapper of pgm_dummy_transition and the input cases the CPU and GPU tests
share.  Every input case is chosen from the reference alone (first_seed over the rule of rollout_case)."""
import copy
import ctypes as C
import functools
import itertools

import numpy as np
import torch

from oracle import ppo as oppo
from pgmorl_amd import _lib, envspec
from pgmorl_amd._lib import DummySpec
from pgmorl_amd.hostenv import DummyMOHostVecEnv

from .branch_inputs import make_policies
from .cat_ref import RefVecNormalize

F64 = torch.float64
ENVS = {2: 'MO-Dummy-v0', 3: 'MO-Dummy3-v0'}
SHORT = {'max_steps': 12, 'bound': 1.25}  # both kinds of episode end inside T = 48
EDGE = 1e-4  # every | |pos| - bound | of a reference rollout stays at least this far from the decision


def _p(a):
    return C.c_void_p(a.ctypes.data)


def transition(K, state, step, episode, env, action, table, max_steps=500, bound=5.0, tlb=1):
    """pgm_dummy_transition -> (state [n, 6], step, episode, obj [n, K], reward, done, bad).  table [count, R, 2]."""
    table = np.ascontiguousarray(table, dtype=np.float64)
    state = np.ascontiguousarray(state, dtype=np.float64)
    step, episode, env = (np.ascontiguousarray(x, dtype=np.int32) for x in (step, episode, env))
    action = np.ascontiguousarray(action, dtype=np.float32)
    n = len(step)
    so, eo, done, bad = (np.full(n, -9, dtype=np.int32) for _ in range(4))
    s2, obj, rew = np.full((n, 6), np.nan), np.full((n, K), np.nan), np.full(n, np.nan)
    spec = DummySpec(max_steps, tlb, bound, _p(table), table.shape[1], table.shape[0])
    rc = _lib.lib().pgm_dummy_transition(C.byref(spec), K, n, _p(state), _p(step), _p(episode), _p(env), _p(action),
                                         _p(s2), _p(so), _p(eo), _p(obj), _p(rew), _p(done), _p(bad))
    _lib.check(rc, 'pgm_dummy_transition')
    return s2, so, eo, obj, rew, done, bad


def host_step(K, state, step, episode, action, max_steps=500, bound=5.0, tlb=1, R=3, seed=0):
    """The same (state, action) pairs through DummyMOHostVecEnv as the n envs of one task, its state set directly
    (pair i is env i: row i of the reset table) -> transition()'s tuple."""
    n = len(step)
    he = DummyMOHostVecEnv(ENVS[K], 1, n, seed=seed, max_steps=max_steps, bound=bound, time_limit_is_bad=bool(tlb), R=R)
    he.reset()
    he._st = {'s': np.array(state, dtype=np.float64)[None].copy(), 'step': np.array(step, dtype=np.int64)[None].copy(),
              'episode': np.array(episode, dtype=np.int64)[None].copy()}
    obs, rew, done, bad, obj = he.step(np.asarray(action, dtype=np.float32)[None])
    assert np.array_equal(obs[0], he._st['s'][0])
    return obs[0], he._st['step'][0], he._st['episode'][0], obj[0], rew[0], done[0], bad[0]


def grid_cases(max_steps, bound):
    """Positions inside the disc, within 1e-12 of the bound on both sides and far outside x zero / non-zero velocity x
    step in {0, 1, max_steps - 2, max_steps - 1} x actions inside, on and beyond the clip -> (state, step, episode,
    action).  The positions are where the env lands: the start is the landing point minus the step's displacement."""
    radii = [0.0, 0.3 * bound, bound - 1e-3, bound - 1e-12, bound, bound + 1e-12, bound + 1e-3, 3.0 * bound]
    angles = [0.0, 0.7, 2.4, -1.9]
    vels = [(0.0, 0.0), (0.05, -0.02), (-0.3, 0.4)]
    acts = [(0.0, 0.0), (0.3, -0.6), (1.0, -1.0), (-1.0, 1.0), (1.7, 0.2), (-0.4, -2.5), (np.nextafter(np.float32(1), 2), 1.0)]
    steps = [0, 1, max_steps - 2, max_steps - 1]
    st, sp, ac = [], [], []
    for (r, th), v, a, s in itertools.product(itertools.product(radii, angles), vels, acts, steps):
        a32 = np.asarray(a, dtype=np.float32)
        acl = np.clip(a32.astype(np.float64), -1.0, 1.0)
        vel = (np.asarray(v) + acl * 0.1) * 0.95
        land = np.array([r * np.cos(th), r * np.sin(th)])
        st.append(np.concatenate([land - vel, v, [0.25 * s, 0.5 * s]]))
        sp.append(s)
        ac.append(a32)
    n = len(sp)
    return np.array(st), np.array(sp, dtype=np.int32), (np.arange(n) % 5).astype(np.int32), np.array(ac, dtype=np.float32)


# ------------------------------------------------------------------------------------------------ the reference
def ref_reset(env, vn, ro):
    ro.obs[0].copy_(torch.from_numpy(vn.reset(env.reset()[0]).astype(np.float32)).double())


def ref_rollout(pol, env, vn, ro, noise, edge=None):
    """morl/mopg.py:103-135: T steps of pol on the one-task host env (P = 1) through vn into ro, then the bootstrap
    value.  noise [T, N, A].  edge, if a dict: the smallest | |pos| - bound | of the landing points ('edge').  The
    policy may be fp32 (the reference's fp32 arm); envs and statistics fp64."""
    net = next(pol.parameters()).dtype
    for t in range(noise.shape[0]):
        with torch.no_grad():
            value, action, logp = pol.act(ro.obs[t].to(net), noise=noise[t])
        if edge is not None:  # the landing points of this step, from the env's own rule on a copy
            probe = copy.deepcopy(env)
            probe.bound = np.inf
            probe.max_steps = 1 << 40
            s = probe.step(action.float().numpy()[None])[0][0]
            edge['edge'] = min(edge.get('edge', np.inf), float(np.abs(np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1])
                                                                     - env.bound).min()))
        obs, rew, done, bad, obj = env.step(action.float().numpy()[None])
        o, r = vn.step(obs[0], rew[0], done[0], obj[0])
        masks = torch.tensor(np.where(done[0], 0.0, 1.0), dtype=F64).unsqueeze(-1)
        bads = torch.tensor(np.where(bad[0], 0.0, 1.0), dtype=F64).unsqueeze(-1)
        ro.insert(torch.from_numpy(o.astype(np.float32)).double(), action.double(), logp.double(), value.double(),
                  torch.from_numpy(r).double(), masks, bads)
    with torch.no_grad():
        ro.value_preds[-1] = pol.get_value(ro.obs[-1].to(net)).double()


def ref_evaluate(pol, env, ob_rms, eval_num, raw=True, gamma=1.0, lengths=None):
    """morl/mopg.py:25-46 on env's evaluation episodes (one task): fp64 normalisation, the mean action."""
    net = next(pol.parameters()).dtype
    obs = env.eval_reset(eval_num)
    alive = np.ones(eval_num, dtype=bool)
    acc, disc = np.zeros((eval_num, env.obj_num)), 1.0
    length = np.zeros(eval_num, dtype=np.int64)
    while alive.any():
        ob = obs[0]
        if ob_rms is not None:
            ob = np.clip((ob - ob_rms.mean) / np.sqrt(ob_rms.var + 1e-8), -10.0, 10.0)
        with torch.no_grad():
            _, action, _ = pol.act(torch.tensor(ob, dtype=net), deterministic=True)
        obs, obj, done = env.eval_step(action.float().numpy()[None])
        acc += np.where(alive[:, None], disc * obj[0], 0.0)
        length += alive
        if not raw:
            disc *= gamma
        alive &= ~done[0]
    if lengths is not None:
        lengths[:] = length
    return acc.sum(0) / eval_num


def ref_mopg(args, pol, env, weights, iters, noise_fn, net=F64):
    """oracle.mopg.mopg_worker on a one-task host env, from fresh statistics: per iteration the rollout, returns,
    scalarised PPO update, after_update and the evaluation -> [(policy, objs, storage)]."""
    T, N, O, A, K = args.num_steps, args.num_processes, env.obs_dim, env.act_dim, env.obj_num
    pol = copy.deepcopy(pol).to(net)
    agent = oppo.PPO(pol, args.clip_param, args.ppo_epoch, args.num_mini_batch, args.value_loss_coef,
                     args.entropy_coef, lr=args.lr, eps=1e-5, max_grad_norm=args.max_grad_norm)
    vn = RefVecNormalize(N, O, args.gamma, args.ob_rms, args.obj_rms)
    ro = oppo.RolloutStorage(T, N, O, A, K)
    ref_reset(env, vn, ro)
    total = int(args.num_env_steps) // T // N
    out = []
    for j in range(iters):
        noise, perms = noise_fn(j)
        agent.set_lr(oppo.linear_lr(j, total, args.lr, args.lr_decay_ratio))
        ref_rollout(pol, env, vn, ro, noise.float().double())
        ro.compute_returns(ro.value_preds[-1].clone(), args.use_gae, args.gamma, args.gae_lambda,
                           args.use_proper_time_limits)
        storage = {k: getattr(ro, k).clone() for k in ('obs', 'actions', 'action_log_probs', 'value_preds', 'rewards',
                                                       'masks', 'bad_masks', 'returns')}
        agent.update(ro, weights, vn.obj_rms.var if vn.obj_rms is not None else None, perms)
        ro.after_update()
        objs = ref_evaluate(pol, env, copy.deepcopy(vn.ob_rms), args.eval_num, args.raw, args.gamma)
        out.append((copy.deepcopy(pol).double(), objs, storage))
    return out


# ------------------------------------------------------------------------------------------------ input cases
def rollout_case(K, P, N, T, R, seed, kw):
    """Policies, noise [R, T, N, 2] and the per-task reference of R carried rollouts -> (pols, noise, refs, violations,
    counts).  refs[p] = ([storage per rollout], RefVecNormalize, host env); counts[p] = (true terminals, time-limit
    ends).  Violations of the input rule: a landing point within EDGE of the bound, or the reference's fp32 arm making
    another episode-end decision."""
    env_name = ENVS[K]
    spec = envspec.make_spec(env_name)
    pols = make_policies(spec, P, seed)
    noise = torch.randn(R, T, N, 2, generator=torch.Generator().manual_seed(seed + 4), dtype=F64).float()
    refs, bad, counts = [], [], []
    for p in range(P):
        arms = []
        for net in (F64, torch.float32):
            env = DummyMOHostVecEnv(env_name, 1, N, seed=0, **kw)
            vn = RefVecNormalize(N, 6, 0.995)
            ro = oppo.RolloutStorage(T, N, 6, 2, K)
            ref_reset(env, vn, ro)
            pol = copy.deepcopy(pols[p]).to(net)
            edge, stores = {}, []
            for r in range(R):
                if r > 0:
                    ro.after_update()
                ref_rollout(pol, env, vn, ro, noise[r].double(), edge if net is F64 else None)
                stores.append(copy.deepcopy(ro))
            arms.append((stores, vn, env, edge))
        (s64, vn, env, edge), (s32, _, _, _) = arms
        if not edge['edge'] >= EDGE:
            bad.append(f'task {p}: a landing point {edge["edge"]:.3g} from the bound')
        for r in range(R):
            if not (torch.equal(s64[r].masks, s32[r].masks) and torch.equal(s64[r].bad_masks, s32[r].bad_masks)):
                bad.append(f'task {p} rollout {r}: the fp32 arm makes another episode-end decision')
        m = torch.cat([s.masks[1:] for s in s64])
        b = torch.cat([s.bad_masks[1:] for s in s64])
        counts.append((int(((m == 0) & (b == 1)).sum()), int(((m == 0) & (b == 0)).sum())))
        refs.append((s64, vn, env))
    return pols, noise, refs, bad, counts


def first_seed(case, tries=20):
    """The first seed counting up from 0 at which case(seed) reports no violation -> (seed, result, skipped), skipped
    = {seed: violations} of the seeds before it."""
    skipped = {}
    for seed in range(tries):
        out = case(seed)
        if not out[3]:
            return seed, out, skipped
        skipped[seed] = out[3]
    raise AssertionError(f'no seed below {tries} meets the input rule: {skipped}')


@functools.lru_cache(maxsize=None)
def reference_case(K, short):
    """The shared reference of the GPU tests at (P, N, T, R) = (2, 4, 48, 2): defaults or SHORT."""
    kw = dict(SHORT) if short else {}
    return first_seed(lambda s: rollout_case(K, 2, 4, 48, 2, s, kw))
