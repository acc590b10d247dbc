"""fp64 reference pieces and test inputs of the runtime-dim kernel family (the *_any entry points), at dims no kernel
is compiled for.  Everything here is built from oracle.*, tests/cat_ref.py, tests/cat_inputs.py and
tests/branch_inputs.py: their constructions, conditions and margins are imported, not restated; what this file adds is
the env names of arbitrary dims (registered through envspec.register_env), the Categorical update inputs at such dims
(cat_inputs.build_inputs is bound to Deep Sea Treasure) and the Gaussian MOPG reference worker on a host env.

Seeds follow the rule of cat_inputs / branch_inputs: the first one, counting up from the base, at which the reference
alone meets every condition (found on the CPU, recorded below and in DESIGN.md; tests/test_anydims.py re-checks them).
"""
import copy
import functools
import math

import numpy as np
import torch

from oracle import ppo as oppo
from oracle.vecenv import RunningMeanStd
from pgmorl_amd import envspec
from pgmorl_amd.hostenv import GymHostVecEnv, HostVecEnv

from . import anydims_envs as envs
from . import branch_inputs as bi
from . import cat_inputs as ci
from . import cat_ref
from .branch_inputs import FAR, GAP, HP_DEFAULT, MARGIN, MIX_RATIO, MIX_VALUE, hparams
from .helpers import small_args, weights_grid

F64 = torch.float64
GAUSS_DIMS = [(5, 1, 2), (24, 4, 3), (32, 8, 3)]
CAT_DIMS = [(2, 3, 3), (8, 5, 2), (32, 8, 3)]
UPDATE_CAT_DIMS = [(2, 3, 3), (32, 8, 3)]


def env_of(dims, discrete):
    """The registered env name of (obs, act, obj) dims: 'AnyG-5-1-2', 'AnyC-2-3-3', ..."""
    name = 'Any{}-{}-{}-{}'.format('C' if discrete else 'G', *dims)
    envspec.register_env(name, *dims, discrete=discrete)
    return name


class StubHostEnv(HostVecEnv):
    """A host env of given dims that steps nothing: what TaskBatch needs to allocate a host-stepped batch whose
    kernels a test then calls directly."""

    def __init__(self, dims, discrete, P, N):
        self.obs_dim, self.act_dim, self.obj_num = dims
        self.discrete, self.capacity, self.P, self.N = bool(discrete), P, P, N

    def set_active(self, P):
        self.P = P


def make_policies(spec, P, seed):
    return cat_ref.make_policies(spec, P, seed) if spec.get('discrete') else bi.make_policies(spec, P, seed)


# ------------------------------------------------------------------------------------------------ forward / eval
def forward_case(dims, discrete, P, N, T, seed):
    """Observations [P][T+1][N][O], the random stream (normals [T][N][A] / uniforms [T][N]) and per task the
    reference's values [T+1], actions [T], logp [T] -> (pols, obs, rnd, refs, violations, margins).  Categorical:
    cat_inputs.forward_case's margin rule at these dims."""
    spec = envspec.make_spec(env_of(dims, discrete))
    O, A = spec['obs_dim'], spec['act_dim']
    pols = make_policies(spec, P, seed)
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(P, T + 1, N, O, generator=g).float()
    refs, bad, m = [], [], {}
    if not discrete:
        rnd = torch.randn(T, N, A, generator=g).float()
        for p in range(P):
            with torch.no_grad():
                v, a, lp = pols[p].act(obs[p, :T].double().reshape(T * N, O), noise=rnd.double().reshape(T * N, A))
                vT = pols[p].get_value(obs[p, T].double())
            refs.append(dict(values=torch.cat([v.reshape(T, N, -1), vT[None]]), actions=a.reshape(T, N, A),
                             logp=lp.reshape(T, N)))
        return pols, obs, rnd, refs, bad, m
    rnd = torch.rand(T, N, generator=g, dtype=torch.float32)
    for p in range(P):
        x = obs[p, :T].double().reshape(T * N, O)
        with torch.no_grad():
            v, a, lp = pols[p].act(x, u=rnd.reshape(-1), margins=m)
            _, am, _ = pols[p].act(x, deterministic=True, margins=m)
            p32 = copy.deepcopy(pols[p]).float()
            _, a32, _ = p32.act(x.float(), u=rnd.reshape(-1))
            _, am32, _ = p32.act(x.float(), deterministic=True)
            vT = pols[p].get_value(obs[p, T].double())
        if not torch.equal(a, a32) or not torch.equal(am, am32):
            bad.append(f'task {p}: the fp32 arm picks other actions')
        refs.append(dict(values=torch.cat([v.reshape(T, N, -1), vT[None]]), actions=a.reshape(T, N),
                         logp=lp.reshape(T, N)))
    for k in ('uniform', 'logit'):
        if not m[k] >= MARGIN:
            bad.append(f'{k} margin {m[k]:.3g} < {MARGIN}')
    return pols, obs, rnd, refs, bad, m


def eval_case(dims, discrete, P, E, seed):
    """test_eval_act's construction at these dims -> (pols, raw [P][E][O], rms, reference actions, violations,
    margins)."""
    spec = envspec.make_spec(env_of(dims, discrete))
    O = spec['obs_dim']
    pols = make_policies(spec, P, seed)
    rng = np.random.RandomState(seed + 7 + E)
    rms = []
    for _ in range(P):
        r = RunningMeanStd(shape=(O,))
        r.update(rng.randn(50, O) * 0.3 + 0.1)
        rms.append(r)
    raw = rng.randn(P, E, O) * 0.3 + 0.1
    raw[:, :, O - 1] = 9.0  # normalises far beyond the clip at 10
    acts, bad, m = [], [], {}
    for p in range(P):
        ob = np.clip((raw[p] - rms[p].mean) / np.sqrt(rms[p].var + 1e-8), -10.0, 10.0)
        with torch.no_grad():
            if discrete:
                _, a, _ = pols[p].act(torch.tensor(ob), deterministic=True, margins=m)
                _, a32, _ = copy.deepcopy(pols[p]).float().act(torch.tensor(ob).float(), deterministic=True)
                if not torch.equal(a, a32):
                    bad.append(f'task {p}: the fp32 arm picks other actions')
                a = a[:, 0]
            else:
                _, a, _ = pols[p].act(torch.tensor(ob), deterministic=True)
        acts.append(a.numpy())
    if discrete and not m['logit'] >= MARGIN:
        bad.append(f'logit margin {m["logit"]:.3g} < {MARGIN}')
    return pols, raw, rms, np.stack(acts), bad, m


# ------------------------------------------------------------------------------------------------ the update
# name -> (P, T, N, E, M): the shapes of the issue
SHAPES = {'main': (2, 64, 4, 2, 2),    # 128-row minibatches, four tiles, both granule parities twice
          'ragged': (2, 50, 3, 1, 3),  # a ragged second tile
          'p9': (9, 32, 4, 1, 4)}      # a partial second group of eight tasks
SHAPE_ROWS = [('main', r) for r in 'abcdef'] + [('ragged', 'a'), ('p9', 'a')]
UPDATE_CASES = ([(d, False, s, r) for d in GAUSS_DIMS for s, r in SHAPE_ROWS] +
                [(d, True, s, r) for d in UPDATE_CAT_DIMS for s, r in SHAPE_ROWS])
COMPILED_CASES = [((17, 6, 2), False, 'main', 'a'), ((3, 4, 2), True, 'main', 'a')]
COMPILED_ENVS = {((17, 6, 2), False): 'MO-Walker2d-v2', ((3, 4, 2), True): 'MO-DeepSeaTreasure-v0'}
SEED_TRIES = 64


def case_env(dims, discrete):
    return COMPILED_ENVS.get((tuple(dims), discrete)) or env_of(dims, discrete)


def build_cat_inputs(env, P, T, N, E, M, seed, hp=None):
    """cat_inputs.build_inputs (its construction, RET_BIAS included) for any registered discrete env."""
    hp = dict(HP_DEFAULT, **(hp or {}))
    clip = hp['clip_param']
    args = small_args(env, num_steps=T, num_processes=N, ppo_epoch=E, num_mini_batch=M,
                      **{k: hp[k] for k in ('clip_param', 'value_loss_coef', 'entropy_coef', 'max_grad_norm')})
    spec = envspec.make_spec(env)
    pols = cat_ref.make_policies(spec, P, seed)
    O, K, B = spec['obs_dim'], spec['obj_num'], T * N
    rng = np.random.RandomState(seed)
    obs = np.clip(rng.randn(P, T + 1, N, O), -3, 3).astype(np.float32)
    uni = rng.rand(P, T, N)
    up, lo = math.log1p(clip), math.log1p(-clip)
    acts, lps, vals = [], [], []
    for p in range(P):
        with torch.no_grad():
            v, a, lp = pols[p].act(torch.from_numpy(obs[p, :T]).double().reshape(B, O),
                                   u=torch.from_numpy(uni[p]).reshape(B))
        group = rng.choice(3, size=B, p=MIX_RATIO)
        u = rng.rand(B)
        log_ratio = np.where(group == 0, lo / 2 + u * (up - lo) / 2,
                             np.where(group == 1, up + GAP + u * FAR, lo - GAP - u * FAR))
        far = rng.rand(B, K) >= MIX_VALUE
        sign = np.where(rng.rand(B, K) < 0.5, -1.0, 1.0)
        u = rng.rand(B, K)
        v_off = np.where(far, sign * (clip + GAP + u * FAR), (u - 0.5) * clip)
        acts.append(a.float().reshape(T, N, 1))
        lps.append((lp[:, 0] - torch.from_numpy(log_ratio)).float().reshape(T, N))
        vals.append((v + torch.from_numpy(v_off)).float().reshape(T, N, K))
    actions, logp, values = torch.stack(acts), torch.stack(lps), torch.stack(vals)
    values = torch.cat([values, torch.zeros(P, 1, N, K)], 1)
    returns = values + torch.from_numpy(ci.RET_BIAS + rng.randn(P, T + 1, N, K) * ci.RET_NOISE).float()
    adv = torch.from_numpy(rng.randn(P, T, N)).float()
    perms = [torch.randperm(B, generator=torch.Generator().manual_seed(seed * 10 + e)) for e in range(E)]
    return args, spec, pols, (obs, actions, logp, values, returns, adv), perms


# Gaussian dims at which branch_inputs' construction keeps the reference's gradient norm below max_grad_norm in every
# row (5 observations and one action dim give a small gradient: none of the first 64 seeds meets the norm condition of
# rows a, b, d, e, f there): the returns get cat_inputs' mean offset RET_BIAS, the construction change cat_inputs makes
# for the same reason.  The conditions are unchanged.
RET_BIAS_DIMS = {(5, 1, 2)}


def build_gauss_inputs(env, P, T, N, E, M, seed, hp=None):
    args, spec, pols, data, perms = bi.build_inputs(env, P, T, N, E, M, seed, hp)
    if (spec['obs_dim'], spec['act_dim'], spec['obj_num']) in RET_BIAS_DIMS:
        obs, actions, logp, values, returns, adv = data
        data = (obs, actions, logp, values, returns + ci.RET_BIAS, adv)
    return args, spec, pols, data, perms


def evaluate_update(dims, discrete, shape_name, row, seed, stop_early=False):
    """One candidate seed of an update case, from the reference alone -> (inputs, per-task fp64 results, violations,
    worst): branch_inputs.conditions and same_decisions at every step of every task; with an entropy term (row f) on a
    Categorical head also cat_inputs' entropy condition.  stop_early: return at the first task with a violation (enough to
    reject a candidate seed; results and worst are then partial)."""
    P, T, N, E, M = SHAPES[shape_name]
    env, hp = case_env(dims, discrete), hparams(row)
    shape = (env, P, T, N, E, M)
    inputs = (build_cat_inputs if discrete else build_gauss_inputs)(env, P, T, N, E, M, seed, hp)
    _, _, pols, data, perms = inputs
    results, bad, worst = [], [], {}
    for p in range(P):
        r64 = bi.run_oracle(pols[p], hp, data, p, perms, shape)
        r32 = bi.run_oracle(pols[p], hp, data, p, perms, shape, dtype=torch.float32)
        b, w = bi.conditions(r64[3], hp)
        bad += [f'task {p}: {x}' for x in b] + [f'task {p}: {x}' for x in bi.same_decisions(r64[3], r32[3], hp)]
        for k, x in w.items():
            worst[k] = min(worst.get(k, math.inf), x)
        if hp['entropy_coef'] != 0.0 and discrete:
            r0 = bi.run_oracle(pols[p], dict(hp, entropy_coef=0.0), data, p, perms, shape)
            ex = ci.entropy_excess(bi.flat_state(r64[0], r64[1])[0], bi.flat_state(r0[0], r0[1])[0])
            worst['entropy term, x band'] = min(worst.get('entropy term, x band', math.inf), ex)
            if not ex > 10.0:
                bad.append(f'task {p}: without the entropy term the parameters move {ex:.3g}x the band (need > 10)')
        results.append(r64)
        if stop_early and bad:
            break
    return inputs, results, bad, worst


def scan_update_seed(dims, discrete, shape_name, row):
    for seed in range(bi.BASE_SEED, bi.BASE_SEED + SEED_TRIES):
        out = evaluate_update(dims, discrete, shape_name, row, seed)
        if not out[2]:
            return seed, out
    raise AssertionError(f'no seed in {SEED_TRIES} for {(dims, discrete, shape_name, row)}: last {out[2][:3]}')


# (dims, discrete, shape, row) -> the first seed from branch_inputs.BASE_SEED at which the reference meets the
# conditions
# (scan_update_seed on the CPU; the worst shares and margins are in DESIGN.md 23)
UPDATE_SEEDS = {c: bi.BASE_SEED for c in UPDATE_CASES + COMPILED_CASES}
UPDATE_SEEDS.update({((5, 1, 2), False, 'main', 'd'): 12, ((5, 1, 2), False, 'p9', 'a'): 39,
                     ((24, 4, 3), False, 'p9', 'a'): 20, ((32, 8, 3), False, 'ragged', 'a'): 12,
                     ((32, 8, 3), False, 'main', 'c'): 12, ((32, 8, 3), False, 'p9', 'a'): 23,
                     ((2, 3, 3), True, 'p9', 'a'): 32, ((32, 8, 3), True, 'ragged', 'a'): 12,
                     ((32, 8, 3), True, 'p9', 'a'): 40})


@functools.lru_cache(maxsize=None)
def update_case(dims, discrete, shape_name, row):
    """The case at its recorded seed, computed once and shared (callers must not modify it)."""
    seed = UPDATE_SEEDS[(dims, discrete, shape_name, row)]
    inputs, results, bad, worst = evaluate_update(dims, discrete, shape_name, row, seed)
    assert not bad, f'{(dims, discrete, shape_name, row)} seed {seed}: the reference misses its conditions: {bad}'
    return inputs, results, worst


# ------------------------------------------------------------------------------------------------ MOPG iterations
MOPG = dict(P=2, T=64, N=4, E=2, M=4, iters=2)
OBJ_BAND = (1e-3, 1e-4)  # the plain objective band of test_mopg_iterations_end_to_end


def gauss_noise_fn(T, N, A, E):
    def fn(j):
        torch.manual_seed(j)
        z = torch.randn(T, N, A, dtype=torch.float32)
        return z, [torch.randperm(T * N) for _ in range(E)]
    return fn


def host_env(name, P, N, seed=0):
    return GymHostVecEnv(envs.make_env, name, P, N, seed)


def ref_rollout_gauss(pol, env, vn, ro, noise, margins=None):
    """cat_ref.ref_rollout for a Gaussian policy: T steps on the one-task host env through vn into ro, then the
    bootstrap value.  margins['bound']: the smallest distance of |x'| from the continuous env's terminal bound."""
    net = next(pol.parameters()).dtype
    for t in range(noise.shape[0]):
        with torch.no_grad():
            value, action, logp = pol.act(ro.obs[t].to(net), noise=noise[t].to(net))
        obs, rew, done, bad, obj = env.step(action.float().numpy()[None])
        if margins is not None:
            gap = min(abs(e.last_x - envs.BOUND) for e in env.envs[0])
            margins['bound'] = min(margins.get('bound', math.inf), gap)
        o, r = vn.step(obs[0], rew[0], done[0], obj[0])
        masks = torch.tensor(np.where(done[0], 0.0, 1.0), dtype=F64).unsqueeze(-1)
        bads = torch.tensor(np.where(bad[0], 0.0, 1.0), dtype=F64).unsqueeze(-1)
        ro.insert(torch.from_numpy(o.astype(np.float32)).double(), action.double(), logp.double(), value.double(),
                  torch.from_numpy(r).double(), masks, bads)
    with torch.no_grad():
        ro.value_preds[-1] = pol.get_value(ro.obs[-1].to(net)).double()


def ref_evaluate_gauss(pol, env, ob_rms, eval_num, raw=True, gamma=1.0):
    net = next(pol.parameters()).dtype
    obs = env.eval_reset(eval_num)
    alive = np.ones(eval_num, dtype=bool)
    acc, disc = np.zeros((eval_num, env.obj_num)), 1.0
    while alive.any():
        ob = obs[0]
        if ob_rms is not None:
            ob = np.clip((ob - ob_rms.mean) / np.sqrt(ob_rms.var + 1e-8), -10.0, 10.0)
        with torch.no_grad():
            _, action, _ = pol.act(torch.tensor(ob, dtype=net), deterministic=True)
        obs, obj, done = env.eval_step(action.float().numpy()[None])
        acc += np.where(alive[:, None], disc * obj[0], 0.0)
        if not raw:
            disc *= gamma
        alive &= ~done[0]
    return acc.sum(0) / eval_num


def ref_mopg_gauss(args, pol, env, weights, iters, noise_fn, net=F64, margins=None):
    """cat_ref.ref_mopg for a Gaussian policy on a one-task host env -> [(policy, objs, storage)]."""
    T, N, O, A, K = args.num_steps, args.num_processes, env.obs_dim, env.act_dim, env.obj_num
    pol = copy.deepcopy(pol).to(net)
    agent = oppo.PPO(pol, args.clip_param, args.ppo_epoch, args.num_mini_batch, args.value_loss_coef,
                     args.entropy_coef, lr=args.lr, eps=1e-5, max_grad_norm=args.max_grad_norm)
    vn = cat_ref.RefVecNormalize(N, O, args.gamma, args.ob_rms, args.obj_rms)
    ro = oppo.RolloutStorage(T, N, O, A, K)
    cat_ref.ref_reset(env, vn, ro)
    total = int(args.num_env_steps) // T // N
    out = []
    for j in range(iters):
        z, perms = noise_fn(j)
        agent.set_lr(oppo.linear_lr(j, total, args.lr, args.lr_decay_ratio))
        ref_rollout_gauss(pol, env, vn, ro, z, margins)
        ro.compute_returns(ro.value_preds[-1].clone(), args.use_gae, args.gamma, args.gae_lambda,
                           args.use_proper_time_limits)
        storage = {k: getattr(ro, k).clone() for k in ('obs', 'actions', 'action_log_probs', 'value_preds', 'rewards',
                                                       'masks', 'bad_masks', 'returns')}
        agent.update(ro, weights, vn.obj_rms.var if vn.obj_rms is not None else None, perms)
        ro.after_update()
        objs = ref_evaluate_gauss(pol, env, copy.deepcopy(vn.ob_rms), args.eval_num, args.raw, args.gamma)
        out.append((copy.deepcopy(pol).double(), objs, storage))
    return out


def mopg_case(discrete, seed):
    """Two host-stepped MOPG iterations of P reference policies on the tiny env behind GymHostVecEnv, fp64 and the
    fp32 arm -> (env name, args, pols, weights, per task [(policy, objs, storage)] per iteration, violations, margins).
    Discrete decisions: the rollout actions (Categorical) and every done / bad flag must agree between the arms, and
    the fp32 arm's objectives stay inside the plain objective band."""
    c = MOPG
    name = envs.DISC if discrete else envs.CONT
    envspec.register_env(name, *((2, 3, 3) if discrete else (5, 1, 2)), discrete=discrete)
    args = small_args(name, num_steps=c['T'], num_processes=c['N'], ppo_epoch=c['E'], num_mini_batch=c['M'],
                      num_env_steps=c['T'] * c['N'] * 10)
    spec = envspec.make_spec(name)
    pols = make_policies(spec, c['P'], seed)
    w = weights_grid(spec['obj_num'], c['P'])
    if discrete:
        fn, worker = ci.mopg_noise_fn(c['T'], c['N'], c['E']), cat_ref.ref_mopg
    else:
        fn, worker = gauss_noise_fn(c['T'], c['N'], spec['act_dim'], c['E']), ref_mopg_gauss
    out, bad, m = [], [], {}
    for p in range(c['P']):
        r64 = worker(args, pols[p], host_env(name, 1, c['N']), w[p], c['iters'], fn, margins=m)
        r32 = worker(args, pols[p], host_env(name, 1, c['N']), w[p], c['iters'], fn, net=torch.float32)
        for j, (a, b) in enumerate(zip(r64, r32)):
            if discrete and not torch.equal(a[2]['actions'], b[2]['actions']):
                bad.append(f'task {p} iteration {j}: the fp32 arm takes other rollout actions')
            if not (torch.equal(a[2]['masks'], b[2]['masks']) and torch.equal(a[2]['bad_masks'], b[2]['bad_masks'])):
                bad.append(f'task {p} iteration {j}: the fp32 arm ends other episodes')
            if not (np.abs(a[1] - b[1]) <= OBJ_BAND[0] + OBJ_BAND[1] * np.abs(a[1])).all():
                bad.append(f'task {p} iteration {j}: the fp32 arm leaves the objective band')
        st = r64[0][2]
        if not int(((st['masks'] == 0) & (st['bad_masks'] == 1)).sum()) > 0:
            bad.append(f'task {p}: no true terminal in the first rollout')
        out.append(r64)
    for k in (('uniform', 'logit') if discrete else ('bound',)):
        if not m[k] >= MARGIN:
            bad.append(f'{k} margin {m[k]:.3g} < {MARGIN}')
    return name, args, pols, w, out, bad, m


MOPG_SEEDS = {True: 1, False: 0}  # discrete -> the first seed from 0 at which mopg_case reports no violation
# (dims, discrete, N) -> the first seed from 0 at which forward_case meets the margin rule, where it is not 0
# (eval_case: 0 everywhere)
FORWARD_SEEDS = {((32, 8, 3), True, 3): 1}
