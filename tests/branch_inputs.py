"""Branch-rich inputs for the PPO update kernels, and the conditions on them that are checked from the oracle alone.

tests/test_gpu_kernels.py _update_setup perturbs the old log-probs by N(0, 0.05) against a clip of 0.2 and leaves every
hyper-parameter at its default: no row of its first epoch has a clipped ratio, and the gradient norm is above
max_grad_norm at every step.  build_inputs draws the same kind of storage (obs, actions, old log-probs, old values,
returns and advantages from the policy's own fp64 forward) with the offsets placed so that every branch of
a2c_ppo_acktr/algo/ppo.py:76-103 is populated at every Adam step:

  * log-ratio offsets from a three-way mixture placed relative to log(1 +- clip_param): a near-1 group inside the
    clip range, a group beyond the upper edge and a group beyond the lower edge, each GAP away from its edge;
    advantages N(0, 1) of either sign, independent of the group, so all four (edge, sign) combinations occur;
  * old-value offsets from a two-way mixture: within +-clip_param / 2, and beyond +-clip_param by at least GAP;
  * returns = old values + N(0, RET_NOISE), so that both arms of torch.max win among the clip-active elements.

Parameters move by several 1e-3 per Adam step and rows do cross boundaries between steps, so the construction alone
keeps no row off a discontinuity.  conditions() therefore checks, from the oracle's per-step trace
(oracle.ppo.PPO(trace=[])), the branch shares and the distance of every row from every discontinuity, and oracle_case()
adds that the oracle's own fp32 arm takes the same decision for every row at every step.  The seed of a case is the
first one, counting up from BASE_SEED, at which the oracle meets all of this (SEEDS; found by scan_seed on the CPU,
never by looking at a device).
"""
import copy
import functools
import math

import numpy as np
import torch

from oracle import ppo as oppo
from oracle.policy import make_policy
from pgmorl_amd import envspec

from .helpers import perturb, small_args

LR = 3e-4
BASE_SEED = 11
MIX_RATIO = (0.4, 0.3, 0.3)  # near 1 | beyond the upper edge | beyond the lower edge
MIX_VALUE = 0.5              # share of old values within the clip range
GAP = 0.05                   # distance of a far group from its edge at the initial parameters
FAR = 0.2                    # a far group is uniform over this much beyond the gap
RET_NOISE = 0.5
MARGIN = 1e-4  # twice the widest forward band of test_act_forward (5e-5 on log-prob, 2e-5 + 1e-5 rel on values)

HP_DEFAULT = dict(clip_param=0.2, value_loss_coef=0.5, entropy_coef=0.0, max_grad_norm=0.5, adam_eps=1e-5, beta1=0.9,
                  beta2=0.999, use_clipped_value_loss=True)
ROWS = {'a': {},
        'b': {'use_clipped_value_loss': False},
        'c': {'max_grad_norm': 10.0},
        'd': {'clip_param': 0.1, 'value_loss_coef': 1.0},
        'e': {'adam_eps': 1e-3, 'beta1': 0.8, 'beta2': 0.99},
        'f': {'entropy_coef': 0.01}}
# name -> (env, P, T, N, E, M)
SHAPES = {'hopper2': ('MO-Hopper-v2', 2, 64, 4, 2, 2),      # 128-row minibatches, 4 steps: both slot parities twice
          'hopper3': ('MO-Hopper-v3', 2, 50, 3, 1, 3),      # K = 3, ragged 50-row minibatches
          'hopper3x64': ('MO-Hopper-v3', 2, 64, 3, 1, 3),   # K = 3 at 64 rows: the feature-split kernel takes no
                                                           # ragged minibatch (the launcher's mb % 16 rule)
          'walker': ('MO-Walker2d-v2', 3, 64, 4, 1, 2),     # O = 17
          'humanoid32': ('MO-Humanoid-v2', 2, 32, 8, 1, 2),
          'humanoid50': ('MO-Humanoid-v2', 2, 50, 3, 1, 3)}
# (shape, layernorm, row) -> the first seed from BASE_SEED at which the oracle meets every condition.
# Found by scan_seed on the CPU; the worst share and margin over every step and task of each are in DESIGN.md 16
# (overall: smallest sign-case share 0.06 at the 50-row shapes, smallest margins 1.1e-4 on the log ratio, 1.3e-4 on
# the value clip and 1.3e-4 on the max tie).  Seeds 12 / 13: the earlier ones break a share or a margin.
SEEDS = {(s, ln, r): BASE_SEED for s, ln, rows in (('hopper2', False, 'abcdef'), ('hopper3', False, 'a'),
                                                   ('hopper3x64', False, 'a'), ('walker', False, 'a'),
                                                   ('humanoid32', False, 'abcdef'), ('humanoid50', False, 'a'),
                                                   ('hopper2', True, 'abcdef'), ('hopper3', True, 'a'))
         for r in rows}
SEEDS.update({('hopper2', False, 'd'): 12, ('hopper3x64', False, 'a'): 13, ('humanoid32', False, 'a'): 12,
              ('humanoid32', False, 'f'): 12})


def hparams(row):
    return dict(HP_DEFAULT, **ROWS[row])


def make_policies(spec, P, seed, layernorm=False):
    """The policies of _batch_with_policies / _ln_batch: reference-initialised, rounded to fp32, perturbed."""
    torch.manual_seed(seed)
    pols = []
    for _ in range(P):
        pol = make_policy(spec['obs_dim'], spec['act_dim'], spec['obj_num'], layernorm=layernorm)
        with torch.no_grad():
            for prm in pol.parameters():
                prm.copy_(prm.float().double())
        pols.append(pol)
    gen = torch.Generator().manual_seed(seed + 100)
    return [perturb(p, 0.05, gen) for p in pols]


def build_inputs(env, P, T, N, E, M, seed, hp=None, layernorm=False):
    """_update_setup's arguments plus the hyper-parameters -> (args, spec, pols, data, perms) without a device:
    data = (obs, actions, logp, values, returns, adv) as fp32 arrays shaped like the TaskBatch buffers."""
    hp = dict(HP_DEFAULT, **(hp or {}))
    clip = hp['clip_param']
    args = small_args(env, num_steps=T, num_processes=N, ppo_epoch=E, num_mini_batch=M, layernorm=layernorm,
                      **{k: hp[k] for k in ('clip_param', 'value_loss_coef', 'entropy_coef', 'max_grad_norm')})
    spec = envspec.make_spec(env)
    pols = make_policies(spec, P, seed, layernorm)
    O, A, K, B = spec['obs_dim'], spec['act_dim'], spec['obj_num'], T * N
    rng = np.random.RandomState(seed)
    obs = np.clip(rng.randn(P, T + 1, N, O), -3, 3).astype(np.float32)
    eps = rng.randn(P, T, N, A)
    up, lo = math.log1p(clip), math.log1p(-clip)
    acts, lps, vals = [], [], []
    for p in range(P):
        with torch.no_grad():
            v, a, lp = pols[p].act(torch.from_numpy(obs[p, :T]).double().reshape(B, O),
                                   noise=torch.from_numpy(eps[p]).reshape(B, A))
        group = rng.choice(3, size=B, p=MIX_RATIO)
        u = rng.rand(B)
        log_ratio = np.where(group == 0, lo / 2 + u * (up - lo) / 2,
                             np.where(group == 1, up + GAP + u * FAR, lo - GAP - u * FAR))
        far = rng.rand(B, K) >= MIX_VALUE
        sign = np.where(rng.rand(B, K) < 0.5, -1.0, 1.0)
        u = rng.rand(B, K)
        v_off = np.where(far, sign * (clip + GAP + u * FAR), (u - 0.5) * clip)
        acts.append(a.float().reshape(T, N, A))
        lps.append((lp[:, 0] - torch.from_numpy(log_ratio)).float().reshape(T, N))
        vals.append((v + torch.from_numpy(v_off)).float().reshape(T, N, K))
    actions, logp, values = torch.stack(acts), torch.stack(lps), torch.stack(vals)
    values = torch.cat([values, torch.zeros(P, 1, N, K)], 1)
    returns = values + torch.from_numpy(rng.randn(P, T + 1, N, K) * RET_NOISE).float()
    adv = torch.from_numpy(rng.randn(P, T, N)).float()
    perms = [torch.randperm(B, generator=torch.Generator().manual_seed(seed * 10 + e)) for e in range(E)]
    return args, spec, pols, (obs, actions, logp, values, returns, adv), perms


def run_oracle(pol, hp, data, p, perms, shape, dtype=torch.float64, ppo_cls=oppo.PPO):
    """The update of task p on a copy of pol (cast to dtype) -> (policy, agent, mean loss stats, per-step trace)."""
    env, _, T, N, E, M = shape
    obs, actions, logp, values, returns, adv = data
    pol = copy.deepcopy(pol).to(dtype)
    trace = []
    agent = ppo_cls(pol, hp['clip_param'], E, M, hp['value_loss_coef'], hp['entropy_coef'], lr=LR, eps=hp['adam_eps'],
                    max_grad_norm=hp['max_grad_norm'], use_clipped_value_loss=hp['use_clipped_value_loss'],
                    betas=(hp['beta1'], hp['beta2']), trace=trace)
    ro = oppo.RolloutStorage(T, N, obs.shape[-1], actions.shape[-1], values.shape[-1])
    ro.obs.copy_(torch.from_numpy(obs[p]).double())
    ro.actions.copy_(actions[p].double())
    ro.action_log_probs.copy_(logp[p].double().unsqueeze(-1))
    ro.value_preds.copy_(values[p].double())
    ro.returns.copy_(returns[p].double())
    stats = np.zeros(3)
    for e in range(E):
        for mbt in ro.minibatches(adv[p].double(), M, perms[e]):
            stats += agent.minibatch_step(*mbt)
    return pol.double(), agent, stats / (E * M), trace


def flat_state(pol, agent):
    """(params, exp_avg, exp_avg_sq) concatenated in parameters() order, fp64 (no device layout needed)."""
    st = agent.optimizer.state
    prm = list(pol.parameters())
    cat = lambda xs: torch.cat([x.detach().double().reshape(-1) for x in xs]).numpy()
    return cat(prm), cat([st[q]['exp_avg'] for q in prm]), cat([st[q]['exp_avg_sq'] for q in prm])


def decisions(rec, hp):
    """The branch every row / element of one traced step takes: (ratio region -1 / 0 / +1, zero-gradient rows,
    value clip active, clipped term wins) and the distances from the discontinuities that decide them."""
    clip = hp['clip_param']
    lr_, adv = torch.log(rec['ratio'].double()), rec['adv'].double()
    up, lo = math.log1p(clip), math.log1p(-clip)
    region = (lr_ > up).int() - (lr_ < lo).int()
    zero_up, zero_lo = (region > 0) & (adv > 0), (region < 0) & (adv < 0)
    v, vo, ret = rec['values'].double(), rec['old_values'].double(), rec['returns'].double()
    active = (v - vo).abs() > clip
    v_clip = vo + (v - vo).clamp(-clip, clip)
    wins = (v_clip - ret).pow(2) > (v - ret).pow(2)  # the clipped term is the max (only possible where active)
    margins = {'ratio': float(torch.minimum((lr_ - up).abs(), (lr_ - lo).abs()).min()),
               'value_clip': float(((v - vo).abs() - clip).abs().min()),
               'max_tie': float((ret - (v + v_clip) / 2).abs()[active].min()) if active.any() else math.inf}
    return {'region': region, 'zero_up': zero_up, 'zero_lo': zero_lo, 'active': active, 'wins': wins & active,
            'margins': margins}


def conditions(trace, hp):
    """The issue's conditions of type 1 (branch shares) and 2 (margins) at every step of one task's trace, plus the
    side of clip_grad_norm_'s clamp.  Returns (violations, worst) -- worst holds the smallest share / margin seen."""
    bad, worst = [], {}

    def need(step, name, got, floor):
        worst[name] = min(worst.get(name, math.inf), got)
        if not got >= floor:
            bad.append(f'step {step}: {name} {got:.4g} < {floor}')
    cap = hp['max_grad_norm']
    for s, rec in enumerate(trace):
        d = decisions(rec, hp)
        share = lambda m: float(m.double().mean())
        need(s, 'zero-gradient rows', share(d['zero_up'] | d['zero_lo']), 0.15)
        need(s, 'zero-gradient rows, ratio above, adv > 0', share(d['zero_up']), 0.05)
        need(s, 'zero-gradient rows, ratio below, adv < 0', share(d['zero_lo']), 0.05)
        need(s, 'outside-but-passing rows', share((d['region'] != 0) & ~(d['zero_up'] | d['zero_lo'])), 0.10)
        need(s, 'inside rows', share(d['region'] == 0), 0.20)
        need(s, 'margin: log ratio from log(1 +- clip)', d['margins']['ratio'], MARGIN)
        if hp['use_clipped_value_loss']:
            need(s, 'value clip active', share(d['active']), 0.25)
            need(s, 'clipped term wins', share(d['wins']), 0.05)
            need(s, 'unclipped term wins while clip-active', share(d['active'] & ~d['wins']), 0.05)
            need(s, 'margin: |v - v_old| from clip', d['margins']['value_clip'], MARGIN)
            need(s, 'margin: return from the max tie', d['margins']['max_tie'], MARGIN)
        g = rec['grad_norm']
        if cap > 1.0:  # row c: the coefficient is exactly 1
            need(s, 'cap / norm (norm < 0.9 cap)', cap / g, 1 / 0.9)
        else:          # every other row: the coefficient is below 1
            need(s, 'norm / cap (norm > 1.1 cap)', g / cap, 1.1)
    return bad, worst


def same_decisions(trace64, trace32, hp):
    """Type 3: the oracle's fp32 arm takes the fp64 arm's decision for every row at every step."""
    bad = []
    keys = ('region', 'zero_up', 'zero_lo') + (('active', 'wins') if hp['use_clipped_value_loss'] else ())
    for s, (a, b) in enumerate(zip(trace64, trace32)):
        da, db = decisions(a, hp), decisions(b, hp)
        for k in keys:
            n = int((da[k] != db[k]).sum())
            if n:
                bad.append(f'step {s}: {n} rows differ in {k} between the fp64 and fp32 arms')
        if (a['grad_norm'] > hp['max_grad_norm']) != (b['grad_norm'] > hp['max_grad_norm']):
            bad.append(f'step {s}: the norm clamp differs between the arms')
    if len(trace64) != len(trace32):
        bad.append('trace lengths differ')
    return bad


def evaluate_case(shape_name, layernorm, row, seed):
    """One candidate seed of a case, from the oracle alone -> (inputs, per-task fp64 results, violations, worst)."""
    shape, hp = SHAPES[shape_name], hparams(row)
    env, P, T, N, E, M = shape
    inputs = build_inputs(env, P, T, N, E, M, seed, hp, layernorm)
    _, _, pols, data, perms = inputs
    results, bad, worst = [], [], {}
    for p in range(P):
        r64 = run_oracle(pols[p], hp, data, p, perms, shape)
        r32 = run_oracle(pols[p], hp, data, p, perms, shape, dtype=torch.float32)
        b, w = conditions(r64[3], hp)
        bad += [f'task {p}: {x}' for x in b] + [f'task {p}: {x}' for x in same_decisions(r64[3], r32[3], hp)]
        for k, x in w.items():
            worst[k] = min(worst.get(k, math.inf), x)
        # how far the fp32 arm ends from the fp64 arm, for the record: (params, exp_avg, exp_avg_sq rel)
        f64, f32 = flat_state(r64[0], r64[1]), flat_state(r32[0], r32[1])
        worst['fp32 arm: params'] = max(worst.get('fp32 arm: params', 0.0), float(np.abs(f64[0] - f32[0]).max()))
        results.append(r64)
    return inputs, results, bad, worst


def scan_seed(shape_name, layernorm, row, tries=40):
    """The first seed from BASE_SEED at which the oracle meets every condition (CPU only)."""
    for seed in range(BASE_SEED, BASE_SEED + tries):
        _, _, bad, worst = evaluate_case(shape_name, layernorm, row, seed)
        if not bad:
            return seed, worst
    raise AssertionError(f'no seed in {tries} tries for {(shape_name, layernorm, row)}: last {bad[:3]}')


@functools.lru_cache(maxsize=None)
def oracle_case(shape_name, layernorm, row):
    """The case at its recorded seed: inputs and the fp64 oracle's result per task, computed once and shared by every
    kernel's test of the case (callers must not modify it).  Asserts the conditions before anything is returned."""
    seed = SEEDS[(shape_name, layernorm, row)]
    inputs, results, bad, worst = evaluate_case(shape_name, layernorm, row, seed)
    assert not bad, f'{(shape_name, layernorm, row)} seed {seed}: the oracle does not meet the input conditions: {bad}'
    return inputs, results, worst
