"""The fp64 reference of the discrete-action (Categorical head) path.  TEST INFRASTRUCTURE ONLY.

oracle/ restates the reference's diagonal-Gaussian policy; this module adds, beside it, what a Discrete(n) action space
changes (a2c_ppo_acktr/model.py:33-35, distributions.py:17-27,54-68):

  * CatPolicy      oracle.policy.Policy whose ``dist`` is the Categorical head's Linear (orthogonal gain 0.01, zero
                   bias), with the SAMPLING RULE of include/pgm_abi.h in place of torch's multinomial draw:
                       p = softmax(z);  action = #{ j < A-1 : p_0 + ... + p_j <= u };  logp = z_a - logsumexp(z);
                       deterministic: argmax z.
                   ``evaluate_actions`` returns (value, logp, mean entropy), so oracle.ppo.PPO runs on it unchanged.
  * ref_rollout    morl/mopg.py:103-135 over a host env through the VecNormalize restatement of
                   tests/test_gpu_hostenv.py (_RefVecNormalize), with the distance of every decision from its
                   discontinuity (uniform vs cumulative probability).
  * ref_evaluate   morl/mopg.py:25-46 on the host env's evaluation episodes (top-two logit gap recorded).
  * ref_mopg       the MOPG iterations of oracle.mopg.mopg_worker with the pieces above.
"""
import copy
import math

import numpy as np
import torch
import torch.nn as nn

from oracle import ppo as oppo
from oracle.policy import MOMLPBase, Policy, _orth
from oracle.vecenv import RunningMeanStd

from .helpers import perturb

F64 = torch.float64


class CategoricalHead(nn.Module):
    """distributions.py:54-68: one Linear, orthogonal gain 0.01, zero bias; forward gives the logits."""

    def __init__(self, num_inputs, num_outputs):
        super().__init__()
        self.linear = _orth(nn.Linear(num_inputs, num_outputs), 0.01)

    def forward(self, x):
        return self.linear(x)


class CatPolicy(Policy):
    def __init__(self, obs_dim, num_actions, obj_num, hidden_size=64):
        nn.Module.__init__(self)
        self.base = MOMLPBase(obs_dim, hidden_size, False, obj_num)  # the reference's construction order
        self.dist = CategoricalHead(hidden_size, num_actions)

    def logits(self, x):
        value, feat = self.base(x)
        return value, self.dist(feat)

    def act(self, x, u=None, deterministic=False, margins=None):
        """-> (value, action long [B, 1], logp [B, 1]).  u [B]: one uniform per row.  margins, if a dict, receives
        the smallest |cumulative probability - u| ('uniform') or top-two logit gap ('logit') of the call."""
        value, z = self.logits(x)
        if deterministic:
            action = z.argmax(-1)
            if margins is not None:
                top = z.topk(2, -1).values
                margins['logit'] = min(margins.get('logit', math.inf), float((top[:, 0] - top[:, 1]).min()))
        else:
            cum = torch.softmax(z, -1)[:, :-1].cumsum(-1)
            uu = u.to(z.dtype).reshape(-1, 1)
            action = (cum <= uu).sum(-1)
            if margins is not None:
                margins['uniform'] = min(margins.get('uniform', math.inf), float((cum - uu).abs().min()))
        logp = torch.log_softmax(z, -1).gather(-1, action.unsqueeze(-1))
        return value, action.unsqueeze(-1), logp

    def evaluate_actions(self, x, action):
        value, z = self.logits(x)
        lsm = torch.log_softmax(z, -1)
        logp = lsm.gather(-1, action.long().reshape(-1, 1))
        entropy = -(lsm.exp() * lsm).sum(-1).mean()
        return value, logp, entropy


def make_cat_policy(obs_dim, num_actions, obj_num, hidden_size=64):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        return CatPolicy(obs_dim, num_actions, obj_num, hidden_size).double()
    finally:
        torch.set_default_dtype(prev)


def make_policies(spec, P, seed, scale=0.05):
    """branch_inputs.make_policies for the Categorical head: reference-initialised, rounded to fp32, perturbed (a
    gain-0.01 head alone gives near-uniform logits that test nothing)."""
    torch.manual_seed(seed)
    pols = []
    for _ in range(P):
        pol = make_cat_policy(spec['obs_dim'], spec['act_dim'], spec['obj_num'])
        with torch.no_grad():
            for prm in pol.parameters():
                prm.copy_(prm.float().double())
        pols.append(pol)
    gen = torch.Generator().manual_seed(seed + 100)
    return [perturb(p, scale, gen) for p in pols]


class RefVecNormalize:
    """tests/test_gpu_hostenv.py _RefVecNormalize (VecNormalize.step_wait / reset on supplied transitions, fp64)."""

    def __init__(self, N, O, gamma, use_ob=True, use_obj=True, clipob=10.0, cliprew=10.0, eps=1e-8):
        self.ob_rms = RunningMeanStd(shape=(O,)) if use_ob else None
        self.ret_rms = RunningMeanStd(shape=())
        self.obj_rms = RunningMeanStd(shape=()) if use_obj else None
        self.gamma, self.clipob, self.cliprew, self.eps = gamma, clipob, cliprew, eps
        self.ret, self.obj = np.zeros(N), None

    def _obfilt(self, obs):
        if self.ob_rms is None:
            return obs
        self.ob_rms.update(obs)
        return np.clip((obs - self.ob_rms.mean) / np.sqrt(self.ob_rms.var + self.eps), -self.clipob, self.clipob)

    def reset(self, obs):
        self.ret = np.zeros_like(self.ret)
        return self._obfilt(obs)

    def step(self, obs, rews, dones, objs):
        self.ret = self.ret * self.gamma + rews
        self.obj = self.obj * self.gamma + objs if self.obj is not None else objs.copy()
        obs = self._obfilt(obs)
        self.ret_rms.update(self.ret)
        if self.obj_rms is not None:
            self.obj_rms.update(self.obj)
            objs = np.clip(objs / np.sqrt(self.obj_rms.var + self.eps), -self.cliprew, self.cliprew)
        self.ret[dones] = 0.0
        self.obj[dones] = 0.0
        return obs, objs


def ref_reset(env, vn, ro):
    """envs.reset() of a one-task host env through VecNormalize + the fp32 cast -> ro.obs[0]."""
    ro.obs[0].copy_(torch.from_numpy(vn.reset(env.reset()[0]).astype(np.float32)).double())


def ref_rollout(pol, env, vn, ro, uniforms, margins=None):
    """morl/mopg.py:103-135: T steps of pol on the one-task host env `env` (P = 1) through vn into ro, then the
    bootstrap value.  uniforms [T, N].  The policy may be fp32 (the reference's fp32 arm); envs and statistics fp64."""
    net = next(pol.parameters()).dtype
    T = uniforms.shape[0]
    for t in range(T):
        with torch.no_grad():
            value, action, logp = pol.act(ro.obs[t].to(net), u=uniforms[t], margins=margins)
        obs, rew, done, bad, obj = env.step(action[:, 0].numpy().astype(np.int32)[None])
        o, r = vn.step(obs[0], rew[0], done[0], obj[0])
        masks = torch.tensor(np.where(done[0], 0.0, 1.0), dtype=F64).unsqueeze(-1)
        bads = torch.tensor(np.where(bad[0], 0.0, 1.0), dtype=F64).unsqueeze(-1)
        ro.insert(torch.from_numpy(o.astype(np.float32)).double(), action.double(), logp.double(), value.double(),
                  torch.from_numpy(r).double(), masks, bads)
    with torch.no_grad():
        ro.value_preds[-1] = pol.get_value(ro.obs[-1].to(net)).double()


def ref_evaluate(pol, env, ob_rms, eval_num, raw=True, gamma=1.0, margins=None):
    """morl/mopg.py:25-46 on env's evaluation episodes (one task): fp64 normalisation, deterministic action."""
    net = next(pol.parameters()).dtype
    obs = env.eval_reset(eval_num)
    alive = np.ones(eval_num, dtype=bool)
    acc, disc = np.zeros((eval_num, env.obj_num)), 1.0
    while alive.any():
        ob = obs[0]
        if ob_rms is not None:
            ob = np.clip((ob - ob_rms.mean) / np.sqrt(ob_rms.var + 1e-8), -10.0, 10.0)
        with torch.no_grad():
            m = {} if margins is not None else None
            _, action, _ = pol.act(torch.tensor(ob[alive], dtype=net), deterministic=True, margins=m)
        if margins is not None:
            margins['logit'] = min(margins.get('logit', math.inf), m['logit'])
        a = np.zeros((1, eval_num), dtype=np.int32)
        a[0, alive] = action[:, 0].numpy()
        obs, obj, done = env.eval_step(a)
        acc += np.where(alive[:, None], disc * obj[0], 0.0)
        if not raw:
            disc *= gamma
        alive &= ~done[0]
    return acc.sum(0) / eval_num


def ref_mopg(args, pol, env, weights, iters, noise_fn, net=F64, margins=None):
    """oracle.mopg.mopg_worker for a Categorical policy on a one-task host env, from fresh statistics: per iteration
    the rollout, returns, scalarised PPO update, after_update and the evaluation -> [(policy, objs, storage)]."""
    T, N, O, K = args.num_steps, args.num_processes, env.obs_dim, env.obj_num
    pol = copy.deepcopy(pol).to(net)
    agent = oppo.PPO(pol, args.clip_param, args.ppo_epoch, args.num_mini_batch, args.value_loss_coef,
                     args.entropy_coef, lr=args.lr, eps=1e-5, max_grad_norm=args.max_grad_norm)
    vn = RefVecNormalize(N, O, args.gamma, args.ob_rms, args.obj_rms)
    ro = oppo.RolloutStorage(T, N, O, 1, K)
    ref_reset(env, vn, ro)
    total = int(args.num_env_steps) // T // N
    out = []
    for j in range(iters):
        u, perms = noise_fn(j)
        agent.set_lr(oppo.linear_lr(j, total, args.lr, args.lr_decay_ratio))
        ref_rollout(pol, env, vn, ro, u, margins)
        ro.compute_returns(ro.value_preds[-1].clone(), args.use_gae, args.gamma, args.gae_lambda,
                           args.use_proper_time_limits)
        storage = {k: getattr(ro, k).clone() for k in ('obs', 'actions', 'action_log_probs', 'value_preds', 'rewards',
                                                       'masks', 'bad_masks', 'returns')}
        agent.update(ro, weights, vn.obj_rms.var if vn.obj_rms is not None else None, perms)
        ro.after_update()
        objs = ref_evaluate(pol, env, copy.deepcopy(vn.ob_rms), args.eval_num, args.raw, args.gamma, margins)
        out.append((copy.deepcopy(pol).double(), objs, storage))
    return out
