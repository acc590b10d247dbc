"""Oracle restatement of the Pareto-set re-evaluation (pgmorl_amd.evaluate / pgm_eval_episodes), CPU fp64.

Deterministic arm: for each policy and start state, ``oracle.mopg.evaluation`` itself with ``eval_num = 1``.
Stochastic arm: the same loop with the action mean + exp(logstd) z, z from ``oracle.streams.normal`` at the index the
device documents (episode e, step t, action dim j -> element (e * max_episode_steps + t) * A + j of stream noise_seed).
"""
import argparse

import numpy as np
import torch

from oracle import streams
from oracle.mopg import evaluation
from oracle.vecenv import SynthEnv


def noise_block(noise_seed, e, max_episode_steps, act_dim):
    """z [max_episode_steps][A] of episode e."""
    n = max_episode_steps * act_dim
    return streams.normal(noise_seed, n, start=e * n).reshape(max_episode_steps, act_dim)


def episodes_ref(spec, starts, policy, ob_rms, raw=True, gamma=0.995, noise_seed=None):
    """Per-episode objective sums [E][K] of one policy from the start states ``starts`` [E][O]; ``ob_rms`` None: no
    observation normalisation.  ``noise_seed`` None: the deterministic policy.  With a noise seed also returns the
    smallest distance of any unclipped oracle action to a clip bound."""
    K, A, tmax = spec['obj_num'], spec['act_dim'], spec['max_episode_steps']
    args = argparse.Namespace(obj_num=K, eval_num=1, ob_rms=ob_rms is not None, raw=raw, gamma=gamma)
    if noise_seed is None:
        return np.stack([evaluation(args, spec, s0[None], policy, ob_rms) for s0 in starts])
    out, margin = np.zeros((len(starts), K)), np.inf
    dtype = next(policy.parameters()).dtype
    with torch.no_grad():
        for e, s0 in enumerate(starts):
            z = torch.from_numpy(noise_block(noise_seed, e, tmax, A))
            env = SynthEnv(spec, s0)
            ob = env.reset()
            done, g, t = False, 1.0, 0
            while not done:  # oracle.mopg.evaluation's loop, the action drawn instead of dist.mean
                if ob_rms is not None:
                    ob = np.clip((ob - ob_rms.mean) / np.sqrt(ob_rms.var + 1e-8), -10.0, 10.0)
                _, action, _ = policy.act(torch.tensor(ob, dtype=dtype).unsqueeze(0), noise=z[t][None])
                a = action[0].numpy()
                margin = min(margin, float(np.min(np.abs(a - spec['act_lo']))), float(np.min(np.abs(a - spec['act_hi']))))
                ob, _, done, info = env.step(a)
                out[e] += g * info['obj']
                if not raw:
                    g *= gamma
                t += 1
    return out, margin
