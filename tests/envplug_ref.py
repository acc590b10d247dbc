"""The fp64 reference of the env plug-in tests: two MOPG iterations of the reference worker (tests/anydims_ref.py's
Gaussian worker, tests/cat_ref.py's Categorical one) on the numpy restatement of a test plug-in behind the HostVecEnv
protocol (tests/envplug_envs.py), and the evaluation case of chain.hpp under cat_inputs' logit-margin rule.

Seeds follow the rule of tests/anydims_ref.py: the first one, counting up from 0, at which the reference alone meets
every condition -- its fp32 arm takes the same discrete decisions as its fp64 arm, every decision margin (action clip,
terminal bound, uniform, logit) is at least MARGIN = 1e-4, and the fp32 arm's objectives stay inside the plain
objective band.  Found on the CPU, recorded below and in DESIGN.md 24; tests/test_envplug.py re-checks them.
"""
import copy
import functools

import numpy as np
import torch

from oracle.vecenv import RunningMeanStd
from pgmorl_amd import envspec

from . import anydims_ref as ar
from . import cat_inputs as ci
from . import cat_ref
from . import envplug_envs as pe
from .branch_inputs import MARGIN
from .helpers import small_args, weights_grid

MOPG = dict(P=2, T=64, N=4, E=2, M=4, iters=2, R=3)
OBJ_BAND = ar.OBJ_BAND


def register(env):
    envspec.register_env(env.ENV, env.O, env.A, env.K, discrete=env.DISCRETE)
    return env.ENV


def mopg_case(env, seed):
    """-> (env name, args, pols, weights, per task [(policy, objs, storage)] per iteration, violations, margins)"""
    c = MOPG
    name = register(env)
    args = small_args(name, num_steps=c['T'], num_processes=c['N'], ppo_epoch=c['E'], num_mini_batch=c['M'],
                      num_env_steps=c['T'] * c['N'] * 10)
    spec = envspec.make_spec(name)
    pols = ar.make_policies(spec, c['P'], seed)
    w = weights_grid(env.K, c['P'])
    disc = env.DISCRETE
    fn = ci.mopg_noise_fn(c['T'], c['N'], c['E']) if disc else ar.gauss_noise_fn(c['T'], c['N'], env.A, c['E'])
    worker = cat_ref.ref_mopg if disc else ar.ref_mopg_gauss
    out, bad, m = [], [], {}
    for p in range(c['P']):
        host = lambda margins=None: pe.NumpyPluginHostVecEnv(env, 1, c['N'], seed=0, R=c['R'], margins=margins)  # noqa: E731
        r64 = worker(args, pols[p], host(m), w[p], c['iters'], fn, **({'margins': m} if disc else {}))
        r32 = worker(args, pols[p], host(), w[p], c['iters'], fn, net=torch.float32)
        for j, (a, b) in enumerate(zip(r64, r32)):
            if disc and not torch.equal(a[2]['actions'], b[2]['actions']):
                bad.append(f'task {p} iteration {j}: the fp32 arm takes other rollout actions')
            if not (torch.equal(a[2]['masks'], b[2]['masks']) and torch.equal(a[2]['bad_masks'], b[2]['bad_masks'])):
                bad.append(f'task {p} iteration {j}: the fp32 arm ends other episodes')
            if not (np.abs(a[1] - b[1]) <= OBJ_BAND[0] + OBJ_BAND[1] * np.abs(a[1])).all():
                bad.append(f'task {p} iteration {j}: the fp32 arm leaves the objective band')
        st = r64[0][2]
        if not int(((st['masks'] == 0) & (st['bad_masks'] == 1)).sum()) > 0:
            bad.append(f'task {p}: no true terminal in the first rollout')
        out.append(r64)
    for k in (('uniform', 'logit') if disc else ('env',)):
        if not m[k] >= MARGIN:
            bad.append(f'{k} margin {m[k]:.3g} < {MARGIN}')
    return name, args, pols, w, out, bad, m


# env NAME -> the first seed from 0 at which mopg_case reports no violation
MOPG_SEEDS = {'line': 0, 'chain': 0}


def chain_eval_case(E, use_ob, seed):
    """The chain's evaluation under cat_inputs' margin rule: along every evaluation episode of the fp64 reference the
    top two logits are >= MARGIN apart and the fp32 arm picks the same actions (so it runs the same episodes)
    -> (pols, rms, reference objectives [P][K] (raw), violations, margins)."""
    env, P = pe.Chain, 3
    spec = envspec.make_spec(register(env))
    pols = ar.make_policies(spec, P, seed)
    rng = np.random.RandomState(seed + 7 + E)
    rms, want, bad, m = [], [], [], {}
    for p in range(P):
        r = RunningMeanStd(shape=(env.O,))
        r.update(rng.rand(50, env.O))
        rms.append(r)
        host = lambda: pe.NumpyPluginHostVecEnv(env, 1, 1, seed=0, R=3)  # noqa: E731
        o64 = cat_ref.ref_evaluate(pols[p], host(), r if use_ob else None, E, margins=m)
        o32 = cat_ref.ref_evaluate(copy.deepcopy(pols[p]).float(), host(), r if use_ob else None, E)
        if not np.array_equal(o64, o32):  # (the chain's objectives are exact sums of k / 6: other actions show)
            bad.append(f'task {p}: the fp32 arm picks other actions')
        want.append(o64)
    if not m['logit'] >= MARGIN:
        bad.append(f'logit margin {m["logit"]:.3g} < {MARGIN}')
    return pols, rms, np.stack(want), bad, m


@functools.lru_cache(maxsize=None)
def chain_eval_seed(E, use_ob):
    return ci.first_seed(lambda s: chain_eval_case(E, use_ob, s))
