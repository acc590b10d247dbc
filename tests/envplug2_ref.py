"""The fp64 reference side of the contract-2 plug-in tests: the reference worker of tests/anydims_ref.py /
tests/cat_ref.py stepping the numpy restatements of tests/envplug2_envs.py, which pass the ctx (the runtime parameters
and the env-noise stream at the fused path's indices).

``conditions`` replays the first rollout of the GPU test's fused-vs-host-stepped case on the CPU and counts what that
case needs to see (true terminals, forced limits, auto-resets, steps on either side of the w0 < p threshold): the
parameter values and seeds of COND were picked with it, and tests/test_envplug2.py re-checks them.  ``mopg_case`` is
tests/envplug_ref.py's iteration for slip.hpp under that file's seed rule.
"""
import numpy as np
import torch

from oracle import ppo as oppo
from pgmorl_amd import envspec

from . import anydims_ref as ar
from . import cat_ref
from . import envplug2_envs as p2
from . import envplug_ref as er
from .branch_inputs import MARGIN
from .helpers import small_args, weights_grid

P, T, R = 3, 40, 3  # the shapes of tests/test_gpu_envplug2.py
# env NAME -> the parameters, the policy seed and the noise seed of the fused-vs-host-stepped case.  Chosen so that
# `conditions` holds at N = 1, 3 and 8 (the counts: test_envplug2.test_recorded_conditions).
COND = {'slip': dict(env_params={'slip': 0.3, 'wind': 0.125}, pol_seed=0, noise_seed=4),
        'gather': dict(env_params={'p_attack': 0.5}, pol_seed=0, noise_seed=4)}
# (env NAME, N) -> (true terminals, forced limits, auto-resets, words below p, words at or above p) of `conditions`
COUNTS = {('slip', 1): (5, 5, 10, 19, 21), ('slip', 3): (31, 7, 38, 54, 66), ('slip', 8): (79, 28, 107, 115, 205),
          ('gather', 1): (5, 9, 14, 22, 18), ('gather', 3): (50, 16, 66, 62, 58), ('gather', 8): (95, 51, 146, 170, 150)}
MOPG = dict(er.MOPG, env_params={'slip': 0.3, 'wind': 0.02})


def register(env):
    return er.register(env)


def policies(env, n, seed):
    return ar.make_policies(envspec.make_spec(register(env)), n, seed)


def noise(env, N, rounds, seed, T=T):
    """The action noise of `rounds` rollouts: uniforms [rounds][T][N] (Categorical) or normals [rounds][T][N][A]."""
    g = torch.Generator().manual_seed(seed)
    if env.DISCRETE:
        return torch.rand(rounds, T, N, generator=g, dtype=torch.float32)
    return torch.randn(rounds, T, N, env.A, generator=g, dtype=torch.float32)


def count(masks, bad_masks, w0, p0):
    """What the first rollout must contain, from its masks / bad_masks [.., T, N] (slots 1..T) and its first env-noise
    word per (step, env) against the first parameter."""
    m, b = np.asarray(masks) == 0, np.asarray(bad_masks) == 0
    return {'terminals': int((m & ~b).sum()), 'limits': int((m & b).sum()), 'resets': int(m.sum()),
            'below': int((np.asarray(w0) < p0).sum()), 'above': int((np.asarray(w0) >= p0).sum())}


def meets(c):
    return c['terminals'] >= 1 and c['limits'] >= 1 and c['resets'] >= 2 and c['below'] >= 1 and c['above'] >= 1


def conditions(env, N, rollout_seed=0):
    """The first rollout of the GPU case replayed by the fp64 reference (one task at a time) -> count()'s dict."""
    c = COND[env.NAME]
    pols = policies(env, P, c['pol_seed'])
    z = noise(env, N, 2, c['noise_seed'])[0]
    masks, bads = [], []
    for pol in pols:
        host = p2.NumpyPlugin2HostVecEnv(env, 1, N, seed=0, R=R, env_params=c['env_params'])
        vn = cat_ref.RefVecNormalize(N, env.O, 0.995, True, True)
        ro = oppo.RolloutStorage(T, N, env.O, 1 if env.DISCRETE else env.A, env.K)
        cat_ref.ref_reset(host, vn, ro)
        host.begin_rollout(p2.env_seed(rollout_seed))
        (cat_ref.ref_rollout if env.DISCRETE else ar.ref_rollout_gauss)(pol, host, vn, ro, z)
        masks.append(ro.masks[1:, :, 0].numpy())
        bads.append(ro.bad_masks[1:, :, 0].numpy())
    w0 = p2.u53(p2.env_seed(rollout_seed), 0, T * N * env.NW).reshape(T, N, env.NW)[..., 0]
    return count(np.stack(masks), np.stack(bads), w0, p2.par_vector(env, c['env_params'])[0])


def mopg_case(env, seed):
    """envplug_ref.mopg_case for a contract-2 header: rollout j draws the env noise of env_seed(j), the evaluation
    that of env_seed(0) (the batch's seed)
    -> (env name, args, pols, weights, per task [(policy, objs, storage)] per iteration, violations, margins)"""
    c = MOPG
    name = register(env)
    args = small_args(name, num_steps=c['T'], num_processes=c['N'], ppo_epoch=c['E'], num_mini_batch=c['M'],
                      num_env_steps=c['T'] * c['N'] * 10)
    pols = policies(env, c['P'], seed)
    w = weights_grid(env.K, c['P'])
    fn = ar.gauss_noise_fn(c['T'], c['N'], env.A, c['E'])
    out, bad, m = [], [], {}
    for p in range(c['P']):
        host = lambda margins=None: p2.NumpyPlugin2HostVecEnv(  # noqa: E731
            env, 1, c['N'], seed=0, R=c['R'], env_params=c['env_params'], margins=margins, T=c['T'],
            rollout_seeds=list(range(c['iters'])))
        r64 = ar.ref_mopg_gauss(args, pols[p], host(m), w[p], c['iters'], fn)
        r32 = ar.ref_mopg_gauss(args, pols[p], host(), w[p], c['iters'], fn, net=torch.float32)
        for j, (a, b) in enumerate(zip(r64, r32)):
            if not (torch.equal(a[2]['masks'], b[2]['masks']) and torch.equal(a[2]['bad_masks'], b[2]['bad_masks'])):
                bad.append(f'task {p} iteration {j}: the fp32 arm ends other episodes')
            if not (np.abs(a[1] - b[1]) <= er.OBJ_BAND[0] + er.OBJ_BAND[1] * np.abs(a[1])).all():
                bad.append(f'task {p} iteration {j}: the fp32 arm leaves the objective band')
        st = r64[0][2]
        if not int(((st['masks'] == 0) & (st['bad_masks'] == 1)).sum()) > 0:
            bad.append(f'task {p}: no true terminal in the first rollout')
        out.append(r64)
    if not m['env'] >= MARGIN:
        bad.append(f'env margin {m["env"]:.3g} < {MARGIN}')
    return name, args, pols, w, out, bad, m


# the first seed from 0 at which mopg_case(Slip, seed) reports no violation
MOPG_SEED = 0
