"""Re-evaluate a saved Pareto set on the device.

    python -m pgmorl_amd.evaluate SAVE_DIR [--episodes 32] [--eval-seed S] [--stochastic] [--noise-seed Z]
                                           [--out DIR] [--device cuda] [--chunk C]

A finished run leaves ``final/EP_policy_i.pt``, ``final/EP_env_params_i.pkl`` and ``final/objs.txt``; every stored
objective vector was measured once, over ``--eval-num`` episodes from the training seed's own reset rows, and the
archive kept whatever measured best.  This module reads the set back and measures every member over many episodes
(``pgm_eval_episodes``: one workgroup per policy and chunk of 8 episodes), from start states the caller chooses, with
the deterministic or the stochastic policy, keeping the per-episode returns.  SynthMO device envs only.

``load_pareto_set`` reads a save dir, ``evaluate_policies`` runs the kernel on flat parameters, ``main`` is the
command: it writes ``objs.txt`` (the re-evaluated means, the reference's ``'{:5f}'`` lines, member order),
``episodes.npy`` [M][E][K] and ``summary.json`` into ``--out`` (default ``SAVE_DIR/eval``).
"""
import argparse
import ast
import ctypes as C
import json
import os
import pickle
import re
import sys

import numpy as np
import torch

from . import envspec
from ._lib import EVAL_EPISODES_MAX, Dims, EnvSpec, PGMError, check, lib, require_eval_episodes
from .layout import ParamLayout
from .pareto import compute_hypervolume, compute_sparsity, get_ep_indices

SPEC_KEYS = ('d', 'U', 'c', 'V', 'ebase', 'ecoef', 'act_lo', 'act_hi')
SCOPE = 'this tool covers the SynthMO device envs'


def noise_index(e, t, j, max_episode_steps, act_dim):
    """Element of the counter stream ``noise_seed`` (oracle/streams.py ``normal``) that episode e, step t, action dim
    j of a stochastic re-evaluation draws -- the same for every policy."""
    return (int(e) * int(max_episode_steps) + int(t)) * int(act_dim) + int(j)


def _synth_spec(env_name, what):
    """envspec's constants of a SynthMO device env; PGMError for every other env family."""
    try:
        sp = envspec.make_spec(env_name)
    except ValueError as e:
        raise PGMError(f'{what}: {e}; {SCOPE}') from e
    if sp.get('native') or sp.get('discrete') or sp.get('user'):
        raise PGMError(f'{what}: {env_name} is not a SynthMO env; {SCOPE}')
    return sp


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def evaluate_policies(env_name, params, ob_mean, ob_var, episodes, eval_seed, stochastic=False, noise_seed=0,
                      gamma=0.995, raw=True, use_ob_rms=True, layernorm=False, device='cuda', max_episode_steps=None,
                      chunk=4096, return_objs=False):
    """``episodes`` episodes of each of the M policies ``params`` [M][L] (flat fp32 rows in the ParamLayout of the env,
    ``layernorm`` selecting the LayerNorm layout) -> the per-episode objective sums [M][episodes][K], numpy fp64
    (discounted by ``gamma`` unless ``raw``); with ``return_objs`` also the device's per-policy means [M][K].
    Episode e starts from ``envspec.reset_table(O, eval_seed, episodes)[e]``; observations are normalised with each
    policy's own frozen ``ob_mean`` / ``ob_var`` [M][O] (``use_ob_rms``).  ``stochastic`` draws the action noise from
    the counter stream ``noise_seed`` (``noise_index``), the same draws for every policy.  ``max_episode_steps``
    overrides the env's episode length.  M is not a population: the policies are uploaded in slices of at most
    ``chunk``, each one launch."""
    what = 'evaluate_policies'
    sp = _synth_spec(env_name, what)
    O, A, K = sp['obs_dim'], sp['act_dim'], sp['obj_num']
    E, chunk = int(episodes), int(chunk)
    if not 1 <= E <= EVAL_EPISODES_MAX:
        raise PGMError(f'{what}: episodes={E} outside [1, {EVAL_EPISODES_MAX}]')
    if chunk < 1:
        raise PGMError(f'{what}: chunk={chunk} policies per launch must be at least 1')
    tmax = int(sp['max_episode_steps'] if max_episode_steps is None else max_episode_steps)
    if tmax < 1:
        raise PGMError(f'{what}: max_episode_steps={tmax} must be at least 1')
    layout = ParamLayout(O, A, K, layernorm=bool(layernorm))
    params = torch.as_tensor(params)
    if params.dim() != 2 or params.shape[1] != layout.total or params.dtype != torch.float32:
        raise PGMError(f'{what}: params must be fp32 [M][{layout.total}] for {env_name}'
                       f'{" with LayerNorm towers" if layernorm else ""}; got {params.dtype} {tuple(params.shape)}')
    M = params.shape[0]
    if M < 1:
        raise PGMError(f'{what}: no policies')
    stats = [None, None]
    if use_ob_rms:
        for i, (name, v) in enumerate((('ob_mean', ob_mean), ('ob_var', ob_var))):
            if v is None:
                raise PGMError(f'{what}: {name} is required with use_ob_rms')
            v = torch.as_tensor(v)
            if tuple(v.shape) != (M, O) or v.dtype != torch.float64:
                raise PGMError(f'{what}: {name} must be fp64 [{M}][{O}]; got {v.dtype} {tuple(v.shape)}')
            stats[i] = v
    require_eval_episodes()
    dev = torch.device(device)
    f64 = dict(dtype=torch.float64, device=dev)
    spec_t = {k: torch.tensor(np.ascontiguousarray(sp[k]), **f64) for k in SPEC_KEYS}
    c_spec = EnvSpec(*(_ptr(spec_t[k]) for k in SPEC_KEYS), tmax, 0)
    starts = torch.tensor(envspec.reset_table(O, int(eval_seed), E), **f64)
    out = np.empty((M, E, K), dtype=np.float64)
    objs = np.empty((M, K), dtype=np.float64)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for lo in range(0, M, chunk):
            hi = min(M, lo + chunk)
            prm = params[lo:hi].to(dev).contiguous()
            mean, var = (None if s is None else s[lo:hi].to(dev).contiguous() for s in stats)
            ep_d = torch.empty(hi - lo, E, K, **f64)
            objs_d = torch.empty(hi - lo, K, **f64)
            d = Dims(hi - lo, 1, 0, O, A, K, 64, int(bool(layernorm)))
            check(lib().pgm_eval_episodes(C.byref(d), _ptr(prm), C.byref(c_spec), _ptr(mean), _ptr(var), _ptr(starts),
                                          E, int(bool(use_ob_rms)), int(bool(raw)), float(gamma),
                                          int(bool(stochastic)), int(noise_seed) & (2**64 - 1), _ptr(ep_d),
                                          _ptr(objs_d), stream), 'pgm_eval_episodes')
            out[lo:hi] = ep_d.cpu().numpy()
            objs[lo:hi] = objs_d.cpu().numpy()
    return (out, objs) if return_objs else out


def _members(final, pattern):
    """Indices i of the files ``pattern`` (with one integer group) in ``final``, sorted."""
    rx = re.compile(pattern)
    return sorted(int(m.group(1)) for m in (rx.fullmatch(n) for n in os.listdir(final)) if m)


def _parse_error(msg):
    raise ValueError(msg)


def load_pareto_set(save_dir):
    """The Pareto set a finished run left in ``save_dir``: ``(args, params, ob_mean, ob_var, stored)`` with the run's
    parsed ``args.txt``, the members' flat parameters [M][L] fp32 (``ParamLayout.flatten`` of every
    ``final/EP_policy_i.pt``), their observation statistics [M][O] fp64 (``ob_rms`` of ``EP_env_params_i.pkl``; mean 0
    and var 1 for a run without --ob-rms) and the stored objectives [M][K] of ``final/objs.txt``.  PGMError when a
    piece is missing, the counts differ, a state dict does not fit the layout, or the run is outside the tool's scope
    (host-stepped, plug-in, MO-Dummy and Deep Sea Treasure runs)."""
    from .run import get_parser
    what = f'load_pareto_set({save_dir!r})'
    args_path, final = os.path.join(save_dir, 'args.txt'), os.path.join(save_dir, 'final')
    if not os.path.isfile(args_path):
        raise PGMError(f'{what}: no args.txt (not the save dir of a finished run)')
    if not os.path.isdir(final):
        raise PGMError(f'{what}: no final/ directory (the run did not finish)')
    try:
        argv = ast.literal_eval(open(args_path).read())
        if not isinstance(argv, list) or not all(isinstance(a, str) for a in argv):
            raise ValueError('not a list of strings')
        ap = get_parser()
        ap.error = _parse_error  # (argparse would exit the process)
        args = ap.parse_args(argv)
    except (ValueError, SyntaxError) as e:
        raise PGMError(f'{what}: args.txt does not hold the argument list of pgmorl_amd.run: {e}') from e
    for flag, v in (('--host-env', args.host_env), ('--device-env', args.device_env),
                    ('--env-plugin', args.env_plugin)):
        if v:
            raise PGMError(f'{what}: the run used {flag}; {SCOPE}')
    sp = _synth_spec(args.env_name, what)
    O, A, K = sp['obs_dim'], sp['act_dim'], sp['obj_num']
    objs_path = os.path.join(final, 'objs.txt')
    if not os.path.isfile(objs_path):
        raise PGMError(f'{what}: no final/objs.txt')
    lines = [ln for ln in open(objs_path).read().splitlines() if ln.strip()]
    pts, pkls = _members(final, r'EP_policy_(\d+)\.pt'), _members(final, r'EP_env_params_(\d+)\.pkl')
    M = len(lines)
    if M == 0 or pts != list(range(M)) or pkls != list(range(M)):
        raise PGMError(f'{what}: final/ holds {len(pts)} EP_policy_i.pt, {len(pkls)} EP_env_params_i.pkl and {M} '
                       f'objs.txt lines; a Pareto set has the same number of each, numbered from 0')
    try:
        stored = np.array([[float(x) for x in ln.split(',')] for ln in lines], dtype=np.float64)
    except ValueError as e:
        raise PGMError(f'{what}: final/objs.txt: {e}') from e
    if stored.ndim != 2 or stored.shape[1] != K:
        raise PGMError(f'{what}: final/objs.txt has {stored.shape[-1]} objectives per line; {args.env_name} has {K}')
    layout = ParamLayout(O, A, K, layernorm=args.layernorm)
    params = np.empty((M, layout.total), dtype=np.float32)
    ob_mean, ob_var = np.zeros((M, O)), np.ones((M, O))
    for i in range(M):
        try:
            sd = torch.load(os.path.join(final, f'EP_policy_{i}.pt'), map_location='cpu', weights_only=True)
            params[i] = layout.flatten(sd)
        except (KeyError, ValueError, TypeError, pickle.UnpicklingError) as e:
            raise PGMError(f'{what}: EP_policy_{i}.pt does not fit the {"LayerNorm" if args.layernorm else "plain"} '
                           f'layout of {args.env_name}: {e}') from e
        if args.ob_rms:
            with open(os.path.join(final, f'EP_env_params_{i}.pkl'), 'rb') as fp:
                rms = (pickle.load(fp) or {}).get('ob_rms')
            mean, var = (np.asarray(getattr(rms, n, None), dtype=np.float64) for n in ('mean', 'var'))
            if mean.shape != (O,) or var.shape != (O,):
                raise PGMError(f'{what}: EP_env_params_{i}.pkl has no ob_rms of shape ({O},) (the run used --ob-rms)')
            ob_mean[i], ob_var[i] = mean, var
    return args, torch.from_numpy(params), torch.from_numpy(ob_mean), torch.from_numpy(ob_var), stored


def summarise(episodes, stored, eval_seed, noise_seed, stochastic):
    """The fields of summary.json from the per-episode sums [M][E][K] and the stored objectives [M][K]."""
    M, E, K = episodes.shape
    means = np.zeros((M, K))
    for e in range(E):  # in index order, as the device sums them
        means += episodes[:, e]
    means /= E
    std = episodes.std(axis=1)  # per policy and objective, over the episodes (population form: zero for E = 1)
    return {
        'M': int(M), 'E': int(E), 'K': int(K), 'eval_seed': int(eval_seed), 'stochastic': bool(stochastic),
        'noise_seed': int(noise_seed),
        'mean_std_per_objective': [float(x) for x in std.mean(axis=0)],
        'stored': {'hypervolume': float(compute_hypervolume(stored)), 'sparsity': float(compute_sparsity(stored))},
        'reevaluated': {'hypervolume': float(compute_hypervolume(means)), 'sparsity': float(compute_sparsity(means))},
        'non_dominated': len(get_ep_indices(means)),
    }


def get_parser():
    ap = argparse.ArgumentParser(prog='python -m pgmorl_amd.evaluate',
                                 description='Re-evaluate the Pareto set of a finished run on the device')
    ap.add_argument('save_dir', metavar='SAVE_DIR')
    ap.add_argument('--episodes', type=int, default=32, help='episodes per policy')
    ap.add_argument('--eval-seed', type=int, default=None,
                    help='episode e starts from the reset state of env seed S + e (default: the run\'s --seed)')
    ap.add_argument('--stochastic', action='store_true', default=False,
                    help='sample the actions (mean + exp(logstd) z) instead of taking the mean')
    ap.add_argument('--noise-seed', type=int, default=0, help='counter stream of the action noise (--stochastic)')
    ap.add_argument('--out', default=None, metavar='DIR', help='default: SAVE_DIR/eval')
    ap.add_argument('--device', default='cuda')
    ap.add_argument('--chunk', type=int, default=4096, help='policies per launch')
    return ap


def main(argv=None):
    a = get_parser().parse_args(sys.argv[1:] if argv is None else argv)
    # every refusal precedes the creation of --out
    if a.episodes < 1 or a.episodes > EVAL_EPISODES_MAX:
        raise PGMError(f'--episodes {a.episodes}: outside [1, {EVAL_EPISODES_MAX}]')
    if a.chunk < 1:
        raise PGMError(f'--chunk {a.chunk}: policies per launch must be at least 1')
    args, params, ob_mean, ob_var, stored = load_pareto_set(a.save_dir)
    eval_seed = args.seed if a.eval_seed is None else a.eval_seed
    episodes, objs = evaluate_policies(args.env_name, params, ob_mean, ob_var, a.episodes, eval_seed,
                                       stochastic=a.stochastic, noise_seed=a.noise_seed, gamma=args.gamma,
                                       raw=args.raw, use_ob_rms=args.ob_rms, layernorm=args.layernorm,
                                       device=a.device, chunk=a.chunk, return_objs=True)
    out = os.path.join(a.save_dir, 'eval') if a.out is None else a.out
    os.makedirs(out, exist_ok=True)
    fmt = '{:5f}' + (objs.shape[1] - 1) * ',{:5f}'
    with open(os.path.join(out, 'objs.txt'), 'w') as fp:
        for obj in objs:
            fp.write((fmt + '\n').format(*obj))
    np.save(os.path.join(out, 'episodes.npy'), episodes)
    summary = summarise(episodes, stored, eval_seed, a.noise_seed, a.stochastic)
    with open(os.path.join(out, 'summary.json'), 'w') as fp:
        json.dump(summary, fp, indent=1)
    print(f'{summary["M"]} policies x {summary["E"]} episodes -> {out}: hypervolume {summary["stored"]["hypervolume"]} '
          f'stored, {summary["reevaluated"]["hypervolume"]} re-evaluated; {summary["non_dominated"]} of '
          f'{summary["M"]} members non-dominated under the re-evaluated means')
    return summary


if __name__ == '__main__':
    main()
