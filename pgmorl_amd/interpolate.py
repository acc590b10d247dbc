"""A dense Pareto front from blended policies.

    python -m pgmorl_amd.interpolate SAVE_DIR [--points 15] [--neighbours 2] [--episodes 1] [--eval-seed S]
                                              [--out DIR] [--save-policies] [--device cuda] [--chunk C] [--simplex]

The final policies of a PG-MORL run fall into a few families in parameter space, and linear interpolation between
neighbouring members of a family yields further Pareto-optimal policies.  This module generates the in-between
policies of a finished run's ``final/`` set, measures all of them on the device and says which neighbour pairs are
connected by non-dominated policies, which families that gives and what the dense front is worth.

A candidate is ``(a, b, alpha)``: member indices and a weight in [0, 1].  Its parameters are

    theta[i] = float32((1 - alpha) * float64(params[a][i]) + alpha * float64(params[b][i]))

(two fp64 products and one fp64 sum, each rounded on its own, then one round to fp32) and its observation statistics
the same expression in fp64 without the last round: ``blend``.  ``pgm_eval_blend`` forms that blend in the kernel's
weight load, one wave per (candidate, episode), so no candidate is ever materialised; LayerNorm runs and MO-Humanoid
go through ``blend`` on bounded slices and ``evaluate.evaluate_policies``.

``neighbour_pairs`` / ``candidate_table`` build the table, ``evaluate_candidates`` measures it, ``analyse`` is the
host-side Pareto analysis and ``main`` the command: ``candidates.txt``, ``objs.txt``, ``episodes.npy`` [Q][E][K],
``segments.txt``, ``front.txt`` and ``summary.json`` in ``--out`` (default ``SAVE_DIR/continuous``); with
``--save-policies`` also ``args.txt`` and ``final/`` holding the dense front's policies, so that ``--out`` is itself
a save dir of ``pgmorl_amd.evaluate``.  SynthMO device envs only.

On a three-objective run the front is a surface, which pair blends only draw lines across.  ``--simplex`` adds the
candidates ``(a, b, c, wa, wb, wc)`` of every triangle of mutually neighbouring members (``neighbour_triangles``):

    theta[i] = float32((wa * float64(params[a][i]) + wb * float64(params[b][i])) + wc * float64(params[c][i]))

(three fp64 products and two fp64 sums, left to right, each rounded on its own; the statistics without the last
round): ``blend3``, formed in ``pgm_eval_blend3``'s weight load.  ``candidate_table3`` / ``evaluate_candidates3`` /
``analyse3`` are the simplex forms; the command then writes ``candidates.txt`` rows as ``a,b,c,wa,wb,wc``, adds
``triangles.txt`` (``a,b,c,filled``) and ``simplex`` / ``num_triangles`` / ``num_filled`` to ``summary.json``.
"""
import argparse
import ctypes as C
import json
import os
import pickle
import shutil
import sys

import numpy as np
import torch

from . import _host, envspec
from ._lib import (EVAL_EPISODES_MAX, Dims, EnvSpec, PGMError, check, lib, require_eval_blend,
                   require_eval_blend3)
from .evaluate import SPEC_KEYS, _ptr, _synth_spec, evaluate_policies, load_pareto_set
from .layout import ParamLayout
from .pareto import compute_hypervolume, compute_sparsity, get_ep_indices

POINTS_MAX = 1024
BLEND_WORK_MAX = 1 << 24  # (candidate, episode) waves of one pgm_eval_blend call
FALLBACK_CHUNK = 4096     # candidates materialised at a time where pgm_eval_blend has no kernel
SUM_TOL = 1e-9            # |wa + wb + wc - 1| of a simplex candidate


def wave_form(obs_dim, obj_num, layernorm=False):
    """True where pgm_eval_blend has a kernel: plain towers and the dims of the wave-per-episode evaluation (every
    SynthMO env but MO-Humanoid)."""
    return not layernorm and obs_dim <= 48 and obs_dim + obj_num + 1 <= 64 and obj_num <= 4


def make_table(rows):
    """``[(a, b, alpha), ...]`` -> the table ``(src int32 [Q][2], alpha fp64 [Q])``."""
    rows = list(rows)
    src = np.array([[r[0], r[1]] for r in rows], dtype=np.int32).reshape(len(rows), 2)
    return src, np.array([float(r[2]) for r in rows], dtype=np.float64)


def _check_table(table, M, what):
    try:
        src, alpha = table
    except (TypeError, ValueError):
        raise PGMError(f'{what}: table must be the pair (src int32 [Q][2], alpha fp64 [Q])') from None
    src, alpha = (t.numpy() if isinstance(t, torch.Tensor) else t for t in (src, alpha))
    if not isinstance(src, np.ndarray) or src.dtype != np.int32 or src.ndim != 2 or src.shape[1] != 2:
        raise PGMError(f'{what}: table src must be int32 [Q][2]; got {getattr(src, "dtype", type(src).__name__)} '
                       f'{getattr(src, "shape", "")}')
    if not isinstance(alpha, np.ndarray) or alpha.dtype != np.float64 or alpha.shape != (len(src),):
        raise PGMError(f'{what}: table alpha must be fp64 [{len(src)}]; got '
                       f'{getattr(alpha, "dtype", type(alpha).__name__)} {getattr(alpha, "shape", "")}')
    if len(src) < 1:
        raise PGMError(f'{what}: no candidates')
    bad = np.flatnonzero(((src < 0) | (src >= M)).any(axis=1))
    if len(bad):
        q = int(bad[0])
        raise PGMError(f'{what}: candidate {q} names members ({src[q, 0]}, {src[q, 1]}) outside [0, {M})')
    bad = np.flatnonzero(~((alpha >= 0.0) & (alpha <= 1.0)))  # (a NaN fails both comparisons)
    if len(bad):
        q = int(bad[0])
        raise PGMError(f'{what}: candidate {q} has alpha={float(alpha[q])!r} outside [0, 1]')
    return np.ascontiguousarray(src), np.ascontiguousarray(alpha)


def _mix(x, src, alpha):
    """(1 - alpha) * x[a] + alpha * x[b] in fp64, every operation rounded on its own (numpy never contracts)."""
    x = np.asarray(x)
    a, b = x[src[:, 0]].astype(np.float64), x[src[:, 1]].astype(np.float64)
    return (1 - alpha)[:, None] * a + alpha[:, None] * b


def blend(params, ob_mean, ob_var, table):
    """The candidates of ``table`` materialised: ``(params [Q][L] fp32, ob_mean [Q][O] fp64, ob_var [Q][O] fp64)`` from
    the members' ``params`` [M][L] fp32 and statistics [M][O] fp64 (either may be None, and stays None).  numpy arrays
    in, numpy arrays out; torch CPU tensors in, torch tensors out.  The definition every other path is tested against:
    ``((1 - alpha) * A.astype(f64) + alpha * B.astype(f64)).astype(f32)`` for the parameters, the same without the
    final round for the statistics, so alpha = 0 is member ``a`` and alpha = 1 member ``b``."""
    as_torch = isinstance(params, torch.Tensor)
    p = params.numpy() if as_torch else np.asarray(params)
    src, alpha = _check_table(table, len(p), 'blend')
    out = [_mix(p, src, alpha).astype(np.float32)]
    for s in (ob_mean, ob_var):
        out.append(None if s is None else _mix(s.numpy() if isinstance(s, torch.Tensor) else s, src, alpha))
    return tuple(None if o is None else torch.from_numpy(o) if as_torch else o for o in out)


def make_table3(rows):
    """``[(a, b, c, wa, wb, wc), ...]`` -> the simplex table ``(src int32 [Q][3], w fp64 [Q][3])``."""
    rows = list(rows)
    src = np.array([[r[0], r[1], r[2]] for r in rows], dtype=np.int32).reshape(len(rows), 3)
    return src, np.array([[float(r[3]), float(r[4]), float(r[5])] for r in rows], dtype=np.float64).reshape(len(rows), 3)


def _check_table3(table, M, what):
    try:
        src, w = table
    except (TypeError, ValueError):
        raise PGMError(f'{what}: table must be the pair (src int32 [Q][3], w fp64 [Q][3])') from None
    src, w = (t.numpy() if isinstance(t, torch.Tensor) else t for t in (src, w))
    if not isinstance(src, np.ndarray) or src.dtype != np.int32 or src.ndim != 2 or src.shape[1] != 3:
        raise PGMError(f'{what}: table src must be int32 [Q][3]; got {getattr(src, "dtype", type(src).__name__)} '
                       f'{getattr(src, "shape", "")}')
    if not isinstance(w, np.ndarray) or w.dtype != np.float64 or w.shape != (len(src), 3):
        raise PGMError(f'{what}: table w must be fp64 [{len(src)}][3]; got '
                       f'{getattr(w, "dtype", type(w).__name__)} {getattr(w, "shape", "")}')
    if len(src) < 1:
        raise PGMError(f'{what}: no candidates')
    bad = np.flatnonzero(((src < 0) | (src >= M)).any(axis=1))
    if len(bad):
        q = int(bad[0])
        raise PGMError(f'{what}: candidate {q} names members ({src[q, 0]}, {src[q, 1]}, {src[q, 2]}) outside [0, {M})')
    bad = np.flatnonzero(~((w >= 0.0) & (w <= 1.0)).all(axis=1))  # (a NaN fails both comparisons)
    if len(bad):
        q = int(bad[0])
        raise PGMError(f'{what}: candidate {q} has weights ({float(w[q, 0])!r}, {float(w[q, 1])!r}, '
                       f'{float(w[q, 2])!r}) outside [0, 1]')
    total = (w[:, 0] + w[:, 1]) + w[:, 2]
    bad = np.flatnonzero(~(np.abs(total - 1.0) <= SUM_TOL))
    if len(bad):
        q = int(bad[0])
        raise PGMError(f'{what}: candidate {q} has weights summing to {float(total[q])!r}, not to 1 within {SUM_TOL:g}')
    return np.ascontiguousarray(src), np.ascontiguousarray(w)


def _mix3(x, src, w):
    """(wa * x[a] + wb * x[b]) + wc * x[c] in fp64, left to right, every operation rounded on its own."""
    x = np.asarray(x)
    a, b, c = (x[src[:, i]].astype(np.float64) for i in range(3))
    return (w[:, 0, None] * a + w[:, 1, None] * b) + w[:, 2, None] * c


def blend3(params, ob_mean, ob_var, table3):
    """``blend`` for a simplex table: candidate ``(a, b, c, wa, wb, wc)`` has the parameters
    ``((wa * A.astype(f64) + wb * B.astype(f64)) + wc * C.astype(f64)).astype(f32)`` and the statistics of the same
    expression without the final round.  ``(i, i, i, 1, 0, 0)`` is member i, ``(a, b, b, 1 - alpha, alpha, 0)`` has the
    value of ``blend``'s ``(a, b, alpha)``, and swapping the first two (index, weight) slots changes no bit."""
    as_torch = isinstance(params, torch.Tensor)
    p = params.numpy() if as_torch else np.asarray(params)
    src, w = _check_table3(table3, len(p), 'blend3')
    out = [_mix3(p, src, w).astype(np.float32)]
    for s in (ob_mean, ob_var):
        out.append(None if s is None else _mix3(s.numpy() if isinstance(s, torch.Tensor) else s, src, w))
    return tuple(None if o is None else torch.from_numpy(o) if as_torch else o for o in out)


def neighbour_pairs(stored, neighbours=2):
    """The unordered pairs ``(lo, hi)`` of members that are among each other's nearest neighbours in objective space,
    sorted: every objective of ``stored`` [M][K] is scaled to [0, 1] by its min and max (a constant objective to 0),
    member i's other members are ranked by (squared Euclidean distance, index) and the first
    ``min(neighbours, M - 1)`` each give a pair."""
    stored = np.asarray(stored, dtype=np.float64)
    if stored.ndim != 2:
        raise PGMError(f'neighbour_pairs: stored objectives must be [M][K]; got {stored.shape}')
    if int(neighbours) < 1:
        raise PGMError(f'neighbour_pairs: neighbours={neighbours} must be at least 1')
    M = len(stored)
    lo, hi = stored.min(axis=0), stored.max(axis=0)
    span = np.where(hi > lo, hi - lo, 1.0)
    x = (stored - lo) / span
    pairs = set()
    for i in range(M):
        d2 = ((x - x[i]) ** 2).sum(axis=1)
        ranked = sorted((float(d2[j]), j) for j in range(M) if j != i)
        for _, j in ranked[:min(int(neighbours), M - 1)]:
            pairs.add((min(i, j), max(i, j)))
    return sorted(pairs)


def candidate_table(M, pairs, points):
    """The table of a front of M members: rows 0..M-1 the members themselves ``(i, i, 0.0)``, then for every pair in
    order its ``points`` interior candidates, alpha_j = j / (points + 1), j = 1..points.  Q = M + len(pairs) * points."""
    rows = [(i, i, 0.0) for i in range(M)]
    for a, b in pairs:
        rows += [(a, b, j / (points + 1)) for j in range(1, points + 1)]
    return make_table(rows)


def neighbour_triangles(stored, neighbours=2, pairs=None):
    """The sorted triples ``a < b < c`` of members whose three edges are all in ``neighbour_pairs(stored, neighbours)``:
    the 3-cliques of the neighbour graph (no triangulation: a triangle exists where three members are mutual
    neighbours, so ``neighbours=2`` leaves about a third of a surface's members outside every triangle and 4 nearly
    none).  ``pairs``: that list, where the caller has it already."""
    if pairs is None:
        pairs = neighbour_pairs(stored, neighbours)
    above = {}
    for a, b in pairs:
        above.setdefault(a, set()).add(b)
    return [(a, b, c) for a, b in pairs for c in sorted(above[a] & above.get(b, set()))]


def candidate_table3(M, pairs, triangles, points):
    """The simplex table of a front of M members: rows 0..M-1 the members ``(i, i, i, 1.0, 0.0, 0.0)``; then for every
    pair in order ``candidate_table``'s ``points`` candidates as ``(a, b, b, 1 - alpha_j, alpha_j, 0.0)``; then for
    every triangle in order its interior lattice points ``(a, b, c, i / n, j / n, k / n)``, n = points + 1,
    i, j, k >= 1, i + j + k = n, i ascending then j ascending.
    Q = M + len(pairs) * points + len(triangles) * points * (points - 1) / 2."""
    n = points + 1
    rows = [(i, i, i, 1.0, 0.0, 0.0) for i in range(M)]
    for a, b in pairs:
        rows += [(a, b, b, 1.0 - j / n, j / n, 0.0) for j in range(1, points + 1)]
    for a, b, c in triangles:
        rows += [(a, b, c, i / n, j / n, (n - i - j) / n) for i in range(1, n - 1) for j in range(1, n - i)]
    return make_table3(rows)


def evaluate_candidates(env_name, params, ob_mean, ob_var, table, episodes, eval_seed, gamma=0.995, raw=True,
                        use_ob_rms=True, layernorm=False, device='cuda', max_episode_steps=None, chunk=65536,
                        return_objs=False):
    """``episodes`` deterministic episodes of each candidate of ``table`` over the M members ``params`` [M][L] fp32,
    ``ob_mean`` / ``ob_var`` [M][O] fp64 -> the per-episode objective sums [Q][episodes][K], numpy fp64; with
    ``return_objs`` also the device's per-candidate means [Q][K].  Start states, ``gamma`` / ``raw`` / ``use_ob_rms``
    and ``max_episode_steps`` as in ``evaluate.evaluate_policies``.  The table is checked on the host before any
    upload.  The members are uploaded once and the table goes to ``pgm_eval_blend`` in slices of at most ``chunk``
    candidates, one launch each; LayerNorm towers and MO-Humanoid materialise slices with ``blend`` and go through
    ``evaluate_policies``, with the same result."""
    return _evaluate('evaluate_candidates', 2, env_name, params, ob_mean, ob_var, table, episodes, eval_seed, gamma, raw,
                     use_ob_rms, layernorm, device, max_episode_steps, chunk, return_objs)


def evaluate_candidates3(env_name, params, ob_mean, ob_var, table3, episodes, eval_seed, gamma=0.995, raw=True,
                         use_ob_rms=True, layernorm=False, device='cuda', max_episode_steps=None, chunk=65536,
                         return_objs=False):
    """``evaluate_candidates`` for a simplex table ``(src int32 [Q][3], w fp64 [Q][3])``: the same arguments, checks,
    slices and results, through ``pgm_eval_blend3``; LayerNorm towers and MO-Humanoid materialise slices with
    ``blend3``."""
    return _evaluate('evaluate_candidates3', 3, env_name, params, ob_mean, ob_var, table3, episodes, eval_seed, gamma,
                     raw, use_ob_rms, layernorm, device, max_episode_steps, chunk, return_objs)


def _evaluate(what, members, env_name, params, ob_mean, ob_var, table, episodes, eval_seed, gamma, raw, use_ob_rms,
              layernorm, device, max_episode_steps, chunk, return_objs):
    """evaluate_candidates (members = 2) and evaluate_candidates3 (members = 3): only the table's check, the
    materialising definition and the entry point differ."""
    if members == 2:
        check_table, blend_fn, require, entry = _check_table, blend, require_eval_blend, 'pgm_eval_blend'
    else:
        check_table, blend_fn, require, entry = _check_table3, blend3, require_eval_blend3, 'pgm_eval_blend3'
    sp = _synth_spec(env_name, what)
    O, A, K = sp['obs_dim'], sp['act_dim'], sp['obj_num']
    E, chunk = int(episodes), int(chunk)
    if not 1 <= E <= EVAL_EPISODES_MAX:
        raise PGMError(f'{what}: episodes={E} outside [1, {EVAL_EPISODES_MAX}]')
    if chunk < 1:
        raise PGMError(f'{what}: chunk={chunk} candidates per launch must be at least 1')
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
        raise PGMError(f'{what}: no members')
    stats = [None, None]
    if use_ob_rms:
        for i, (name, v) in enumerate((('ob_mean', ob_mean), ('ob_var', ob_var))):
            if v is None:
                raise PGMError(f'{what}: {name} is required with use_ob_rms')
            v = torch.as_tensor(v)
            if tuple(v.shape) != (M, O) or v.dtype != torch.float64:
                raise PGMError(f'{what}: {name} must be fp64 [{M}][{O}]; got {v.dtype} {tuple(v.shape)}')
            stats[i] = v
    src, wts = check_table(table, M, what)
    Q = len(src)
    out = np.empty((Q, E, K), dtype=np.float64)
    objs = np.empty((Q, K), dtype=np.float64)
    if not wave_form(O, K, layernorm):
        step = min(chunk, FALLBACK_CHUNK)
        for lo in range(0, Q, step):
            hi = min(Q, lo + step)
            prm, mean, var = blend_fn(params, stats[0], stats[1], (src[lo:hi], wts[lo:hi]))
            out[lo:hi], objs[lo:hi] = evaluate_policies(
                env_name, prm, mean, var, E, eval_seed, gamma=gamma, raw=raw, use_ob_rms=use_ob_rms,
                layernorm=layernorm, device=device, max_episode_steps=tmax, chunk=step, return_objs=True)
        return (out, objs) if return_objs else out
    require()
    dev = torch.device(device)
    f64 = dict(dtype=torch.float64, device=dev)
    spec_t = {k: torch.tensor(np.ascontiguousarray(sp[k]), **f64) for k in SPEC_KEYS}
    c_spec = EnvSpec(*(_ptr(spec_t[k]) for k in SPEC_KEYS), tmax, 0)
    starts = torch.tensor(envspec.reset_table(O, int(eval_seed), E), **f64)
    step = max(1, min(chunk, BLEND_WORK_MAX // E))
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        prm = params.to(dev).contiguous()  # the members: the only parameters that are uploaded
        mean, var = (None if s is None else s.to(dev).contiguous() for s in stats)
        for lo in range(0, Q, step):
            hi = min(Q, lo + step)
            src_d = torch.from_numpy(src[lo:hi]).to(dev)
            wts_d = torch.from_numpy(wts[lo:hi]).to(dev)
            ep_d = torch.empty(hi - lo, E, K, **f64)
            objs_d = torch.empty(hi - lo, K, **f64)
            d = Dims(hi - lo, 1, 0, O, A, K, 64, 0)
            check(getattr(lib(), entry)(C.byref(d), _ptr(prm), M, _ptr(mean), _ptr(var), _ptr(src_d), _ptr(wts_d),
                                        C.byref(c_spec), _ptr(starts), E, int(bool(use_ob_rms)), int(bool(raw)),
                                        float(gamma), _ptr(ep_d), _ptr(objs_d), stream), entry)
            out[lo:hi] = ep_d.cpu().numpy()
            objs[lo:hi] = objs_d.cpu().numpy()
    return (out, objs) if return_objs else out


def _dominated_by_any(x, members):
    """True if some row of ``members`` dominates x as pgmorl_amd.pareto defines it: >= in all, > in any objective."""
    return bool(((members >= x).all(axis=1) & (members > x).any(axis=1)).any())


def analyse(table, means, M, points):
    """The Pareto analysis of measured candidates, host only.  ``table`` as ``candidate_table`` lays it out (M member
    rows, then ``points`` rows per pair), ``means`` [Q][K].  Returns a dict:
    ``front`` the candidate indices of the dense front (``pareto.get_ep_indices`` over all Q rows); ``pairs`` [(a, b)];
    ``connected`` one bool per pair, True iff none of the pair's interior candidates is dominated by any member's
    re-measured mean; ``family`` the label of every member, the smallest member index of its connected component
    under the connected pairs; ``families`` the components in label order; and the counts, hypervolumes and sparsities
    of summary.json that need no stored objectives."""
    src, alpha = _check_table(table, M, 'analyse')
    means = np.asarray(means, dtype=np.float64)
    Q, points = len(src), int(points)
    if means.ndim != 2 or len(means) != Q:
        raise PGMError(f'analyse: means must be [{Q}][K]; got {means.shape}')
    if M < 1 or points < 1 or Q < M or (Q - M) % points:
        raise PGMError(f'analyse: {Q} candidates are not {M} members and {points} points per pair')
    if not (src[:M] == np.arange(M)[:, None]).all():
        raise PGMError('analyse: the first M rows of the table are not the members themselves')
    n_pairs = (Q - M) // points
    seg = _segments('analyse', src, means, M, points, n_pairs)
    front = [int(i) for i in get_ep_indices(means)]
    return _analysis(seg, means, M, points, front)


def _segments(what, src, means, M, points, n_pairs):
    """``(pairs, connected, family, families)`` from the member rows and the ``n_pairs * points`` pair rows after them
    (columns 0 and 1 of ``src`` name a pair row's members)."""
    pairs, connected = [], []
    parent = list(range(M))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for p in range(n_pairs):
        rows = range(M + p * points, M + (p + 1) * points)
        a, b = (int(v) for v in src[rows[0], :2])
        if not all(int(src[r, 0]) == a and int(src[r, 1]) == b for r in rows):
            raise PGMError(f'{what}: rows {rows[0]}..{rows[-1]} of the table are not one pair')
        ok = not any(_dominated_by_any(means[r], means[:M]) for r in rows)
        pairs.append((a, b))
        connected.append(ok)
        if ok:
            ra, rb = find(a), find(b)
            parent[max(ra, rb)] = min(ra, rb)  # the root of a component is its smallest member
    family = [find(i) for i in range(M)]
    families = [[i for i in range(M) if family[i] == f] for f in sorted(set(family))]
    return pairs, connected, family, families


def _hypervolume3(front):
    """``pareto.compute_hypervolume`` for the analysis of a simplex table: a three-objective front goes to the
    generation boundary's native incremental staircase (libpgm_host.so; the same rounded value), which a dense front
    of 10^5 points needs -- the slicing form in Python is quadratic in interpreted steps."""
    f = np.asarray(front, dtype=np.float64)
    return _host.hypervolume(f) if f.ndim == 2 and f.shape[1] == 3 and len(f) else compute_hypervolume(f)


def _analysis(seg, means, M, points, front, compute_hypervolume=compute_hypervolume):
    """analyse's dict from ``_segments``' result and the dense front's candidate indices."""
    pairs, connected, family, families = seg
    dense = means[front] if front else means[:0]
    return {
        'front': front, 'pairs': pairs, 'connected': connected, 'family': family, 'families': families,
        'M': int(M), 'Q': int(len(means)), 'points': points, 'num_pairs': len(pairs),
        'num_connected': int(sum(connected)),
        'num_families': len(families), 'family_sizes': [len(f) for f in families],
        'members': {'hypervolume': float(compute_hypervolume(means[:M])),
                    'sparsity': float(compute_sparsity(means[:M]))},
        'dense': {'hypervolume': float(compute_hypervolume(dense)), 'sparsity': float(compute_sparsity(dense))},
        'dense_front_size': len(front), 'dense_front_interpolants': int(sum(i >= M for i in front)),
    }


def analyse3(table3, means, M, points, n_pairs, n_triangles):
    """``analyse`` for a simplex table as ``candidate_table3`` lays it out (M member rows, ``points`` rows per pair,
    ``points * (points - 1) / 2`` rows per triangle), ``means`` [Q][K].  Everything ``analyse`` returns, the pair
    results from the member and pair rows exactly as there and the dense front over all Q rows, plus ``triangles``
    [(a, b, c)], ``filled`` one bool per triangle, True iff none of the triangle's interior candidates is dominated by
    any member's re-measured mean, and ``num_triangles`` / ``num_filled``."""
    src, _ = _check_table3(table3, M, 'analyse3')
    means = np.asarray(means, dtype=np.float64)
    Q, points, n_pairs, n_triangles = len(src), int(points), int(n_pairs), int(n_triangles)
    if means.ndim != 2 or len(means) != Q:
        raise PGMError(f'analyse3: means must be [{Q}][K]; got {means.shape}')
    per = points * (points - 1) // 2
    if (M < 1 or points < 1 or n_pairs < 0 or n_triangles < 0 or (n_triangles and points < 2) or
            Q != M + n_pairs * points + n_triangles * per):
        raise PGMError(f'analyse3: {Q} candidates are not {M} members, {n_pairs} pairs of {points} points and '
                       f'{n_triangles} triangles of {per} points')
    if not (src[:M] == np.arange(M)[:, None]).all():
        raise PGMError('analyse3: the first M rows of the table are not the members themselves')
    first = M + n_pairs * points
    if not (src[M:first, 1] == src[M:first, 2]).all():
        raise PGMError(f'analyse3: rows {M}..{first - 1} of the table are not pair rows (a, b, b)')
    seg = _segments('analyse3', src, means, M, points, n_pairs)
    triangles, filled = [], []
    for t in range(n_triangles):
        rows = range(first + t * per, first + (t + 1) * per)
        tri = tuple(int(v) for v in src[rows[0]])
        if not (src[rows.start:rows.stop] == src[rows[0]]).all():
            raise PGMError(f'analyse3: rows {rows.start}..{rows.stop - 1} of the table are not one triangle')
        triangles.append(tri)
        filled.append(not any(_dominated_by_any(means[r], means[:M]) for r in rows))
    an = _analysis(seg, means, M, points, [int(i) for i in get_ep_indices(means)], _hypervolume3)
    an.update({'triangles': triangles, 'filled': filled, 'num_triangles': n_triangles, 'num_filled': int(sum(filled))})
    return an


SUMMARY_FROM_ANALYSIS = ('M', 'Q', 'points', 'num_pairs', 'num_connected', 'num_families', 'family_sizes', 'members',
                         'dense', 'dense_front_size', 'dense_front_interpolants')


def summarise(an, stored, neighbours, E, eval_seed, run_seed, compute_hypervolume=compute_hypervolume):
    """The fields of summary.json from ``analyse``'s result and the stored objectives [M][K]."""
    s = {k: an[k] for k in SUMMARY_FROM_ANALYSIS}
    s.update({'neighbours': int(neighbours), 'E': int(E), 'eval_seed': int(eval_seed), 'run_seed': int(run_seed),
              'stored': {'hypervolume': float(compute_hypervolume(stored)),
                         'sparsity': float(compute_sparsity(stored))}})
    return s


def _fmt(K):
    return '{:5f}' + (K - 1) * ',{:5f}'


def write_policies(out, args_path, layout, table, params, ob_mean, ob_var, means, front, use_ob_rms):
    """``out/args.txt`` (a copy) and ``out/final/``: the dense front's policies, numbered from 0 in ``front`` order, as
    morl.write_final lays a Pareto set out (state dicts through ParamLayout.unflatten, the frozen normaliser as the
    ``ob_rms`` of EP_env_params_i.pkl)."""
    from .sample import RunningMeanStd
    final = os.path.join(out, 'final')
    os.makedirs(final, exist_ok=True)
    shutil.copyfile(args_path, os.path.join(out, 'args.txt'))
    src, wts = table
    blend_fn = blend3 if src.shape[1] == 3 else blend  # (a simplex table)
    O = ob_mean.shape[1]
    for lo in range(0, len(front), FALLBACK_CHUNK):  # materialised in bounded slices
        idx = np.asarray(front[lo:lo + FALLBACK_CHUNK], dtype=np.int64)
        prm, mean, var = blend_fn(np.asarray(params), np.asarray(ob_mean), np.asarray(ob_var), (src[idx], wts[idx]))
        for j in range(len(idx)):
            torch.save(layout.unflatten(prm[j]), os.path.join(final, f'EP_policy_{lo + j}.pt'))
            env_params = {}
            if use_ob_rms:
                rms = RunningMeanStd(shape=(O,))
                rms.mean, rms.var = mean[j].copy(), var[j].copy()
                env_params['ob_rms'] = rms
            with open(os.path.join(final, f'EP_env_params_{lo + j}.pkl'), 'wb') as fp:
                pickle.dump(env_params, fp)
    fmt = _fmt(means.shape[1])
    with open(os.path.join(final, 'objs.txt'), 'w') as fp:
        for i in front:
            fp.write((fmt + '\n').format(*means[i]))


def get_parser():
    ap = argparse.ArgumentParser(prog='python -m pgmorl_amd.interpolate',
                                 description='A dense Pareto front from policies blended between neighbouring members '
                                             'of a finished run\'s Pareto set')
    ap.add_argument('save_dir', metavar='SAVE_DIR')
    ap.add_argument('--points', type=int, default=15, help='interior candidates per neighbour pair')
    ap.add_argument('--neighbours', type=int, default=2, help='nearest members (in objective space) each member pairs with')
    ap.add_argument('--episodes', type=int, default=1, help='episodes per candidate')
    ap.add_argument('--eval-seed', type=int, default=None,
                    help='episode e starts from the reset state of env seed S + e (default: the run\'s --seed)')
    ap.add_argument('--out', default=None, metavar='DIR', help='default: SAVE_DIR/continuous')
    ap.add_argument('--save-policies', action='store_true', default=False,
                    help='also write args.txt and final/ with the dense front\'s policies')
    ap.add_argument('--device', default='cuda')
    ap.add_argument('--chunk', type=int, default=65536, help='candidates per launch')
    ap.add_argument('--simplex', action='store_true', default=False,
                    help='three-objective runs: also blend the triangles of mutually neighbouring members')
    return ap


def main(argv=None):
    a = get_parser().parse_args(sys.argv[1:] if argv is None else argv)
    # every refusal precedes the creation of --out
    if not 1 <= a.points <= POINTS_MAX:
        raise PGMError(f'--points {a.points}: outside [1, {POINTS_MAX}]')
    if a.neighbours < 1:
        raise PGMError(f'--neighbours {a.neighbours}: must be at least 1')
    if not 1 <= a.episodes <= EVAL_EPISODES_MAX:
        raise PGMError(f'--episodes {a.episodes}: outside [1, {EVAL_EPISODES_MAX}]')
    if a.chunk < 1:
        raise PGMError(f'--chunk {a.chunk}: candidates per launch must be at least 1')
    if a.simplex and a.points < 2:
        raise PGMError(f'--simplex with --points {a.points}: a triangle has interior lattice points from --points 2 on')
    args, params, ob_mean, ob_var, stored = load_pareto_set(a.save_dir)
    if a.simplex and args.obj_num != 3:
        raise PGMError(f'--simplex: the run has --obj-num {args.obj_num}; a two-objective front is a curve, which the '
                       f'neighbour pairs cover (three objectives only)')
    eval_seed = args.seed if a.eval_seed is None else a.eval_seed
    M = len(stored)
    pairs = neighbour_pairs(stored, a.neighbours)
    how = dict(gamma=args.gamma, raw=args.raw, use_ob_rms=args.ob_rms, layernorm=args.layernorm, device=a.device,
               chunk=a.chunk, return_objs=True)
    if a.simplex:
        triangles = neighbour_triangles(stored, a.neighbours, pairs)
        table = candidate_table3(M, pairs, triangles, a.points)
        episodes, means = evaluate_candidates3(args.env_name, params, ob_mean, ob_var, table, a.episodes, eval_seed,
                                               **how)
        an = analyse3(table, means, M, a.points, len(pairs), len(triangles))
    else:
        table = candidate_table(M, pairs, a.points)
        episodes, means = evaluate_candidates(args.env_name, params, ob_mean, ob_var, table, a.episodes, eval_seed,
                                              **how)
        an = analyse(table, means, M, a.points)
    summary = summarise(an, stored, a.neighbours, a.episodes, eval_seed, args.seed,
                        _hypervolume3 if a.simplex else compute_hypervolume)
    if a.simplex:
        summary.update({'simplex': True, 'num_triangles': an['num_triangles'], 'num_filled': an['num_filled']})
    out = os.path.join(a.save_dir, 'continuous') if a.out is None else a.out
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'candidates.txt'), 'w') as fp:
        if a.simplex:
            for (ia, ib, ic), (wa, wb, wc) in zip(*table):
                fp.write(f'{ia},{ib},{ic},{float(wa)!r},{float(wb)!r},{float(wc)!r}\n')
        else:
            for (ia, ib), al in zip(*table):
                fp.write(f'{ia},{ib},{float(al)!r}\n')
    fmt = _fmt(means.shape[1])
    with open(os.path.join(out, 'objs.txt'), 'w') as fp:
        for obj in means:
            fp.write((fmt + '\n').format(*obj))
    np.save(os.path.join(out, 'episodes.npy'), episodes)
    with open(os.path.join(out, 'segments.txt'), 'w') as fp:
        for (ia, ib), ok in zip(an['pairs'], an['connected']):
            fp.write(f'{ia},{ib},{int(ok)},{an["family"][ia]}\n')
    if a.simplex:
        with open(os.path.join(out, 'triangles.txt'), 'w') as fp:
            for (ia, ib, ic), ok in zip(an['triangles'], an['filled']):
                fp.write(f'{ia},{ib},{ic},{int(ok)}\n')
    with open(os.path.join(out, 'front.txt'), 'w') as fp:
        for i in an['front']:
            fp.write(f'{i}\n')
    with open(os.path.join(out, 'summary.json'), 'w') as fp:
        json.dump(summary, fp, indent=1)
    if a.save_policies:
        sp = _synth_spec(args.env_name, 'interpolate')
        layout = ParamLayout(sp['obs_dim'], sp['act_dim'], sp['obj_num'], layernorm=args.layernorm)
        write_policies(out, os.path.join(a.save_dir, 'args.txt'), layout, table, params, ob_mean, ob_var, means,
                       an['front'], args.ob_rms)
    simplex = f', {an["num_filled"]} of {an["num_triangles"]} triangles filled' if a.simplex else ''
    print(f'{M} members, {summary["num_pairs"]} pairs x {a.points} points x {a.episodes} episodes -> {out}: '
          f'{summary["num_connected"]} connected pairs, {summary["num_families"]} families{simplex}; hypervolume '
          f'{summary["stored"]["hypervolume"]} stored, {summary["members"]["hypervolume"]} re-measured, '
          f'{summary["dense"]["hypervolume"]} dense ({summary["dense_front_size"]} points, '
          f'{summary["dense_front_interpolants"]} of them interpolants)')
    return summary


if __name__ == '__main__':
    main()
