"""Mixed-row inputs for the per-task PPO settings (pgm_ppo_update_tasks), decided from the oracle alone.

A mixed case has P = 4 tasks; task p takes row 'acdf'[p] of branch_inputs.ROWS (a: defaults; c: max_grad_norm 10, the
side of clip_grad_norm_'s clamp with coefficient exactly 1; d: clip_param 0.1 and value_loss_coef 1.0; f: entropy_coef
0.01), so the four tasks of one launch differ in every field of pgm_task_hparams.  Task p's storage is task p of
branch_inputs.build_inputs(..., seed, hparams(row_p)): at one seed the draws are the same for every row, so the policies
and the permutations are common and only the offsets placed relative to the row's clip_param differ.

The seed of a case is the first one from branch_inputs.BASE_SEED at which every task, under its own row, meets
branch_inputs.conditions and same_decisions (SEEDS; found by scan_seed on the CPU).  swap_factors shows that the cases
discriminate: task p's oracle under another task's row leaves the parameter band 2e-6 + 1e-5 |ref| by a large factor.
"""
import functools
import math

import numpy as np
import torch

from . import branch_inputs as bi

ROWS = 'acdf'
P = len(ROWS)
# name -> (env, T, N, E, M, layernorm)
CASES = {'hopper': ('MO-Hopper-v2', 64, 4, 2, 2, False),
         'hopper_ln': ('MO-Hopper-v2', 64, 4, 2, 2, True),
         'walker': ('MO-Walker2d-v2', 64, 4, 1, 2, False),
         'humanoid': ('MO-Humanoid-v2', 32, 8, 1, 2, False)}
# the first seed from BASE_SEED at which all four tasks meet the conditions under their own rows (scan_seed).
# hopper_ln: seed 11 misses the max-tie margin on task 3, step 2 (8.07e-5 < 1e-4); smallest margin at 12: 1.04e-4.
SEEDS = {'hopper': 11, 'hopper_ln': 12, 'walker': 11, 'humanoid': 11}
SWAP_CHECKED = ('hopper', 'hopper_ln', 'humanoid')
# two-task halves (rows a, d and c, f) for a forced placement that does not take P = 4: none needed one on a 256-CU
# device, the builder takes any row string


def hp_of(p, rows=ROWS):
    return bi.hparams(rows[p])


def shape_of(name, rows=ROWS):
    env, T, N, E, M, _ = CASES[name]
    return (env, len(rows), T, N, E, M)


def build(name, seed, rows=ROWS):
    """(args of row a, spec, pols, data, perms): data[field][p] is task p of build_inputs under row rows[p]."""
    env, T, N, E, M, ln = CASES[name]
    n = len(rows)
    per_row = {r: bi.build_inputs(env, n, T, N, E, M, seed, bi.hparams(r), ln) for r in set(rows)}
    args, spec, pols, _, perms = per_row[rows[0]]
    for r, other in per_row.items():  # the draws do not depend on the row: policies and permutations are common
        assert all(torch.equal(a, b) for a, b in zip(perms, other[4]))
        for pa, pb in zip(pols, other[2]):
            assert all(torch.equal(x, y) for x, y in zip(pa.state_dict().values(), pb.state_dict().values()))
    fields = []
    for f in range(6):
        parts = [per_row[rows[p]][3][f][p] for p in range(n)]
        fields.append(np.stack(parts) if isinstance(parts[0], np.ndarray) else torch.stack(parts))
    return args, spec, pols, tuple(fields), perms


def evaluate(name, seed, rows=ROWS):
    """One candidate seed, from the oracle alone -> (inputs, per-task fp64 results, violations, worst)."""
    inputs = build(name, seed, rows)
    _, _, pols, data, perms = inputs
    shape = shape_of(name, rows)
    results, bad, worst = [], [], {}
    for p in range(len(rows)):
        hp = hp_of(p, rows)
        r64 = bi.run_oracle(pols[p], hp, data, p, perms, shape)
        r32 = bi.run_oracle(pols[p], hp, data, p, perms, shape, dtype=torch.float32)
        b, w = bi.conditions(r64[3], hp)
        bad += [f'task {p}: {x}' for x in b] + [f'task {p}: {x}' for x in bi.same_decisions(r64[3], r32[3], hp)]
        for k, x in w.items():
            worst[k] = min(worst.get(k, math.inf), x)
        results.append(r64)
    return inputs, results, bad, worst


def scan_seed(name, rows=ROWS, tries=40):
    for seed in range(bi.BASE_SEED, bi.BASE_SEED + tries):
        _, _, bad, worst = evaluate(name, seed, rows)
        if not bad:
            return seed, worst
    raise AssertionError(f'no seed in {tries} tries for {name}: last {bad[:3]}')


@functools.lru_cache(maxsize=None)
def mixed_case(name):
    """The case at its recorded seed: inputs and the fp64 oracle's result per task, computed once and shared (callers
    must not modify it).  Asserts the conditions before anything is returned."""
    inputs, results, bad, worst = evaluate(name, SEEDS[name])
    assert not bad, f'{name} seed {SEEDS[name]}: the oracle does not meet the input conditions: {bad}'
    return inputs, results, worst


def swap_factors(name):
    """{(p, q)}: how far, in units of the band 2e-6 + 1e-5 |ref|, the parameters of task p's oracle under task q's row
    end from those under its own row (the largest element), for every ordered pair p != q."""
    (_, _, pols, data, perms), results, _ = mixed_case(name)
    shape = shape_of(name)
    out = {}
    for p in range(P):
        ref = bi.flat_state(results[p][0], results[p][1])[0]
        for q in range(P):
            if q == p:
                continue
            pol, agent, _, _ = bi.run_oracle(pols[p], hp_of(q), data, p, perms, shape)
            got = bi.flat_state(pol, agent)[0]
            out[(p, q)] = float((np.abs(got - ref) / (2e-6 + 1e-5 * np.abs(ref))).max())
    return out
