"""The wide PPO update (pgm_ppo_wide.hip, obs_dim > 32) at every placement and minibatch edge, against the fp64 oracle.

The launcher compiles the kernel as NS = 4 (with its ONE instance at 512-row minibatches), NS = 2 and NS = 1 workgroups
per tower.  Every case here names the placement it ran (the exact TaskBatch.update_variant string), compares every task
of the launch with oracle.ppo.PPO in fp64 on test_ppo_update's bands, and calls check_update:

  a. the rows of a part (r0 = hs mb / NS, mbs = (hs + 1) mb / NS - r0, passes of 128 rows) where they degenerate: parts
     of 0 and 1 rows, one ragged tile, a last pass of one wave or of one row, several full passes, epoch boundaries;
  b. the block -> (task, tower, part) map beyond the first tasks of the first group of four;
  c. the launcher's automatic choice at the task counts where it switches, from the device's CU count, and its refusal;
  d. a second launch on the same batch (step0 != 0, moments read back from HBM, the workspace reused);
  e. two launches from identical state, bit for bit (the parts' images are summed in part order).

Inputs are test_gpu_kernels._update_setup's.  Before any device result is read, each case runs the oracle's fp32 arm (the
same update with the policy cast to float32) and asserts that it ends within FP32_ARM of every band of the fp64 arm: a
band that fp32 arithmetic in another summation order cannot hold would make the comparison a test of luck.  A case whose
inputs miss that takes another seed (SEEDS), never another band.
"""
import copy

import numpy as np
import pytest
import torch

from oracle import ppo as oppo
from pgmorl_amd._lib import PGMError
from pgmorl_amd.runtime import TaskBatch

from .test_gpu_kernels import _close, _load_update_data, _update_data, _update_setup

pytestmark = pytest.mark.gpu

ENV, LR, SEED = 'MO-Humanoid-v2', 3e-4, 11
# test_ppo_update's bands: array -> (atol, rtol)
BANDS = {'params': (2e-6, 1e-5), 'exp_avg': (1e-7, 1e-3), 'exp_avg_sq': (1e-10, 1e-3), 'loss stats': (1e-5, 1e-4)}
FP32_ARM = 0.5
SPLIT = {1: '1', 2: '2', 4: None}  # PGM_UPDATE_SPLIT that forces NS at the small P of these cases
# (P, T, N, E, M, rounds) -> the seed of a case whose inputs at SEED miss the fp32-arm condition (none does)
SEEDS = {}


def _variant(ns):
    return f'ppo_update_wide_kernel (NS={ns})'


def _force(monkeypatch, ns):
    monkeypatch.delenv('PGM_UPDATE_KERNEL', raising=False)
    if SPLIT[ns] is None:
        monkeypatch.delenv('PGM_UPDATE_SPLIT', raising=False)
    else:
        monkeypatch.setenv('PGM_UPDATE_SPLIT', SPLIT[ns])


def _expected_ns(P, cus, cap=4):
    """The launcher's rule: NS = 4 while the 32-block groups of 4 tasks fit the CUs, else 2 while the 16-block groups
    do, else 1 (which it launches only while 2P <= CUs)."""
    groups = -(-P // 4)
    return 4 if cap >= 4 and 32 * groups <= cus else 2 if cap >= 2 and 16 * groups <= cus else 1


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _fractions(got, ref):
    """{array: worst |got - ref| / (atol + rtol |ref|)} of one task."""
    out = {}
    for (name, (atol, rtol)), g, r in zip(BANDS.items(), got, ref):
        g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
        out[name] = float((np.abs(g - r) / (atol + rtol * np.abs(r))).max())
    return out


def _worst(fracs):
    return {name: max(f[name] for f in fracs) for name in BANDS}


def _oracle_arm(pol, args, spec, layout, p, rounds, T, N, E, M, dtype):
    """One optimizer carried through every round's update of task p, as test_ppo_update drives it ->
    (params, exp_avg, exp_avg_sq, the last round's loss stats), the Adam step count, the updated policy."""
    pol = copy.deepcopy(pol).to(dtype)
    agent = oppo.PPO(pol, args.clip_param, E, M, args.value_loss_coef, args.entropy_coef, lr=LR, eps=1e-5,
                     max_grad_norm=args.max_grad_norm)
    for (obs, actions, logp, values, returns, adv), perms in rounds:
        ro = oppo.RolloutStorage(T, N, spec['obs_dim'], spec['act_dim'], spec['obj_num'])
        ro.obs.copy_(torch.from_numpy(obs[p]).double())
        ro.actions.copy_(actions[p].double())
        ro.action_log_probs.copy_(logp[p].double().unsqueeze(-1))
        ro.value_preds.copy_(values[p].double())
        ro.returns.copy_(returns[p].double())
        stats = np.zeros(3)
        for e in range(E):
            for mbt in ro.minibatches(adv[p].double(), M, perms[e]):
                stats += agent.minibatch_step(*mbt)
        stats /= E * M
    m, v, step = layout.adam_from_optimizer_state(agent.optimizer.state_dict()['state'])
    return (layout.flatten(pol.state_dict(), dtype=np.float64), m, v, stats), step, pol.double()


def _reference(args, spec, layout, pols, rounds, T, N, E, M, what):
    """Both arms for every task; asserts the input condition from the oracle alone -> [(fp64 arrays, step)]."""
    refs, arm = [], []
    for p, pol in enumerate(pols):
        r64, step, _ = _oracle_arm(pol, args, spec, layout, p, rounds, T, N, E, M, torch.float64)
        r32, step32, _ = _oracle_arm(pol, args, spec, layout, p, rounds, T, N, E, M, torch.float32)
        assert step == step32 == len(rounds) * E * M
        arm.append(_fractions(r32, r64))
        refs.append((r64, step))
    arm = _worst(arm)
    assert max(arm.values()) <= FP32_ARM, \
        f'{what}: the oracle\'s fp32 arm ends at {arm} of the bands (> {FP32_ARM}): take another seed'
    return refs, arm


# (P, T, N, E, M, seed) -> (refs, arm) of a one-round case: _update_setup's inputs depend on nothing else, so the cases
# of one shape (NS = 1 / 2 / 4, the reproducibility runs) share one reference; never modified
_REF_CACHE = {}


def _seed(P, T, N, E, M, rounds=1):
    return SEEDS.get((P, T, N, E, M, rounds), SEED)


def _compare(tb, refs, arm, what):
    P = len(refs)
    assert int(tb.update_ws[2 * P]) == 0, 'workspace word 2P: an exchange timed out'
    tb.check_update()
    params, am, av = tb.params.cpu().numpy(), tb.adam_m.cpu().numpy(), tb.adam_v.cpu().numpy()
    steps, stats = tb.adam_step.cpu(), tb.stats.cpu().numpy()
    dev = _worst([_fractions((params[p], am[p], av[p], stats[p]), refs[p][0]) for p in range(P)])
    print(f'{what}: of the band, device / fp32 arm: ' +
          ', '.join(f'{name} {dev[name]:.3f} / {arm[name]:.3f}' for name in BANDS))
    for p, (ref, step) in enumerate(refs):
        assert int(steps[p]) == step, f'{what} task {p}: adam_step {int(steps[p])} != {step}'
        for (name, (atol, rtol)), g, r in zip(BANDS.items(), (params[p], am[p], av[p], stats[p]), ref):
            _close(g, r, atol, rtol, f'{what} task {p}: {name}')


def _one_launch(monkeypatch, ns, P, T, N, E, M, what, forced=True):
    """_update_setup's batch, the reference (and its input condition), then one launch at the asserted placement."""
    if forced:
        _force(monkeypatch, ns)
    seed = _seed(P, T, N, E, M)
    args, spec, tb, pols, data, perms = _update_setup(ENV, P, T, N, E, M, seed=seed)
    assert T * N // M * M == T * N and spec['obs_dim'] > 32
    key = (P, T, N, E, M, seed)
    if key not in _REF_CACHE:
        _REF_CACHE[key] = _reference(args, spec, tb.layout, pols, [(data, perms)], T, N, E, M, what)
    refs, arm = _REF_CACHE[key]
    assert tb.update_variant() == _variant(ns), tb.update_variant()
    tb.lr.fill_(LR)
    tb.ppo_update(torch.stack(perms).numpy())
    return tb, refs, arm


# ---------------------------------------------------------------------------------------------------- a. shape matrix
# (NS, (T, N, E, M)): mb = T N / M rows per minibatch, part hs of NS takes rows [hs mb / NS, (hs + 1) mb / NS)
SHAPES = [
    (1, (2, 2, 1, 2)),     # mb 2: one tile of two rows
    (1, (50, 3, 1, 3)),    # mb 50: one ragged pass, two waves
    (1, (64, 8, 2, 4)),    # mb 128: one full pass, 8 steps over an epoch boundary
    (1, (40, 8, 1, 2)),    # mb 160: the second pass holds one wave
    (1, (128, 8, 2, 2)),   # mb 512: four full passes, E = 2
    (2, (2, 2, 1, 2)),     # mb 2: parts of 1 and 1 row
    (2, (3, 1, 2, 1)),     # mb 3: parts of 1 and 2 rows, E = 2
    (2, (129, 4, 1, 2)),   # mb 258: parts of 129 rows, the last pass holds one row
    (4, (2, 2, 1, 2)),     # mb 2: parts of 0 / 1 / 0 / 1 rows
    (4, (3, 1, 2, 1)),     # mb 3: parts of 0 / 1 / 1 / 1 rows, E = 2
    (4, (129, 8, 1, 2)),   # mb 516: parts of 129 rows
    (4, (128, 8, 2, 2)),   # mb 512: the ONE instance over an epoch boundary, 4 steps
    (4, (64, 8, 2, 4)),    # mb 128: not ONE, E = 2, 8 steps
]


@pytest.mark.parametrize('ns,shape', SHAPES, ids=[f'NS{ns}-T{s[0]}N{s[1]}E{s[2]}M{s[3]}' for ns, s in SHAPES])
def test_rows_of_a_part(gpu, monkeypatch, ns, shape):
    what = f'wide NS={ns} P=2 (T, N, E, M)={shape} mb {shape[0] * shape[1] // shape[3]}'
    tb, refs, arm = _one_launch(monkeypatch, ns, 2, *shape, what)
    _compare(tb, refs, arm, what)


# ---------------------------------------------------------------------------------------------------- b. task map
@pytest.mark.parametrize('ns,P', [(2, 5), (4, 5), (1, 9)])
def test_task_map(gpu, monkeypatch, ns, P):
    """A whole group of four tasks plus one of the next (NS > 1: blocks of 8 NS per group); NS = 1: blocks 2p + m."""
    what = f'wide NS={ns} P={P} (T, N, E, M)=(4, 8, 2, 1)'
    tb, refs, arm = _one_launch(monkeypatch, ns, P, 4, 8, 2, 1, what)
    _compare(tb, refs, arm, what)


# ---------------------------------------------------------------------------------------------------- c. automatic choice
def _smallest_p(cus, want):
    return next(P for P in range(1, cus + 2) if _expected_ns(P, cus) == want)


def test_automatic_choice_at_the_switch_points(gpu, monkeypatch):
    _force(monkeypatch, 4)  # no knob
    cus = _cus()
    tb = TaskBatch(ENV, 128, num_processes=8, num_steps=4, ppo_epoch=2, num_mini_batch=1)
    seen = []
    for P in (32, 33, 64, 65, 128):
        tb.set_active(P)
        ns = _expected_ns(P, cus)
        assert tb.update_variant() == _variant(ns), (P, cus, tb.update_variant())
        seen.append(ns)
    if cus == 256:
        assert seen == [4, 2, 2, 1, 1]
    # the caps: TASK (0) and TOWER (1) are one workgroup per tower, HALVES (2) two
    tb.set_active(2)
    for split, ns in (('0', 1), ('1', 1), ('2', 2), ('4', 4)):
        monkeypatch.setenv('PGM_UPDATE_SPLIT', split)
        assert tb.update_variant() == _variant(ns), (split, tb.update_variant())


@pytest.mark.parametrize('ns', [2, 1])
def test_automatic_choice_launch(gpu, monkeypatch, ns):
    """The smallest task count at which the launcher leaves NS = 4 (NS = 2) on its own: 33 (65) on 256 CUs."""
    _force(monkeypatch, 4)  # no knob
    P = _smallest_p(_cus(), ns)
    what = f'wide automatic NS={ns} P={P} (T, N, E, M)=(4, 8, 2, 1)'
    tb, refs, arm = _one_launch(monkeypatch, ns, P, 4, 8, 2, 1, what, forced=False)
    _compare(tb, refs, arm, what)


def test_refusal_leaves_the_state_alone(gpu, monkeypatch):
    _force(monkeypatch, 4)  # no knob
    cus = _cus()
    P = cus // 2 + 1
    assert _expected_ns(P, cus) == 1  # (any device of >= 16 CUs: 16 ceil(P / 4) > 2P > CUs)
    args, spec, tb, pols, data, perms = _update_setup(ENV, P, 4, 8, 2, 1, seed=SEED)
    g = torch.Generator().manual_seed(SEED)
    for dst in (tb.adam_m, tb.adam_v):  # moments a launch would not leave as they are
        dst.copy_(torch.randn(dst.shape, generator=g).abs() * 1e-3)
    tb.adam_step.fill_(7)
    tb.lr.fill_(LR)
    before = [x.cpu().clone() for x in (tb.params, tb.adam_m, tb.adam_v, tb.adam_step)]
    assert tb.update_variant() == _variant(1)
    with pytest.raises(PGMError, match='2P <= CUs'):
        tb.ppo_update(torch.stack(perms).numpy())
    torch.cuda.synchronize()
    for name, b, x in zip(('params', 'exp_avg', 'exp_avg_sq', 'adam_step'), before,
                          (tb.params, tb.adam_m, tb.adam_v, tb.adam_step)):
        assert torch.equal(b, x.cpu()), f'{name} changed under a refused launch'


# ---------------------------------------------------------------------------------------------------- d. second launch
@pytest.mark.parametrize('ns', [1, 2, 4])
def test_second_launch(gpu, monkeypatch, ns):
    """Two ppo_update calls on one batch against one oracle optimizer carried through both.  The second round's storage
    and permutations are drawn like _update_setup's, from the fp64 oracle's policies after the first round (so from the
    CPU alone); the three placements share the rounds and the reference."""
    P, T, N, E, M = 2, 64, 8, 2, 4
    what = f'wide NS={ns} second launch P={P} (T, N, E, M)={(T, N, E, M)}'
    _force(monkeypatch, ns)
    seed = _seed(P, T, N, E, M, rounds=2)
    args, spec, tb, pols, data, perms = _update_setup(ENV, P, T, N, E, M, seed=seed)
    key = (P, T, N, E, M, seed, 2)
    if key not in _REF_CACHE:
        after = [_oracle_arm(pol, args, spec, tb.layout, p, [(data, perms)], T, N, E, M, torch.float64)[2]
                 for p, pol in enumerate(pols)]
        data2, perms2 = _update_data(spec, after, T, N, E, seed + 1000)
        rounds = [(data, perms), (data2, perms2)]
        _REF_CACHE[key] = (rounds,) + _reference(args, spec, tb.layout, pols, rounds, T, N, E, M, what)
    rounds, refs, arm = _REF_CACHE[key]
    assert tb.update_variant() == _variant(ns), tb.update_variant()
    tb.lr.fill_(LR)
    tb.ppo_update(torch.stack(perms).numpy())
    assert int(tb.adam_step[0]) == E * M
    _load_update_data(tb, rounds[1][0])
    tb.ppo_update(torch.stack(rounds[1][1]).numpy())
    _compare(tb, refs, arm, what)


# ---------------------------------------------------------------------------------------------------- e. reproducibility
@pytest.mark.parametrize('ns', [1, 2, 4])
def test_two_launches_from_identical_state_are_bitwise_equal(gpu, monkeypatch, ns):
    P, shape = 2, (64, 8, 2, 4)
    what = f'wide NS={ns} repeat P={P} (T, N, E, M)={shape}'
    runs = []
    for _ in range(2):
        tb, refs, arm = _one_launch(monkeypatch, ns, P, *shape, what)
        _compare(tb, refs, arm, what)
        runs.append([x.cpu().clone() for x in (tb.params, tb.adam_m, tb.adam_v, tb.stats, tb.adam_step)])
    for name, x, y in zip(('params', 'exp_avg', 'exp_avg_sq', 'loss stats', 'adam_step'), *runs):
        assert torch.equal(x, y), f'{what}: {name} differs between two launches from identical state'
