"""LayerNorm towers (--layernorm), host side: the 17-tensor parameter layout of ABI 5, the state-dict and Adam
mappings over it, the reference's RNG draws at initialisation and the command line.  No kernel is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ppo as oppo
from oracle.policy import make_policy
from pgmorl_amd import _lib
from pgmorl_amd.layout import STATE_KEYS, STATE_KEYS_LN, ParamLayout
from pgmorl_amd.policy import new_policy
from pgmorl_amd.run import get_parser, main, merge_argv

from .helpers import perturb, small_args

LN_DIMS = [(17, 6, 2), (11, 3, 2), (11, 3, 3), (27, 8, 2), (8, 2, 2)]
H = 64


def _sizes_ln(O, A, K):
    tower = [O * H, H, H, H * H, H, H]
    return tower + tower + [H * K, K, H * A, A, A]


@pytest.mark.parametrize('O,A,K', LN_DIMS)
def test_param_layout_ln(O, A, K):
    offs = (C.c_int32 * 17)()
    tot = C.c_int32()
    assert _lib.lib().pgm_param_layout_ln(O, A, K, H, offs, C.byref(tot)) == _lib.PGM_OK
    offs, sizes = list(offs), _sizes_ln(O, A, K)
    assert len(_lib.PARAM_TENSORS_LN) == 17 and offs[0] == 0
    for i in range(17):
        assert offs[i] % 4 == 0, (i, offs[i])  # 16-byte aligned
        end = offs[i] + sizes[i]
        nxt = offs[i + 1] if i + 1 < 17 else tot.value
        assert end <= nxt, f'tensor {i} overlaps the next one'  # in order, non-overlapping
        assert nxt - end < (4 if i + 1 < 17 else 64 + 4)  # no slack beyond the alignment padding
    assert tot.value % 64 == 0
    d, total = _lib.param_layout_ln(O, A, K)
    assert list(d) == _lib.PARAM_TENSORS_LN and list(d.values()) == offs and total == tot.value
    # the plain layout is what it was: 13 offsets, each tensor packed behind the previous one
    p13 = (C.c_int32 * 13)()
    t13 = C.c_int32()
    assert _lib.lib().pgm_param_layout(O, A, K, H, p13, C.byref(t13)) == _lib.PGM_OK
    tw = [O * H, H, H * H, H]
    want, p = [], 0
    for n in tw + tw + [H * K, K, H * A, A, A]:
        want.append(p)
        p = -(-(p + n) // 4) * 4
    assert list(p13) == want and t13.value == -(-p // 64) * 64


def test_param_layout_ln_rejects_bad_arguments():
    tot = C.c_int32()
    assert _lib.lib().pgm_param_layout_ln(17, 6, 2, H, None, C.byref(tot)) == _lib.PGM_E_INVALID_ARG
    assert _lib.lib().pgm_param_layout_ln(0, 6, 2, H, (C.c_int32 * 17)(), C.byref(tot)) == _lib.PGM_E_INVALID_ARG


def _ln_policy(O, A, K, seed):
    torch.manual_seed(seed)
    pol = make_policy(O, A, K, layernorm=True)
    return perturb(pol, 0.05, torch.Generator().manual_seed(seed + 1))


@pytest.mark.parametrize('O,A,K', LN_DIMS)
def test_state_dict_roundtrip_ln(O, A, K):
    pol = _ln_policy(O, A, K, 3)
    sd = pol.state_dict()
    assert [k for k, _, _ in STATE_KEYS_LN] == list(sd.keys()) and len(sd) == 17
    assert [k for k, _, _ in STATE_KEYS_LN] == [n for n, _ in pol.named_parameters()]
    lay = ParamLayout(O, A, K, layernorm=True)
    assert lay.total % 64 == 0
    flat = lay.flatten(sd, dtype=np.float64)
    back = lay.unflatten(flat)
    assert list(back) == list(sd)
    for k in sd:
        assert torch.equal(back[k], sd[k]), k
    # weights are stored transposed, gamma / beta as they are
    w = sd['base.critic.3.weight']
    assert flat[lay.offsets['critic_w2'] + 2 * H + 5] == float(w[5, 2])
    assert flat[lay.offsets['actor_g2'] + 7] == float(sd['base.actor.4.weight'][7])
    assert flat[lay.offsets['critic_be1'] + 9] == float(sd['base.critic.1.bias'][9])
    n_params = sum(v.numel() for v in sd.values())
    assert n_params == 2 * (O * H + 2 * H + H * H + 2 * H) + H * K + K + H * A + A + A
    # unflatten_batch rows equal unflatten (numpy and torch inputs)
    pol2 = _ln_policy(O, A, K, 4)
    flats = np.stack([flat, lay.flatten(pol2.state_dict(), dtype=np.float64)])
    for blocks in (lay.unflatten_batch(flats), lay.unflatten_batch(torch.from_numpy(flats))):
        assert len(blocks) == 17
        for i in range(2):
            one = lay.unflatten(flats[i])
            for blk, (key, _, _) in zip(blocks, STATE_KEYS_LN):
                assert np.array_equal(blk[i], one[key].numpy()), key
    # the plain layout refuses a LayerNorm state dict instead of dropping tensors
    with pytest.raises(KeyError):
        ParamLayout(O, A, K).flatten(sd)


def test_plain_layout_is_unchanged():
    lay = ParamLayout(17, 6, 2)
    assert lay.layernorm is False and lay.keys is STATE_KEYS and len(lay.offsets) == 13
    torch.manual_seed(3)
    sd = make_policy(17, 6, 2).state_dict()
    back = lay.unflatten(lay.flatten(sd, dtype=np.float64))
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)


def test_adam_mapping_ln():
    """One oracle PPO minibatch step on a LayerNorm policy: torch keeps 17 Adam states, and the flat images carry
    every one of them there and back."""
    O, A, K, B = 11, 3, 2, 24
    pol = _ln_policy(O, A, K, 5)
    args = small_args('MO-Hopper-v2', layernorm=True)
    agent = oppo.PPO(pol, args.clip_param, 1, 1, args.value_loss_coef, args.entropy_coef, lr=3e-4, eps=1e-5,
                     max_grad_norm=args.max_grad_norm)
    g = torch.Generator().manual_seed(6)
    ro = oppo.RolloutStorage(B, 1, O, A, K)
    ro.obs.copy_(torch.randn(ro.obs.shape, generator=g, dtype=torch.float64))
    with torch.no_grad():
        v, a, lp = pol.act(ro.obs[:B, 0], noise=torch.randn(B, A, generator=g, dtype=torch.float64))
    ro.actions.copy_(a.reshape(B, 1, A))
    ro.action_log_probs.copy_((lp + 0.05 * torch.randn(lp.shape, generator=g, dtype=torch.float64)).reshape(B, 1, 1))
    ro.value_preds[:B].copy_(v.reshape(B, 1, K))
    ro.returns.copy_(ro.value_preds + 0.5 * torch.randn(ro.returns.shape, generator=g, dtype=torch.float64))
    adv = torch.randn(B, 1, generator=g, dtype=torch.float64)
    for mbt in ro.minibatches(adv, 1, torch.randperm(B, generator=g)):
        agent.minibatch_step(*mbt)
    st = agent.optimizer.state_dict()['state']
    assert len(st) == 17
    lay = ParamLayout(O, A, K, layernorm=True)
    m, v, step = lay.adam_from_optimizer_state(st)
    assert step == 1 and m.shape == (lay.total,)
    back = lay.adam_to_optimizer_state(m.astype(np.float64), v.astype(np.float64), step)
    assert sorted(back) == list(range(17))
    for i in range(17):
        for k in ('exp_avg', 'exp_avg_sq'):
            ref = st[i][k].double()
            assert back[i][k].shape == ref.shape
            assert torch.equal(back[i][k], ref.float().double()), (i, k)  # the device image is fp32
        assert float(back[i]['step']) == 1.0
    # the LayerNorm gradients are really there
    for i in (1, 2, 4, 5, 7, 8, 10, 11):
        assert float(st[i]['exp_avg'].abs().max()) > 0
    assert lay.adam_to_optimizer_state(m, v, 0) == {}
    m0, v0, s0 = lay.adam_from_optimizer_state({})
    assert s0 == 0 and not m0.any() and not v0.any()


@pytest.mark.parametrize('seed,dims', [(0, [(17, 6, 2)] * 3), (7, [(11, 3, 3), (11, 3, 3)]),
                                       (123, [(27, 8, 2), (8, 2, 2), (11, 3, 2), (17, 6, 2)])])
@pytest.mark.parametrize('layernorm', [True, False])
def test_new_policy_draws_the_oracle_rng(seed, dims, layernorm):
    """A sequence of P warm-up policies under one seed: the same torch RNG draws as the oracle's constructor
    (Linear(bias=False) draws only its weight, LayerNorm nothing, the discarded 1-output head is still drawn)."""
    torch.manual_seed(seed)
    ours = [new_policy(O, A, K, layernorm=layernorm).state_dict() for O, A, K in dims]
    torch.manual_seed(seed)
    ref = [make_policy(O, A, K, layernorm=layernorm).state_dict() for O, A, K in dims]
    for a, b in zip(ours, ref):
        assert list(a) == list(b)
        for k in b:
            assert a[k].dtype == torch.float64 and torch.equal(a[k], b[k]), k
    if layernorm:
        assert torch.equal(ours[0]['base.actor.1.weight'], torch.ones(H, dtype=torch.float64))
        assert not ours[0]['base.critic.4.bias'].any()


def test_dims_carry_ln_and_unsupported_dims_are_refused():
    """pgm_dims.LN: appended, default 0; LN = 1 with Humanoid's dims is PGM_E_UNSUPPORTED (decided before any device
    work), LN outside {0, 1} invalid."""
    assert [n for n, _ in _lib.Dims._fields_] == ['P', 'N', 'T', 'O', 'A', 'K', 'H', 'LN']
    assert _lib.Dims(2, 4, 8, 17, 6, 2, 64).LN == 0 and _lib.PGM_ABI_VERSION == 5
    L = _lib.lib()
    hp = _lib.PPOHParams(0.2, 0.5, 0.0, 0.5, 1e-5, 0.9, 0.999, 0.0, 1, 2, 1, 0)
    buf = C.create_string_buffer(128)
    one = C.c_void_p(1)
    d = _lib.Dims(2, 4, 64, 376, 17, 2, 64, 1)
    assert L.pgm_ppo_update_variant(C.byref(d), C.byref(hp), None, buf, 128) == _lib.PGM_E_UNSUPPORTED
    assert b'LayerNorm' in L.pgm_last_error() and b'obs_dim' in L.pgm_last_error()
    assert L.pgm_act_forward(C.byref(d), one, one, one, 0, one, one, one, None) == _lib.PGM_E_UNSUPPORTED
    assert L.pgm_ppo_update_reset(C.byref(d), one, None) == _lib.PGM_E_UNSUPPORTED
    assert L.pgm_ppo_update_workspace_bytes(C.byref(d)) == 0
    d = _lib.Dims(2, 4, 64, 17, 6, 2, 64, 1)
    assert L.pgm_ppo_update_variant(C.byref(d), C.byref(hp), None, buf, 128) == _lib.PGM_OK
    assert buf.value.startswith(b'ppo_update_ln_kernel')
    assert L.pgm_ppo_update_workspace_bytes(C.byref(d)) > 0
    d = _lib.Dims(2, 4, 64, 17, 6, 2, 64, 2)
    assert L.pgm_ppo_update_variant(C.byref(d), C.byref(hp), None, buf, 128) == _lib.PGM_E_INVALID_ARG


def test_cli_layernorm_flag():
    assert get_parser().parse_args(merge_argv(['--layernorm'])).layernorm is True
    assert get_parser().parse_args(merge_argv([])).layernorm is False


def test_cli_refuses_layernorm_humanoid_before_the_device(tmp_path, monkeypatch):
    """--layernorm with MO-Humanoid-v2 stops at the start with the limit spelled out: no save dir, no run."""
    import pgmorl_amd.morl as morl
    monkeypatch.setattr(morl, 'run', lambda *a, **k: pytest.fail('run() was reached'))
    prev = torch.get_default_dtype()
    save = tmp_path / 'out'
    try:
        with pytest.raises(_lib.PGMError) as ei:
            main(['--layernorm', '--env-name', 'MO-Humanoid-v2', '--save-dir', str(save)])
    finally:
        torch.set_default_dtype(prev)
    msg = str(ei.value)
    assert 'MO-Humanoid-v2' in msg and 'obs_dim <= 32' in msg and '376' in msg
    assert not save.exists()
