"""CPU-side checks of the Pareto-set re-evaluation: pgm_eval_episodes' argument refusals (before any device work, in
the order include/pgm_abi.h documents), the unchanged version pair and feature values, load_pareto_set on a final/
tree written by morl.write_final, the refusals of ``python -m pgmorl_amd.evaluate`` and the noise index map.  No kernel
is launched here."""
import argparse
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

from oracle import streams
from pgmorl_amd import _lib, evaluate
from pgmorl_amd._lib import PGM_E_INVALID_ARG, PGM_E_SHAPE, PGM_E_UNSUPPORTED, PGMError
from pgmorl_amd.layout import ParamLayout
from pgmorl_amd.run import merge_argv

ONE = C.c_void_p(1)  # a non-NULL pointer nothing dereferences: every refusal below precedes device work
NAME = 'pgm_eval_episodes'


def _err():
    return _lib.lib().pgm_last_error().decode()


def test_symbol_is_present_and_the_abi_values_are_unchanged():
    L = _lib.lib()
    assert _lib.has_eval_episodes() and all(hasattr(L, s) for s in _lib.EVAL_EPISODES_SYMBOLS)
    _lib.require_eval_episodes()
    assert (L.pgm_abi_version(), L.pgm_abi_minor()) == (5, 1)
    assert L.pgm_abi_features() == 7 and L.pgm_abi_feature_mask() == 15


def _call(dims=None, params=ONE, spec_null=False, E=9, use_ob=1, ob_mean=ONE, ob_var=ONE, starts=ONE, out=ONE,
          objs=ONE, spec_steps=20, spec_ptr=True):
    d = dict(P=3, N=4, T=64, O=17, A=6, K=2, H=64, LN=0)
    d.update(dims or {})
    spec = _lib.EnvSpec(*([None if spec_null else ONE] * 8), spec_steps, 0)
    return _lib.lib().pgm_eval_episodes(C.byref(_lib.Dims(*(d[k] for k in ('P', 'N', 'T', 'O', 'A', 'K', 'H', 'LN')))),
                                        params, C.byref(spec) if spec_ptr else None, ob_mean, ob_var, starts, E, use_ob,
                                        1, 0.995, 0, 0, out, objs, None)


# the documented order: (what is wrong, status, a piece of the message); every entry is tried with every later entry
# wrong as well (where two entries change the same field, the later entry's other variants are tried instead)
ORDER = [
    ('null', [dict(params=None), dict(starts=None), dict(out=None), dict(ob_mean=None), dict(ob_var=None),
              dict(spec_ptr=False)], PGM_E_INVALID_ARG, 'null pointer'),
    ('dims', [dict(dims=dict(P=0)), dict(dims=dict(K=0))], PGM_E_SHAPE, 'non-positive dims'),
    ('dims H', [dict(dims=dict(H=32))], PGM_E_UNSUPPORTED, 'hidden size'),
    ('LN', [dict(dims=dict(LN=2))], PGM_E_INVALID_ARG, 'pgm_dims.LN'),
    ('LN Humanoid', [dict(dims=dict(O=376, A=17, LN=1))], PGM_E_UNSUPPORTED, 'LayerNorm towers'),
    ('spec', [dict(spec_null=True), dict(spec_steps=0)], PGM_E_INVALID_ARG, 'env spec'),
    ('E', [dict(E=0), dict(E=65537), dict(E=-3)], PGM_E_SHAPE, 'episodes per policy outside [1, 65536]'),
    ('dim set', [dict(dims=dict(O=19))], PGM_E_UNSUPPORTED, 'unsupported dims O=19 A=6 K=2'),
]


def _merge(a, b):
    out = dict(a)
    for k, v in b.items():
        out[k] = dict(v, **out[k]) if k == 'dims' and k in out else out.get(k, v)  # the earlier entry's fields win
    return out


def test_refusals_in_the_documented_order():
    for i, (what, variants, rc, text) in enumerate(ORDER):
        for kw in variants:
            assert _call(**kw) == rc and text in _err() and _err().startswith(NAME + ':'), (what, kw, _err())
            later = dict(kw)
            for _, later_variants, _, _ in ORDER[i + 1:]:
                later = _merge(later, later_variants[0])
            got = _call(**later)
            assert got == rc and text in _err() and _err().startswith(NAME + ':'), (what, later, got, _err())


def test_optional_pointers_and_ignored_dims():
    # ob_mean / ob_var are read with use_ob_rms only and objs_out may be NULL: the call gets as far as the E check
    assert _call(use_ob=0, ob_mean=None, ob_var=None, objs=None, E=0) == PGM_E_SHAPE and 'E=0' in _err()
    assert _call(use_ob=1, ob_mean=None, E=0) == PGM_E_INVALID_ARG
    # d->N and d->T are not this call's: N = 9 (refused by every training entry point) and T = -1 pass the dims check
    assert _call(dims=dict(N=9, T=-1), E=0) == PGM_E_SHAPE and 'E=0' in _err()
    # the LayerNorm dim sets stop at obs_dim 32; Humanoid plain is a compiled dim set (E is what is refused)
    assert _call(dims=dict(O=376, A=17), E=65537) == PGM_E_SHAPE and 'E=65537' in _err()
    assert _call(dims=dict(O=19, LN=1)) == PGM_E_UNSUPPORTED and 'unsupported dims' in _err()


def test_noise_index_map():
    """Episode e, step t, action dim j of a stochastic re-evaluation draws element (e T + t) A + j of the stream."""
    E, T, A, seed = 3, 20, 6, 11
    full = streams.normal(seed, E * T * A).reshape(E, T, A)
    for e, t, j in ((0, 0, 0), (1, 7, 4), (E - 1, T - 1, A - 1)):
        i = evaluate.noise_index(e, t, j, T, A)
        assert i == (e * T + t) * A + j
        assert streams.normal(seed, 1, start=i)[0] == full[e, t, j]
    assert evaluate.noise_index(E - 1, T - 1, A - 1, T, A) == E * T * A - 1


# ------------------------------------------------------------------------------------------------ save dirs
def _write_run(save_dir, env='MO-Hopper-v2', O=11, A=3, K=2, layernorm=False, M=4, extra=(), seed=5):
    """args.txt as pgmorl_amd.run writes it and a final/ tree from morl.write_final; returns the archive."""
    from pgmorl_amd.morl import write_final
    from pgmorl_amd.pareto import EP
    from pgmorl_amd.sample import DeviceSnapshot, RunningMeanStd, Sample
    lay = ParamLayout(O, A, K, layernorm=layernorm)
    rng = np.random.RandomState(7)
    samples = []
    for k in range(M):
        z = torch.zeros(lay.total)
        snap = DeviceSnapshot(lay, torch.from_numpy(rng.randn(lay.total).astype(np.float32)), z, z, 10 * k)
        ob = RunningMeanStd(shape=(O,))
        ob.mean, ob.var = rng.randn(O), rng.rand(O) + 0.5
        obj = RunningMeanStd(shape=())
        obj.mean, obj.var = rng.randn(K), rng.rand(K) + 0.5
        objs = np.array([k + 1.25, M - k + 0.5] + [1.0] * (K - 2))  # a strict front: every sample stays a member
        samples.append(Sample.from_snapshot(snap, {'ob_rms': ob, 'ret_rms': RunningMeanStd(shape=()), 'obj_rms': obj},
                                            objs=objs))
    ep = EP()
    ep.update(samples)
    assert len(ep.sample_batch) == M
    os.makedirs(save_dir, exist_ok=True)
    argv = ['--env-name', env, '--obj-num', str(K), '--seed', str(seed), '--save-dir', str(save_dir),
            *(['--layernorm'] if layernorm else []), *extra]
    with open(os.path.join(save_dir, 'args.txt'), 'w') as fp:
        fp.write(str(merge_argv(argv)))
    write_final(argparse.Namespace(obj_num=K, obj_rms=True, save_dir=str(save_dir)), ep)
    return ep


@pytest.mark.parametrize('layernorm', [False, True])
def test_load_pareto_set_round_trips_write_final(tmp_path, layernorm):
    ep = _write_run(tmp_path / 'run', layernorm=layernorm)
    args, params, ob_mean, ob_var, stored = evaluate.load_pareto_set(str(tmp_path / 'run'))
    assert (args.env_name, args.seed, args.layernorm, args.ob_rms, args.raw) == ('MO-Hopper-v2', 5, layernorm, True, True)
    assert args.gamma == 0.995 and args.eval_num == 1
    M, lay = len(ep.sample_batch), ParamLayout(11, 3, 2, layernorm=layernorm)
    assert params.dtype == torch.float32 and tuple(params.shape) == (M, lay.total)
    assert ob_mean.dtype == ob_var.dtype == torch.float64 and tuple(ob_mean.shape) == tuple(ob_var.shape) == (M, 11)
    for i, smp in enumerate(ep.sample_batch):
        flat = smp.snapshot.params.cpu()
        sd = lay.unflatten(flat)  # (the random flat vector also filled the layout's padding, which no tensor owns)
        assert torch.equal(params[i], torch.from_numpy(lay.flatten(sd))), i
        used = np.zeros(lay.total, dtype=bool)
        for key, name, _ in lay.keys:
            used[lay.offsets[name]:lay.offsets[name] + sd[key].numel()] = True
        assert torch.equal(params[i][torch.from_numpy(used)], flat[torch.from_numpy(used)]), i
        np.testing.assert_array_equal(ob_mean[i].numpy(), smp.env_params['ob_rms'].mean)
        np.testing.assert_array_equal(ob_var[i].numpy(), smp.env_params['ob_rms'].var)
    np.testing.assert_array_equal(stored, np.array([[float('{:5f}'.format(x)) for x in o] for o in ep.obj_batch]))


def _refused(argv, text, *dirs):
    with pytest.raises(PGMError, match=text):
        evaluate.main([str(a) for a in argv])
    for d in dirs:
        assert not os.path.exists(d), f'{d} was created by a refused call'


def test_cli_refusals_leave_no_out_dir(tmp_path):
    out = tmp_path / 'elsewhere'

    def both(run, text):
        _refused([run], text, run / 'eval')
        _refused([run, '--out', out], text, out, run / 'eval')

    both(tmp_path / 'nothing', 'no args.txt')
    run = tmp_path / 'a'
    _write_run(run)
    for bad in ('0', '-4', '65537'):
        _refused([run, '--episodes', bad], '--episodes', run / 'eval')
    _refused([run, '--episodes', '0', '--out', out], '--episodes', out, run / 'eval')
    _refused([run, '--chunk', '0'], '--chunk', run / 'eval')
    # a state dict that does not fit the layout the run's args name
    r = tmp_path / 'shape0'  # Hopper-shaped (11/3/2) dicts under args that name Walker2d
    _write_run(r, env='MO-Walker2d-v2')
    both(r, 'does not fit the plain layout of MO-Walker2d-v2')
    for i, (ln_dicts, text) in enumerate([(True, 'does not fit the plain layout'),
                                          (False, 'does not fit the LayerNorm layout')], 1):
        r = tmp_path / f'shape{i}'  # LayerNorm dicts under args without --layernorm, and the reverse
        _write_run(r, layernorm=ln_dicts)
        argv = ['--env-name', 'MO-Hopper-v2', '--save-dir', str(r)] + ([] if ln_dicts else ['--layernorm'])
        (r / 'args.txt').write_text(str(merge_argv(argv)))
        both(r, text)
    # the counts of .pt, .pkl and objs.txt lines
    for i, breakit in enumerate([lambda f: os.remove(f / 'EP_policy_3.pt'), lambda f: os.remove(f / 'EP_env_params_0.pkl'),
                                 lambda f: (f / 'objs.txt').write_text(''.join((f / 'objs.txt').read_text()
                                                                                 .splitlines(True)[:-1])),
                                 lambda f: os.rename(f / 'EP_policy_3.pt', f / 'EP_policy_7.pt')]):
        r = tmp_path / f'count{i}'
        _write_run(r)
        breakit(r / 'final')
        both(r, 'the same number of each')
    r = tmp_path / 'nofinal'
    _write_run(r)
    os.rename(r / 'final', r / 'final_moved')
    both(r, 'no final/')
    r = tmp_path / 'noargs'
    _write_run(r)
    os.remove(r / 'args.txt')
    both(r, 'no args.txt')
    # runs outside the tool's scope: the message says what it covers
    scope = 'covers the SynthMO device envs'
    for i, (kw, flag) in enumerate([(dict(extra=['--host-env', 'synth']), '--host-env'),
                                    (dict(extra=['--device-env']), '--device-env'),
                                    (dict(extra=['--env-plugin', 'some/env.hpp']), '--env-plugin'),
                                    (dict(env='MO-Dummy-v0'), 'MO-Dummy-v0'), (dict(env='MO-Dummy3-v0'), 'MO-Dummy3-v0'),
                                    (dict(env='MO-DeepSeaTreasure-v0'), 'MO-DeepSeaTreasure-v0'),
                                    (dict(env='Tiny-v0'), 'Tiny-v0')]):
        r = tmp_path / f'scope{i}'
        _write_run(r, **kw)
        with pytest.raises(PGMError, match=scope) as ei:
            evaluate.main([str(r)])
        assert flag in str(ei.value)
        both(r, scope)


def test_evaluate_policies_refuses_bad_arguments_before_the_device():
    lay = ParamLayout(11, 3, 2)
    prm, st = torch.zeros(2, lay.total), torch.zeros(2, 11, dtype=torch.float64)
    ok = dict(episodes=4, eval_seed=0, device='cpu')
    for kw, text in [(dict(ok, episodes=0), 'episodes=0'), (dict(ok, episodes=65537), 'episodes=65537'),
                     (dict(ok, chunk=0), 'chunk=0'), (dict(ok, max_episode_steps=0), 'max_episode_steps=0')]:
        with pytest.raises(PGMError, match=text):
            evaluate.evaluate_policies('MO-Hopper-v2', prm, st, st, **kw)
    with pytest.raises(PGMError, match='params must be fp32'):
        evaluate.evaluate_policies('MO-Hopper-v2', prm[:, :-1], st, st, **ok)
    with pytest.raises(PGMError, match='params must be fp32'):
        evaluate.evaluate_policies('MO-Hopper-v2', prm, st, st, layernorm=True, **ok)
    with pytest.raises(PGMError, match='ob_var must be fp64'):
        evaluate.evaluate_policies('MO-Hopper-v2', prm, st, st.float(), **ok)
    with pytest.raises(PGMError, match='ob_mean is required'):
        evaluate.evaluate_policies('MO-Hopper-v2', prm, None, st, **ok)
    with pytest.raises(PGMError, match='covers the SynthMO device envs'):
        evaluate.evaluate_policies('MO-Dummy-v0', prm, st, st, **ok)


def test_summary_fields():
    rng = np.random.RandomState(3)
    ep = np.abs(rng.randn(5, 7, 2)) + 1.0
    stored = np.abs(rng.randn(5, 2)) + 1.0
    s = evaluate.summarise(ep, stored, eval_seed=9, noise_seed=4, stochastic=True)
    from pgmorl_amd.pareto import compute_hypervolume, compute_sparsity, get_ep_indices
    means = ep.mean(axis=1)
    assert (s['M'], s['E'], s['K'], s['eval_seed'], s['noise_seed'], s['stochastic']) == (5, 7, 2, 9, 4, True)
    np.testing.assert_allclose(s['mean_std_per_objective'], ep.std(axis=1).mean(axis=0), rtol=1e-12)
    assert s['stored'] == {'hypervolume': compute_hypervolume(stored), 'sparsity': compute_sparsity(stored)}
    assert s['reevaluated']['hypervolume'] == pytest.approx(compute_hypervolume(means), abs=1e-3)
    assert s['reevaluated']['sparsity'] == pytest.approx(compute_sparsity(means), rel=1e-9)
    assert s['non_dominated'] == len(get_ep_indices(means)) and 1 <= s['non_dominated'] <= 5
