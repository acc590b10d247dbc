"""Every PPO update kernel on every loss branch and hyper-parameter, against the fp64 oracle.

Eight kernels -- the feature-split kernel (pgm_ppo_fs.hip), the four row-split placements (pgm_ppo_mfma.hip: 16-row
tiles on four workgroups per tower, MODE 2 / 1 / 0), the VALU kernel (pgm_ppo_update.hip), the wide Humanoid kernel
(pgm_ppo_wide.hip, at each of its placements: 4, 2 and 1 workgroups per tower) and the LayerNorm kernel
(pgm_ppo_ln.hip) -- each read pgm_ppo_hparams on their own and each wire
the clipped surrogate, the clipped value loss, clip_grad_norm_ and Adam (a2c_ppo_acktr/algo/ppo.py:76-103) into their
own tiles.  The arithmetic is shared where that left the register-critical kernels' code unchanged
(pgm_ppo_terms.hpp, tested on the CPU by tests/test_ppo_terms.py) and restated at the sites DESIGN.md 19 lists, so
every kernel still runs every row.  The
inputs are tests/branch_inputs.py's: at every Adam step at least 20 % of the rows are clamped to zero gradient (each
sign case at least 6 %), at least 20 % are outside the clip range but pass, the value clip is active in at least 43 %
of the elements and each arm of the max wins in at least 8 %; six hyper-parameter rows move every field the kernels read off its default, row c to the side of
clip_grad_norm_'s clamp (coefficient exactly 1) that no other test reaches.  tests/test_update_branches.py shows on the
CPU that each plausible defect leaves these bands by >= 10x on its row.

The conditions on the inputs (shares, margins >= 1e-4 from every discontinuity, fp32-arm agreement) are asserted from
the oracle alone before the device is looked at; the seeds were chosen the same way.  The bands are those of
test_ppo_update / test_ppo_update_ln.  Every case asserts the kernel that runs (TaskBatch.update_variant).
"""
import numpy as np
import pytest
import torch

from pgmorl_amd.runtime import TaskBatch

from . import branch_inputs as bi
from .test_gpu_kernels import _close

pytestmark = pytest.mark.gpu

# kernel -> (PGM_UPDATE_KERNEL, PGM_UPDATE_SPLIT, the launcher's description, its shapes; rows b-f at the first)
KERNELS = {
    # (the feature-split kernel takes minibatches of whole 16-row tiles only: K = 3 at 64 rows instead of 50)
    'fs': ('fs', None, 'ppo_update_fs_kernel (', ('hopper2', 'hopper3x64', 'walker')),
    'mfma4': ('mfma', '4', 'ppo_update_t16_kernel (NS=4, W=4)', ('hopper2', 'hopper3', 'walker')),
    'mfma2': ('mfma', '2', 'ppo_update_mfma_kernel (MODE 2)', ('hopper2', 'hopper3', 'walker')),
    'mfma1': ('mfma', '1', 'ppo_update_mfma_kernel (MODE 1)', ('hopper2', 'hopper3', 'walker')),
    'mfma0': ('mfma', '0', 'ppo_update_mfma_kernel (MODE 0)', ('hopper2', 'hopper3', 'walker')),
    'valu': ('valu', None, 'ppo_update_kernel (VALU, A/B)', ('hopper2', 'hopper3')),
    # the wide kernel's three placements: NS = 4 workgroups per tower (the launcher's own choice at these P), 2 and 1
    'wide': (None, None, 'ppo_update_wide_kernel (NS=4)', ('humanoid32', 'humanoid50')),
    'wide2': (None, '2', 'ppo_update_wide_kernel (NS=2)', ('humanoid32', 'humanoid50')),
    'wide1': (None, '1', 'ppo_update_wide_kernel (NS=1)', ('humanoid32', 'humanoid50')),
    'ln': (None, None, 'ppo_update_ln_kernel (', ('hopper2', 'hopper3')),
}
MATRIX = [(k, s, 'a') for k, v in KERNELS.items() for s in v[3]] + \
         [(k, v[3][0], r) for k, v in KERNELS.items() for r in 'bcdef']


@pytest.mark.parametrize('kernel,shape,row', MATRIX)
def test_update_branches(gpu, monkeypatch, kernel, shape, row):
    knob, split, variant, _ = KERNELS[kernel]
    ln = kernel == 'ln'
    # the inputs and the reference, from the oracle alone: oracle_case asserts the shares, margins and fp32-arm
    # agreement of this case before any device result exists
    (args, spec, pols, data, perms), results, _ = bi.oracle_case(shape, ln, row)
    hp = bi.hparams(row)
    env, P, T, N, E, M = bi.SHAPES[shape]
    for name, val in (('PGM_UPDATE_KERNEL', knob), ('PGM_UPDATE_SPLIT', split)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    tb = TaskBatch(env, P, num_processes=N, num_steps=T, ppo_epoch=E, num_mini_batch=M, layernorm=ln,
                   clip_param=hp['clip_param'], value_loss_coef=hp['value_loss_coef'],
                   entropy_coef=hp['entropy_coef'], max_grad_norm=hp['max_grad_norm'],
                   use_clipped_value_loss=hp['use_clipped_value_loss'])
    tb.hp.adam_eps, tb.hp.beta1, tb.hp.beta2 = hp['adam_eps'], hp['beta1'], hp['beta2']
    got = tb.update_variant()
    assert got.startswith(variant) if variant.endswith('(') else got == variant, got
    for p, pol in enumerate(pols):
        tb.set_task(p, pol.state_dict())
    obs, actions, logp, values, returns, adv = data
    for dst, src in ((tb.obs, torch.from_numpy(obs)), (tb.actions, actions), (tb.logp, logp), (tb.values, values),
                     (tb.returns, returns), (tb.adv, adv)):
        dst.copy_(src)
    tb.lr.fill_(bi.LR)
    tb.ppo_update(torch.stack(perms).numpy())
    assert int(tb.update_ws[2 * P]) == 0, 'tower exchange timed out'
    tb.check_update()
    params, am, av = tb.params.cpu().numpy(), tb.adam_m.cpu().numpy(), tb.adam_v.cpu().numpy()
    steps, stats = tb.adam_step.cpu(), tb.stats.cpu()
    lay = tb.layout
    what = f'{kernel} {shape} row {row}'
    for p, (pol, agent, st, _) in enumerate(results):
        ref = lay.flatten(pol.state_dict(), dtype=np.float64)
        m_ref, v_ref, step = lay.adam_from_optimizer_state(agent.optimizer.state_dict()['state'])
        for name, g, r, atol, rtol in (('params', params[p], ref, 2e-6, 1e-5), ('exp_avg', am[p], m_ref, 1e-7, 1e-3),
                                       ('exp_avg_sq', av[p], v_ref, 1e-10, 1e-3),
                                       ('loss stats', stats[p].numpy(), st, 1e-5, 1e-4)):
            err = np.abs(np.asarray(g, np.float64) - r)
            print(f'{what} task {p}: {name} max abs err {err.max():.3e}, '
                  f'{(err / (atol + rtol * np.abs(r))).max():.3f} of the band')
        assert int(steps[p]) == step == E * M
        _close(params[p], ref, 2e-6, 1e-5, f'{what} task {p}: params')
        _close(am[p], m_ref, 1e-7, 1e-3, f'{what} task {p}: exp_avg')
        _close(av[p], v_ref, 1e-10, 1e-3, f'{what} task {p}: exp_avg_sq')
        _close(stats[p], st, 1e-5, 1e-4, f'{what} task {p}: loss stats')
        if ln and row == 'f':  # the entropy term's own gradient: the logstd slice of exp_avg
            o, A = lay.offsets['logstd'], spec['act_dim']
            assert np.abs(am[p][o:o + A]).min() > 0
            _close(am[p][o:o + A], m_ref[o:o + A], 1e-7, 1e-3, f'{what} task {p}: exp_avg logstd')
