"""The feature-split update (pgm_ppo_fs.hip) on ragged tile deals: 6 parts per tower, at most 3 16-row tiles per part,
minibatches whose tile count is no multiple of 6, so that some parts run a tile fewer than others -- 208 rows
(3/2/2/2/2/2), 224 (3/3/2/2/2/2), 240 (3/3/3/2/2/2) -- where a part's tile count selects the code it runs.  Every task
against the fp64 oracle's PPO as tests/test_gpu_fs.py checks it (parameters, both Adam moments, step count, loss
statistics, the exchange-timeout word), on Walker (obs_dim 17: a VALU layer-1 tail), HalfCheetah with a partial task
group (P = 33) and Hopper-v3 (three objectives, obs_dim 11: no tail); and one full deal with the loss options that
are fixed per tower instance: a nonzero entropy coefficient and the unclipped value loss."""
import functools

import pytest

from . import test_gpu_fs as fs

pytestmark = pytest.mark.gpu

VARIANT = 'ppo_update_fs_kernel (NS=6, R=3, 2 per CU)'


@pytest.mark.parametrize('mb', [208, 224, 240])
@pytest.mark.parametrize('env,P', [('MO-Walker2d-v2', 40), ('MO-HalfCheetah-v2', 33), ('MO-Hopper-v3', 40)])
def test_fs_ragged_tile_deals(gpu, monkeypatch, env, P, mb):
    monkeypatch.setenv('PGM_UPDATE_KERNEL', 'fs')
    monkeypatch.setenv('PGM_FS_DUAL', '1')
    fs._check_update(env, P, 4, E=2, M=2, mb=mb, seed=53, variant=VARIANT)  # 4 Adam steps: both slot parities twice


def test_fs_entropy_and_unclipped_value_loss(gpu, monkeypatch):
    """entropy_coef = 0.01 and use_clipped_value_loss off at Walker P = 40, 256 rows (3/3/3/3/2/2): the batch's
    hyper-parameter and the oracle's PPO both switched to the unclipped value loss (ppo.py:87-88)."""
    monkeypatch.setenv('PGM_UPDATE_KERNEL', 'fs')
    monkeypatch.setenv('PGM_FS_DUAL', '1')
    setup = fs._update_setup

    def unclipped_setup(*a, **kw):
        out = setup(*a, **kw)
        out[2].hp.use_clipped_value_loss = 0
        return out

    class Oracle:
        PPO = staticmethod(functools.partial(fs.oppo.PPO, use_clipped_value_loss=False))
        RolloutStorage = fs.oppo.RolloutStorage

    monkeypatch.setattr(fs, '_update_setup', unclipped_setup)
    monkeypatch.setattr(fs, 'oppo', Oracle)
    fs._check_update('MO-Walker2d-v2', 40, 4, E=2, M=2, mb=256, seed=53, entropy_coef=0.01, variant=VARIANT)
