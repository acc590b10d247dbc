"""The shared PPO loss terms (pgmorl_amd/csrc/pgm_ppo_terms.hpp) against torch fp32 autograd, off the GPU.

Every update kernel takes its value-loss and clipped-surrogate gradients from value_loss_term / surrogate_term.  The
header's loss terms are plain C++, so this test compiles them with the host compiler into a ctypes shim
(tests/native/ppo_terms_shim.cpp) and compares them with autograd of the reference's expressions
(a2c_ppo_acktr/algo/ppo.py:76-103) on a dyadic grid: every input is a multiple of 2^-6 and clip = 0.25, so every
product and sum is exact in fp32 and the comparison is bit for bit.  The grid hits the ties and edges on purpose:
V == Vold (l1 == l2, torch.max splits the gradient 0.5 / 0.5), V - Vold == +-clip (the clamp's closed interval),
adv == 0 (s1 == s2), ratio == 1 +- clip, both signs of adv inside and outside the clip range.

The 0.5 of the value loss is left out on both sides (the kernels carry it in their batch scale).  surrogate_term
returns d min(s1, s2) / d ratio next to the loss -min(s1, s2); the kernels' -1 / mb scale holds the sign, so the
loss's autograd gradient is its exact negation.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP = 0.25
U = 2.0 ** -6


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('ppo_terms') / 'libppo_terms_shim.so')
    cmd = [os.environ.get('CXX', 'g++'), '-O2', '-std=c++17', '-fPIC', '-shared', '-I',
           os.path.join(ROOT, 'pgmorl_amd', 'csrc'), os.path.join(ROOT, 'tests', 'native', 'ppo_terms_shim.cpp'),
           '-o', so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f'{" ".join(cmd)}\n{r.stdout}\n{r.stderr}'
    lib = ctypes.CDLL(so)
    fp = ctypes.POINTER(ctypes.c_float)
    lib.pgm_test_value_loss_term.argtypes = [ctypes.c_int, fp, fp, fp, ctypes.c_float, ctypes.c_int, fp, fp]
    lib.pgm_test_value_loss_term.restype = None
    lib.pgm_test_surrogate_term.argtypes = [ctypes.c_int, fp, fp, ctypes.c_float, fp, fp]
    lib.pgm_test_surrogate_term.restype = None
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _bits(x):
    """fp32 bit patterns with -0.0 folded onto +0.0 (a zero gradient has no sign to get wrong)."""
    return (np.ascontiguousarray(x, dtype=np.float32) + np.float32(0.0)).view(np.int32)


def _value_grid():
    # Vold on a coarse grid; V - Vold from well outside the clip range through +-clip exactly, one unit either side
    # of each edge, and 0 (the l1 == l2 tie); R on both sides of V and Vold and equal to each
    dv = np.array([-48, -17, -16, -15, -3, 0, 1, 15, 16, 17, 48], dtype=np.float32) * U
    vold = np.array([-40, 0, 24], dtype=np.float32) * U
    r = np.array([-64, -40, -9, 0, 7, 24, 32, 80], dtype=np.float32) * U
    g = np.stack(np.meshgrid(dv, vold, r, indexing='ij'), -1).reshape(-1, 3)
    vold_, r_ = g[:, 1].copy(), g[:, 2].copy()
    return vold_ + g[:, 0], vold_, r_


def _surrogate_grid():
    # ratio through 1 - clip and 1 + clip exactly, one unit either side of each, inside and far outside; adv of both
    # signs and 0 (the s1 == s2 tie)
    ratio = np.array([16, 47, 48, 49, 60, 64, 70, 79, 80, 81, 160], dtype=np.float32) * U
    adv = np.array([-96, -64, -1, 0, 1, 37, 128], dtype=np.float32) * U
    g = np.stack(np.meshgrid(ratio, adv, indexing='ij'), -1).reshape(-1, 2)
    return g[:, 0].copy(), g[:, 1].copy()


@pytest.mark.parametrize('clipped', [True, False])
def test_value_loss_term_matches_torch_autograd(shim, clipped):
    v, vold, r = _value_grid()
    assert np.any(v == vold) and np.any(v - vold == CLIP) and np.any(v - vold == -CLIP)
    grad, loss = np.empty_like(v), np.empty_like(v)
    shim.pgm_test_value_loss_term(len(v), _ptr(v), _ptr(vold), _ptr(r), CLIP, int(clipped), _ptr(grad), _ptr(loss))

    tv = torch.tensor(v, requires_grad=True)
    tvold, tr = torch.tensor(vold), torch.tensor(r)
    if clipped:
        vc = tvold + (tv - tvold).clamp(-CLIP, CLIP)
        ref = torch.max((tv - tr).pow(2), (vc - tr).pow(2))
    else:
        ref = (tr - tv).pow(2)
    ref.sum().backward()
    assert np.array_equal(_bits(loss), _bits(ref.detach().numpy()))
    assert np.array_equal(_bits(grad), _bits(tv.grad.numpy()))
    if clipped:  # the tie really splits: V == Vold with V != R gives exactly half of each branch, (V - R) twice
        tie = (v == vold) & (v != r)
        assert tie.any() and np.array_equal(grad[tie], 2 * (v - r)[tie])


def test_surrogate_term_matches_torch_autograd(shim):
    ratio, adv = _surrogate_grid()
    assert np.any(ratio == 1 - CLIP) and np.any(ratio == 1 + CLIP) and np.any(adv == 0)
    grad, loss = np.empty_like(ratio), np.empty_like(ratio)
    shim.pgm_test_surrogate_term(len(ratio), _ptr(ratio), _ptr(adv), CLIP, _ptr(grad), _ptr(loss))

    tr = torch.tensor(ratio, requires_grad=True)
    ta = torch.tensor(adv)
    ref = -torch.min(tr * ta, tr.clamp(1 - CLIP, 1 + CLIP) * ta)
    ref.sum().backward()
    assert np.array_equal(_bits(loss), _bits(ref.detach().numpy()))
    assert np.array_equal(_bits(-grad), _bits(tr.grad.numpy()))
    # outside the range on the clipped side the gradient is zero, inside it is adv
    assert np.all(grad[(ratio > 1 + CLIP) & (adv > 0)] == 0) and np.all(grad[(ratio < 1 - CLIP) & (adv < 0)] == 0)
    inside = (ratio > 1 - CLIP) & (ratio < 1 + CLIP)
    assert np.array_equal(grad[inside], adv[inside])
