"""CPU suite of the depth priors (DS-NeRF's expected-depth and ray-termination losses): the cases of tests/depth_prior_cases.py on the
wave emulator -- the kernel against the definition in torch at every chunk boundary, parameter and ray gradients against the oracle's
autograd, every backward mode, the culled step -- and the host side of the new class and keywords that needs no device.  The emulator
runs the smaller of the render shapes; the GPU suite (tests/test_gpu_depth_prior.py) runs all of them on every net."""
import numpy as np
import pytest
import torch

import depth_prior_cases as D


@pytest.mark.parametrize("kind", D.KERNEL_KINDS)
def test_kernel_against_the_definition(emu, kind):
    D.case_kernel(emu, kind)


def test_kernel_long_rays(emu):
    """32 chunks of 64 with a ragged last one, and the largest S the entry point takes: the sums, with the weights given."""
    D.check_kernel_sums(emu, "noise_draws", 2, 2011, 8, seed=7)
    D.check_kernel_sums(emu, "noise_stream", 3, 8192, 11, seed=8)


def test_kernel_refusals(emu):
    D.case_kernel_refusals(emu)


def test_the_definition_has_the_closed_form_gradient():
    """The reference alone: autograd of the restated losses equals the header's dE/dw and dTm/dw (fp64), and rows without a prior are
    exact zeros whatever they carry."""
    c = D.kernel_inputs("tied_depths", 7, 40, 8, 3, 3)
    wts = (0.7, 0.03)
    loss, grad, w = D.depth_reference(c["raw"], c["z"], c["rays"], c["prior"], 0.0, None, torch.float64, wts)
    z, rays, p, has, w = c["z"].astype(np.float64), c["rays"].astype(np.float64), c["prior"].astype(np.float64), c["has"], w.numpy()
    assert (np.diff(z, axis=1) == 0).any() and (z[:, -1] > rays[:, 7]).any() and has.any() and not has.all()
    delta = np.concatenate((np.diff(z, axis=1), np.maximum(rays[:, 7:8] - z[:, -1:], 0.0)), axis=1)
    with np.errstate(invalid="ignore"):
        k = np.exp(-(z - p[:, 0:1]) ** 2 / (2.0 * p[:, 2:3] ** 2))
        dhat = (w * z).sum(axis=1, keepdims=True)
        want = wts[0] * 2.0 * p[:, 1:2] * (dhat - p[:, 0:1]) * z - wts[1] * p[:, 1:2] * k * delta / (w + D.EPS)
    assert np.abs(grad.numpy()[has] - want[has]).max() <= 1e-12 * np.abs(want[has]).max()
    assert (loss.numpy()[has] > 0).all() and not loss.numpy()[~has].any() and not grad.numpy()[~has].any()


@pytest.mark.parametrize("net,arith", [("w64", "fp32"), ("w128", "fp32"), ("w40of64", "f16x3_train")])
def test_parameter_gradients_against_the_oracle(emu, net, arith):
    D.case_param_grads(emu, net, arith, shapes=D.RENDER_SHAPES[:1])


def test_backward_modes_with_the_depth_cotangent(emu):
    D.case_compacted(emu, "w64", "fp32", (True, "recompute", "fused", "fused_compact", "fused_stash"))


def test_backward_modes_with_the_depth_cotangent_f16(emu):
    D.case_compacted(emu, "w40of64", "f16x3_train", (True, "recompute"))


def test_culled_step_with_a_prior(emu):
    D.case_culled_step(emu, "w64", "fp32", 0)


def test_ray_gradient_with_a_prior(emu):
    D.case_rays_w(emu, "w64")


def test_exported_symbol():
    import nerf_pytorch_amd._lib as L
    assert "nerfhip_depth_prior_loss" in L.EXPORTED_SYMBOLS
    assert len(L._PROTOS["nerfhip_depth_prior_loss"][1]) == 23
