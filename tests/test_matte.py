"""CPU suite of the alpha-matte loss: the cases of tests/matte_cases.py on the wave emulator -- the kernel against the definition in
torch at the wave and block edges, the bit identities, the refusals, parameter and ray gradients against the oracle's autograd, every
backward mode, the culled step -- and what needs no library at all: the definition's closed-form g_acc and the reference's loss.  The
GPU suite (tests/test_gpu_matte.py) runs the same cases on the product library and the public routes."""
import numpy as np
import pytest
import torch

import matte_cases as M


@pytest.mark.parametrize("mode", [0, 1])
def test_kernel_against_the_definition(emu, mode):
    M.case_kernel(emu, mode)


def test_kernel_propagates_nan_to_its_ray_only(emu):
    M.case_nan(emu)


def test_kernel_bit_identities(emu):
    M.case_bit_identities(emu)


def test_kernel_refusals(emu):
    M.case_refusals(emu)


def test_the_definition_has_the_closed_form_g_acc():
    """The definition alone: autograd of the restated loss equals the header's closed form of g_acc in fp64 -- minus sum_c g_rgb_c b_c,
    the alpha term and dH/dacc = log((1 - x) / x) inside the clamp, exactly 0 where the clamp acted."""
    n, gs, lam = 200, 0.37, (0.3, 0.05)
    c = M.kernel_inputs(n, 5, 11)
    _, g_rgb, g_acc = M.matte_reference(c["rgb"], c["acc"], c["tgt"], 0, c["bg"], lam, gs, torch.float64)
    acc, a, bg = c["acc"].astype(np.float64), np.clip(c["tgt"][:, 3].astype(np.float64), 0.0, 1.0), c["bg"].astype(np.float64)
    inside = (acc >= M.EPS) & (acc <= 1.0 - M.EPS)
    assert inside.any() and (~inside).sum() >= 4
    x = np.clip(acc, M.EPS, 1.0 - M.EPS)
    dH = np.where(inside, np.log((1.0 - x) / x), 0.0)
    want = -(g_rgb.numpy() * bg).sum(axis=1) + 2.0 * lam[0] / n * gs * (acc - a) + lam[1] / n * gs * dH
    assert np.abs(g_acc.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    # ... and g_rgb is 2 (p - t) / (3 n) grad_scale
    C = c["tgt"][:, :3].astype(np.float64)
    d = c["rgb"].astype(np.float64) + (1.0 - acc)[:, None] * bg - (a[:, None] * C + (1.0 - a)[:, None] * bg)
    assert np.abs(g_rgb.numpy() - 2.0 * d / (3 * n) * gs).max() <= 1e-15


def test_matte_over_white_is_the_reference_loss():
    """The definition alone: matte mode over background (1, 1, 1) with both weights 0 is the reference's loss -- RGBA targets
    composited onto white on the host (train_nerf.py:65-66: rgb * a + (1 - a)) against the white-background render rgb + (1 - acc)."""
    n = 300
    c = M.kernel_inputs(n, 4, 13)
    tgt = c["tgt"].copy()
    tgt[:, 3] = np.clip(tgt[:, 3], 0.0, 1.0)   # (an image's alpha)
    white = np.ones((n, 3), np.float32)
    loss, g_rgb, g_acc = M.matte_reference(c["rgb"], c["acc"], tgt, 0, white, (0.0, 0.0), 1.0, torch.float64)
    rgb = torch.as_tensor(c["rgb"]).double().requires_grad_(True)
    acc = torch.as_tensor(c["acc"]).double().requires_grad_(True)
    t = torch.as_tensor(tgt).double()
    target_white = t[:, :3] * t[:, 3:] + (1.0 - t[:, 3:])
    ref = torch.nn.functional.mse_loss(rgb + (1.0 - acc[:, None]), target_white)
    ref.backward()
    assert abs(float(loss[0]) - float(ref.detach())) <= 1e-15
    assert float((g_rgb - rgb.grad).abs().max()) <= 1e-15 and float((g_acc - acc.grad).abs().max()) <= 1e-15


@pytest.mark.parametrize("net,arith", M.RENDER_NETS)
def test_parameter_gradients_against_the_oracle(emu, net, arith):
    M.case_param_grads(emu, net, arith, shapes=M.RENDER_SHAPES[:1])


def test_parameter_gradients_against_the_oracle_at_64_samples(emu):
    M.case_param_grads(emu, "w64", "fp32", shapes=M.RENDER_SHAPES[1:])


def test_backward_modes_with_the_opacity_cotangent(emu):
    M.case_compacted(emu, "w64", "fp32", (True, "recompute", "fused", "fused_compact", "fused_stash"))


def test_backward_modes_with_mixed_alphas(emu):
    M.case_compacted(emu, "w64", "fp32", (True, "recompute", "fused", "fused_compact", "fused_stash"), opaque=False)


def test_backward_modes_with_the_opacity_cotangent_f16(emu):
    M.case_compacted(emu, "w40of64", "f16x3_train", (True, "recompute"))


def test_culled_step_with_the_matte_loss(emu):
    M.case_culled_step(emu, "w64", "fp32", 0)


def test_ray_gradient_with_the_matte_loss(emu):
    M.case_ray_grad(emu, "w64")


def test_exported_symbol():
    import nerf_pytorch_amd._lib as L
    assert "nerfhip_matte_loss_fwd_bwd" in L.EXPORTED_SYMBOLS
    assert len(L._PROTOS["nerfhip_matte_loss_fwd_bwd"][1]) == 20
