"""CPU suite of the ray-weight spread loss (mip-NeRF 360's L_dist): the cases of tests/spread_cases.py on the wave emulator -- the kernel
against the S^2 definition in torch at every chunk boundary, the weight cotangent through the fused backward bit for bit against the
hand-assembled compositing backward, parameter and ray gradients against the oracle's autograd, every backward mode, the culled step
-- and the host side of the new keywords that needs no device.  The emulator runs the smaller of the render shapes; the GPU suite
(tests/test_gpu_spread.py) runs all of them on every net."""
import numpy as np
import pytest
import torch

import spread_cases as S


@pytest.mark.parametrize("kind", S.KERNEL_KINDS)
def test_kernel_against_the_definition(emu, kind):
    S.case_kernel(emu, kind)


def test_kernel_many_chunks(emu):
    """32 chunks of 64 and a ragged last one: the sums, with the weights given."""
    S.check_kernel_sums(emu, "noise_draws", 2, 2048 - 37, 8, seed=7)
    S.check_kernel_sums(emu, "noise_stream", 3, 8192, 11, seed=8)   # (the largest S the entry point takes)


def test_kernel_refusals(emu):
    S.case_kernel_refusals(emu)


def test_the_definition_is_the_prefix_form():
    """The reference alone: the S^2 sum's autograd gradient equals the issue's closed form with prefix and suffix sums (fp64)."""
    c = S.kernel_inputs("tied_depths", 6, 40, 8, 3)
    loss, grad, w = S.spread_reference(c["raw"], c["z"], c["rays"], 0.0, None, torch.float64)
    z, rays, w = c["z"].astype(np.float64), c["rays"].astype(np.float64), w.numpy()
    s = (z - rays[:, 6:7]) / (rays[:, 7:8] - rays[:, 6:7])
    e = np.concatenate((s[:, 1:], np.maximum(s[:, -1:], 1.0)), axis=1)
    m, d = 0.5 * (s + e), e - s
    assert np.all(np.diff(m, axis=1) >= 0) and (np.diff(z, axis=1) == 0).any()
    Wl, Ml = np.cumsum(w, 1) - w, np.cumsum(w * m, 1) - w * m
    Wg, Mg = w.sum(1, keepdims=True) - Wl - w, (w * m).sum(1, keepdims=True) - Ml - w * m
    want = 2.0 * (m * (Wl - Wg) - (Ml - Mg)) + (2.0 / 3.0) * w * d
    assert np.abs(grad.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    assert (loss.numpy() > 0).all()


@pytest.mark.parametrize("net,arith,layout", [("w64", "fp32", 1), ("w40of64", "f16x3_train", 2)])
def test_w_entry_points_bit_checks(emu, net, arith, layout):
    S.case_w_bits(emu, net, arith, layout, shapes=S.RENDER_SHAPES[:1])


@pytest.mark.parametrize("net,arith", [("w64", "fp32"), ("w128", "fp32"), ("w40of64", "f16x3_train")])
def test_parameter_gradients_against_the_oracle(emu, net, arith):
    S.case_param_grads(emu, net, arith, shapes=S.RENDER_SHAPES[:1])


def test_backward_modes_with_a_weight_cotangent(emu):
    S.case_compacted(emu, "w64", "fp32", (True, "recompute", "fused", "fused_compact", "fused_stash"))


def test_backward_modes_with_a_weight_cotangent_f16(emu):
    S.case_compacted(emu, "w40of64", "f16x3_train", (True, "recompute"))


@pytest.mark.parametrize("net,arith,outside", [("w64", "fp32", 0), ("w40of64", "f16x3_train", 1)])
def test_culled_step_with_spread(emu, net, arith, outside):
    S.case_culled_step(emu, net, arith, outside)


def test_ray_gradient_with_spread(emu):
    S.case_rays_w(emu, "w64")


def test_exported_symbols_and_struct():
    import nerf_pytorch_amd._lib as L
    assert {"nerfhip_spread_loss", "nerfhip_render_bwd_parts_w", "nerfhip_render_bwd_rays_w"} <= set(L.EXPORTED_SYMBOLS)
    names = [k for k, _ in L.RenderCotangentsW._fields_]
    assert names[:6] == [k for k, _ in L.RenderCotangents._fields_] and names[6:] == ["g_weights_coarse", "g_weights_fine"]
