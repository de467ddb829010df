"""GPU suite (-m gpu): the product library libnerfhip.so on a real MI355X against the oracle / reference goldens,
through the C ABI (tests/backends.py GpuBackend) and through the Python drop-in API."""
import ast

import numpy as np
import pytest
import torch

import nerf_oracle as O
import parity_cases as P
import tolerances as T
from backends import model_cfg
from conftest import gold

pytestmark = pytest.mark.gpu


def test_native_library_is_the_one_loaded(gpu):
    assert gpu.lib.is_emulated() == 0
    assert gpu.lib.path.endswith("nerf-pytorch_amd/libnerfhip.so")


def test_rays(gpu):
    P.case_rays(gpu)


def test_posenc(gpu):
    P.case_posenc(gpu)


def test_stratified(gpu):
    P.case_stratified(gpu)


def test_cumprod(gpu):
    P.case_cumprod(gpu)


def test_volume_render(gpu):
    P.case_volume_render(gpu)


def test_volume_render_bwd(gpu):
    P.case_volume_render_bwd(gpu)


def test_sample_pdf_indices_bit_exact(gpu):
    P.case_sample_pdf(gpu)


def test_loss_adam(gpu):
    P.case_loss_adam(gpu)


def test_mlp_forward_all_geometries(gpu):
    P.case_mlp_forward(gpu, m=1000)


def test_mlp_forward_reference_goldens(gpu):
    P.case_mlp_golden(gpu)


def test_mlp_64_wide_instances(gpu):
    names = ("llff4x64_skip3_L6", "deep8x64_skip4", "novw3x64_skip1", "one_layer_64")
    P.case_mlp_forward(gpu, names=names, m=1000)
    P.case_mlp_backward(gpu, names=names, m=1500)
    P.case_mlp_input_grad(gpu, names=("llff4x64_skip3_L6",), m=1500)


def test_render_64_wide_llff_config_vs_oracle(gpu):
    """config/llff.yml nets (4x64, skip 3, 6 xyz frequencies) on 64 + 64 samples with gradients."""
    P.case_render_vs_oracle(gpu, P.MLP_GEOMETRIES["llff4x64_skip3_L6"], n=300, nc=64, nf=64, noise=1.0, with_grads=True,
                            tag="llff64_300", grad_tol=(1e-3, 2e-2))


def test_mlp_512_wide_instances(gpu):
    names = ("wide3x512_skip2", "wide2x320", "novw2x512")
    P.case_mlp_forward(gpu, names=names, m=1000)
    P.case_mlp_backward(gpu, names=names, m=1500)
    P.case_mlp_input_grad(gpu, names=("wide3x512_skip2", "wide2x320"), m=1500)


def test_render_512_wide_vs_oracle(gpu):
    """An 8x512 net pair (hidden_size 512: nerf/models.py:186-196 takes it) through the fused render with gradients."""
    P.case_render_vs_oracle(gpu, model_cfg(8, 512, 4, 10, 4), n=96, nc=64, nf=64, with_grads=True, tag="wide8x512_96",
                            grad_tol=(3.4e-3, 2e-2))


# ---- the fp16-piece plans (NERFHIP_PRECISION_F16X3*): the fp32 kernels' own bounds (tests/tolerances.py: one entry per quantity) ----
def test_mlp_forward_f16x3(gpu):
    """Twelve geometries: within the fp32 kernels' 2e-5 of the oracle and at an fp32-sized distance from the fp64 forward; the
    fused inference render: coarse maps at 1e-5, the fine pass no further from the oracle than the fp32 kernels' own."""
    P.case_mlp_forward_f16x3(gpu, m=3000, precision=P.F16X3)
    P.case_render_f16x3(gpu, P.MLP_GEOMETRIES["default4x128"], n=300, nc=64, nf=64, tag="4x128_300", precision=P.F16X3)
    P.case_render_f16x3(gpu, P.MLP_GEOMETRIES["northstar8x256"], n=128, nc=64, nf=128, tag="8x256_128", precision=P.F16X3)


@pytest.mark.parametrize("level", ["fwd", "fwd_dgrad", "train"])
def test_mlp_f16x3_training_levels_hold_the_fp32_gradient_bounds(gpu, level):
    """case_mlp_backward / case_mlp_input_grad / case_render_vs_oracle exactly as the fp32 kernels run them (test_mlp_backward,
    test_render_northstar_geometry): 2e-5 of max|g| teacher-forced at m = 1500 with the 1e-6 ReLU margin, default render bounds."""
    prec = {"fwd": P.F16X3_FWD, "fwd_dgrad": P.F16X3_FWD_DGRAD, "train": P.F16X3_TRAIN}[level]
    P.case_mlp_backward(gpu, names=("default4x128", "fern8x128_skip3_L6", "novw4x128", "skip_every_layer_256", "odd5x99_skip2",
                                    "one_layer", "two_layer_L4_L2", "northstar8x256"), m=1500, precision=prec)
    if level != "fwd":
        P.case_mlp_backward(gpu, names=("default4x128", "northstar8x256"), m=1500, precision=prec, g_scale=2e-8)  # (tiny cotangents)
        # weights 3x torch's init (8x256: activations in the thousands, d(pre-activation) ~1e6 x d(raw output)) and 0.3x (both tiny)
        P.case_mlp_backward(gpu, names=("northstar8x256", "skip_every_layer_256"), m=1500, precision=prec, w_gain=3.0, g_scale=1e-3)
        P.case_mlp_backward(gpu, names=("northstar8x256",), m=1500, precision=prec, w_gain=0.3)
        P.case_mlp_input_grad(gpu, names=("default4x128", "novw4x128", "northstar8x256"), m=1500, precision=prec)
    P.case_render_vs_oracle(gpu, P.MLP_GEOMETRIES["northstar8x256"], n=48, nc=64, nf=128, with_grads=True, tag="f16x3_%s_8x256_48" % level,
                            grad_tol=(T.bound("unit.render_grad.coarse_fp64_yardstick", P.ARITH_NAME[prec]), T.bound("unit.render_grad.fine_sanity", P.ARITH_NAME[prec])), precision=prec)  # (test_northstar_render_and_gradients_vs_oracle's bounds)
    P.case_render_vs_oracle(gpu, P.MLP_GEOMETRIES["default4x128"], n=200, nc=64, nf=64, white=True, noise=1.0, with_grads=True,
                            tag="f16x3_%s_default200_white_noise1" % level, grad_tol=(T.bound("unit.render_grad.coarse_fp64_yardstick", P.ARITH_NAME[prec]), T.bound("unit.render_grad.fine_sanity", P.ARITH_NAME[prec])), precision=prec)  # (test_default_model_render_white_background's)


def test_f16x3_scale_fuzz(gpu):
    P.case_f16x3_scale_fuzz(gpu, m=700)


def test_f16x3_dead_layers(gpu):
    P.case_f16x3_dead_layers(gpu, m=1500)


def test_f16x3_range_extremes(gpu):
    P.case_f16x3_range_extremes(gpu, m=1500)


def test_mlp_f16x3_64_wide_instances(gpu):
    """The 64-wide instances of the fp16-piece kernels (config/fern.yml's declared 4 x 64, config/llff.yml; round 5): what
    test_mlp_64_wide_instances / test_render_64_wide_llff_config_vs_oracle assert of the fp32 kernels, every training level (the
    weight-gradient GEMMs of 64-wide nets all stay on the fp32 kernel: _TRAIN is _FWD_DGRAD there)."""
    names = ("llff4x64_skip3_L6", "deep8x64_skip4", "novw3x64_skip1", "one_layer_64")
    for prec in (P.F16X3_FWD, P.F16X3_FWD_DGRAD, P.F16X3_TRAIN):
        P.case_mlp_backward(gpu, names=names, m=1500, precision=prec)
    P.case_mlp_input_grad(gpu, names=("llff4x64_skip3_L6",), m=1500, precision=P.F16X3_FWD_DGRAD)
    P.case_render_vs_oracle(gpu, P.MLP_GEOMETRIES["llff4x64_skip3_L6"], n=300, nc=64, nf=64, noise=1.0, with_grads=True,
                            tag="f16x3_llff64_300", grad_tol=(1e-3, 2e-2), precision=P.F16X3_TRAIN)


@pytest.mark.parametrize("name", ["e2e_a.npz", "e2e_b.npz", "e2e_c.npz", "e2e_d.npz", "e2e_northstar.npz"])
def test_e2e_reference_goldens_f16x3_train(gpu, name):
    """The goldens recorded from the REAL reference (outputs, loss, every gradient tensor), every kernel of the step on fp16 pieces:
    the same assertions as test_e2e_reference_goldens / test_e2e_northstar_reference_golden."""
    if name == "e2e_northstar.npz":
        P.case_e2e_northstar_golden(gpu, precision=P.F16X3_TRAIN)
    else:
        P.case_e2e_golden(gpu, name, precision=P.F16X3_TRAIN)


def test_ndc_rays_backward(gpu):
    P.case_ndc_rays_bwd(gpu, n=5000)


def test_mlp_extended_encodings(gpu):
    """num_encoding_fn_xyz up to 16 / num_encoding_fn_dir up to 10: the extended slot registers, every kernel width."""
    P.case_mlp_forward(gpu, names=P.EXT_GEOMETRIES, m=1000)
    P.case_mlp_backward(gpu, names=P.EXT_GEOMETRIES, m=1500)
    P.case_mlp_input_grad(gpu, names=("L12_4x128", "Ld5_4x128_skip2", "L16_Ld6_8x256"), m=1500)
    P.case_render_vs_oracle(gpu, P.MLP_GEOMETRIES["L12_4x128"], n=200, nc=64, nf=64, with_grads=True, tag="L12_200")
    P.case_ray_grad(gpu, P.MLP_GEOMETRIES["L12_4x128"], n=100, nc=32, nf=32)


def test_mlp_padded_hidden_sizes(gpu):
    names = ("narrow3x40", "odd5x99_skip2", "wide3x200_skip1", "novw2x130")
    P.case_mlp_forward(gpu, names=names, m=700)
    P.case_mlp_backward(gpu, names=names, m=1500)


def test_mlp_input_gradient(gpu):
    P.case_mlp_input_grad(gpu, names=("default4x128", "fern8x128_skip3_L6", "novw4x128", "odd5x99_skip2", "northstar8x256"),
                          m=1500)


def test_mlp_backward(gpu):
    P.case_mlp_backward(gpu, names=("default4x128", "deep8x128_skip4", "fern8x128_skip3_L6", "novw4x128",
                                    "northstar8x256"), m=1500)


# ---- exact row counts at every tile edge (parity_cases.ROW_EDGES): one plan per test ------------------------------------------------
_ROW_EDGE_PLANS = [(n, 0) for n in ("default4x128", "novw4x128", "northstar8x256", "llff4x64_skip3_L6", "wide2x320", "odd5x99_skip2",
                                    "L12_4x128")] \
    + [(n, P.F16X3_TRAIN) for n in ("default4x128", "northstar8x256", "llff4x64_skip3_L6")] \
    + [("novw4x128", P.F16X3_FWD_DGRAD)] + [(n, P.F16X3) for n in ("default4x128", "northstar8x256")]


@pytest.mark.parametrize("name,precision", _ROW_EDGE_PLANS, ids=["%s-%s" % (n, P.ARITH_NAME[p]) for n, p in _ROW_EDGE_PLANS])
def test_mlp_row_edges(gpu, name, precision):
    """Forward, backward, the reference's own conditioning and prefix invariance at 1 ... 257 rows: one below, on and one above 16, 32,
    48, 64, 128 and 256 (wide2x320: the 512-wide instances; odd5x99_skip2: zero-padded; L12_4x128: the extended slots; F16X3:
    inference-only, the forward assertions)."""
    P.case_mlp_row_edges(gpu, name, precision)


_PERSISTENT_PLANS = [("default4x128", P.F16X3_TRAIN, (0, 1, 2)), ("default4x128", 0, (0, 1, 2)), ("default4x128", P.F16X3, (0, 1, 2))] \
    + [("northstar8x256", P.F16X3_TRAIN, (i,)) for i in (0, 1, 2)]


@pytest.mark.parametrize("name,precision,which", _PERSISTENT_PLANS,
                         ids=["%s-%s-%s" % (n, P.ARITH_NAME[p], "".join("abc"[i] for i in w)) for n, p, w in _PERSISTENT_PLANS])
def test_mlp_persistent_round_edges(gpu, name, precision, which):
    """Dense batches of 128 C (a), 128 C + 1 (b) and 128 (C + 1) + 17 (c) rows on the device's C compute units: exactly one round of the
    persistent fp16-piece kernels, a second round of one row, two second rounds with a ragged last one (8x256: one count per test,
    the reference's autograd over 33,000 rows takes seconds)."""
    P.case_persistent_round_edges(gpu, name, precision, which)


@pytest.mark.parametrize("name,precision", [("default4x128", 0), ("default4x128", P.F16X3_TRAIN), ("northstar8x256", 0), ("llff4x64_skip3_L6", 0)],
                         ids=lambda v: P.ARITH_NAME[v] if isinstance(v, int) else v)
def test_compacted_backward_kept_count_edges(gpu, name, precision):
    """Exactly 290 rows, of which exactly k carry a cotangent -- k on, one below and one above the list path's 32-row tiles and 128-row
    groups, as the first rows, as the last rows, and (33, 129) strided over the batch."""
    P.case_mlp_backward_compacted(gpu, names=(name,), precision=precision, rows=290, fractions=(), kept_counts=(1, 31, 32, 33, 127, 128, 129, 289))


_RAGGED_RENDERS = [("default4x128", 96, 19, 13), ("northstar8x256", 48, 43, 22)]


@pytest.mark.parametrize("arith", ["fp32", "f16x3_train"])
@pytest.mark.parametrize("name,n,nc,nf", _RAGGED_RENDERS, ids=[r[0] for r in _RAGGED_RENDERS])
def test_render_samples_per_ray_not_a_multiple_of_16(gpu, name, n, nc, nf, arith):
    """19 + 13 and 43 + 22 samples per ray: a wave's 16 samples straddle two rays in both passes of the 128- / 256-wide and fp16-piece
    kernels (every other render of theirs here uses multiples of 16).  Render with gradients at test_northstar_render_and_gradients_vs_oracle's
    bounds, and the backward's dense / compacted / recomputed modes.  (Not fewer rays: on three rays of 8x256 the end-to-end fine-net
    gradient is ill-conditioned by the reference's own account, see tests/test_emu_parity.py's case of the same name.)"""
    prec = {"fp32": 0, "f16x3_train": P.F16X3_TRAIN}[arith]
    tag = "ragged%d+%d_%s_%d_%s" % (nc, nf, name, n, arith)
    P.case_render_vs_oracle(gpu, P.MLP_GEOMETRIES[name], n=n, nc=nc, nf=nf, with_grads=True, tag=tag, precision=prec,
                            grad_tol=(T.bound("unit.render_grad.coarse_fp64_yardstick", arith), T.bound("unit.render_grad.fine_sanity", arith)))
    P.case_render_compacted(gpu, P.MLP_GEOMETRIES[name], n=n, nc=nc, nf=nf, precision=prec, tag=tag)


@pytest.mark.parametrize("arith", ["fp32", "f16x3_fwd_dgrad", "f16x3_train"])
def test_compacted_backward_equals_dense(gpu, arith):
    """nerfhip_plan_set_bwd_compaction (round 6): the backward over the samples whose d(raw output) row is not all zero == the dense
    backward of the same plan (`unit.compact_vs_dense`), and both within the oracle's autograd bound; zero fractions 0 ... 1, a batch
    whose only non-zero row is its last sample; every kernel width."""
    prec = {"fp32": 0, "f16x3_fwd_dgrad": P.F16X3_FWD_DGRAD, "f16x3_train": P.F16X3_TRAIN}[arith]
    P.case_mlp_backward_compacted(gpu, names=("northstar8x256", "default4x128", "fern8x128_skip3_L6", "novw4x128", "llff4x64_skip3_L6"),
                                  m=1500, precision=prec)
    if arith == "fp32":
        P.case_mlp_backward_compacted(gpu, names=("wide3x512_skip2", "odd5x99_skip2", "one_layer"), m=700, fractions=(0.5, 0.97))
    else:
        P.case_mlp_backward_compacted(gpu, names=("default4x128",), m=1500, precision=prec, fractions=(0.6,), g_scale=3e-7)


@pytest.mark.parametrize("arith", ["fp32", "f16x3_train"])
def test_render_backward_modes_dense_compacted_recomputed(gpu, arith):
    prec = {"fp32": 0, "f16x3_train": P.F16X3_TRAIN}[arith]
    P.case_render_compacted(gpu, P.MLP_GEOMETRIES["northstar8x256"], n=96, nc=64, nf=128, precision=prec, tag="northstar96")
    P.case_render_compacted(gpu, P.MLP_GEOMETRIES["default4x128"], n=300, nc=64, nf=64, precision=prec, tag="default300", white=True, noise=1.0)
    P.case_render_compacted(gpu, P.MLP_GEOMETRIES["llff4x64_skip3_L6"], n=200, nc=64, nf=64, precision=prec, tag="llff200")


def test_fused_backward_of_64_wide_nets(gpu):
    """csrc/mlp64r.hip on MI355X (tests/test_emu_parity.py has the same cases on the emulator): 256 persistent workgroups, several
    rounds each, a ragged last round; 4 x 64 (config/fern.yml), one layer, 40 of 64 units; every sample and the compaction list."""
    P.case_render_compacted(gpu, P.MLP_GEOMETRIES["llff4x64_skip3_L6"], n=4096, nc=64, nf=64, tag="llff4096_fused", noise=1.0, fused=True)
    P.case_render_compacted(gpu, P.MLP_GEOMETRIES["llff4x64_skip3_L6"], n=777, nc=24, nf=9, tag="llff777_fused", white=True, fused=True)
    P.case_render_compacted(gpu, P.MLP_GEOMETRIES["one_layer_64"], n=300, nc=16, nf=16, tag="one64_fused", noise=0.0, fused=True)
    P.case_render_compacted(gpu, P.MLP_GEOMETRIES["narrow3x40"], n=500, nc=24, nf=16, tag="narrow40_fused", fused=True)
    P.case_render_compacted(gpu, P.MLP_GEOMETRIES["two_layer_64"], n=400, nc=32, nf=16, tag="two64_fused", fused=True)
    P.case_render_compacted(gpu, P.MLP_GEOMETRIES["three_layer_48"], n=400, nc=16, nf=24, tag="three48_fused", white=True, fused=True)
    P.case_render_fused_edges(gpu, P.MLP_GEOMETRIES["llff4x64_skip3_L6"])
    P.case_ray_grad(gpu, P.MLP_GEOMETRIES["llff4x64_skip3_L6"], n=12, nc=8, nf=8, compact="fused_compact")
    P.case_ray_grad(gpu, P.MLP_GEOMETRIES["llff4x64_skip3_L6"], n=333, nc=24, nf=16, compact="fused_stash")


@pytest.mark.parametrize("arith", ["fp32", "f16x3_train"])
def test_full_size_compacted_backward_equals_dense(gpu, arith):
    """BASELINE configs[1] at full size (4096 rays, 64 + 128, 8x256): the fused render's backward with both plans compacted against the
    same backward dense -- the cotangents are the renderer's own, so the rows dropped are exactly those relu(sigma + noise) and the
    transmittance zero (nerf/volume_rendering_utils.py:38-42).  Both compacted modes: stash rows gathered (1), and stash-free forward +
    recomputation of the kept samples (2: outputs bit-identical to the stash-writing forward's)."""
    prec = {"fp32": 0, "f16x3_train": P.F16X3_TRAIN}[arith]
    cfg = P.MLP_GEOMETRIES["northstar8x256"]
    pc, _, _, packed_c = P.mlp_setup(gpu, cfg, seed=11, precision=prec)
    pf, _, _, packed_f = P.mlp_setup(gpu, cfg, seed=12, precision=prec)
    _, _, _, _, _, rays, opt, tgt = _full_setup(gpu)
    n = rays.shape[0]
    fwd = gpu.render(pc, pf, packed_c, packed_f, rays, opt, None, seed=5, training=True)
    _, gc, gf = gpu.mse_loss(fwd["rgb_coarse"], fwd["rgb_fine"], tgt)
    dense = gpu.render(pc, pf, packed_c, packed_f, rays, opt, None, seed=5, training=True, g_rgb=(gc, gf))
    tol = T.bound("e2e.compact_vs_dense")
    rec = {}
    for mode in (True, "recompute"):
        gpu.set_compaction(pc, mode)
        gpu.set_compaction(pf, mode)
        comp = gpu.render(pc, pf, packed_c, packed_f, rays, opt, None, seed=5, training=True, g_rgb=(gc, gf))
        again = gpu.render(pc, pf, packed_c, packed_f, rays, opt, None, seed=5, training=True, g_rgb=(gc, gf))
        for k in ("rgb_coarse", "rgb_fine", "acc_fine", "depth_fine", "disp_fine"):
            assert np.array_equal(comp[k], dense[k], equal_nan=True), (mode, k)   # (mode 2: the stash-free training forward)
        for key, name, total in (("g_params_coarse", "coarse", n * 64), ("g_params_fine", "fine", n * 192)):
            kept, tot = comp["bwd_kept_" + name]
            assert tot == total and 0 < kept < total, (name, kept, tot)
            assert np.array_equal(comp[key], again[key]), key           # fixed order: bit-reproducible
            assert np.isfinite(comp[key]).all()
            worst = 0.0
            plan = pc if name == "coarse" else pf
            gd, gk = gpu.unflatten(plan, dense[key]), gpu.unflatten(plan, comp[key])
            for k in gd:
                d = float(np.abs(gk[k] - gd[k]).max()) / (float(np.abs(gd[k]).max()) + 1e-30)
                worst = max(worst, d)
                assert d <= tol, (arith, mode, key, k, d, tol)
            rec["%s_%s" % (name, mode)] = dict(kept=kept, total=tot, zero_fraction=round(1.0 - kept / tot, 4), worst_vs_dense=worst)
    P.note("full_size_compact_vs_dense_%s" % arith, **{"%s_%s" % (a, b): v for a, r in rec.items() for b, v in r.items()})
    for p in (pc, pf):
        gpu.lib.plan_destroy(p)


@pytest.mark.parametrize("name", ["e2e_a.npz", "e2e_b.npz", "e2e_c.npz", "e2e_d.npz"])
def test_e2e_reference_goldens(gpu, name):
    P.case_e2e_golden(gpu, name)


def test_northstar_render_and_gradients_vs_oracle(gpu):
    P.case_render_vs_oracle(gpu, P.MLP_GEOMETRIES["northstar8x256"], n=48, nc=64, nf=128, with_grads=True, tag="northstar48",
                            grad_tol=(T.bound("unit.render_grad.coarse_fp64_yardstick"), T.bound("unit.render_grad.fine_sanity")))


def test_default_model_render_white_background(gpu):
    P.case_render_vs_oracle(gpu, P.MLP_GEOMETRIES["default4x128"], n=200, nc=64, nf=64, white=True, noise=1.0,
                            with_grads=True, tag="default200_white_noise1",
                            grad_tol=(T.bound("unit.render_grad.coarse_fp64_yardstick"), T.bound("unit.render_grad.fine_sanity")))


def test_ray_gradients_c_abi(gpu):
    P.case_ray_grad(gpu, P.MLP_GEOMETRIES["default4x128"], n=300, nc=64, nf=64)
    P.case_ray_grad(gpu, P.MLP_GEOMETRIES["northstar8x256"], n=64, nc=32, nf=32, noise=0.2)
    P.case_ray_grad(gpu, P.MLP_GEOMETRIES["novw3x64_skip1"], n=100, white=True, noise=0.5)
    P.case_ray_grad(gpu, P.MLP_GEOMETRIES["wide2x320"], n=40)
    # (round 6: through the compacted d(pre-activation) images, both modes)
    P.case_ray_grad(gpu, P.MLP_GEOMETRIES["default4x128"], n=300, nc=64, nf=64, compact=True)
    P.case_ray_grad(gpu, P.MLP_GEOMETRIES["northstar8x256"], n=64, nc=32, nf=32, noise=0.2, compact="recompute")


def test_internal_rng_equals_external_draws(gpu):
    P.case_internal_rng(gpu)


# ---- full size (BASELINE configs[1]: 4096 rays, 64+128, 8x256): size-independent properties ----------------------------
def _full_setup(gpu, n=4096):
    cfg = P.MLP_GEOMETRIES["northstar8x256"]
    pc, _, _, packed_c = P.mlp_setup(gpu, cfg, seed=11)
    pf, _, _, packed_f = P.mlp_setup(gpu, cfg, seed=12)
    g = torch.Generator().manual_seed(3)
    ro = torch.tensor([0.0, 0.0, 4.0]).expand(n, 3) + 0.02 * torch.randn(n, 3, generator=g)
    rd = torch.randn(n, 3, generator=g) * 0.35
    rd[:, 2] = -1.0
    rays = O.pack_rays(ro, rd, 2.0, 6.0, rd).numpy()
    opt = dict(num_coarse=64, num_fine=128, perturb=True, lindisp=False, white_background=False, noise_std=0.2)
    return cfg, pc, pf, packed_c, packed_f, rays, opt, torch.rand(n, 3, generator=g).numpy()


def test_full_size_chunk_invariance_and_reproducibility(gpu):
    """Rendering 4096 rays at once == rendering them in two halves with the matching ray_offset (chunking is
    semantically transparent), bit for bit; and a repeat run is bit-identical."""
    cfg, pc, pf, packed_c, packed_f, rays, opt, tgt = _full_setup(gpu)
    a = gpu.render(pc, pf, packed_c, packed_f, rays, opt, None, seed=77, ray_offset=0)
    b = gpu.render(pc, pf, packed_c, packed_f, rays, opt, None, seed=77, ray_offset=0)
    h1 = gpu.render(pc, pf, packed_c, packed_f, rays[:2048], opt, None, seed=77, ray_offset=0)
    h2 = gpu.render(pc, pf, packed_c, packed_f, rays[2048:], opt, None, seed=77, ray_offset=2048)
    for k in ("rgb_coarse", "rgb_fine", "acc_fine", "depth_fine", "disp_fine"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert np.array_equal(a[k], np.concatenate([h1[k], h2[k]]), equal_nan=True), k
    assert np.isfinite(a["rgb_fine"]).all() and (a["acc_fine"] >= 0).all() and (a["acc_fine"] <= 1.0 + 1e-4).all()


def test_full_size_gradient_linearity(gpu):
    """grad(all 4096 rays) == grad(first half) + grad(second half) for the same cotangents (the weight gradient is a
    sum over samples): checks the split-K reduction at full size."""
    cfg, pc, pf, packed_c, packed_f, rays, opt, tgt = _full_setup(gpu)
    n = rays.shape[0]
    full = gpu.render(pc, pf, packed_c, packed_f, rays, opt, None, seed=5, training=True)
    _, gc, gf = gpu.mse_loss(full["rgb_coarse"], full["rgb_fine"], tgt)
    full = gpu.render(pc, pf, packed_c, packed_f, rays, opt, None, seed=5, training=True, g_rgb=(gc, gf))
    h = n // 2
    p1 = gpu.render(pc, pf, packed_c, packed_f, rays[:h], opt, None, seed=5, ray_offset=0, training=True,
                    g_rgb=(gc[:h], gf[:h]))
    p2 = gpu.render(pc, pf, packed_c, packed_f, rays[h:], opt, None, seed=5, ray_offset=h, training=True,
                    g_rgb=(gc[h:], gf[h:]))
    for key in ("g_params_coarse", "g_params_fine"):
        s = p1[key] + p2[key]
        scale = float(np.abs(full[key]).max())
        assert scale > 0
        assert float(np.abs(full[key] - s).max()) <= 2e-4 * scale, key


def test_full_size_fern_config_ndc_chunk_invariance_and_oracle_rows(gpu):
    """BASELINE config 4 shape (fern: NDC rays with near 0 / far 1, 6 xyz frequencies -> Dx = 39, 64 + 64 samples,
    noise std 1.0, 4096 rays, the 8x128 skip-3 nets of the e2e_c golden): chunk-invariant and reproducible at full size,
    and the first 24 rays equal the oracle fed with the kernels' own random draws."""
    cfg = P.MLP_GEOMETRIES["fern8x128_skip3_L6"]
    pc, par_c, _, packed_c = P.mlp_setup(gpu, cfg, seed=21)
    pf, par_f, _, packed_f = P.mlp_setup(gpu, cfg, seed=22)
    n, H, W, focal = 4096, 378, 504, 407.5
    g = torch.Generator().manual_seed(8)
    ro = torch.tensor([0.0, 0.0, 0.3]).expand(n, 3) + 0.05 * torch.randn(n, 3, generator=g)
    rd = torch.randn(n, 3, generator=g) * 0.3
    rd[:, 2] = -1.0
    no, nd = O.ndc_rays(H, W, focal, 1.0, ro, rd)
    rays = O.pack_rays(no, nd, 0.0, 1.0, rd).numpy()          # viewdirs from the pre-NDC directions (train_utils.py:143-168)
    opt = dict(num_coarse=64, num_fine=64, perturb=True, lindisp=False, white_background=False, noise_std=1.0)
    a = gpu.render(pc, pf, packed_c, packed_f, rays, opt, None, seed=31, ray_offset=0)
    h1 = gpu.render(pc, pf, packed_c, packed_f, rays[:1000], opt, None, seed=31, ray_offset=0)
    h2 = gpu.render(pc, pf, packed_c, packed_f, rays[1000:], opt, None, seed=31, ray_offset=1000)
    for k in ("rgb_coarse", "rgb_fine", "acc_fine", "depth_fine"):
        assert np.array_equal(a[k], np.concatenate([h1[k], h2[k]]), equal_nan=True), k
    assert np.isfinite(a["rgb_fine"]).all()
    m = 24
    nc, nf = 64, 64
    rand = dict(t_rand=torch.from_numpy(gpu.rng_fill(0, 31, 0, 0, m * nc).reshape(m, nc)),
                noise_coarse=torch.from_numpy(gpu.rng_fill(1, 31, 1, 0, m * nc).reshape(m, nc)),
                u=torch.from_numpy(gpu.rng_fill(0, 31, 2, 0, m * nf).reshape(m, nf)),
                noise_fine=torch.from_numpy(gpu.rng_fill(1, 31, 3, 0, m * (nc + nf)).reshape(m, nc + nf)))
    want = O.render_rays(torch.from_numpy(rays[:m]), par_c, par_f, cfg, cfg, opt, rand)
    P.close(a["rgb_coarse"][:m], want["rgb_coarse"].numpy(), 1e-5, what="fern rgb_coarse")
    P.close(a["rgb_fine"][:m], want["rgb_fine"].numpy(), 2e-4, what="fern rgb_fine")


# ---- the Python drop-in API --------------------------------------------------------------------------------------------
def _inject(draws, dev):
    q = [torch.as_tensor(d).to(dev) for d in draws]
    return q


def test_python_api_run_one_iter_matches_reference_golden():
    import nerf_pytorch_amd as N
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda", 0)
    g = gold("e2e_b.npz")
    meta = ast.literal_eval(str(g["meta"]))
    cfg = meta["cfg_c"]
    mc, mf = N.FlexibleNeRFModel(**cfg), N.FlexibleNeRFModel(**cfg)
    mc.load_state_dict(O.init_params(cfg, seed=meta["seed"] * 2 + 1))
    mf.load_state_dict(O.init_params(cfg, seed=meta["seed"] * 2 + 2))
    mc, mf = mc.to(dev), mf.to(dev)
    opts = N.make_options(meta["nc"], meta["nf"], perturb=meta["perturb"], lindisp=meta["lindisp"],
                          white_background=meta["white"], radiance_field_noise_std=meta["noise"])
    ex = N.get_embedding_function(cfg["num_encoding_fn_xyz"], True, True)
    ed = N.get_embedding_function(cfg["num_encoding_fn_dir"], True, True)
    q = _inject([g["t_rand"], g["noise_coarse"], g["u"], g["noise_fine"]], dev)
    real = torch.rand, torch.randn
    torch.rand = lambda *a, **k: q.pop(0)
    torch.randn = lambda *a, **k: q.pop(0)
    try:
        out = N.run_one_iter_of_nerf(int(g["H"]), int(g["W"]), float(g["focal"]), mc, mf, torch.from_numpy(g["ro"]).to(dev),
                                     torch.from_numpy(g["rd"]).to(dev), opts, mode="train", encode_position_fn=ex,
                                     encode_direction_fn=ed)
    finally:
        torch.rand, torch.randn = real
    tgt = torch.from_numpy(g["target"]).to(dev)
    loss = N.img2mse(out[0], tgt) + N.img2mse(out[3], tgt)
    loss.backward()
    for i, k in enumerate(("rgb_coarse", "disp_coarse", "acc_coarse", "rgb_fine", "disp_fine", "acc_fine")):
        P.close(out[i].detach().cpu().numpy(), g[k], 1e-4, 1e-4, what="api " + k)
    assert abs(float(loss) - float(g["loss"])) < 1e-5
    for tag, m in (("gc_", mc), ("gf_", mf)):
        for k, p in m.named_parameters():
            ref = g[tag + k]
            scale = float(np.abs(ref).max()) + 1e-12
            P.close(p.grad.cpu().numpy(), ref, 5e-5 * scale + 1e-9, 5e-4, what="api grad " + tag + k)


def test_python_api_unfused_composition_and_model_autograd():
    """A user network_fn that is NOT a FlexibleNeRFModel takes the generic composition path; FlexibleNeRFModel.forward
    with autograd (the unit API) matches the oracle."""
    import nerf_pytorch_amd as N
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda", 0)
    cfg = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    m = N.FlexibleNeRFModel(**cfg)
    par = O.init_params(cfg, seed=9)
    m.load_state_dict(par)
    m = m.to(dev)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(300, 90, generator=g)
    go = torch.randn(300, 4, generator=g)
    y = m(x.to(dev))
    (y * go.to(dev)).sum().backward()
    p = {k: v.clone().requires_grad_(True) for k, v in par.items()}
    yw = O.mlp_forward(p, x, cfg)
    (yw * go).sum().backward()
    P.close(y.detach().cpu().numpy(), yw.detach().numpy(), 2e-5, 2e-5, what="model forward")
    for k, v in m.named_parameters():
        ref = p[k].grad.numpy()
        scale = float(np.abs(ref).max()) + 1e-12
        P.close(v.grad.cpu().numpy(), ref, 2e-5 * scale + 1e-7, 2e-4, what="model grad " + k)
    # generic path: wrap the model in a plain callable so that the fused path is not taken
    opts = N.make_options(16, 16, perturb=False, radiance_field_noise_std=0.0)
    ex, ed = N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)
    ro = torch.tensor([0.0, 0.0, 4.0]).expand(10, 3).contiguous()
    rd = torch.randn(10, 3, generator=g) * 0.3
    rd[:, 2] = -1.0
    wrapped = lambda t: m(t)  # noqa: E731
    with torch.no_grad():
        a = N.run_one_iter_of_nerf(10, 10, 10.0, wrapped, wrapped, ro.to(dev), rd.to(dev), opts, encode_position_fn=ex,
                                   encode_direction_fn=ed)
        b = N.run_one_iter_of_nerf(10, 10, 10.0, m, m, ro.to(dev), rd.to(dev), opts, encode_position_fn=ex,
                                   encode_direction_fn=ed)
    for u, v in zip(a, b):
        P.close(u.cpu().numpy(), v.cpu().numpy(), 2e-5, 2e-5, what="generic vs fused")
    # gradients w.r.t. the encoded inputs (autograd gives them for nerf/models.py:233-256): parameters frozen or not
    for freeze in (False, True):
        m.zero_grad()
        for q in m.parameters():
            q.requires_grad_(not freeze)
        xin = x.to(dev).requires_grad_(True)
        (m(xin) * go.to(dev)).sum().backward()
        xr = x.clone().requires_grad_(True)
        (O.mlp_forward({k: v.detach() for k, v in p.items()}, xr, cfg) * go).sum().backward()
        ref = xr.grad.numpy()
        P.close(xin.grad.cpu().numpy(), ref, 2e-5 * float(np.abs(ref).max()) + 1e-7, 2e-4, what="input grad")
        assert all((q.grad is None or not freeze) for q in m.parameters())


def test_python_api_unused_outputs_and_other_float_dtypes():
    """ A loss on the fine colour map alone must not run the coarse net's backward: cotangents of untouched
    outputs arrive as None (set_materialize_grads(False)), the coarse net's gradients come back as exact zeros and the
    fine net's equal those of the two-term loss.  cumprod_exclusive accepts any floating dtype like the reference
    (nerf/nerf_helpers.py:43-64) and differentiates through the cast."""
    import nerf_pytorch_amd as N
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda", 0)
    cfg = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    mc, mf = N.FlexibleNeRFModel(**cfg), N.FlexibleNeRFModel(**cfg)
    mc.load_state_dict(O.init_params(cfg, seed=5))
    mf.load_state_dict(O.init_params(cfg, seed=6))
    mc, mf = mc.to(dev), mf.to(dev)
    g = torch.Generator().manual_seed(12)
    n = 64
    ro = torch.tensor([0.0, 0.0, 4.0]).expand(n, 3).contiguous().to(dev)
    rd = torch.randn(n, 3, generator=g) * 0.3
    rd[:, 2] = -1.0
    rd = rd.to(dev)
    tgt = torch.rand(n, 3, generator=g).to(dev)
    opts = N.make_options(32, 32, perturb=False, radiance_field_noise_std=0.0)
    ex, ed = N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)

    def grads(loss_fn):
        mc.zero_grad()
        mf.zero_grad()
        out = N.run_one_iter_of_nerf(8, 8, 8.0, mc, mf, ro, rd, opts, encode_position_fn=ex, encode_direction_fn=ed)
        loss_fn(out).backward()
        return [p.grad.clone() for p in mc.parameters()], [p.grad.clone() for p in mf.parameters()]

    gc_both, gf_both = grads(lambda o: N.img2mse(o[0], tgt) + N.img2mse(o[3], tgt))
    gc_fine, gf_fine = grads(lambda o: N.img2mse(o[3], tgt))
    assert all(float(t.abs().max()) == 0.0 for t in gc_fine)
    assert any(float(t.abs().max()) > 0.0 for t in gc_both)
    for a, b in zip(gf_fine, gf_both):
        assert torch.equal(a, b)
    # a loss on the accumulation map only (no colour cotangent at all)
    gc_acc, gf_acc = grads(lambda o: o[5].sum())
    assert all(float(t.abs().max()) == 0.0 for t in gc_acc) and any(float(t.abs().max()) > 0.0 for t in gf_acc)

    x = (torch.rand(5, 40, generator=g) * 0.2 + 0.9)
    for dt, tol in ((torch.float64, 2e-7), (torch.float16, 2e-3), (torch.bfloat16, 2e-2)):
        xd = x.to(dev).to(dt).requires_grad_(True)
        y = N.cumprod_exclusive(xd)
        assert y.dtype == dt
        y.sum().backward()
        xr = xd.detach().cpu().double().requires_grad_(True)
        yr = O.cumprod_exclusive(xr)
        yr.sum().backward()
        assert xd.grad.dtype == dt
        P.close(y.detach().double().cpu().numpy(), yr.detach().numpy(), 0, tol, what="cumprod %s" % dt)
        P.close(xd.grad.double().cpu().numpy(), xr.grad.numpy(), 0, 5 * tol, what="cumprod grad %s" % dt)


def test_gradients_wrt_rays_through_the_fused_render_vs_oracle_autograd():
    """nerf/train_utils.py:67,107 and nerf/volume_rendering_utils.py:24: under autograd the reference differentiates
    pts = ro + rd * z, the viewdirs and dists * ||rd|| w.r.t. the ray batch (pose optimisation).  The fused render's
    d(loss)/d(ray_origins, ray_directions) through run_one_iter_of_nerf against the oracle's autograd on 256 rays, for a
    loss on colour, accumulation and depth-derived disparity of both passes."""
    import nerf_pytorch_amd as N
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda", 0)
    for cfg, seeds in ((model_cfg(4, 128, 4, 10, 4), (5, 6)), (model_cfg(8, 256, 4, 6, 2), (7, 8))):
        kw = {k: cfg[k] for k in ("num_layers", "hidden_size", "skip_connect_every", "num_encoding_fn_xyz", "num_encoding_fn_dir")}
        mc, mf = N.FlexibleNeRFModel(**kw), N.FlexibleNeRFModel(**kw)
        par_c, par_f = O.init_params(cfg, seed=seeds[0]), O.init_params(cfg, seed=seeds[1])
        mc.load_state_dict(par_c)
        mf.load_state_dict(par_f)
        mc, mf = mc.to(dev), mf.to(dev)
        g = torch.Generator().manual_seed(21)
        n, nc, nf = 256, 32, 32
        ro = (torch.tensor([0.1, -0.2, 4.0]).expand(n, 3) + 0.05 * torch.randn(n, 3, generator=g)).contiguous()
        rd = torch.randn(n, 3, generator=g) * 0.3
        rd[:, 2] = -1.0
        tgt = torch.rand(n, 3, generator=g)
        opts = N.make_options(nc, nf, perturb=False, radiance_field_noise_std=0.0)
        ex = N.get_embedding_function(cfg["num_encoding_fn_xyz"], True, True)
        ed = N.get_embedding_function(cfg["num_encoding_fn_dir"], True, True)

        def loss_of(o):
            rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f = o
            return ((rgb_f - tgt.to(rgb_f.device)) ** 2).mean() + ((rgb_c - tgt.to(rgb_f.device)) ** 2).mean() \
                + 0.3 * (acc_f ** 2).mean() + 0.1 * torch.nan_to_num(disp_f).mean() + 0.2 * (acc_c ** 2).mean()

        ro_g, rd_g = ro.to(dev).requires_grad_(True), rd.to(dev).requires_grad_(True)
        out = N.run_one_iter_of_nerf(16, 16, 16.0, mc, mf, ro_g, rd_g, opts, encode_position_fn=ex, encode_direction_fn=ed)
        loss_of(out).backward()
        ro_r, rd_r = ro.clone().requires_grad_(True), rd.clone().requires_grad_(True)
        rays = O.pack_rays(ro_r, rd_r, 2.0, 6.0, rd_r)
        want = O.render_rays(rays, par_c, par_f, cfg, cfg, dict(num_coarse=nc, num_fine=nf, perturb=False, lindisp=False,
                                                                 white_background=False, noise_std=0.0))
        loss_of((want["rgb_coarse"], want["disp_coarse"], want["acc_coarse"], want["rgb_fine"], want["disp_fine"],
                 want["acc_fine"])).backward()
        # the yardstick: the oracle's autograd in fp64 (see case_ray_grad: ray gradients are ill-conditioned; the oracle's own
        # fp32 run is 1e-2 of max|g| away from it on a few per cent of the rays)
        ro_d, rd_d = ro.double().requires_grad_(True), rd.double().requires_grad_(True)
        w64 = O.render_rays(O.pack_rays(ro_d, rd_d, 2.0, 6.0, rd_d), {k: v.double() for k, v in par_c.items()},
                            {k: v.double() for k, v in par_f.items()}, cfg, cfg,
                            dict(num_coarse=nc, num_fine=nf, perturb=False, lindisp=False, white_background=False, noise_std=0.0))
        tgt64 = tgt.double()
        (((w64["rgb_fine"] - tgt64) ** 2).mean() + ((w64["rgb_coarse"] - tgt64) ** 2).mean() + 0.3 * (w64["acc_fine"] ** 2).mean()
         + 0.1 * torch.nan_to_num(w64["disp_fine"]).mean() + 0.2 * (w64["acc_coarse"] ** 2).mean()).backward()
        for name, got, ref, r64 in (("ray_origins", ro_g.grad, ro_r.grad, ro_d.grad), ("ray_directions", rd_g.grad, rd_r.grad, rd_d.grad)):
            ref, r64 = ref.numpy(), r64.numpy()
            scale = float(np.abs(r64).max())
            assert scale > 0
            e_hip = np.abs(got.cpu().numpy() - ref).max(axis=1) / scale
            e_yard = np.abs(ref - r64).max(axis=1) / scale
            what = "d loss / d %s (%dx%d): %s" % (name, cfg["num_layers"], cfg["hidden_size"],
                                                 dict(hip_median=float(np.median(e_hip)), yard_median=float(np.median(e_yard)),
                                                      hip_over=int((e_hip > 2e-3).sum()), yard_over=int((e_yard > 2e-3).sum())))
            assert np.median(e_hip) <= 3.0 * np.median(e_yard) + 2e-6, what
            assert (e_hip > 2e-3).sum() <= 2 * (e_yard > 2e-3).sum() + 3, what
        # the parameters got their gradients in the same backward
        assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in mf.parameters())
    # LLFF branch (no_ndc: False): the gradient flows through ndc_rays too (train_utils.py:156-160, nerf_helpers.py:170-197)
    Hn, Wn, fn = 378, 504, 407.5
    opts_ndc = N.make_options(nc, nf, perturb=False, radiance_field_noise_std=0.0, no_ndc=False, near=0.0, far=1.0)
    g = torch.Generator().manual_seed(22)
    ro = (torch.tensor([0.1, -0.2, 0.3]).expand(n, 3) + 0.1 * torch.randn(n, 3, generator=g)).contiguous()
    rd = torch.randn(n, 3, generator=g) * 0.3
    rd[:, 2] = -1.0
    ro_g, rd_g = ro.to(dev).requires_grad_(True), rd.to(dev).requires_grad_(True)
    out = N.run_one_iter_of_nerf(Hn, Wn, fn, mc, mf, ro_g, rd_g, opts_ndc, encode_position_fn=ex, encode_direction_fn=ed)
    loss_of(out).backward()
    ropt = dict(num_coarse=nc, num_fine=nf, perturb=False, lindisp=False, white_background=False, noise_std=0.0)
    grads = {}
    for dt in (torch.float32, torch.float64):
        o_r, d_r = ro.to(dt).clone().requires_grad_(True), rd.to(dt).clone().requires_grad_(True)
        no, nd = O.ndc_rays(Hn, Wn, fn, 1.0, o_r, d_r)
        want = O.render_rays(O.pack_rays(no, nd, 0.0, 1.0, d_r), {k: v.to(dt) for k, v in par_c.items()},
                             {k: v.to(dt) for k, v in par_f.items()}, cfg, cfg, ropt)
        t = tgt.to(dt)
        (((want["rgb_fine"] - t) ** 2).mean() + ((want["rgb_coarse"] - t) ** 2).mean() + 0.3 * (want["acc_fine"] ** 2).mean()
         + 0.1 * torch.nan_to_num(want["disp_fine"]).mean() + 0.2 * (want["acc_coarse"] ** 2).mean()).backward()
        grads[dt] = (o_r.grad.double().numpy(), d_r.grad.double().numpy())
    for name, got, ref, r64 in (("ray_origins", ro_g.grad, grads[torch.float32][0], grads[torch.float64][0]),
                                ("ray_directions", rd_g.grad, grads[torch.float32][1], grads[torch.float64][1])):
        scale = float(np.abs(r64).max())
        assert scale > 0 and got is not None
        e_hip = np.abs(got.cpu().double().numpy() - ref).max(axis=1) / scale
        e_yard = np.abs(ref - r64).max(axis=1) / scale
        what = "ndc d loss / d %s: %s" % (name, dict(hip_median=float(np.median(e_hip)), yard_median=float(np.median(e_yard)),
                                                   hip_over=int((e_hip > 2e-3).sum()), yard_over=int((e_yard > 2e-3).sum())))
        assert np.median(e_hip) <= 3.0 * np.median(e_yard) + 2e-6, what
        assert (e_hip > 2e-3).sum() <= 2 * (e_yard > 2e-3).sum() + 3, what


def test_pretrained_lego_checkpoint_renders_like_the_reference():
    """Reference-format state_dict (pretrained/lego-lowres, 4x128 nets) loads unchanged and the 64+64 deterministic
    render of pose_spherical(30,-30,4) matches the reference's image rows (trained nets: SURVEY 0.11 noise floor)."""
    import nerf_pytorch_amd as N
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda", 0)
    w, r = gold("lego_lowres_weights.npz"), gold("lego_lowres_render.npz")
    cfg = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    mc, mf = N.FlexibleNeRFModel(**cfg), N.FlexibleNeRFModel(**cfg)
    mc.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("c_")})
    mf.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("f_")})
    mc, mf = mc.to(dev), mf.to(dev)
    H, W, focal = int(r["H"]), int(r["W"]), float(r["focal"])
    opts = N.make_options(64, 64, perturb=False, white_background=True, radiance_field_noise_std=0.0)
    ex, ed = N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)
    ro, rd = N.get_ray_bundle(H, W, focal, torch.from_numpy(r["pose"])[:3, :4].to(dev))
    with torch.no_grad():
        out = N.run_one_iter_of_nerf(H, W, focal, mc, mf, ro, rd, opts, mode="validation", encode_position_fn=ex,
                                     encode_direction_fn=ed)
    rows = torch.from_numpy(r["rows"]).to(dev)
    rgb = out[3][rows].cpu().numpy()
    acc = out[5][rows].cpu().numpy()
    err = np.abs(rgb - r["rgb_fine"])
    # trained nets: the inverse CDF is ill-conditioned on flat plateaus; the reference itself moves by up to 6e-4
    # between fp32 and fp64.  Require the bulk within 1e-4 and the tail within 2e-3.
    assert float(np.quantile(err, 0.999)) < 2e-4, float(np.quantile(err, 0.999))
    assert float(err.max()) < 2e-3, float(err.max())
    assert float(np.abs(acc - r["acc_fine"]).max()) < 2e-3
    full_mean = float(out[3].mean())
    assert abs(full_mean - float(r["rgb_fine_mean"])) < 1e-4


def test_validation_mode_image_shapes_and_coarse_only():
    """mode="validation" reshapes to the image (train_utils.py:187-200); num_fine == 0 returns None for the fine
    outputs (train_utils.py:92-95,127); chunking over rays is transparent (A.9)."""
    import nerf_pytorch_amd as N
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda", 0)
    cfg = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    par = O.init_params(cfg, seed=3)
    m = N.FlexibleNeRFModel(**cfg)
    m.load_state_dict(par)
    m = m.to(dev)
    H, W, focal = 12, 20, 15.0
    pose = torch.eye(4)
    pose[2, 3] = 4.0
    ex, ed = N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)
    ro, rd = N.get_ray_bundle(H, W, focal, pose.to(dev))
    opts = N.make_options(32, 0, perturb=False, radiance_field_noise_std=0.0, chunksize=64)
    with torch.no_grad():
        out = N.run_one_iter_of_nerf(H, W, focal, m, None, ro, rd, opts, mode="validation", encode_position_fn=ex,
                                     encode_direction_fn=ed)
    assert len(out) == 6 and out[3] is None and out[4] is None and out[5] is None
    assert tuple(out[0].shape) == (H, W, 3) and tuple(out[1].shape) == (H, W) and tuple(out[2].shape) == (H, W)
    oro, ord_ = O.get_ray_bundle(H, W, focal, pose)
    rays = O.pack_rays(oro, ord_, 2.0, 6.0, ord_)
    want = O.render_rays(rays, par, None, cfg, None, dict(num_coarse=32, num_fine=0, perturb=False, noise_std=0.0))
    P.close(out[0].cpu().numpy().reshape(-1, 3), want["rgb_coarse"].numpy(), 1e-5, what="coarse-only rgb")
    P.close(out[2].cpu().numpy().reshape(-1), want["acc_coarse"].numpy(), 1e-5, what="coarse-only acc")
    opts2 = N.make_options(32, 0, perturb=False, radiance_field_noise_std=0.0, chunksize=1 << 17)
    with torch.no_grad():
        out2 = N.run_one_iter_of_nerf(H, W, focal, m, None, ro, rd, opts2, mode="validation", encode_position_fn=ex,
                                      encode_direction_fn=ed)
    assert torch.equal(out[0], out2[0]) and torch.equal(out[2], out2[2])


def test_edge_cases(gpu):
    P.case_edges(gpu)


def test_select_rays(gpu):
    P.case_select(gpu)


def test_select_uniformity(gpu):
    P.case_select_uniformity(gpu)


def test_image_output(gpu):
    P.case_image_output(gpu)


def test_python_api_select_step_resume_and_writer(tmp_path):
    """The rows next to the path through their Python surface: select_training_rays == the reference's gathers
    (golden), TrainEngine.step_on_image trains, a checkpoint written in the reference's format resumes bit-exactly,
    and ImageWriter's PNGs hold the reference's 8-bit casts."""
    import zlib
    import nerf_pytorch_amd as N
    from nerf_pytorch_amd import io_utils as IO
    from nerf_pytorch_amd.engine import TrainEngine
    from nerf_pytorch_amd.eval_utils import ImageWriter, cast_to_disparity_image, cast_to_image
    from nerf_pytorch_amd.train_utils import select_cached_training_rays, select_training_rays
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda", 0)
    g = gold("dataio.npz")
    H, W, focal = 20, 16, float(g["sel_b_hwfc"][2])
    pose, img, inds = torch.from_numpy(g["sel_b_pose"]).to(dev), torch.from_numpy(g["sel_b_img"]).to(dev), g["sel_b_inds"]
    opts = N.make_options(16, 16)
    rays, tgt, used = select_training_rays(H, W, focal, pose, img, len(inds), opts, select_inds=inds)
    want = O.pack_rays(torch.from_numpy(g["sel_b_ro"]), torch.from_numpy(g["sel_b_rd"]), 2.0, 6.0, torch.from_numpy(g["sel_b_rd"]))
    P.close(rays.cpu().numpy(), want.numpy(), 1e-6, what="select_training_rays")
    assert np.array_equal(tgt.cpu().numpy(), g["sel_b_target"]) and np.array_equal(used.cpu().numpy(), inds)
    ro, rd = N.get_ray_bundle(H, W, focal, pose[:3, :4])
    cache = {"height": H, "width": W, "focal_length": focal, "ray_bundle": torch.stack([ro, rd], 0), "target": img}
    rays_c, tgt_c, _ = select_cached_training_rays(cache, 32, opts, seed=5, step=2)
    rays_i, tgt_i, used_i = select_training_rays(H, W, focal, pose, img, 32, opts, seed=5, step=2)
    # cached rows are row-major (k = row*W + col) while the image branch reads k as (k % H, k // H): same draw, the
    # rays differ but each is the ray of its own target pixel
    flat = (ro.reshape(-1, 3), img.reshape(-1, 3))
    assert torch.equal(rays_c[:, :3], flat[0][used_i]) and torch.equal(tgt_c, flat[1][used_i])
    assert torch.equal(tgt_i, img[used_i % H, used_i // H])

    cfg = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)

    def make():
        mc, mf = N.FlexibleNeRFModel(**cfg), N.FlexibleNeRFModel(**cfg)
        mc.load_state_dict(O.init_params(cfg, seed=1))
        mf.load_state_dict(O.init_params(cfg, seed=2))
        mc, mf = mc.to(dev), mf.to(dev)
        return mc, mf, TrainEngine(mc, mf, 16, 16, perturb=True, noise_std=0.2, lr=5e-3, seed=9, world_size=1, rank=0)

    mc, mf, eng = make()
    losses = [float(eng.step_on_image(img, pose, H, W, focal, opts, 64)[2]) for _ in range(6)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    # uninterrupted run of 4 more steps vs save -> fresh engine -> load -> 4 steps
    path = str(tmp_path / "checkpoint00005.ckpt")
    IO.save_checkpoint(path, 5, mc, mf, IO.engine_optimizer_state_dict(eng), eng.loss[2].clone(), 0.0)
    tail = [float(eng.step_on_image(img, pose, H, W, focal, opts, 64)[2]) for _ in range(4)]
    mc2, mf2, eng2 = make()
    ck = IO.load_checkpoint(path, mc2, mf2, engine=eng2)
    assert ck["iter"] == 5 and eng2.step_count == 6
    tail2 = [float(eng2.step_on_image(img, pose, H, W, focal, opts, 64)[2]) for _ in range(4)]
    assert tail == tail2, (tail, tail2)
    assert torch.equal(mc.flat_params, mc2.flat_params) and torch.equal(mf.flat_params, mf2.flat_params)
    # a torch.optim.Adam built the reference's way accepts the saved optimizer state (train_nerf.py:138-143,161)
    opt = torch.optim.Adam(list(mc2.parameters()) + list(mf2.parameters()), lr=5e-3)
    opt.load_state_dict(torch.load(path, weights_only=False)["optimizer_state_dict"])

    rgb, disp = torch.from_numpy(g["img_in"]).to(dev), torch.from_numpy(g["disp0_in"]).to(dev)
    assert np.array_equal(cast_to_image(rgb, "blender"), g["img_out"])
    assert np.array_equal(cast_to_disparity_image(disp), g["disp0_out"])
    wr = ImageWriter(workers=2)
    wr.submit(str(tmp_path / "out" / "0000.png"), rgb)
    wr.submit(str(tmp_path / "out" / "disparity" / "0000.png"), disp, disparity=True)
    paths = wr.close()
    for pth, want8 in zip(paths, (g["img_out"], g["disp0_out"])):
        data = open(pth, "rb").read()
        n = int.from_bytes(data[33:37], "big")
        raw = np.frombuffer(zlib.decompress(data[41:41 + n]), np.uint8).reshape(want8.shape[0], -1)
        assert np.array_equal(raw[:, 1:].reshape(want8.shape), want8)


def test_e2e_northstar_reference_golden(gpu):
    P.case_e2e_northstar_golden(gpu)
