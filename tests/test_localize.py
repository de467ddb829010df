"""CPU suite: the frozen ray gradient (csrc/nh_raygrad.h: k_point_grad_pack, k_point_grad, k_ray_grad_sum; csrc/fused.hip:
nerfhip_render_grad_rays) on the wave emulator -- the cases of tests/localize_cases.py, shared with tests/test_gpu_localize.py, at
the geometries of that suite and sample counts the emulator walks in a second or two -- and the host side of the Python surface."""
import pytest

import localize_cases as LC
import parity_cases as PC

# (geometry, rays, coarse, fine, backward mode, precision, problem options): what each exercises is in tests/test_gpu_localize.py
CASES = [
    ("default4x128", 12, 8, 8, False, 0, {}),
    ("northstar8x256", 5, 8, 8, False, 0, dict(noise=0.2)),
    ("novw3x64_skip1", 10, 16, 16, False, 0, dict(white=True, noise=0.5)),
    ("wide2x320", 6, 8, 8, False, 0, {}),
    ("odd5x99_skip2", 6, 8, 8, False, 0, {}),
    ("L12_4x128", 8, 8, 8, False, 0, {}),
    ("L16_Ld6_8x256", 5, 8, 8, False, 0, dict(noise=0.2)),
    ("L16_Ld6_8x256", 11, 8, 16, True, 0, dict(noise=0.2)),
    ("llff4x64_skip3_L6", 12, 8, 8, "fused_stash", 0, {}),
    ("llff4x64_skip3_L6", 7, 24, 16, "fused_stash", 0, {}),
    ("default4x128", 12, 8, 8, False, PC.F16X3_TRAIN, {}),
    ("default4x128", 1, 8, 8, True, 0, {}),
]
IDS = ["%s-n%d-%d+%d-%s-p%d" % c[:6] for c in CASES]
# teacher-forced on the kernels' own depths: (..., all six cotangents?) -- tests/test_gpu_localize.py's table at ray counts the emulator
# walks in seconds (what each row exercises is written there)
TF_CASES = [
    ("default4x128", 12, 8, 8, False, 0, {}, True),
    ("default4x128", 12, 8, 8, False, PC.F16X3_TRAIN, {}, False),
    ("northstar8x256", 8, 8, 8, False, 0, dict(noise=0.2), True),
    ("novw3x64_skip1", 10, 16, 16, False, 0, dict(white=True, noise=0.5), False),
    ("noinput_linear", 10, 8, 8, False, 0, dict(noise=1.0), False),
    ("narrow3x40", 9, 24, 16, True, 0, {}, False),
    ("Ld5_4x128_skip2", 10, 8, 8, False, 0, {}, False),
    ("L11_novw3x64_skip1", 10, 8, 8, False, 0, dict(noise=0.5), False),
    ("L12_Ld10_2x512", 6, 8, 8, False, 0, dict(noise=0.5), False),
    ("wide3x512_skip2", 6, 8, 8, True, 0, dict(noise=0.5), False),
    ("L16_Ld6_8x256", 8, 8, 8, False, 0, dict(noise=0.2), False),
    ("L16_Ld6_8x256", 8, 8, 8, "recompute", 0, dict(noise=0.2), False),
    ("odd5x99_skip2", 8, 8, 8, False, 0, {}, False),
    ("wide2x320", 6, 8, 8, False, 0, {}, False),
    ("one_layer", 8, 8, 8, False, 0, dict(noise=0.5), False),
    ("llff4x64_skip3_L6", 7, 24, 16, "fused_stash", 0, {}, False),
    ("default4x128", 1, 8, 8, True, 0, {}, False),
]
TF_IDS = ["%s-n%d-%d+%d-%s-p%d" % c[:6] + ("-allcot" if c[7] else "") for c in TF_CASES]


@pytest.mark.parametrize("name,n,nc,nf,mode,precision,kw,allcot", TF_CASES, ids=TF_IDS)
def test_both_ray_gradient_chains_match_fp64_on_their_own_depths_ray_for_ray(emu, name, n, nc, nf, mode, precision, kw, allcot):
    LC.case_teacher_forced(emu, name, n, nc, nf, mode, precision, allcot, floor=LC.DECIDED_EMU, **kw)


@pytest.mark.parametrize("name,n,nc,nf,mode,precision,kw", CASES, ids=IDS)
def test_frozen_ray_gradient_matches_the_oracle(emu, name, n, nc, nf, mode, precision, kw):
    LC.case_vs_oracle(emu, name, n, nc, nf, mode, precision, **kw)


@pytest.mark.parametrize("name,n,nc,nf,mode,precision,kw", CASES, ids=IDS)
def test_frozen_ray_gradient_matches_the_trainable_path(emu, name, n, nc, nf, mode, precision, kw):
    LC.case_vs_trainable_path(emu, name, n, nc, nf, mode, precision, **kw)


def test_backward_modes_give_the_same_bits(emu):
    LC.case_modes_give_the_same_bits(emu)


def test_fused_modes_run_as_mode_2_and_give_the_same_bits(emu):
    LC.case_modes_give_the_same_bits(emu, "llff4x64_skip3_L6", n=9, nc=8, nf=8, modes=(False, "recompute", "fused", "fused_compact", "fused_stash"))


def test_streamed_weight_slices_give_the_same_bits_in_every_mode(emu):
    """L16_Ld6_8x256: two 112-slot xyz images of 114 KB and a 64-slot direction image -- 261 KB, beyond the 160 KB of LDS: every term is
    staged behind its barriers for every 128-row tile (6 x 24 = 144 fine rows: two tiles, the second one ragged)."""
    LC.case_modes_give_the_same_bits(emu, "L16_Ld6_8x256", n=6, nc=8, nf=16)


def test_parts_layouts_and_open_window_on_the_bits(emu):
    LC.case_parts_layouts_window(emu)


def test_entry_point_rejects_bad_arguments(emu):
    LC.case_refusals(emu)


def test_python_surface_without_a_gpu():
    import inspect
    import nerf_pytorch_amd as N
    import nerf_pytorch_amd._lib as L
    assert {"nerfhip_render_grad_rays", "nerfhip_render_grad_rays_tmp_bytes"} <= set(L.EXPORTED_SYMBOLS)
    sig = inspect.signature(N.TrainEngine.forward_backward).parameters
    assert sig["frozen"].default is False
    for name in ("localize_on_image", "localize_on_views"):
        assert callable(getattr(N.TrainEngine, name))
    m = N.FlexibleNeRFModel(**PC.MLP_GEOMETRIES["llff4x64_skip3_L6"])
    keys = list(m.state_dict())
    assert m.frozen is False and m.set_frozen(True) is m and m.frozen is True and list(m.state_dict()) == keys
    assert m.set_frozen(False).frozen is False
