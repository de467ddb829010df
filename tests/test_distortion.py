"""CPU suite: the device-resident lens distortion (csrc/nh_rays.h: nh_undistort / nh_undistort_vjp; csrc/dataio.hip:
nerfhip_select_rays_views_dist / _dist_bwd; csrc/elementwise.hip: nerfhip_ray_bundle_dist) on the wave emulator, and the fp64
reference of tests/distortion_cases.py (shared with tests/test_gpu_distortion.py) against itself."""
import pytest

import distortion_cases as DC


# ---- the reference alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("kappa", ["barrel", "pincushion"])
def test_reference_equals_central_differences(ndc, view, kappa):
    DC.case_reference_against_itself(ndc, view, kappa)


def test_fp64_newton_is_converged_two_steps_before_the_kernel_stops():
    DC.case_iteration_count()


def test_every_tested_pixel_is_inside_the_domain():
    DC.case_domain()


# ---- the kernels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("kappa", ["barrel", "pincushion"])
def test_selection_rows_against_fp64(emu, ndc, view, kappa):
    DC.case_forward_fp64(emu, ndc, view, kappa)


def test_selection_rows_against_fp64_on_the_scalar_camera(emu):
    DC.case_forward_fp64(emu, True, True, "pincushion", with_intr=False)


def test_ray_bundle_under_distortion(emu):
    DC.case_bundle(emu)


@pytest.mark.parametrize("n", [1, 63, 256, 257, 700])
@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("two,stride", [(False, 11), (True, 16), (True, 11), (False, 16)])
def test_vjp_against_fp64(emu, n, ndc, view, two, stride):
    DC.case_vjp(emu, n, ndc, view, two, stride)


@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("layout", ["4x4", "embedded"])
def test_zero_distortion_selects_the_rows_of_the_call_without_it(emu, ndc, view, layout):
    DC.case_zero_selection_bits(emu, ndc, view, layout)


@pytest.mark.parametrize("n", [1, 63, 256, 257, 700])
@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
def test_zero_distortion_gives_the_existing_gradients_bits(emu, n, ndc, view):
    DC.case_zero_vjp_bits(emu, n, ndc, view)


@pytest.mark.parametrize("mask", DC.MASKS, ids=["".join(map(str, m)) for m in DC.MASKS])
def test_masked_coefficients_get_exact_zeros_and_never_move(emu, mask):
    DC.case_mask(emu, mask)


def test_vjp_of_no_rays_an_empty_view_and_dropped_indices(emu):
    DC.case_vjp_edges(emu)


def test_entry_points_reject_bad_arguments(emu):
    DC.case_refusals(emu)
