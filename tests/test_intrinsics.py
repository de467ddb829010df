"""CPU suite: the device-resident intrinsics (csrc/dataio.hip: nerfhip_select_rays_views_intr / _intr_bwd; csrc/elementwise.hip:
nerfhip_ray_bundle_intr, nerfhip_intrinsics_fwd / _bwd) on the wave emulator -- the scalar entry points' bits where the intrinsics
restate the scalar camera, fp64 autograd under the derived bounds elsewhere.  The cases live in tests/intrinsics_cases.py (shared
with tests/test_gpu_intrinsics.py)."""
import pytest

import intrinsics_cases as IC


@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("layout", ["4x4", "embedded"])
def test_selection_with_the_scalar_camera_as_intrinsics_has_the_scalar_bits(emu, ndc, view, layout):
    IC.case_selection_bits(emu, ndc, view, layout)


def test_ray_bundle_from_intrinsics(emu):
    IC.case_bundle_bits(emu)


@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
def test_selection_rows_against_fp64(emu, ndc, view):
    IC.case_selection_fp64(emu, ndc, view)


@pytest.mark.parametrize("n", [1, 63, 256, 257, 700])
@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("two,stride", [(False, 11), (True, 16), (True, 11), (False, 16)])
def test_vjp_against_fp64(emu, n, ndc, view, two, stride):
    IC.case_vjp(emu, n, ndc, view, two, stride)


@pytest.mark.parametrize("n", [1, 63, 256, 257, 700])
@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
def test_vjp_pose_gradient_has_the_scalar_bits(emu, n, ndc, view):
    IC.case_vjp_poses_equal_the_scalar_form(emu, n, ndc, view)


def test_vjp_of_no_rays_an_empty_view_and_dropped_indices(emu):
    IC.case_vjp_edges(emu)


@pytest.mark.parametrize("tie", [False, True])
def test_parametrisation_forward(emu, tie):
    IC.case_param_fwd(emu, tie)


@pytest.mark.parametrize("tie", [False, True])
@pytest.mark.parametrize("mask", IC.MASKS, ids=["".join(map(str, m)) for m in IC.MASKS])
def test_parametrisation_pull_back_and_masks(emu, tie, mask):
    IC.case_param_bwd(emu, tie, mask)


def test_entry_points_reject_bad_arguments(emu):
    IC.case_refusals(emu)
