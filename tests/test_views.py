"""CPU suite: the multi-view ray batch (csrc/dataio.hip: nerfhip_select_rays_views, nerfhip_select_rays_views_bwd) on the wave
emulator -- every row and every per-view gradient against the single-view entry points on the bits, the gradients also against fp64
autograd under the bound of tests/pose_vjp.py.  The cases live in tests/views_cases.py (shared with tests/test_gpu_views.py)."""
import pytest

import views_cases as VC


@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("channels", [3, 4, None])
def test_selection_rows_equal_the_single_view_rows(emu, ndc, view, channels):
    VC.case_selection(emu, ndc, view, channels, "4x4")


def test_selection_reads_a_strided_pose_table(emu):
    VC.case_selection(emu, True, True, 3, "embedded")


@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("channels", [3, 4, None])
def test_selection_of_one_view_is_select_rays(emu, ndc, view, channels):
    VC.case_single_view_is_select_rays(emu, ndc, view, channels)


def test_single_view_entry_points_read_a_row_stride_other_than_4(emu):
    VC.case_single_view_row_stride(emu)


@pytest.mark.parametrize("view", [False, True])
def test_cached_selection_rows_equal_the_select_rays_rows(emu, view):
    VC.case_cached_rows_are_select_rays_rows(emu, view)


def test_selection_honours_explicit_indices_and_rank_slices_are_disjoint(emu):
    VC.case_explicit_indices_and_rank_slices(emu)


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("two", [False, True])
def test_views_vjp_equals_the_single_view_vjp_per_view(emu, which, ndc, view, two):
    VC.case_vjp(emu, which, ndc, view, two)


@pytest.mark.parametrize("n", [1, 257, 256 * 64 + 1])
def test_single_view_vjp_sum_at_its_edges(emu, n):
    VC.case_single_view_vjp_sum_edges(emu, n)


def test_views_vjp_of_no_rays_is_zero(emu):
    VC.case_vjp_no_rays(emu)


def test_views_entry_points_reject_bad_arguments(emu):
    VC.case_refusals(emu)
