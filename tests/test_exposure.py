"""CPU suite: the per-view exposure (csrc/elementwise.hip: nerfhip_mse_loss_views_fwd_bwd; csrc/dataio.hip: nerfhip_exposure_bwd,
nerfhip_exposure_grad_tmp_bytes) on the wave emulator, and the fp64 reference of tests/exposure_cases.py (shared with
tests/test_gpu_exposure.py) against itself."""
import pytest

import exposure_cases as EC


# ---- the reference alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fine", [False, True])
def test_reference_equals_central_differences(fine):
    EC.case_reference_against_itself(fine)


def test_every_gradient_batch_is_a_hundred_bounds_away_from_zero():
    EC.case_batches_are_well_conditioned()


# ---- the kernels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", [1.0, 0.75])
@pytest.mark.parametrize("n,V,stride,fine", EC.GRID, ids=EC.GRID_IDS)
def test_loss_and_cotangents_against_fp64(emu, n, V, stride, fine, gs):
    EC.case_loss_fp64(emu, n, V, stride, fine, gs)


@pytest.mark.parametrize("gs", [1.0, 0.75])
@pytest.mark.parametrize("n,V,stride,fine", EC.GRID, ids=EC.GRID_IDS)
def test_table_gradient_against_fp64(emu, n, V, stride, fine, gs):
    EC.case_grad_fp64(emu, n, V, stride, fine, gs)


@pytest.mark.parametrize("n,V,stride,fine,kind", EC.BIG, ids=EC.BIG_IDS)
def test_table_gradient_against_fp64_over_many_views_and_in_one(emu, n, V, stride, fine, kind):
    EC.case_grad_fp64(emu, n, V, stride, fine, 1.0, kind)


@pytest.mark.parametrize("gs", [1.0, 0.75])
@pytest.mark.parametrize("n,V,stride,fine", EC.GRID, ids=EC.GRID_IDS)
def test_zero_table_gives_the_plain_loss_bits(emu, n, V, stride, fine, gs):
    EC.case_zero_table_bits(emu, n, V, stride, fine, gs)


def test_table_gradient_bits_do_not_depend_on_how_the_views_interleave(emu):
    EC.case_view_order_bits(emu)


@pytest.mark.parametrize("mask", EC.MASKS)
def test_masked_entries_get_exact_zeros_and_never_move(emu, mask):
    EC.case_mask(emu, mask)


def test_no_rays_and_indices_of_no_view(emu):
    EC.case_edges(emu)


def test_hundreds_of_indices_of_no_view_on_either_side(emu):
    EC.case_many_indices_of_no_view(emu)


def test_entry_points_reject_bad_arguments(emu):
    EC.case_refusals(emu)
