"""CPU suite of the occupancy grid in training: the cases of tests/occupancy_train_cases.py on the wave emulator (the culled training
forward against the recomputing step and against the hand-substituted dense arm, the density kernels against numpy, refusals), the
case generators' own promises, and the host side of OccupancyGrid / TrainEngine that needs no device."""
import numpy as np
import pytest

import occupancy_train_cases as OT


@pytest.mark.parametrize("net,arith", [("w64", "fp32"), ("w128", "fp32"), ("w40of64", "fp32"), ("novw128", "fp32"), ("w128", "f16x3_train"),
                                       ("w64", "f16x3_train")])
def test_all_ones_grid_is_the_recomputing_step(emu, net, arith):
    OT.case_all_ones(emu, net, arith, n=9)


@pytest.mark.parametrize("net,arith,outside", [("w128", "fp32", 0), ("w128", "fp32", 1), ("w64", "fp32", 0), ("w40of64", "f16x3_train", 1)])
def test_half_empty_grid_is_the_substituted_dense_arm(emu, net, arith, outside):
    OT.case_half_empty(emu, net, arith, outside)


@pytest.mark.parametrize("net,arith", [("w128", "fp32"), ("w64", "fp32")])
def test_all_zero_grid(emu, net, arith):
    OT.case_all_zero(emu, net, arith)


@pytest.mark.parametrize("res,ranges", [((1, 1, 32), ((0, 32),)), ((4, 6, 8), ((32, 96),)), ((8, 8, 8), ((0, 256), (256, 256)))])
def test_density_update_against_numpy(emu, res, ranges):
    OT.case_density_update(emu, "w128", "fp32", res, ranges)


def test_density_update_nan_raw_keeps_the_decayed_value(emu):
    OT.case_density_update(emu, "w64", "fp32", (1, 1, 32), ((0, 32),), nan_weights=True)


@pytest.mark.parametrize("res", [(1, 1, 32), (4, 6, 8), (64, 64, 64)])
def test_density_bits_against_numpy(emu, res):
    OT.case_density_bits(emu, res)


@pytest.mark.parametrize("res", [(1, 1, 32), (4, 6, 8), (64, 64, 64)])
def test_density_bits_reference_excludes_nothing(res):
    for below in (True, False):
        OT.bits_case(res, 31, below)   # (asserts the generator's promises itself)


def test_refusals(emu):
    OT.case_refusals(emu)


def test_update_slabs_cover_the_grid():
    """OccupancyGrid.update_slab: 32-aligned contiguous slabs; ceil(1 / fraction) consecutive steps cover every cell exactly once."""
    import nerf_pytorch_amd as N
    g = N.OccupancyGrid.__new__(N.OccupancyGrid)
    for res, fraction in (((4, 6, 8), 0.25), ((64, 64, 64), 0.25), ((1, 1, 32), 0.25), ((4, 6, 8), 0.3), ((8, 8, 8), 1.0), ((4, 6, 8), 0.01)):
        g.resolution = res
        n = int(-(-1.0 // fraction))
        seen = np.zeros(g.num_cells, int)
        for step in range(7 * n, 8 * n):
            first, count = g.update_slab(step, fraction)
            assert first % 32 == 0 and count % 32 == 0 and 0 <= first and first + count <= g.num_cells
            seen[first:first + count] += 1
        assert (seen == 1).all(), (res, fraction)
    with pytest.raises(ValueError):
        g.update_slab(0, 0.0)
