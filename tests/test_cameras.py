"""CPU suite: the camera table (csrc/dataio.hip: nerfhip_pose_table_fwd / nerfhip_pose_table_bwd) on the wave emulator -- composed
poses and twist gradients against the fp64 matrix exponential under the counted bounds of tests/cameras_cases.py (shared with
tests/test_gpu_cameras.py), the `active` mask, the refusals, and the Python module's import without a GPU."""
import pytest

import cameras_cases as CC


@pytest.mark.parametrize("V", CC.VIEW_COUNTS)
def test_composed_poses_are_within_the_counted_bound(emu, V):
    CC.case_forward(emu, V)


def test_composed_poses_read_a_strided_base_table(emu):
    CC.case_forward(emu, 65, "embedded")


@pytest.mark.parametrize("V", CC.VIEW_COUNTS)
def test_twist_gradients_are_within_the_counted_bound(emu, V):
    CC.case_vjp(emu, V)


def test_composed_poses_of_twists_that_wrap_round(emu):
    CC.case_forward_wrapped(emu)


def test_twist_gradients_read_a_strided_base_table(emu):
    CC.case_vjp(emu, 65, "embedded")


def test_inactive_views_get_exact_zeros(emu):
    CC.case_active(emu)


def test_entry_points_reject_bad_arguments(emu):
    CC.case_refusals(emu)


def test_cameras_module_imports_without_a_gpu_and_is_exported():
    import nerf_pytorch_amd as N
    import nerf_pytorch_amd.cameras as cam
    import nerf_pytorch_amd._lib as L
    assert N.CameraTable is cam.CameraTable and N.se3_poses is cam.se3_poses
    assert {"nerfhip_pose_table_fwd", "nerfhip_pose_table_bwd"} <= set(L.EXPORTED_SYMBOLS)
    import inspect
    assert "cameras" in inspect.signature(N.TrainEngine.step_on_views).parameters
