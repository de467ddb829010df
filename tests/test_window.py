"""CPU suite: the coarse-to-fine encoding window (csrc/plan.cpp: nerfhip_plan_window_index; csrc/elementwise.hip: nerfhip_window_params /
nerfhip_window_grads) on the wave emulator -- the cases of tests/window_cases.py (shared with tests/test_gpu_window.py) -- and the
host side of the Python surface (the band weights the model hands to the kernels, the engine's schedule) without a GPU."""
import numpy as np
import pytest

import parity_cases as PC
import window_cases as WC


@pytest.mark.parametrize("name", list(WC.GEOMETRIES))
def test_code_table_is_the_tensor_table_restated(emu, name):
    WC.case_code_table(emu, name)


def test_kernels_are_numpy_fp32_multiplies_on_the_bits(emu):
    WC.case_kernels_bit_exact(emu)


def test_entry_points_reject_bad_arguments(emu):
    WC.case_refusals(emu)


def test_open_window_is_no_window_on_the_bits(emu):
    WC.case_open_window_is_no_window(emu)


def test_integer_alpha_is_zeroed_columns_on_the_bits(emu):
    WC.case_integer_alpha_is_zeroed_columns(emu)


@pytest.mark.parametrize("name,precision", [("fern4x64", 0), ("skip8x128", 0), ("fern4x64", PC.F16X3)])
def test_windowed_forward_matches_the_fp64_wrapper(emu, name, precision):
    WC.case_forward_fractional(emu, name, precision)


@pytest.mark.parametrize("name", ["fern4x64", "skip8x128"])
def test_windowed_backward_matches_fp64_autograd_of_the_wrapper(emu, name):
    WC.case_backward_fractional(emu, name)


def test_windowed_fused_render_matches_the_fp64_oracle_render(emu):
    WC.case_render(emu)


def test_model_and_engine_surface_without_a_gpu():
    """The weights the model passes by value are the definition's, bit for bit; None clears; the schedule is plain arithmetic."""
    import inspect
    import nerf_pytorch_amd as N
    import nerf_pytorch_amd._lib as L
    from nerf_pytorch_amd.nerf_helpers import encoding_window_weights
    assert {"nerfhip_plan_window_index", "nerfhip_window_params", "nerfhip_window_grads"} <= set(L.EXPORTED_SYMBOLS)
    cfg = WC.GEOMETRIES["fern4x64"]
    m = N.FlexibleNeRFModel(**cfg)
    keys = list(m.state_dict())
    assert m.encoding_window is None and m._window_w is None
    for ax, ad in ((2.6, 1.3), (-1.0, 0.0), (0.5, 4.0), (6.0, 5.0), (1.0, None), (None, 2.25)):
        assert m.set_encoding_window(ax, ad) is m and m.encoding_window == (ax, ad)
        want = WC.window_struct(cfg, 100.0 if ax is None else ax, 100.0 if ad is None else ad)
        assert np.array_equal(WC.bits(np.array(m._window_w.xyz[:])), WC.bits(np.array(want.xyz[:])))
        assert np.array_equal(WC.bits(np.array(m._window_w.dir[:])), WC.bits(np.array(want.dir[:])))
    assert np.array_equal(WC.bits(np.float32(encoding_window_weights(2.25, 4))), WC.bits(WC.band_weights(2.25, 4)))
    assert [float(v) for v in WC.band_weights(2.5, 4)] == [1.0, 1.0, 0.5, 0.0]
    m.set_encoding_window()
    assert m.encoding_window is None and m._window_w is None and list(m.state_dict()) == keys
    sig = inspect.signature(N.TrainEngine.__init__).parameters
    assert "window" in sig and "total_steps" in sig and sig["window"].default is None
