"""CPU suite of the robust photometric loss: the cases of tests/robust_cases.py on the wave emulator -- the kernel against the definition
in torch at the wave and block edges with and without a trim, ties, the bit identities, NaN, the refusals, parameter gradients against
the oracle's autograd, every backward mode under a trim -- and what needs no library at all: the definition's closed-form cotangent and
the conditions the cases rely on.  The GPU suite (tests/test_gpu_robust.py) runs the same cases on the product library and the public
routes."""
import numpy as np
import pytest
import torch

import robust_cases as R


@pytest.mark.parametrize("kind,param", R.KERNEL_KINDS)
def test_kernel_against_the_definition(emu, kind, param):
    R.case_kernel(emu, kind, param)


def test_kernel_keeps_every_tie(emu):
    R.case_ties(emu)


def test_kernel_bit_identities(emu):
    R.case_bit_identities(emu)


def test_kernel_keeps_a_nan_ray_and_reports_it(emu):
    R.case_nan(emu)


def test_kernel_refusals(emu):
    R.case_refusals(emu)


def test_the_definition_has_the_closed_form_cotangent():
    """The definition alone: autograd of the restated loss equals the header's h k in fp64, for every kind."""
    n, gs = 200, 0.37
    for kind, param in R.KERNEL_KINDS:
        rgb, tgt = R.kernel_inputs(n, 4, 11 + kind, kind, param)
        _, g, _ = R.robust_reference(rgb, tgt, kind, param, gs, torch.float64)
        p = rgb.astype(np.float64)
        d = p - tgt[:, :3].astype(np.float64)
        h = {0: lambda: d, 1: lambda: 0.5 * np.sign(d), 2: lambda: np.where(np.abs(d) <= param, d, param * np.sign(d)),
             3: lambda: 0.5 * d / np.sqrt(d * d + param * param), 4: lambda: d / (p + param) ** 2}[kind]()
        want = h * 2.0 / (3 * n) * gs
        assert np.abs(g.numpy() - want).max() <= 1e-12 * np.abs(want).max(), kind
        assert (d == 0.0).any() and (kind != 2 or ((np.abs(d) > param).any() and (np.abs(d) <= param).any()))


def test_the_input_conditions_of_the_cases():
    """What the kernel cases rely on, from the reference alone: the Huber inputs populate both branches, and wherever 1 < kk < n the
    definition trims at least one ray and keeps at least one."""
    for kind, param in R.KERNEL_KINDS:
        seed = 1000 * kind
        for n in R.SHAPES_N:
            for stride in R.STRIDES:
                seed += 1
                rgb, tgt = R.kernel_inputs(n, stride, seed, kind, param)
                d = rgb.astype(np.float64) - tgt[:, :3].astype(np.float64)
                if kind == 2 and n >= 63:
                    assert 0.1 <= (np.abs(d) > param).mean() <= 0.9, (n, stride)
                e64 = R.robust_reference(rgb, tgt, kind, param, 1.0, torch.float64)[2]
                assert torch.isfinite(e64).all() and (e64 >= 0).all()
                for keep in R.keeps_of(n):
                    kk = R.keep_count(keep, n)
                    m, _ = R.trim_mask(e64, keep)
                    if 1 < kk < n:
                        assert 0 < int(m.sum()) < n, (kind, n, keep)
                    assert int(m.sum()) >= kk
    assert R.keep_count(0.999, 3073) == 3070 and R.keep_count(0.5, 1) == 1 and R.keep_count(1.0 / 63, 63) in (1, 2)


def test_corruption_is_a_fixed_draw_per_pixel_and_view():
    clean = torch.rand(3, 4096, 3, generator=torch.Generator().manual_seed(0)) * 0.5 + 0.25
    a, hit = R.corrupt(clean)
    b, hit2 = R.corrupt(clean)
    assert torch.equal(a, b) and torch.equal(hit, hit2)
    assert all(abs(float(hit[v].float().mean()) - R.CORRUPTION_RATE) < 0.03 for v in range(3)) and not torch.equal(hit[0], hit[1])
    assert torch.equal(a[~hit], clean[~hit]) and set(a[hit].unique().tolist()) == {0.0, 1.0}


def test_parameter_gradients_against_the_oracle(emu):
    R.case_param_grads(emu, "w64", "fp32")


def test_backward_modes_under_a_trim(emu):
    R.case_modes(emu, "w64", "fp32", (True, "recompute", "fused", "fused_compact", "fused_stash"))


def test_engine_keywords_parse_without_a_device():
    """TrainEngine's photometric= / trim= parser is host code: every form and every refusal, naming the keyword."""
    from nerf_pytorch_amd.engine import TrainEngine as E
    p = E._parse_robust
    assert p(None, None, True) is None and p("l2", 1.0, True) is None and p(None, (1.0, 1.0), True) is None
    assert p("l1", None, True) == ((1, 0.0, 1.0), (1, 0.0, 1.0))
    assert p(("huber", 0.1), 0.8, True) == ((2, 0.1, 0.8), (2, 0.1, 0.8))
    assert p((("charbonnier", 1e-3), "l1"), (0.5, None), True) == ((3, 1e-3, 0.5), (1, 0.0, 1.0))
    assert p(("l1", ("relative", 0.01)), None, True) == ((1, 0.0, 1.0), (4, 0.01, 1.0))
    assert p(None, 0.6, True) == ((0, 0.0, 0.6), (0, 0.0, 0.6))
    assert p(("huber", 0.1), (0.5, 0.7), False) == ((2, 0.1, 0.5), (0, 0.0, 1.0))
    for bad in ("tukey", ("tukey", 0.1), ("huber",), ("huber", 0.0), ("huber", -1.0), ("huber", float("nan")), ("huber", float("inf")),
                ("huber", "x"), ("l1", 0.1, 0.2), 3, ("huber", True), (("l1", 0.5), None)):
        with pytest.raises(ValueError, match="photometric"):
            p(bad, None, True)
    for bad in (0.0, -0.1, 1.5, float("nan"), "x", True, (0.5,), (0.5, 0.5, 0.5), (0.5, 2.0)):
        with pytest.raises(ValueError, match="trim"):
            p(None, bad, True)


def test_exported_symbols():
    import nerf_pytorch_amd._lib as L
    assert {"nerfhip_robust_loss_fwd_bwd", "nerfhip_robust_loss_tmp_bytes"} <= set(L.EXPORTED_SYMBOLS)
    assert len(L._PROTOS["nerfhip_robust_loss_fwd_bwd"][1]) == 15 and len(L._PROTOS["nerfhip_robust_loss_tmp_bytes"][1]) == 1
