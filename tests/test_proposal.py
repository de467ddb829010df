"""CPU suite of the interlevel proposal loss (mip-NeRF 360's L_prop): the cases of tests/proposal_cases.py on the wave emulator -- the
kernel against the definition in fp64 torch on the library's own weights at every chunk boundary, its contract, the coarse weight
cotangent through the fused backward against the oracle's autograd in every backward mode and in the culled step -- and the host side
of the new keywords that needs no device.  The GPU suite (tests/test_gpu_proposal.py) runs the same cases on the product library."""
import numpy as np
import pytest
import torch

import proposal_cases as PC


@pytest.mark.parametrize("kind", PC.KERNEL_KINDS)
def test_kernel_against_the_definition(emu, kind):
    PC.case_kernel(emu, kind)


def test_kernel_long_rays(emu):
    PC.case_kernel_long_rays(emu)


def test_kernel_refusals(emu):
    PC.case_kernel_refusals(emu)


def test_the_definition_is_the_overlap_enumeration():
    """The reference alone: the searchsorted form of lo, hi equals a brute-force enumeration of the coarse intervals that overlap each
    fine interval (open overlap; a fine interval that overlaps none takes the clamped index), refining, free and tied depths."""
    for kind, Sc, Sf in (("refining", 7, 19), ("free", 7, 3), ("tied_depths", 9, 14), ("last_beyond_far", 5, 8)):
        c = PC.kernel_inputs(kind, 6, Sc, Sf, 8, 3)
        zc, zf, far = c["z_c"], c["z_f"], c["rays"][:, 7:8]
        lo, hi = (t.numpy() for t in PC.proposal_ranges(torch.as_tensor(zc), torch.as_tensor(zf), torch.as_tensor(far)))
        ec = np.concatenate((zc, np.maximum(far, zc[:, -1:])), axis=1)
        ef = np.concatenate((zf, np.maximum(far, zf[:, -1:])), axis=1)
        for r in range(6):
            for i in range(Sf):
                over = [j for j in range(Sc) if ec[r, j] < ef[r, i + 1] and ec[r, j + 1] > ef[r, i]]
                if over:
                    assert (lo[r, i], hi[r, i]) == (over[0], over[-1]), (kind, r, i, over, lo[r, i], hi[r, i])
                else:
                    assert lo[r, i] == hi[r, i] and 0 <= lo[r, i] < Sc, (kind, r, i)
        assert (np.diff(lo, axis=1) >= 0).all() and (np.diff(hi, axis=1) >= 0).all()


@pytest.mark.parametrize("net,arith", [("w64", "fp32"), ("w40of64", "f16x3_train")])
def test_parameter_gradients_against_the_oracle(emu, net, arith):
    PC.case_param_grads(emu, net, arith, shapes=PC.S.RENDER_SHAPES[:1])


def test_backward_modes_with_the_proposal_cotangent(emu):
    PC.case_compacted(emu, "w64", "fp32", (True, "recompute", "fused", "fused_compact", "fused_stash"))


def test_culled_step_with_the_proposal_term(emu):
    PC.case_culled_step(emu, "w64", "fp32", 0)


def test_render_call_proposal_is_the_raw_call(emu):
    PC.case_render_call(emu)


def test_ray_gradient_with_the_proposal_term(emu):
    PC.case_rays_w(emu, "w64")


def test_exported_symbol_and_render_call():
    import nerf_pytorch_amd._lib as L
    from nerf_pytorch_amd.render_call import RenderCall
    assert "nerfhip_proposal_loss" in L.EXPORTED_SYMBOLS
    assert len(L._PROTOS["nerfhip_proposal_loss"][1]) == 20
    assert callable(RenderCall.proposal)
