"""CPU suite: the pose VJP kernels (csrc/dataio.hip: nerfhip_ray_bundle_bwd, nerfhip_select_rays_bwd) on the wave emulator,
against fp64 torch autograd of the oracle's get_ray_bundle -> ndc_rays -> pack_rays, under the bound derived from the
kernel's summation order in tests/pose_vjp.py."""
import ctypes as C

import numpy as np
import pytest

import nerf_pytorch_amd._lib as L
import pose_vjp as P


def _pose(seed):
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3) * 0.2
    import torch
    R = P.rodrigues(torch.tensor(w, dtype=torch.float64)).numpy()
    c2w = np.zeros((4, 4), dtype=np.float32)
    c2w[:3, :3] = R
    c2w[:3, 3] = rng.normal(size=3) * 0.5 + np.array([0.0, 0.0, 3.0])
    c2w[3, 3] = 1.0
    return c2w


def _bundle_bwd(emu, H, W, focal, pixels, g_o, g_d):
    lib = emu.lib
    n = H * W if pixels is None else len(pixels)
    tb = lib.pose_grad_tmp_bytes(n)
    tmp = np.full(max(tb // 4, 1), np.nan, dtype=np.float32)
    out = np.full(12, np.nan, dtype=np.float32)
    pix = None if pixels is None else np.ascontiguousarray(pixels, dtype=np.int64)
    lib.ray_bundle_bwd(H, W, focal, emu.p(pix), n, emu.p(g_o), emu.p(g_d), tmp.ctypes.data, tb, out.ctypes.data, None)
    return out.reshape(3, 4), tb


def _cfg(H, W, focal, ndc, view):
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    return L.SelectCfg(height=H, width=W, focal=focal, near=2.0, far=6.0, use_viewdirs=int(view), ndc=int(ndc), ndc_near=1.0,
                       ndc_cw=f32(-1.0 / (W / (2.0 * focal))), ndc_ch=f32(-1.0 / (H / (2.0 * focal))), ndc_two_near=2.0,
                       ndc_neg_two_near=-2.0, channels=3, seed=0, step=0, first=0)


def _select_bwd(emu, cfg, c2w, inds, g, g2, stride):
    n = len(inds)
    tb = emu.lib.pose_grad_tmp_bytes(n)
    tmp = np.full(max(tb // 4, 1), np.nan, dtype=np.float32)
    out = np.full(12, np.nan, dtype=np.float32)
    c2w = np.ascontiguousarray(c2w, dtype=np.float32)
    emu.lib.select_rays_bwd(C.byref(cfg), c2w.ctypes.data, c2w.shape[1], np.ascontiguousarray(inds, dtype=np.int64).ctypes.data,
                            n, g.ctypes.data, emu.p(g2), stride, tmp.ctypes.data, tb, out.ctypes.data, None)
    return out.reshape(3, 4)


def _check(got, want, mag, n):
    b = P.bound(n, mag)
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(np.isfinite(got)), got
    assert np.all(err <= b), (err / np.maximum(b, 1e-300)).max()


@pytest.mark.parametrize("H,W,pixels", [(9, 13, None), (8, 8, None), (37, 23, "all-but-some"), (17, 11, 1), (40, 40, 300),
                                        (100, 100, 2100)])
def test_ray_bundle_bwd_matches_fp64_autograd(emu, H, W, pixels):
    rng = np.random.default_rng(H * 100 + W)
    focal = float(np.float32(1.3 * max(H, W)))
    c2w = _pose(H + W)
    if pixels is None:
        pix = None
        n = H * W
    elif pixels == "all-but-some":
        pix = rng.permutation(H * W)[:H * W - 7]
        n = len(pix)
    else:
        pix = rng.integers(0, H * W, size=pixels)
        n = pixels
    g_o = rng.normal(size=(n, 3)).astype(np.float32)
    g_d = rng.normal(size=(n, 3)).astype(np.float32)
    got, tb = _bundle_bwd(emu, H, W, focal, pix, g_o, g_d)
    assert tb == P.wgs(n) * 12 * 4
    want = P.oracle_bundle_vjp(H, W, focal, c2w, pix, g_o, g_d)
    _check(got, want, P.magnitude(H, W, focal, c2w, pix, False, g_o=g_o, g_d=g_d), n)
    # one cotangent absent (NULL = zero), as autograd hands over when only one output is used
    got_d, _ = _bundle_bwd(emu, H, W, focal, pix, None, g_d)
    want_d = P.oracle_bundle_vjp(H, W, focal, c2w, pix, None, g_d)
    _check(got_d, want_d, P.magnitude(H, W, focal, c2w, pix, False, g_d=g_d), n)
    assert np.all(got_d[:, 3] == 0.0)
    # bit-reproducible
    again, _ = _bundle_bwd(emu, H, W, focal, pix, g_o, g_d)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("n", [1, 333])
def test_select_rays_bwd_matches_fp64_autograd(emu, ndc, view, two, n):
    H, W = 27, 35
    focal = float(np.float32(31.7))
    rng = np.random.default_rng(7 + n + 2 * ndc + 4 * view + 8 * two)
    c2w = _pose(5)
    if ndc:  # an LLFF-style camera: in front of the scene, looking down -z, near plane at z = -1
        c2w[:3, 3] = np.array([0.1, -0.05, 0.2], dtype=np.float32)
    cfg = _cfg(H, W, focal, ndc, view)
    stride = 12 if view else 9          # (a row stride wider than the row: the padding columns are never read)
    inds = rng.permutation(H * W)[:n]
    g = rng.normal(size=(n, stride)).astype(np.float32)
    g2 = rng.normal(size=(n, stride)).astype(np.float32) if two else None
    got = _select_bwd(emu, cfg, c2w, inds, g, g2, stride)
    gsum = g.astype(np.float64) + (g2.astype(np.float64) if two else 0.0)
    gsum[:, 6:8] = rng.normal(size=(n, 2))   # near / far carry no gradient: whatever the cotangent there, it is ignored
    want = P.oracle_select_vjp(H, W, focal, c2w, inds, gsum, ndc, view)
    gmag = np.abs(g.astype(np.float64)) + (np.abs(g2.astype(np.float64)) if two else 0.0)
    _check(got, want, P.magnitude(H, W, focal, c2w, inds, True, g_rays=gmag, ndc=ndc, view=view), n)
    again = _select_bwd(emu, cfg, c2w, inds, g, g2, stride)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    if two:  # the two inputs are added row by row first: swapping them gives the same bits (IEEE addition commutes)
        swapped = _select_bwd(emu, cfg, c2w, inds, g2, g, stride)
        assert np.array_equal(got.view(np.uint32), swapped.view(np.uint32))


def test_select_rays_bwd_is_the_bundle_bwd_of_the_selected_rays(emu):
    """Without NDC and viewdirs the select form is the bundle form at the selected pixels: same per-ray terms, same sums."""
    H, W, n = 19, 29, 257
    focal = float(np.float32(20.5))
    rng = np.random.default_rng(3)
    c2w = _pose(9)
    inds = rng.permutation(H * W)[:n]
    g = rng.normal(size=(n, 8)).astype(np.float32)
    got = _select_bwd(emu, _cfg(H, W, focal, False, False), c2w, inds, g, None, 8)
    pix = (inds % H) * W + inds // H
    ref, _ = _bundle_bwd(emu, H, W, focal, pix, np.ascontiguousarray(g[:, 0:3]), np.ascontiguousarray(g[:, 3:6]))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_pose_vjp_of_no_rays_is_zero(emu):
    out, tb = _bundle_bwd(emu, 4, 4, 3.0, np.zeros(0, dtype=np.int64), None, None)
    assert tb == 0 and np.all(out == 0.0)


def test_pose_vjp_rejects_bad_arguments(emu):
    lib = emu.lib
    out = np.zeros(12, dtype=np.float32)
    tmp = np.zeros(64, dtype=np.float32)
    g = np.zeros((4, 11), dtype=np.float32)
    inds = np.arange(4, dtype=np.int64)
    c2w = np.eye(4, dtype=np.float32)
    assert lib.pose_grad_tmp_bytes(-1) == -1
    raw_b = lib._dll.nerfhip_ray_bundle_bwd
    raw_s = lib._dll.nerfhip_select_rays_bwd
    # whole image with n != H * W; no cotangent at all; no output; tmp too small; bad image size
    assert raw_b(4, 4, 3.0, None, 15, g.ctypes.data, g.ctypes.data, tmp.ctypes.data, 256, out.ctypes.data, None) == L_ERR_ARG
    assert raw_b(4, 4, 3.0, inds.ctypes.data, 4, None, None, tmp.ctypes.data, 256, out.ctypes.data, None) == L_ERR_ARG
    assert raw_b(4, 4, 3.0, inds.ctypes.data, 4, g.ctypes.data, None, tmp.ctypes.data, 256, None, None) == L_ERR_ARG
    assert raw_b(4, 4, 3.0, inds.ctypes.data, 4, g.ctypes.data, None, tmp.ctypes.data, 8, out.ctypes.data, None) == L_ERR_ARG
    assert raw_b(0, 4, 3.0, inds.ctypes.data, 4, g.ctypes.data, None, tmp.ctypes.data, 256, out.ctypes.data, None) == L_ERR_ARG
    cfg = _cfg(4, 4, 3.0, False, True)
    # row stride narrower than the 11 columns; no indices; c2w_ld < 4; NULL cfg
    assert raw_s(C.byref(cfg), c2w.ctypes.data, 4, inds.ctypes.data, 4, g.ctypes.data, None, 8, tmp.ctypes.data, 256,
                 out.ctypes.data, None) == L_ERR_ARG
    assert raw_s(C.byref(cfg), c2w.ctypes.data, 4, None, 4, g.ctypes.data, None, 11, tmp.ctypes.data, 256, out.ctypes.data,
                 None) == L_ERR_ARG
    assert raw_s(C.byref(cfg), c2w.ctypes.data, 3, inds.ctypes.data, 4, g.ctypes.data, None, 11, tmp.ctypes.data, 256,
                 out.ctypes.data, None) == L_ERR_ARG
    assert raw_s(None, c2w.ctypes.data, 4, inds.ctypes.data, 4, g.ctypes.data, None, 11, tmp.ctypes.data, 256, out.ctypes.data,
                 None) == L_ERR_ARG
    assert lib._dll.nerfhip_last_error()  # (the message of the last refusal)


L_ERR_ARG = -1  # NERFHIP_ERR_ARG
