"""Cases of the device-resident intrinsics (nerfhip_select_rays_views_intr / _intr_bwd, nerfhip_ray_bundle_intr,
nerfhip_intrinsics_fwd / _bwd), written once against a backend of tests/backends.py: tests/test_intrinsics.py runs them on the wave
emulator, tests/test_gpu_intrinsics.py on the product library.

Definitions (include/nerfhip.h): intr = (fx, fy, cx, cy), pixel (row, col) has the camera direction
dc = ((col - cx) / fx, -(row - cy) / fy, -1); the NDC constants are those of cfg and do not follow intr.

Reference value: torch autograd in fp64 through a restatement, local to this file, of pin-hole -> (cfg's fixed NDC) -> packing
(`rays64`), with intr and the pose table as leaves.  The restatement is fed the fp32 values the kernel reads.

Bound of the intrinsics gradient, per entry, in the form of tests/pose_vjp.py:

    |g_intr - exact| <= (D(n) + C_INTR) * 2^-24 * sum_i A_i

* D(n) = pose_vjp.reduction_depth(n): the sum runs along the single-view tree over all n rays of the batch.
* A_i: the ray term evaluated on the absolute values of its operands (subtractions as additions), in fp64 (`magnitudes`).
* C_INTR bounds the roundings along the longest dependency chain of a ray term (csrc/dataio.hip, k_intr_vjp_part): the chain up to
  g_d, the cotangent of the pre-NDC direction, is the pose VJP's -- camera direction 2, pre-NDC direction 4, t 2, p 2, 1/pz 1,
  d/d(pz) 6, d/dt 3, d/d(dz) 5: 25 on the NDC path; the viewdir normalisation's backward (12) and the coarse + fine add (1) are a
  shorter chain into the same add --, then R^T g_d 3 (a product and two adds), the camera direction that multiplies it 2, the
  product 1, the division by the focal 1: 32; plus 2 for the fp32 inputs read against the reference's: 34, taken as 40.
  (As in tests/pose_vjp.py the abs-evaluation bounds a division's error only while its denominator is not the result of
  cancellation: dz ~ -1 and pz = -near hold for the forward-facing cameras the NDC cases use.)

g_poses is held by pose_vjp.bound with n = the number of rays of the view, on magnitudes restated here for dc from intr.
"""
import ctypes as C

import numpy as np
import torch

import pose_vjp as P
import views_cases as VC

ERR_ARG = -1  # NERFHIP_ERR_ARG
U32 = 2.0 ** -24
C_INTR = 40
bits = VC.bits

# the scene of cases 1 - 3: non-square, fx != fy, an off-centre principal point (a swap or a wrong sign shows)
V3, H3, W3 = 3, 5, 7
FOCAL3 = float(np.float32(6.3))
INTR3 = np.array([6.3, 5.1, 3.9, 2.2], dtype=np.float32)


def centred(H, W, focal):
    """The intrinsics that restate the scalar camera of (H, W, focal)."""
    return np.array([focal, focal, np.float32(W * 0.5), np.float32(H * 0.5)], dtype=np.float32)


def ndc_consts(cfg):
    return dict(near=float(cfg.ndc_near), cw=float(cfg.ndc_cw), ch=float(cfg.ndc_ch), two_near=float(cfg.ndc_two_near),
                neg_two_near=float(cfg.ndc_neg_two_near))


# ---- the fp64 restatement -------------------------------------------------------------------------------------------------------
def rays64(H, W, intr, poses, inds, ndc, view, near=2.0, far=6.0):
    """Packed rows [n, 8 | 11] (torch fp64, differentiable in intr [4] and poses [V, 3, 4]) of the global select indices `inds`
    (view g // (H W), row k % H, col k // H); ndc: None or the constants of ndc_consts."""
    inds = torch.as_tensor(inds, dtype=torch.int64)
    vid, k = inds // (H * W), inds % (H * W)
    row, col = (k % H).double(), (k // H).double()
    dc = torch.stack([(col - intr[2]) / intr[0], -(row - intr[3]) / intr[1], -torch.ones_like(col)], -1)
    R, t = poses[vid][:, :, :3], poses[vid][:, :, 3]
    d = (R * dc[:, None, :]).sum(-1)
    o, src = t, d
    if ndc is not None:
        tt = -(ndc["near"] + o[:, 2]) / d[:, 2]
        p = o + tt[:, None] * d
        o = torch.stack([ndc["cw"] * p[:, 0] / p[:, 2], ndc["ch"] * p[:, 1] / p[:, 2], 1.0 + ndc["two_near"] / p[:, 2]], -1)
        d = torch.stack([ndc["cw"] * (d[:, 0] / d[:, 2] - p[:, 0] / p[:, 2]), ndc["ch"] * (d[:, 1] / d[:, 2] - p[:, 1] / p[:, 2]),
                         ndc["neg_two_near"] / p[:, 2]], -1)
    cols = [o, d, torch.full((len(inds), 1), near, dtype=torch.float64), torch.full((len(inds), 1), far, dtype=torch.float64)]
    if view:
        cols.append(src / src.norm(dim=-1, keepdim=True))
    return torch.cat(cols, -1)


def rows_scale(H, W, intr, poses, inds, ndc, view, near=2.0, far=6.0):
    """rays64 evaluated on absolute values (numpy fp64): the scale the forward's roundings are relative to."""
    intr, poses = np.asarray(intr, np.float64), np.asarray(poses, np.float64)
    inds = np.asarray(inds, np.int64)
    vid, k = inds // (H * W), inds % (H * W)
    row, col = (k % H).astype(np.float64), (k // H).astype(np.float64)
    dca = np.stack([(col + intr[2]) / intr[0], (row + intr[3]) / intr[1], np.ones_like(col)], -1)
    dc = np.stack([(col - intr[2]) / intr[0], -(row - intr[3]) / intr[1], -np.ones_like(col)], -1)
    R, t = poses[vid][:, :, :3], poses[vid][:, :, 3]
    d_true = (R * dc[:, None, :]).sum(-1)
    d = (np.abs(R) * dca[:, None, :]).sum(-1)
    o, src = np.abs(t), d
    if ndc is not None:
        cw, ch, nr = abs(ndc["cw"]), abs(ndc["ch"]), ndc["near"]
        dz = np.abs(d_true[:, 2])
        tt = (nr + o[:, 2]) / dz
        p = o + tt[:, None] * d
        pz = nr  # (pz = -near)
        o = np.stack([cw * p[:, 0] / pz, ch * p[:, 1] / pz, (1.0 + 2.0 * nr / pz) * np.ones_like(dz)], -1)
        d = np.stack([cw * (d[:, 0] / dz + p[:, 0] / pz), ch * (d[:, 1] / dz + p[:, 1] / pz), 2.0 * nr / pz * np.ones_like(dz)], -1)
    cols = [o, d, np.full((len(inds), 1), near), np.full((len(inds), 1), far)]
    if view:
        cols.append(src / np.linalg.norm(d_true, axis=-1, keepdims=True))
    return np.concatenate(cols, -1)


def oracle_vjp(H, W, intr, poses, inds, g_rays, ndc, view):
    """(g_poses [V, 3, 4], g_intr [4]) by fp64 autograd through rays64."""
    it = torch.tensor(np.asarray(intr, np.float64), requires_grad=True)
    pt = torch.tensor(np.asarray(poses, np.float64)[:, :3, :4], requires_grad=True)
    rays = rays64(H, W, it, pt, inds, ndc, view)
    (rays * torch.as_tensor(g_rays[:, :rays.shape[1]], dtype=torch.float64)).sum().backward()
    return pt.grad.numpy(), it.grad.numpy()


def magnitudes(H, W, intr, poses, inds, g_abs, ndc, view):
    """Per ray, every term on absolute values (fp64): (pose terms [n, 3, 4], intrinsics terms A_i [n, 4])."""
    intr = torch.as_tensor(np.asarray(intr, np.float64))
    poses = torch.as_tensor(np.asarray(poses, np.float64)[:, :3, :4])
    inds = torch.as_tensor(np.asarray(inds), dtype=torch.int64)
    n = len(inds)
    vid, k = inds // (H * W), inds % (H * W)
    row, col = (k % H).double(), (k // H).double()
    dc_true = torch.stack([(col - intr[2]) / intr[0], -(row - intr[3]) / intr[1], -torch.ones_like(col)], -1)
    dc = torch.stack([(col + intr[2]) / intr[0], (row + intr[3]) / intr[1], torch.ones_like(col)], -1)
    Rt, R, o = poses[vid][:, :, :3], poses[vid][:, :, :3].abs(), poses[vid][:, :, 3].abs()
    d_true = (Rt * dc_true[:, None, :]).sum(-1)
    d = (R * dc[:, None, :]).sum(-1)
    g = torch.as_tensor(g_abs, dtype=torch.float64)
    go, gd = g[:, 0:3], g[:, 3:6]
    if ndc is not None:  # (tests/pose_vjp.py, magnitude: nh_ndc_ray_vjp on absolute values)
        cw, ch, near = abs(ndc["cw"]), abs(ndc["ch"]), ndc["near"]
        dz = d_true[:, 2].abs()
        tt = (near + o[:, 2]) / dz
        px, py = o[:, 0] + tt * d[:, 0], o[:, 1] + tt * d[:, 1]
        ipz = 1.0 / near
        gO, gD = go, gd
        ax, ay = cw * (gO[:, 0] + gD[:, 0]), ch * (gO[:, 1] + gD[:, 1])
        gpx, gpy = ax * ipz, ay * ipz
        gpz = (ax * px + ay * py + 2 * near * gO[:, 2] + 2 * near * gD[:, 2]) * ipz * ipz
        gdx, gdy = cw * gD[:, 0] / dz, ch * gD[:, 1] / dz
        gdz = (cw * gD[:, 0] * d[:, 0] + ch * gD[:, 1] * d[:, 1]) / dz / dz
        gt = gpx * d[:, 0] + gpy * d[:, 1] + gpz * d[:, 2]
        gdx, gdy, gdz = gdx + tt * gpx, gdy + tt * gpy, gdz + tt * gpz
        gpz = gpz + gt / dz
        gdz = gdz + gt * (near + o[:, 2]) / dz / dz
        go, gd = torch.stack([gpx, gpy, gpz], -1), torch.stack([gdx, gdy, gdz], -1)
    if view:
        nrm = d_true.norm(dim=-1, keepdim=True)
        u = d / nrm
        gv = g[:, 8:11]
        gd = gd + (gv + u * (u * gv).sum(-1, keepdim=True)) / nrm
    pose_terms = torch.zeros(n, 3, 4, dtype=torch.float64)
    pose_terms[:, :, :3] = gd[:, :, None] * dc[:, None, :]
    pose_terms[:, :, 3] = go
    gdc = (gd[:, :, None] * R).sum(1)  # |g_d|^T |R|
    a = torch.stack([gdc[:, 0] * dc[:, 0] / intr[0], gdc[:, 1] * dc[:, 1] / intr[1], gdc[:, 0] / intr[0], gdc[:, 1] / intr[1]], -1)
    return pose_terms.numpy(), a.numpy()


def intr_bound(n, a_sum):
    return (P.reduction_depth(n) + C_INTR) * U32 * a_sum


# ---- the entry points on numpy arrays -------------------------------------------------------------------------------------------
def select_intr(b, cfg, intr, table, vstride, ld, V, images, n, inds=None):
    use_view, ch = bool(cfg.use_viewdirs), cfg.channels
    dp, di, dn, dk = b.dev(table), b.devopt(images), b.devopt(inds, np.int64), b.dev(np.ascontiguousarray(intr, np.float32))
    rays, tgt, used = b.empty((n, 11 if use_view else 8)), b.empty((n, ch)), b.empty((n,), np.int64)
    b.lib.select_rays_views_intr(C.byref(cfg), b.ptr(dk), V, b.ptr(dp), vstride, ld, b.p(di), b.p(dn), n, b.ptr(rays),
                                 b.ptr(tgt) if images is not None else None, b.ptr(used), b.stream())
    return b.host(rays), (b.host(tgt) if images is not None else None), b.host(used)


def intr_bwd(b, cfg, intr, table, vstride, ld, V, inds, g, g2, stride, want_poses=True, want_intr=True, tmp_slack=0):
    n = len(inds)
    tb = b.lib.intr_grad_views_tmp_bytes(n, V)
    assert tb >= 0
    tmp = b.empty((max(tb // 4, 1) + tmp_slack,))
    gp, gi = (b.empty((V, 3, 4)) if want_poses else None), (b.empty((4,)) if want_intr else None)
    dp, dn, dk = b.dev(table), b.dev(np.ascontiguousarray(inds, np.int64)), b.dev(np.ascontiguousarray(intr, np.float32))
    dg, dg2 = b.devopt(g), b.devopt(g2)
    b.lib.select_rays_views_intr_bwd(C.byref(cfg), b.ptr(dk), V, b.ptr(dp), vstride, ld, b.ptr(dn), n, b.p(dg), b.p(dg2), stride,
                                     b.ptr(tmp), tb, b.p(gp), b.p(gi), b.stream())
    return (b.host(gp) if want_poses else None), (b.host(gi) if want_intr else None)


def bundle_intr(b, H, W, intr, c2w, pixels=None):
    c2w = np.ascontiguousarray(c2w, np.float32)
    n = H * W if pixels is None else len(pixels)
    dc, dp, dk = b.dev(c2w), b.devopt(pixels, np.int64), b.dev(np.ascontiguousarray(intr, np.float32))
    ro, rd = b.empty((n, 3)), b.empty((n, 3))
    b.lib.ray_bundle_intr(H, W, b.ptr(dk), b.ptr(dc), c2w.shape[1], b.p(dp), n, b.ptr(ro), b.ptr(rd), b.stream())
    return b.host(ro), b.host(rd)


def param_fwd(b, q, base, tie):
    dq, db, out = b.dev(np.asarray(q, np.float32)), b.dev(np.asarray(base, np.float32)), b.empty((4,))
    b.lib.intrinsics_fwd(b.ptr(dq), b.ptr(db), int(tie), b.ptr(out), b.stream())
    return b.host(out)


def param_bwd(b, q, base, tie, g_intr, mask):
    dq, db, dg = b.dev(np.asarray(q, np.float32)), b.dev(np.asarray(base, np.float32)), b.dev(np.asarray(g_intr, np.float32))
    dm = b.devopt(mask, np.uint8)
    out = b.empty((4,))
    b.lib.intrinsics_bwd(b.ptr(dq), b.ptr(db), int(tie), b.ptr(dg), b.p(dm), b.ptr(out), b.stream())
    return b.host(out)


def scene3(ndc):
    return np.stack([VC.pose(20 + v, llff=ndc) for v in range(V3)])


# ---- 1. selection on the bits ---------------------------------------------------------------------------------------------------
def case_selection_bits(b, ndc, view, layout):
    """intr = (f, f, fp32(W/2), fp32(H/2)) gives the scalar entry points' bits: the whole population of V = 3 views of 5 x 7, and
    V = 1 against nerfhip_select_rays."""
    V, H, W, focal = V3, H3, W3, FOCAL3
    poses = scene3(ndc)
    images = np.random.default_rng(12).random((V, H, W, 3), dtype=np.float32)
    cfg = VC.cfg_of(b, H, W, focal, ndc, view, 3, seed=5, step=2, first=0)
    table, vs, ld = VC.pose_table(poses, layout)
    n = V * H * W
    intr = centred(H, W, focal)
    rays, tgt, used = select_intr(b, cfg, intr, table, vs, ld, V, images, n)
    want = VC.select_views(b, cfg, table, vs, ld, V, images, n)
    assert sorted(used.tolist()) == list(range(n)) and np.all(np.isfinite(rays))
    assert np.array_equal(used, want[2]) and np.array_equal(bits(rays), bits(want[0])) and np.array_equal(bits(tgt), bits(want[1]))
    # V = 1: the single-view form
    n1 = H * W
    cfg1 = VC.cfg_of(b, H, W, focal, ndc, view, 3, seed=7, step=1, first=0)
    t1, vs1, ld1 = VC.pose_table(poses[1:2], layout)
    r1, g1, u1 = select_intr(b, cfg1, intr, t1, vs1, ld1, 1, images[1:2], n1)
    w1 = b.select_rays(H, W, focal, poses[1], images[1], n1, 2.0, 6.0, use_viewdirs=view, ndc=ndc, seed=7, step=1, first=0)
    assert np.array_equal(u1, w1[2]) and np.array_equal(bits(r1), bits(w1[0])) and np.array_equal(bits(g1), bits(w1[1]))


def case_bundle_bits(b):
    H, W, focal = H3, W3, FOCAL3
    c2w = VC.pose(5)
    intr = centred(H, W, focal)
    for pixels in (None, np.array([34, 0, 7, 6, 13, 13, 20], dtype=np.int64)):
        ro, rd = bundle_intr(b, H, W, intr, c2w, pixels)
        wo, wd = b.ray_bundle(H, W, focal, c2w, pixels)
        assert np.all(np.isfinite(rd)) and np.array_equal(bits(ro), bits(wo)) and np.array_equal(bits(rd), bits(wd))
    # fx != fy, an off-centre principal point: against fp64 (a pixel list in (row * W + col) order)
    pix = np.arange(H * W, dtype=np.int64)
    ro, rd = bundle_intr(b, H, W, INTR3, c2w, pix)
    k = (pix % W) * H + pix // W   # the select index of pixel (row, col) = (pix // W, pix % W)
    want = rays64(H, W, torch.tensor(INTR3.astype(np.float64)), torch.tensor(c2w[None, :3, :4].astype(np.float64)), k, None, False).numpy()
    scale = rows_scale(H, W, INTR3, c2w[None, :3, :4], k, None, False)
    assert np.all(np.abs(ro - want[:, 0:3]) <= 4 * 2.0 ** -23 * scale[:, 0:3])
    assert np.all(np.abs(rd - want[:, 3:6]) <= 4 * 2.0 ** -23 * scale[:, 3:6])


# ---- 2. selection against fp64 --------------------------------------------------------------------------------------------------
def case_selection_fp64(b, ndc, view):
    """intr = (6.3, 5.1, 3.9, 2.2): every entry of every row within 4 ulp (2^-23) of its scale -- the row evaluated on absolute
    values -- of the fp64 restatement.  A swapped fx / fy or cx / cy or a wrong sign moves entries by whole units of that scale."""
    V, H, W = V3, H3, W3
    poses = scene3(ndc)
    cfg = VC.cfg_of(b, H, W, FOCAL3, ndc, view, 3, seed=5, step=2, first=0)
    n = V * H * W
    rays, _, used = select_intr(b, cfg, INTR3, poses, 16, 4, V, None, n)
    assert sorted(used.tolist()) == list(range(n))
    nd = ndc_consts(cfg) if ndc else None
    p64 = poses[:, :3, :4].astype(np.float64)
    want = rays64(H, W, torch.tensor(INTR3.astype(np.float64)), torch.tensor(p64), used, nd, view).numpy()
    scale = rows_scale(H, W, INTR3, p64, used, nd, view)
    err = np.abs(rays.astype(np.float64) - want)
    tol = 4 * 2.0 ** -23 * scale
    print("selection vs fp64 (ndc %d, viewdirs %d): worst error / tolerance = %.3f" % (ndc, view, float((err / tol).max())))
    assert np.all(err <= tol), float((err / tol).max())
    # the test has teeth: the swapped intrinsics are far outside the tolerance
    for wrong in (INTR3[[1, 0, 2, 3]], INTR3[[0, 1, 3, 2]]):
        w = rays64(H, W, torch.tensor(wrong.astype(np.float64)), torch.tensor(p64), used, nd, view).numpy()
        assert np.any(np.abs(w - want) > 1000 * tol)


# ---- 3. the VJP -----------------------------------------------------------------------------------------------------------------
BIG = dict(V=100, H=40, W=40, focal=float(np.float32(45.0)), intr=np.array([45.0, 41.5, 21.25, 18.5], dtype=np.float32))


def vjp_scene(big, ndc):
    if big:
        poses = np.stack([VC.pose(300 + v, llff=ndc) for v in range(BIG["V"])])
        return BIG["V"], BIG["H"], BIG["W"], BIG["focal"], BIG["intr"], poses
    return V3, H3, W3, FOCAL3, INTR3, scene3(ndc)


def case_vjp(b, n, ndc, view, two, stride, big=False):
    """g_intr and g_poses against fp64 autograd under their bounds; views interleave (indices from rng.integers)."""
    V, H, W, focal, intr, poses = vjp_scene(big, ndc)
    cfg = VC.cfg_of(b, H, W, focal, ndc, view)
    nd = ndc_consts(cfg) if ndc else None
    hw = H * W
    # the batch: the first of 20 seeds at which, by the reference alone, every exact entry is >= 100 x its bound (a random sum
    # can come out small against the sum of its terms' magnitudes; such a draw would let a zero result pass)
    for attempt in range(20):
        rng = np.random.default_rng(1000 + 16 * n + 8 * big + 4 * ndc + 2 * view + two + 100000 * attempt)
        inds = rng.integers(0, V * hw, size=n).astype(np.int64)
        g = rng.normal(size=(n, stride)).astype(np.float32)
        g2 = rng.normal(size=(n, stride)).astype(np.float32) if two else None
        gsum = g.astype(np.float64) + (g2.astype(np.float64) if two else 0.0)
        gmag = np.abs(g.astype(np.float64)) + (np.abs(g2.astype(np.float64)) if two else 0.0)
        want_p, want_i = oracle_vjp(H, W, intr, poses, inds, gsum, nd, view)
        pose_terms, a = magnitudes(H, W, intr, poses, inds, gmag, nd, view)
        if np.all(np.abs(want_i) >= 100 * intr_bound(n, a.sum(0))):
            break
    gp, gi = intr_bwd(b, cfg, intr, poses, 16, 4, V, inds, g, g2, stride)
    assert gp.shape == (V, 3, 4) and gi.shape == (4,) and np.all(np.isfinite(gp)) and np.all(np.isfinite(gi))
    # the intrinsics: one tree over all n rays
    bound = intr_bound(n, a.sum(0))
    err = np.abs(gi.astype(np.float64) - want_i)
    print("g_intr, n = %d (ndc %d, viewdirs %d, two %d): exact %s, error / bound %s, |exact| / bound %s"
          % (n, ndc, view, two, want_i, err / bound, np.abs(want_i) / bound))
    assert np.all(np.abs(want_i) >= 100 * bound), (want_i, bound)   # not vacuous: a zero result is far outside the bound
    assert np.all(err <= bound), (err / bound)
    # the poses: each view's tree over its own rays
    vid = inds // hw
    for v in range(V):
        rows = np.nonzero(vid == v)[0]
        if len(rows) == 0:
            assert np.array_equal(bits(gp[v]), np.zeros((3, 4), np.uint32))
            continue
        pb = P.bound(len(rows), pose_terms[rows].sum(0))
        pe = np.abs(gp[v].astype(np.float64) - want_p[v])
        assert np.all(pe <= pb), (v, float((pe / np.maximum(pb, 1e-300)).max()))
    # each output asked alone has the bits it has when both are asked; a second call (another tmp size) gives the same bits
    only_p, none_i = intr_bwd(b, cfg, intr, poses, 16, 4, V, inds, g, g2, stride, want_intr=False)
    none_p, only_i = intr_bwd(b, cfg, intr, poses, 16, 4, V, inds, g, g2, stride, want_poses=False, tmp_slack=5)
    assert none_i is None and none_p is None
    assert np.array_equal(bits(only_p), bits(gp)) and np.array_equal(bits(only_i), bits(gi))
    gp2, gi2 = intr_bwd(b, cfg, intr, poses, 16, 4, V, inds, g, g2, stride, tmp_slack=7)
    assert np.array_equal(bits(gp2), bits(gp)) and np.array_equal(bits(gi2), bits(gi))
    # the embedded pose table gives the same bits
    table, vs, ld = VC.pose_table(poses, "embedded")
    gp3, gi3 = intr_bwd(b, cfg, intr, table, vs, ld, V, inds, g, g2, stride)
    assert np.array_equal(bits(gp3), bits(gp)) and np.array_equal(bits(gi3), bits(gi))


def case_vjp_poses_equal_the_scalar_form(b, n, ndc, view):
    """With intr = (f, f, fp32(W/2), fp32(H/2)), g_poses has the bits of nerfhip_select_rays_views_bwd."""
    V, H, W, focal = V3, H3, W3, FOCAL3
    poses = scene3(ndc)
    rng = np.random.default_rng(77 + n)
    cfg = VC.cfg_of(b, H, W, focal, ndc, view)
    inds = rng.integers(0, V * H * W, size=n).astype(np.int64)
    g, g2 = rng.normal(size=(n, 11)).astype(np.float32), rng.normal(size=(n, 11)).astype(np.float32)
    gp, gi = intr_bwd(b, cfg, centred(H, W, focal), poses, 16, 4, V, inds, g, g2, 11)
    want = VC.views_bwd(b, cfg, poses, 16, 4, V, inds, g, g2, 11)
    assert np.all(np.isfinite(gp)) and float(np.abs(gp).sum()) > 0 and np.all(np.isfinite(gi))
    assert np.array_equal(bits(gp), bits(want))


def case_vjp_edges(b):
    """n = 0: exact zeros; a view without rays: a zero pose row; an out-of-range index: dropped by both outputs."""
    V, H, W, focal, hw = V3, H3, W3, FOCAL3, H3 * W3
    poses = scene3(False)
    cfg = VC.cfg_of(b, H, W, focal, False, True)
    lib = b.lib
    assert lib.intr_grad_views_tmp_bytes(0, V) == 0 and lib.intr_grad_views_tmp_bytes(-1, V) == -1
    assert lib.intr_grad_views_tmp_bytes(5, 0) == -1
    assert lib.intr_grad_views_tmp_bytes(700, 4) == lib.pose_grad_views_tmp_bytes(700, 4) + 4 * 4 * P.wgs(700)
    # n = 0 (tmp, inds, g_rays may be NULL)
    gp, gi = b.empty((V, 3, 4)), b.empty((4,))
    dp, dk = b.dev(poses), b.dev(INTR3)
    lib.select_rays_views_intr_bwd(C.byref(cfg), b.ptr(dk), V, b.ptr(dp), 16, 4, None, 0, None, None, 11, None, 0, b.ptr(gp),
                                   b.ptr(gi), b.stream())
    assert np.array_equal(bits(b.host(gp)), np.zeros((V, 3, 4), np.uint32)) and np.array_equal(bits(b.host(gi)), np.zeros(4, np.uint32))
    # view 1 gets no ray
    rng = np.random.default_rng(5)
    n = 300
    inds = (rng.choice([0, 2], size=n) * hw + rng.integers(0, hw, size=n)).astype(np.int64)
    g = rng.normal(size=(n, 11)).astype(np.float32)
    gp, gi = intr_bwd(b, cfg, INTR3, poses, 16, 4, V, inds, g, None, 11)
    assert np.array_equal(bits(gp[1]), np.zeros((3, 4), np.uint32))
    assert float(np.abs(gp[0]).sum()) > 0 and float(np.abs(gp[2]).sum()) > 0 and np.all(gi != 0)
    # indices outside [0, V H W): g_poses is that of the batch without them (each view keeps its rays and their order); g_intr is
    # that of the batch with their rows zeroed at a valid index (the tree's shape is n's; a dropped ray adds nothing)
    out = np.array([3, 17, 130, 255, 256, 299])
    bad = inds.copy()
    bad[out] = np.array([-1, V * hw, V * hw + 9, -hw, 2 ** 40, -2 ** 40])
    gp_b, gi_b = intr_bwd(b, cfg, INTR3, poses, 16, 4, V, bad, g, None, 11)
    keep = np.setdiff1d(np.arange(n), out)
    gp_k, _ = intr_bwd(b, cfg, INTR3, poses, 16, 4, V, inds[keep], np.ascontiguousarray(g[keep]), None, 11)
    gz = g.copy()
    gz[out] = 0.0
    _, gi_z = intr_bwd(b, cfg, INTR3, poses, 16, 4, V, inds, gz, None, 11)
    assert np.all(np.isfinite(gp_b)) and np.all(np.isfinite(gi_b))
    assert np.array_equal(bits(gp_b), bits(gp_k)) and np.array_equal(bits(gi_b), bits(gi_z))
    assert not np.array_equal(bits(gi_b), bits(gi))


# ---- 4. the parametrisation -----------------------------------------------------------------------------------------------------
BASE = np.array([612.25, 598.5, 321.75, 243.125], dtype=np.float32)
MASKS = [tuple((m >> k) & 1 for k in range(4)) for m in range(16)]


def case_param_fwd(b, tie):
    got = param_fwd(b, np.zeros(4, np.float32), BASE, tie)
    assert np.array_equal(bits(got), bits(BASE))
    got = param_fwd(b, np.array([-0.0, 0.0, -0.0, 0.0], np.float32), BASE, tie)
    assert np.array_equal(bits(got), bits(BASE))
    rng = np.random.default_rng(3 + tie)
    for _ in range(8):
        q = (rng.normal(size=4) * np.array([0.2, 0.2, 5.0, 5.0])).astype(np.float32)
        got = param_fwd(b, q, BASE, tie).astype(np.float64)
        q64, b64 = q.astype(np.float64), BASE.astype(np.float64)
        want = np.array([b64[0] * np.exp(q64[0]), b64[1] * np.exp(q64[0 if tie else 1]), b64[2] + q64[2], b64[3] + q64[3]])
        assert np.all(np.abs(got - want) <= 4 * U32 * np.abs(want)), (q, got, want)
        assert got[0] > 0 and got[1] > 0


def case_param_bwd(b, tie, mask):
    rng = np.random.default_rng(40 + 2 * sum(m << k for k, m in enumerate(mask)) + tie)
    q = (rng.normal(size=4) * np.array([0.2, 0.2, 5.0, 5.0])).astype(np.float32)
    g = rng.normal(size=4).astype(np.float32)
    m8 = np.array(mask, dtype=np.uint8)
    got = param_bwd(b, q, BASE, tie, g, m8)
    q64, b64, g64 = q.astype(np.float64), BASE.astype(np.float64), g.astype(np.float64)
    fx, fy = b64[0] * np.exp(q64[0]), b64[1] * np.exp(q64[0 if tie else 1])
    terms = [[g64[0] * fx] + ([g64[1] * fy] if tie else []), [] if tie else [g64[1] * fy], [g64[2]], [g64[3]]]
    for k in range(4):
        if not mask[k] or (tie and k == 1):
            assert bits(got[k:k + 1])[0] == 0, (k, got)   # an exact +0.0
            continue
        assert abs(float(got[k]) - sum(terms[k])) <= 8 * U32 * sum(abs(t) for t in terms[k]), (k, got, terms)
        assert got[k] != 0
    if all(mask):  # NULL mask: every entry learned
        assert np.array_equal(bits(param_bwd(b, q, BASE, tie, g, None)), bits(got))
    # three Adam steps: a masked entry of q keeps its bits, a learned one moves
    p, m, v = q.copy(), np.zeros(4, np.float32), np.zeros(4, np.float32)
    for step in (1, 2, 3):
        gq = param_bwd(b, p, BASE, tie, g, m8)
        p, m, v = b.adam_step(p, gq, m, v, 1e-2, step)
    for k in range(4):
        frozen = not mask[k] or (tie and k == 1)
        assert (bits(p[k:k + 1])[0] == bits(q[k:k + 1])[0]) == frozen, (k, p, q)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def case_refusals(b):
    lib = b.lib
    V, H, W = 3, 4, 4
    raw_s, raw_b, raw_r = (lib._dll.nerfhip_select_rays_views_intr, lib._dll.nerfhip_select_rays_views_intr_bwd,
                           lib._dll.nerfhip_ray_bundle_intr)
    cfg = VC.cfg_of(b, H, W, 3.0, False, True)
    poses = b.dev(np.stack([np.eye(4, dtype=np.float32)] * V))
    intr = b.dev(centred(H, W, 3.0))
    rays, used = b.empty((4, 11)), b.empty((4,), np.int64)
    inds = b.dev(np.arange(4, dtype=np.int64))
    g = b.dev(np.zeros((4, 11), np.float32))
    tb = lib.intr_grad_views_tmp_bytes(4, V)
    tmp, gp, gi = b.empty((tb // 4,)), b.empty((V, 3, 4)), b.empty((4,))
    pk, pp, pr, pu, pi, pg, pt, st = (b.ptr(intr), b.ptr(poses), b.ptr(rays), b.ptr(used), b.ptr(inds), b.ptr(g), b.ptr(tmp),
                                      b.stream())
    pgp, pgi = b.ptr(gp), b.ptr(gi)

    def refused(rc, *words):
        msg = lib._dll.nerfhip_last_error().decode()
        assert rc == ERR_ARG and all(w in msg for w in words), (rc, msg, words)

    ok = lambda c=cfg, k=pk, v=V, p=pp, vs=16, ld=4, n=4, r=pr: raw_s(C.byref(c) if c else None, k, v, p, vs, ld, None, None, n,  # noqa: E731
                                                                      r, None, pu, st)
    assert ok() == 0
    refused(ok(k=None), "select_rays_views_intr", "intr")
    refused(ok(ld=3), "select_rays_views_intr", "pose_ld")
    refused(ok(vs=11), "select_rays_views_intr", "pose_view_stride")
    refused(ok(vs=13, ld=5), "select_rays_views_intr", "pose_view_stride")
    refused(ok(v=0), "select_rays_views_intr", "num_views")
    refused(ok(c=None), "select_rays_views_intr")
    okb = lambda c=cfg, k=pk, v=V, p=pp, vs=16, ld=4, i=pi, gs=11, t=pt, tbytes=tb, o=pgp, oi=pgi: raw_b(  # noqa: E731
        C.byref(c) if c else None, k, v, p, vs, ld, i, 4, pg, None, gs, t, tbytes, o, oi, st)
    assert okb() == 0 and okb(o=None) == 0 and okb(oi=None) == 0
    refused(okb(k=None), "select_rays_views_intr_bwd", "intr")
    refused(okb(o=None, oi=None), "select_rays_views_intr_bwd", "g_poses", "g_intr")
    refused(okb(tbytes=tb - 4), "select_rays_views_intr_bwd", "nerfhip_intr_grad_views_tmp_bytes")
    refused(okb(tbytes=lib.pose_grad_views_tmp_bytes(4, V)), "select_rays_views_intr_bwd", "tmp")
    refused(okb(t=None), "select_rays_views_intr_bwd", "tmp")
    refused(okb(ld=3), "select_rays_views_intr_bwd", "pose_ld")
    refused(okb(vs=11), "select_rays_views_intr_bwd", "pose_view_stride")
    refused(okb(v=VC.L_MAX_VIEWS + 1), "select_rays_views_intr_bwd", "num_views")
    refused(okb(gs=8), "select_rays_views_intr_bwd", "g_rays_stride")
    refused(okb(i=None), "select_rays_views_intr_bwd")
    c2w = b.dev(np.eye(4, dtype=np.float32))
    ro, rd = b.empty((H * W, 3)), b.empty((H * W, 3))
    okr = lambda k=pk, ld=4, n=H * W: raw_r(H, W, k, b.ptr(c2w), ld, None, n, b.ptr(ro), b.ptr(rd), st)  # noqa: E731
    assert okr() == 0
    refused(okr(k=None), "ray_bundle_intr", "intr")
    refused(okr(ld=3), "ray_bundle_intr")
    refused(okr(n=3), "ray_bundle_intr", "height*width")
    q = b.dev(np.zeros(4, np.float32))
    refused(lib._dll.nerfhip_intrinsics_fwd(None, pk, 0, pgi, st), "intrinsics_fwd")
    refused(lib._dll.nerfhip_intrinsics_bwd(b.ptr(q), pk, 0, None, None, pgi, st), "intrinsics_bwd")
