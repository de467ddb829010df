"""Cases of the device-resident lens distortion (nerfhip_select_rays_views_dist / _dist_bwd, nerfhip_dist_grad_views_tmp_bytes,
nerfhip_ray_bundle_dist), written once against a backend of tests/backends.py: tests/test_distortion.py runs them on the wave
emulator, tests/test_gpu_distortion.py on the product library.

Definitions (include/nerfhip.h): dist = (k1, k2, p1, p2); (x, y) the undistorted normalised point (y down), (xd, yd) =
((col - cx) / fx, (row - cy) / fy) the observed one, (xd, yd) = F(x, y; dist); the kernels solve F = (xd, yd) by
NERFHIP_UNDISTORT_ITERS Newton steps in fp32 and use dc = (x, -y, -1).

Reference value (local to this file, fp64): Newton until the residual is below 1e-15 (`solve64`), then ONE differentiable Newton
step from that detached solution with the Jacobian held fixed (`newton_step`) -- its derivative is the implicit-function theorem's,
-J^-1 dF/d(dist) and J^-1 d(xd, yd)/d(intr), exactly --, then the restatement of rotation -> (cfg's fixed NDC) -> packing of
tests/intrinsics_cases.py (`rows_from`); torch autograd gives g_poses, g_intr and g_dist.  The restatement is fed the fp32 values the
kernel reads.  `case_reference_against_itself` holds it to central differences.

Bounds.  u = 2^-24.

* The solve.  The kernel's (x, y) is off by at most e = C_UND u s in each coordinate,
      s = (|xd| + |yd| + Fx_abs + Fy_abs) || |J^-1| ||_inf,
  with F_abs = F evaluated on |x|, |y|, |dist| and |J^-1| = the adjugate on absolute values over the true determinant.  (|xd| is the
  observed point's true magnitude: col, cx and fx are fp32 values the reference reads too, and each of the two operations of
  (col - cx) / fx rounds relative to its own result.)  At the fixed point of the fp32 iteration the error is J^-1 times the error
  of the evaluated residual (the step itself is then a few u long, so the roundings of J, of the determinant and of the division
  act on it in second order), plus the last subtraction's rounding.  C_UND counts the roundings of the residual along its longest
  chain (csrc/nh_rays.h, nh_distort): x^2 1, r2 1, r2^2 1, k2 r2^2 1, the add into rad 1, x rad 1, the add of the p1 term 1, the add
  of the p2 term 1: 8 for F, relative to F_abs; the subtraction F - xd 1, relative to F_abs + |xd|; xd itself 2 (subtraction,
  division), relative to |xd|: 9 u F_abs + 3 u |xd|, taken as 9 u (F_abs + |xd|) per component; the row sum of |J^-1| over the two
  components gives the product above.  The last subtraction x - step adds u |x|: one more unit where || |J^-1| ||_inf >= 1
  (|x| <= Fx_abs, as rad_abs >= 1); where it is below 1 -- the pincushion set, |x| <= |xd| -- the 6 u |xd| || |J^-1| || given away
  just above cover it while || |J^-1| ||_inf >= 1/6, which `case_domain` shows on every tested pixel.  C_UND = 10.  That the fp32
  iteration has reached its fixed point after NERFHIP_UNDISTORT_ITERS steps follows from `case_iteration_count` (in fp64 the
  quadratic phase is over two steps earlier, on the corners of every tested domain).
* The forward rows: 4 * 2^-23 * rows_scale (tests/intrinsics_cases.py's bound for the part behind dc, with |dc| = (|x|, |y|, 1))
  plus the image of the box [x - e, x + e] x [y - e, y + e] under the exact downstream map, to first order: the largest change of
  the row's entry over the box's four corners (the map is smooth and e ~ 1e-6, so what the linearisation leaves out is ~ 1e-12).
* The VJP: per entry
      |g_dist - exact| <= (D(n) + C_DIST) u sum_i A_i,      g_intr: the same with C_INTRP and its own A_i,
  D(n) = pose_vjp.reduction_depth(n).  A_i is the ray term on absolute values at (|x|, |y|) (`magnitudes`), lambda on the adjugate
  on absolute values over the true determinant.  C_DIST: the chain to g_d is the pose VJP's, 25 (tests/intrinsics_cases.py);
  R^T g_d 3: 28.  An entry of J: rad 5, dr = 2 (k1 + 2 k2 r2) 4, dr x^2 1 more than x^2's 1: the sum ((rad + dr xx) + .) + . is 8
  deep.  A product's roundings are those of its operands plus one, so the numerator d g0 - b g1 has 8 + 28 + 1 + 1 = 38 and the
  determinant a d - b b 8 + 8 + 1 + 1 = 18, relative to ITS evaluation on absolute values: RHO = 3 times the true determinant at
  most on every tested ray (`case_domain` shows it by the reference alone), so 54 relative to the determinant; the division 1:
  lambda 93.  The longest coefficient term is k2's, r2^2 (lambda . (x, y)): the dot product 93 + 1 + 1, r2^2 3, the product 1: 99,
  plus 2 for the fp32 inputs as in the other bounds: C_DIST = 101.  C_INTRP: lambda 93, xd 2, the product 1, the division by the
  focal 1, plus 2: 99.  The counts take (x, y) as the terms' operands: the kernel evaluates each term at ITS fp32 solution, off by
  e above, and that perturbation of the operands is not among the counted roundings; the bounds are asserted as they stand (the
  measured error stays below a twentieth of them).
  g_poses is held by pose_vjp.bound with n = the number of rays of the view, on magnitudes with |dc| = (|x|, |y|, 1).
"""
import ctypes as C
import os
import re

import numpy as np
import torch

import intrinsics_cases as IC
import pose_vjp as P
import views_cases as VC

ERR_ARG = -1  # NERFHIP_ERR_ARG
U32 = 2.0 ** -24
C_UND, C_DIST, C_INTRP, RHO = 10, 101, 99, 3.0
bits = VC.bits
V3, H3, W3, FOCAL3, INTR3 = IC.V3, IC.H3, IC.W3, IC.FOCAL3, IC.INTR3

KAPPA_BARREL = np.array([-0.15, 0.04, 3e-3, -2e-3], dtype=np.float32)
KAPPA_PINCUSHION = np.array([0.2, 0.05, -3e-3, 3e-3], dtype=np.float32)
KAPPAS = {"barrel": KAPPA_BARREL, "pincushion": KAPPA_PINCUSHION}
ZERO4 = np.zeros(4, dtype=np.float32)


def undistort_iters():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerfhip.h")).read()
    return int(re.search(r"#define\s+NERFHIP_UNDISTORT_ITERS\s+(\d+)", hdr).group(1))


# ---- the fp64 restatement -------------------------------------------------------------------------------------------------------
def distort(x, y, k):
    """F and its Jacobian [[a, b], [b, d]] (numpy or torch operands)."""
    k1, k2, p1, p2 = k[0], k[1], k[2], k[3]
    r2 = x * x + y * y
    rad = 1.0 + k1 * r2 + k2 * r2 * r2
    dr = 2.0 * (k1 + 2.0 * k2 * r2)
    Fx = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    Fy = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    a = rad + dr * x * x + 2.0 * p1 * y + 6.0 * p2 * x
    b = dr * x * y + 2.0 * p1 * x + 2.0 * p2 * y
    d = rad + dr * y * y + 6.0 * p1 * y + 2.0 * p2 * x
    return Fx, Fy, a, b, d


def newton64(xd, yd, k, iters):
    """`iters` Newton steps from (xd, yd) in numpy fp64 -> (x, y, the smallest det J met on the path)."""
    x, y = np.array(xd, np.float64, copy=True), np.array(yd, np.float64, copy=True)
    low = np.full(x.shape, np.inf)
    for _ in range(iters):
        Fx, Fy, a, b, d = distort(x, y, k)
        det = a * d - b * b
        low = np.minimum(low, det)
        rx, ry = Fx - xd, Fy - yd
        x, y = x - (d * rx - b * ry) / det, y - (a * ry - b * rx) / det
    return x, y, low


def residual(x, y, xd, yd, k):
    Fx, Fy, _, _, _ = distort(x, y, k)
    return np.maximum(np.abs(Fx - xd), np.abs(Fy - yd))


def solve64(xd, yd, k):
    """The converged solution: Newton until the residual is below 1e-15."""
    k = np.asarray(k, np.float64)
    for iters in range(1, 60):
        x, y, low = newton64(xd, yd, k, iters)
        if float(residual(x, y, xd, yd, k).max(initial=0.0)) < 1e-15:
            return x, y, low
    raise AssertionError("Newton did not reach 1e-15")


def observed(H, W, intr, inds):
    """(view, xd, yd, xd on absolute values, yd on absolute values) of the global select indices; torch when intr is."""
    inds = torch.as_tensor(np.asarray(inds), dtype=torch.int64)
    vid, k = inds // (H * W), inds % (H * W)
    row, col = (k % H).double(), (k // H).double()
    if not isinstance(intr, torch.Tensor):
        intr = torch.as_tensor(np.asarray(intr, np.float64))
    return vid, (col - intr[2]) / intr[0], (row - intr[3]) / intr[1], (col + intr[2]) / intr[0], (row + intr[3]) / intr[1]


def newton_step(xd, yd, kt, x0, y0):
    """One differentiable Newton step from the detached solution (x0, y0), the Jacobian held at its value there."""
    x0t, y0t = torch.as_tensor(x0), torch.as_tensor(y0)
    Fx, Fy, _, _, _ = distort(x0t, y0t, kt)
    _, _, a, b, d = (torch.as_tensor(v) for v in distort(x0, y0, kt.detach().numpy()))
    det = a * d - b * b
    rx, ry = Fx - xd, Fy - yd
    return x0t - (d * rx - b * ry) / det, y0t - (a * ry - b * rx) / det


def rows_from(xy, pr, ndc, view, near=2.0, far=6.0):
    """Packed rows [n, 8 | 11] (torch fp64) from the undistorted points xy [n, 2] and each ray's own pose pr [n, 3, 4]: what
    tests/intrinsics_cases.py's rays64 does behind its camera direction."""
    n = xy.shape[0]
    dc = torch.stack([xy[:, 0], -xy[:, 1], -torch.ones(n, dtype=torch.float64)], -1)
    R, t = pr[:, :, :3], pr[:, :, 3]
    d = (R * dc[:, None, :]).sum(-1)
    o, src = t, d
    if ndc is not None:
        tt = -(ndc["near"] + o[:, 2]) / d[:, 2]
        p = o + tt[:, None] * d
        o = torch.stack([ndc["cw"] * p[:, 0] / p[:, 2], ndc["ch"] * p[:, 1] / p[:, 2], 1.0 + ndc["two_near"] / p[:, 2]], -1)
        d = torch.stack([ndc["cw"] * (d[:, 0] / d[:, 2] - p[:, 0] / p[:, 2]), ndc["ch"] * (d[:, 1] / d[:, 2] - p[:, 1] / p[:, 2]),
                         ndc["neg_two_near"] / p[:, 2]], -1)
    cols = [o, d, torch.full((n, 1), near, dtype=torch.float64), torch.full((n, 1), far, dtype=torch.float64)]
    if view:
        cols.append(src / src.norm(dim=-1, keepdim=True))
    return torch.cat(cols, -1)


def rays64(H, W, intr, dist, poses, inds, ndc, view):
    """tests/intrinsics_cases.py's rays64 extended with the distortion: differentiable in intr [4], dist [4] and poses [V, 3, 4]."""
    vid, xd, yd, _, _ = observed(H, W, intr, inds)
    x0, y0, _ = solve64(xd.detach().numpy(), yd.detach().numpy(), dist.detach().numpy())
    x, y = newton_step(xd, yd, dist, x0, y0)
    return rows_from(torch.stack([x, y], -1), poses[vid], ndc, view)


def leaves(intr, dist, poses):
    return (torch.tensor(np.asarray(intr, np.float64), requires_grad=True), torch.tensor(np.asarray(dist, np.float64), requires_grad=True),
            torch.tensor(np.asarray(poses, np.float64)[:, :3, :4], requires_grad=True))


def oracle_vjp(H, W, intr, dist, poses, inds, g_rays, ndc, view):
    """(g_poses [V, 3, 4], g_intr [4], g_dist [4]) by fp64 autograd through rays64."""
    it, kt, pt = leaves(intr, dist, poses)
    rays = rays64(H, W, it, kt, pt, inds, ndc, view)
    (rays * torch.as_tensor(g_rays[:, :rays.shape[1]], dtype=torch.float64)).sum().backward()
    return pt.grad.numpy(), it.grad.numpy(), kt.grad.numpy()


def solved(H, W, intr, dist, inds):
    """numpy fp64: dict of the exact solution and what the bounds need of it, per ray."""
    vid, xd, yd, xda, yda = (t.numpy() for t in observed(H, W, intr, inds))
    k = np.asarray(dist, np.float64)
    x, y, low = solve64(xd, yd, k)
    _, _, a, b, d = distort(x, y, k)
    Fxa, Fya, aa, ba, da = distort(np.abs(x), np.abs(y), np.abs(k))
    det = a * d - b * b
    inv_norm = np.maximum(aa + ba, da + ba) / det   # || adj|J| / det ||_inf
    s = (np.abs(xd) + np.abs(yd) + Fxa + Fya) * inv_norm
    return dict(vid=vid, xd=xd, yd=yd, xda=xda, yda=yda, x=x, y=y, low=low, a=a, b=b, d=d, det=det, aa=aa, ba=ba, da=da,
                det_abs=aa * da + ba * ba, inv_norm=inv_norm, e=C_UND * U32 * s)


CORNERS = ((1, 1), (1, -1), (-1, 1), (-1, -1))


def ray_terms(H, W, intr, dist, poses, inds, g_rays, ndc, view, sol):
    """The exact per-ray terms: (pose terms [n, 3, 4], intrinsics terms [n, 4], distortion terms
    [n, 4]) -- autograd to each ray's own copy of its pose and of its point, then the implicit-function theorem in closed form."""
    intr, k = np.asarray(intr, np.float64), np.asarray(dist, np.float64)
    x, y = sol["x"], sol["y"]
    xy = torch.tensor(np.stack([x, y], -1), requires_grad=True)
    pr = torch.tensor(np.asarray(poses, np.float64)[:, :3, :4][sol["vid"]], requires_grad=True)
    rows = rows_from(xy, pr, ndc, view)
    (rows * torch.as_tensor(g_rays[:, :rows.shape[1]], dtype=torch.float64)).sum().backward()
    g = xy.grad.numpy()
    _, _, a, b, d = distort(x, y, k)
    det = a * d - b * b
    l0, l1 = (d * g[:, 0] - b * g[:, 1]) / det, (a * g[:, 1] - b * g[:, 0]) / det
    r2, lp = x * x + y * y, l0 * x + l1 * y
    t_dist = -np.stack([r2 * lp, r2 * r2 * lp, l0 * 2 * x * y + l1 * (r2 + 2 * y * y), l0 * (r2 + 2 * x * x) + l1 * 2 * x * y], -1)
    t_intr = -np.stack([l0 * sol["xd"] / intr[0], l1 * sol["yd"] / intr[1], l0 / intr[0], l1 / intr[1]], -1)
    return pr.grad.numpy(), t_intr, t_dist


def magnitudes(H, W, intr, dist, poses, inds, g_abs, ndc, view, sol):
    """Per ray, every term on absolute values (fp64): tests/intrinsics_cases.py's `magnitudes` with |dc| = (|x|, |y|, 1), then
    lambda on the adjugate on absolute values over the true determinant -> (pose terms [n, 3, 4], A_i of the intrinsics [n, 4],
    A_i of the distortion [n, 4])."""
    intr = np.asarray(intr, np.float64)
    poses = torch.as_tensor(np.asarray(poses, np.float64)[:, :3, :4])
    n = len(inds)
    vid = torch.as_tensor(sol["vid"])
    xa, ya = torch.as_tensor(np.abs(sol["x"])), torch.as_tensor(np.abs(sol["y"]))
    dc_true = torch.stack([torch.as_tensor(sol["x"]), -torch.as_tensor(sol["y"]), -torch.ones(n, dtype=torch.float64)], -1)
    dc = torch.stack([xa, ya, torch.ones(n, dtype=torch.float64)], -1)
    Rt, R, o = poses[vid][:, :, :3], poses[vid][:, :, :3].abs(), poses[vid][:, :, 3].abs()
    d_true = (Rt * dc_true[:, None, :]).sum(-1)
    d = (R * dc[:, None, :]).sum(-1)
    g = torch.as_tensor(g_abs, dtype=torch.float64)
    go, gd = g[:, 0:3], g[:, 3:6]
    if ndc is not None:
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
    gdc = (gd[:, :, None] * R).sum(1).numpy()  # |g_d|^T |R|
    xa, ya = xa.numpy(), ya.numpy()
    l0 = (sol["da"] * gdc[:, 0] + sol["ba"] * gdc[:, 1]) / sol["det"]
    l1 = (sol["aa"] * gdc[:, 1] + sol["ba"] * gdc[:, 0]) / sol["det"]
    r2, lp = xa * xa + ya * ya, l0 * xa + l1 * ya
    a_dist = np.stack([r2 * lp, r2 * r2 * lp, l0 * 2 * xa * ya + l1 * (r2 + 2 * ya * ya), l0 * (r2 + 2 * xa * xa) + l1 * 2 * xa * ya], -1)
    a_intr = np.stack([l0 * sol["xda"] / intr[0], l1 * sol["yda"] / intr[1], l0 / intr[0], l1 / intr[1]], -1)
    return pose_terms.numpy(), a_intr, a_dist


def vjp_bound(c, n, a_sum):
    return (P.reduction_depth(n) + c) * U32 * a_sum


# ---- the entry points on numpy arrays -------------------------------------------------------------------------------------------
def f32(a):
    return np.ascontiguousarray(a, np.float32)


def select_dist(b, cfg, intr, dist, table, vstride, ld, V, images, n, inds=None):
    use_view, ch = bool(cfg.use_viewdirs), cfg.channels
    dp, di, dn, dk, dd = b.dev(table), b.devopt(images), b.devopt(inds, np.int64), b.devopt(intr), b.dev(f32(dist))
    rays, tgt, used = b.empty((n, 11 if use_view else 8)), b.empty((n, ch)), b.empty((n,), np.int64)
    b.lib.select_rays_views_dist(C.byref(cfg), b.p(dk), b.ptr(dd), V, b.ptr(dp), vstride, ld, b.p(di), b.p(dn), n, b.ptr(rays),
                                 b.ptr(tgt) if images is not None else None, b.ptr(used), b.stream())
    return b.host(rays), (b.host(tgt) if images is not None else None), b.host(used)


def dist_bwd(b, cfg, intr, dist, table, vstride, ld, V, inds, g, g2, stride, want=(True, True, True), mask=None, tmp_slack=0):
    """(g_poses, g_intr, g_dist), None where not wanted."""
    n = len(inds)
    tb = b.lib.dist_grad_views_tmp_bytes(n, V)
    assert tb >= 0
    tmp = b.empty((max(tb // 4, 1) + tmp_slack,))
    outs = [b.empty(shape) if w else None for w, shape in zip(want, ((V, 3, 4), (4,), (4,)))]
    dp, dn, dk, dd = b.dev(table), b.dev(np.ascontiguousarray(inds, np.int64)), b.devopt(intr), b.dev(f32(dist))
    dg, dg2, dm = b.devopt(g), b.devopt(g2), b.devopt(mask, np.uint8)
    b.lib.select_rays_views_dist_bwd(C.byref(cfg), b.p(dk), b.ptr(dd), V, b.ptr(dp), vstride, ld, b.ptr(dn), n, b.p(dg), b.p(dg2), stride,
                                     b.ptr(tmp), tb, b.p(outs[0]), b.p(outs[1]), b.p(outs[2]), b.p(dm), b.stream())
    return tuple(b.host(o) if o is not None else None for o in outs)


def bundle_dist(b, H, W, focal, intr, dist, c2w, pixels=None):
    c2w = f32(c2w)
    n = H * W if pixels is None else len(pixels)
    dc, dp, dk, dd = b.dev(c2w), b.devopt(pixels, np.int64), b.devopt(intr), b.dev(f32(dist))
    ro, rd = b.empty((n, 3)), b.empty((n, 3))
    b.lib.ray_bundle_dist(H, W, float(focal), b.p(dk), b.ptr(dd), b.ptr(dc), c2w.shape[1], b.p(dp), n, b.ptr(ro), b.ptr(rd), b.stream())
    return b.host(ro), b.host(rd)


# ---- 1. the reference against itself (CPU only: no backend) ------------------------------------------------------------------------
def case_reference_against_itself(ndc, view, kappa):
    """Central differences in fp64, relative 1e-6, on every entry of g_dist and g_intr and on the pose entries; and the per-ray
    terms of `ray_terms` sum to the autograd result."""
    V, H, W = V3, H3, W3
    poses = IC.scene3(ndc).astype(np.float64)[:, :3, :4]
    intr, dist = INTR3.astype(np.float64), KAPPAS[kappa].astype(np.float64)
    nd = dict(near=1.0, cw=-2.0 * FOCAL3 / W, ch=-2.0 * FOCAL3 / H, two_near=2.0, neg_two_near=-2.0) if ndc else None
    rng = np.random.default_rng(31)
    inds = rng.permutation(V * H * W)[:60].astype(np.int64)
    g = rng.normal(size=(len(inds), 11))

    def loss(i, k, p):
        with torch.no_grad():
            rays = rays64(H, W, torch.tensor(i), torch.tensor(k), torch.tensor(p), inds, nd, view)
            return float((rays * torch.as_tensor(g[:, :rays.shape[1]])).sum())
    gp, gi, gd = oracle_vjp(H, W, intr, dist, poses, inds, g, nd, view)
    h = 1e-6
    for name, base, grad in (("dist", dist, gd), ("intr", intr, gi), ("poses", poses, gp)):
        flat = base.reshape(-1)
        scale = float(np.abs(grad).max())
        for j in range(flat.size):
            up, dn = flat.copy(), flat.copy()
            up[j] += h
            dn[j] -= h
            args = dict(dist=dist, intr=intr, poses=poses)
            args[name] = up.reshape(base.shape)
            lu = loss(args["intr"], args["dist"], args["poses"])
            args[name] = dn.reshape(base.shape)
            ld = loss(args["intr"], args["dist"], args["poses"])
            fd = (lu - ld) / (2 * h)
            assert abs(fd - grad.reshape(-1)[j]) <= 1e-6 * scale, (name, j, fd, grad.reshape(-1)[j])
    sol = solved(H, W, intr, dist, inds)
    tp, ti, td = ray_terms(H, W, intr, dist, poses, inds, g, nd, view, sol)
    assert np.allclose(ti.sum(0), gi, rtol=0, atol=1e-10 * np.abs(gi).max()) and np.allclose(td.sum(0), gd, rtol=0, atol=1e-10 * np.abs(gd).max())
    for v in range(V):
        assert np.allclose(tp[sol["vid"] == v].sum(0), gp[v], rtol=0, atol=1e-10 * np.abs(gp).max())
    assert np.all(np.abs(gd) > 0) and np.all(np.abs(gi) > 0)


def domains():
    """The (intrinsics, H, W) of every scene the cases use."""
    return ((INTR3, H3, W3), (IC.BIG["intr"], IC.BIG["H"], IC.BIG["W"]))


def case_iteration_count():
    """In fp64, on the corners of every tested domain and for both coefficient sets, NERFHIP_UNDISTORT_ITERS - 2 Newton steps are
    already below 1e-12: the two steps the kernel runs beyond that are spent at the fp32 floor."""
    iters = undistort_iters()
    assert iters >= 4
    for intr, H, W in domains():
        inds = np.array([0, H - 1, (W - 1) * H, H * W - 1], dtype=np.int64)   # (row, col) = (0, 0), (H-1, 0), (0, W-1), (H-1, W-1)
        _, xd, yd, _, _ = (t.numpy() for t in observed(H, W, intr, inds))
        for k in KAPPAS.values():
            x, y, low = newton64(xd, yd, k.astype(np.float64), iters - 2)
            res = residual(x, y, xd, yd, k.astype(np.float64))
            assert np.all(res < 1e-12) and np.all(low >= 0.5), (res, low)


def case_domain():
    """By the reference alone: on every pixel of every tested scene det J >= 1/2 along the Newton path, and the determinant on
    absolute values is at most RHO times the true one (the C_DIST count relies on it), and || |J^-1| ||_inf >= 1/6 (the C_UND count)."""
    for intr, H, W in domains():
        inds = np.arange(H * W, dtype=np.int64)
        for k in KAPPAS.values():
            sol = solved(H, W, intr, k, inds)
            assert np.all(sol["low"] >= 0.5) and np.all(sol["det"] >= 0.5), float(sol["low"].min())
            assert np.all(sol["det_abs"] <= RHO * sol["det"]), float((sol["det_abs"] / sol["det"]).max())
            assert np.all(sol["inv_norm"] >= 1.0 / 6.0), float(sol["inv_norm"].min())


# ---- 2. forward rows against fp64 -----------------------------------------------------------------------------------------------
def rows_scale(poses, sol, ndc, view):
    """tests/intrinsics_cases.py's rows_scale with |dc| = (|x|, |y|, 1) (numpy fp64)."""
    vid = sol["vid"]
    n = len(vid)
    dca = np.stack([np.abs(sol["x"]), np.abs(sol["y"]), np.ones(n)], -1)
    dc = np.stack([sol["x"], -sol["y"], -np.ones(n)], -1)
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
    cols = [o, d, np.full((n, 1), 2.0), np.full((n, 1), 6.0)]
    if view:
        cols.append(src / np.linalg.norm(d_true, axis=-1, keepdims=True))
    return np.concatenate(cols, -1)


def forward_bound(poses, sol, ndc, view):
    """Per entry of every row: 4 * 2^-23 * rows_scale + the image of the solve's error box (module docstring)."""
    pr = torch.as_tensor(poses[sol["vid"]])
    at = lambda dx, dy: rows_from(torch.as_tensor(np.stack([sol["x"] + dx, sol["y"] + dy], -1)), pr, ndc, view).numpy()  # noqa: E731
    base = at(0.0, 0.0)
    moved = np.zeros_like(base)
    for sx, sy in CORNERS:
        moved = np.maximum(moved, np.abs(at(sx * sol["e"], sy * sol["e"]) - base))
    return 4 * 2.0 ** -23 * rows_scale(poses, sol, ndc, view) + moved, base


def case_forward_fp64(b, ndc, view, kappa, with_intr=True):
    """Every pixel of every view of the 3 x 5 x 7 scene against the fp64 restatement under the forward bound; by the reference
    alone: det J >= 1/2 on every pixel, and at least 90 % of the rows move, between dist and 0, by at least 1000 x the bound in one
    of their entries.  Returns the worst measured error over its bound."""
    V, H, W = V3, H3, W3
    dist = KAPPAS[kappa]
    intr = INTR3 if with_intr else IC.centred(H, W, FOCAL3)
    poses = IC.scene3(ndc)
    cfg = VC.cfg_of(b, H, W, FOCAL3, ndc, view, 3, seed=5, step=2, first=0)
    n = V * H * W
    rays, _, used = select_dist(b, cfg, intr if with_intr else None, dist, poses, 16, 4, V, None, n)
    assert sorted(used.tolist()) == list(range(n)) and np.all(np.isfinite(rays))
    nd = IC.ndc_consts(cfg) if ndc else None
    p64 = poses[:, :3, :4].astype(np.float64)
    sol = solved(H, W, intr, dist, used)
    assert np.all(sol["low"] >= 0.5)
    tol, want = forward_bound(p64, sol, nd, view)
    ref = rays64(H, W, torch.tensor(intr.astype(np.float64)), torch.tensor(dist.astype(np.float64)), torch.tensor(p64), used, nd, view)
    assert np.allclose(ref.numpy(), want, rtol=0, atol=1e-13)
    err = np.abs(rays.astype(np.float64) - want)
    live = tol > 0
    ratio = float((err[live] / tol[live]).max())
    print("distortion rows vs fp64 (%s, ndc %d, viewdirs %d, intr %d): worst error / bound = %.3f" % (kappa, ndc, view, with_intr, ratio))
    # teeth, by the reference alone
    zero = solved(H, W, intr, ZERO4, used)
    plain = rows_from(torch.as_tensor(np.stack([zero["x"], zero["y"]], -1)), torch.as_tensor(p64[sol["vid"]]), nd, view).numpy()
    moved = np.any(np.abs(plain - want) >= 1000 * tol, axis=1)
    assert moved.mean() >= 0.9, float(moved.mean())
    assert np.all(err <= tol), ratio
    return ratio


def case_bundle(b):
    """nerfhip_ray_bundle_dist: dist = 0 gives the bits of nerfhip_ray_bundle (intr NULL) and of nerfhip_ray_bundle_intr; under
    distortion its directions are the selection's pre-NDC ones, bit for bit (one shared routine), whole image and pixel list."""
    H, W, focal = H3, W3, FOCAL3
    c2w = VC.pose(5)
    for pixels in (None, np.array([34, 0, 7, 6, 13, 13, 20], dtype=np.int64)):
        wo, wd = b.ray_bundle(H, W, focal, c2w, pixels)
        ro, rd = bundle_dist(b, H, W, focal, None, ZERO4, c2w, pixels)
        assert np.all(np.isfinite(rd)) and np.array_equal(bits(ro), bits(wo)) and np.array_equal(bits(rd), bits(wd))
        wo, wd = IC.bundle_intr(b, H, W, INTR3, c2w, pixels)
        ro, rd = bundle_dist(b, H, W, 0.0, INTR3, ZERO4, c2w, pixels)
        assert np.array_equal(bits(ro), bits(wo)) and np.array_equal(bits(rd), bits(wd))
    pix = np.arange(H * W, dtype=np.int64)
    k = (pix % W) * H + pix // W   # the select index of pixel (row, col) = (pix // W, pix % W)
    cfg = VC.cfg_of(b, H, W, focal, False, False)
    for intr in (INTR3, None):
        ro, rd = bundle_dist(b, H, W, focal, intr, KAPPA_BARREL, c2w, pix)
        rows, _, _ = select_dist(b, cfg, intr, KAPPA_BARREL, c2w[None], 16, 4, 1, None, H * W, k)
        assert np.array_equal(bits(ro), bits(rows[:, 0:3])) and np.array_equal(bits(rd), bits(rows[:, 3:6]))
        plain = IC.bundle_intr(b, H, W, INTR3, c2w, pix)[1] if intr is not None else b.ray_bundle(H, W, focal, c2w, pix)[1]
        assert not np.array_equal(bits(rd), bits(plain))


# ---- 3. the VJP -----------------------------------------------------------------------------------------------------------------
def vjp_batch(n, ndc, view, two, stride, big, kappa, H, W, V, intr, poses, nd):
    """The batch of a VJP case: the first of 20 seeds at which, by the reference alone, every exact entry of g_dist is at least 100 x
    its bound (a random sum can come out small against its terms' magnitudes; such a draw would let a zero result pass)."""
    hw = H * W
    dist = KAPPAS[kappa]
    for attempt in range(20):
        rng = np.random.default_rng(2000 + 16 * n + 8 * big + 4 * ndc + 2 * view + two + 100000 * attempt)
        inds = rng.integers(0, V * hw, size=n).astype(np.int64)
        g = rng.normal(size=(n, stride)).astype(np.float32)
        g2 = rng.normal(size=(n, stride)).astype(np.float32) if two else None
        gsum = g.astype(np.float64) + (g2.astype(np.float64) if two else 0.0)
        gmag = np.abs(g.astype(np.float64)) + (np.abs(g2.astype(np.float64)) if two else 0.0)
        sol = solved(H, W, intr, dist, inds)
        exact = oracle_vjp(H, W, intr, dist, poses, inds, gsum, nd, view)
        mags = magnitudes(H, W, intr, dist, poses, inds, gmag, nd, view, sol)
        bound_d = vjp_bound(C_DIST, n, mags[2].sum(0))
        if np.all(np.abs(exact[2]) >= 100 * bound_d):
            break
    return inds, g, g2, sol, exact, mags


def case_vjp(b, n, ndc, view, two, stride, big=False, kappa=None):
    """g_dist, g_intr and g_poses against fp64 autograd under their bounds; views interleave (indices from rng.integers)."""
    kappa = kappa or ("pincushion" if two else "barrel")
    V, H, W, focal, intr, poses = IC.vjp_scene(big, ndc)
    cfg = VC.cfg_of(b, H, W, focal, ndc, view)
    nd = IC.ndc_consts(cfg) if ndc else None
    dist = KAPPAS[kappa]
    inds, g, g2, sol, (want_p, want_i, want_d), (pose_terms, a_i, a_d) = vjp_batch(
        n, ndc, view, two, stride, big, kappa, H, W, V, intr, poses, nd)
    gp, gi, gd = dist_bwd(b, cfg, intr, dist, poses, 16, 4, V, inds, g, g2, stride)
    assert gp.shape == (V, 3, 4) and gi.shape == (4,) and gd.shape == (4,)
    assert np.all(np.isfinite(gp)) and np.all(np.isfinite(gi)) and np.all(np.isfinite(gd))
    worst = {}
    for name, got, want, c, a in (("g_dist", gd, want_d, C_DIST, a_d), ("g_intr", gi, want_i, C_INTRP, a_i)):
        bound = vjp_bound(c, n, a.sum(0))
        err = np.abs(got.astype(np.float64) - want)
        print("%s, n = %d (%s, ndc %d, viewdirs %d, two %d): exact %s, error / bound %s, |exact| / bound %s"
              % (name, n, kappa, ndc, view, two, want, err / bound, np.abs(want) / bound))
        if name == "g_dist":
            assert np.all(np.abs(want) >= 100 * bound), (want, bound)   # not vacuous: a zero, swapped or sign-flipped result fails
        assert np.all(err <= bound), (name, err / bound)
        worst[name] = float((err / bound).max())
    vid = inds // (H * W)
    for v in range(V):
        rows = np.nonzero(vid == v)[0]
        if len(rows) == 0:
            assert np.array_equal(bits(gp[v]), np.zeros((3, 4), np.uint32))
            continue
        pb = P.bound(len(rows), pose_terms[rows].sum(0))
        pe = np.abs(gp[v].astype(np.float64) - want_p[v])
        assert np.all(pe <= pb), (v, float((pe / np.maximum(pb, 1e-300)).max()))
    # each output has the same bits whether or not the others are asked; another tmp size and the embedded table change nothing
    for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        got = dist_bwd(b, cfg, intr, dist, poses, 16, 4, V, inds, g, g2, stride, want=want, tmp_slack=sum(want))
        for w, o, full in zip(want, got, (gp, gi, gd)):
            assert (o is None) == (not w) and (o is None or np.array_equal(bits(o), bits(full))), want
    table, vs, ld = VC.pose_table(poses, "embedded")
    for o, full in zip(dist_bwd(b, cfg, intr, dist, table, vs, ld, V, inds, g, g2, stride, tmp_slack=7), (gp, gi, gd)):
        assert np.array_equal(bits(o), bits(full))
    return worst


# ---- 4. the bit contracts -------------------------------------------------------------------------------------------------------
def case_zero_selection_bits(b, ndc, view, layout):
    """dist = (0, 0, 0, 0) gives the rows of the call without dist: against nerfhip_select_rays_views_intr (intr given) and
    nerfhip_select_rays_views (intr NULL), the whole population of the 3 x 5 x 7 scene; a -0.0 coefficient as well."""
    V, H, W, focal = V3, H3, W3, FOCAL3
    poses = IC.scene3(ndc)
    images = np.random.default_rng(12).random((V, H, W, 3), dtype=np.float32)
    cfg = VC.cfg_of(b, H, W, focal, ndc, view, 3, seed=5, step=2, first=0)
    table, vs, ld = VC.pose_table(poses, layout)
    n = V * H * W
    for intr in (INTR3, IC.centred(H, W, focal), None):
        want = IC.select_intr(b, cfg, intr, table, vs, ld, V, images, n) if intr is not None else \
            VC.select_views(b, cfg, table, vs, ld, V, images, n)
        for zero in (ZERO4, np.array([-0.0, 0.0, -0.0, 0.0], np.float32)):
            rays, tgt, used = select_dist(b, cfg, intr, zero, table, vs, ld, V, images, n)
            assert np.all(np.isfinite(rays)) and np.array_equal(used, want[2])
            assert np.array_equal(rays, want[0]) and np.array_equal(bits(rays), bits(want[0])) and np.array_equal(bits(tgt), bits(want[1]))
    moved = select_dist(b, cfg, INTR3, KAPPA_BARREL, table, vs, ld, V, images, n)[0]
    assert not np.array_equal(bits(moved), bits(IC.select_intr(b, cfg, INTR3, table, vs, ld, V, images, n)[0]))


def case_zero_vjp_bits(b, n, ndc, view):
    """dist = 0 gives the g_poses and g_intr of nerfhip_select_rays_views_intr_bwd (and, intr NULL, the g_poses of
    nerfhip_select_rays_views_bwd) bit for bit."""
    V, H, W, focal = V3, H3, W3, FOCAL3
    poses = IC.scene3(ndc)
    rng = np.random.default_rng(177 + n)
    cfg = VC.cfg_of(b, H, W, focal, ndc, view)
    inds = rng.integers(0, V * H * W, size=n).astype(np.int64)
    g, g2 = rng.normal(size=(n, 11)).astype(np.float32), rng.normal(size=(n, 11)).astype(np.float32)
    gp, gi, gd = dist_bwd(b, cfg, INTR3, ZERO4, poses, 16, 4, V, inds, g, g2, 11)
    want_p, want_i = IC.intr_bwd(b, cfg, INTR3, poses, 16, 4, V, inds, g, g2, 11)
    assert np.all(np.isfinite(gp)) and float(np.abs(gp).sum()) > 0 and np.all(gi != 0) and np.all(np.isfinite(gd)) and np.all(gd != 0)
    assert np.array_equal(gp, want_p) and np.array_equal(bits(gp), bits(want_p))
    assert np.array_equal(gi, want_i) and np.array_equal(bits(gi), bits(want_i))
    gp0, none_i, _ = dist_bwd(b, cfg, None, ZERO4, poses, 16, 4, V, inds, g, g2, 11, want=(True, False, True))
    assert none_i is None and np.array_equal(bits(gp0), bits(VC.views_bwd(b, cfg, poses, 16, 4, V, inds, g, g2, 11)))


# ---- 5. masks, edges, refusals ----------------------------------------------------------------------------------------------------
MASKS = [tuple((m >> k) & 1 for k in range(4)) for m in range(16)]


def case_mask(b, mask):
    """A masked entry of g_dist is an exact +0.0; the others keep the bits of the unmasked call; g_poses and g_intr do not see the
    mask.  Three Adam steps on g_dist: a masked coefficient keeps its bits, a learned one moves."""
    V, H, W, n = V3, H3, W3, 300
    poses = IC.scene3(False)
    cfg = VC.cfg_of(b, H, W, FOCAL3, False, True)
    rng = np.random.default_rng(900)
    inds = rng.integers(0, V * H * W, size=n).astype(np.int64)
    g = rng.normal(size=(n, 11)).astype(np.float32)
    full = dist_bwd(b, cfg, INTR3, KAPPA_BARREL, poses, 16, 4, V, inds, g, None, 11)
    assert np.all(full[2] != 0)
    m8 = np.array(mask, dtype=np.uint8)
    got = dist_bwd(b, cfg, INTR3, KAPPA_BARREL, poses, 16, 4, V, inds, g, None, 11, mask=m8)
    assert np.array_equal(bits(got[0]), bits(full[0])) and np.array_equal(bits(got[1]), bits(full[1]))
    for k in range(4):
        assert bits(got[2][k:k + 1])[0] == (bits(full[2][k:k + 1])[0] if mask[k] else 0), (k, got[2])
    p, m, v = KAPPA_BARREL.copy(), np.zeros(4, np.float32), np.zeros(4, np.float32)
    for step in (1, 2, 3):
        gd = dist_bwd(b, cfg, INTR3, p, poses, 16, 4, V, inds, g, None, 11, want=(False, False, True), mask=m8)[2]
        p, m, v = b.adam_step(p, gd, m, v, 1e-3, step)
    for k in range(4):
        assert (bits(p[k:k + 1])[0] == bits(KAPPA_BARREL[k:k + 1])[0]) == (not mask[k]), (k, p)


def case_vjp_edges(b):
    """n = 0: exact zeros, every output written; a view without rays: a zero pose row; an index outside [0, V H W): dropped."""
    V, H, W, hw = V3, H3, W3, H3 * W3
    poses = IC.scene3(False)
    cfg = VC.cfg_of(b, H, W, FOCAL3, False, True)
    lib = b.lib
    assert lib.dist_grad_views_tmp_bytes(0, V) == 0 and lib.dist_grad_views_tmp_bytes(-1, V) == -1
    assert lib.dist_grad_views_tmp_bytes(5, 0) == -1
    assert lib.dist_grad_views_tmp_bytes(700, 4) == lib.intr_grad_views_tmp_bytes(700, 4) + 4 * 4 * P.wgs(700)
    gp, gi, gd = b.empty((V, 3, 4)), b.empty((4,)), b.empty((4,))
    dp, dk, dd = b.dev(poses), b.dev(INTR3), b.dev(KAPPA_BARREL)
    lib.select_rays_views_dist_bwd(C.byref(cfg), b.ptr(dk), b.ptr(dd), V, b.ptr(dp), 16, 4, None, 0, None, None, 11, None, 0, b.ptr(gp),
                                   b.ptr(gi), b.ptr(gd), None, b.stream())
    for o, shape in ((gp, (V, 3, 4)), (gi, 4), (gd, 4)):
        assert np.array_equal(bits(b.host(o)), np.zeros(shape, np.uint32))
    rng = np.random.default_rng(5)
    n = 300
    inds = (rng.choice([0, 2], size=n) * hw + rng.integers(0, hw, size=n)).astype(np.int64)
    g = rng.normal(size=(n, 11)).astype(np.float32)
    gp, gi, gd = dist_bwd(b, cfg, INTR3, KAPPA_BARREL, poses, 16, 4, V, inds, g, None, 11)
    assert np.array_equal(bits(gp[1]), np.zeros((3, 4), np.uint32))
    assert float(np.abs(gp[0]).sum()) > 0 and float(np.abs(gp[2]).sum()) > 0 and np.all(gi != 0) and np.all(gd != 0)
    # dropped indices: g_poses is that of the batch without them; g_intr and g_dist are those of the batch with their rows zeroed
    out = np.array([3, 17, 130, 255, 256, 299])
    bad = inds.copy()
    bad[out] = np.array([-1, V * hw, V * hw + 9, -hw, 2 ** 40, -2 ** 40])
    gp_b, gi_b, gd_b = dist_bwd(b, cfg, INTR3, KAPPA_BARREL, poses, 16, 4, V, bad, g, None, 11)
    keep = np.setdiff1d(np.arange(n), out)
    gp_k = dist_bwd(b, cfg, INTR3, KAPPA_BARREL, poses, 16, 4, V, inds[keep], np.ascontiguousarray(g[keep]), None, 11)[0]
    gz = g.copy()
    gz[out] = 0.0
    _, gi_z, gd_z = dist_bwd(b, cfg, INTR3, KAPPA_BARREL, poses, 16, 4, V, inds, gz, None, 11)
    assert np.all(np.isfinite(gp_b)) and np.all(np.isfinite(gi_b)) and np.all(np.isfinite(gd_b))
    assert np.array_equal(bits(gp_b), bits(gp_k)) and np.array_equal(bits(gi_b), bits(gi_z)) and np.array_equal(bits(gd_b), bits(gd_z))
    assert not np.array_equal(bits(gd_b), bits(gd))


def case_refusals(b):
    lib = b.lib
    V, H, W = 3, 4, 4
    raw_s, raw_b, raw_r = (lib._dll.nerfhip_select_rays_views_dist, lib._dll.nerfhip_select_rays_views_dist_bwd,
                           lib._dll.nerfhip_ray_bundle_dist)
    cfg = VC.cfg_of(b, H, W, 3.0, False, True)
    poses = b.dev(np.stack([np.eye(4, dtype=np.float32)] * V))
    intr, dist = b.dev(IC.centred(H, W, 3.0)), b.dev(KAPPA_BARREL)
    rays, used = b.empty((4, 11)), b.empty((4,), np.int64)
    inds = b.dev(np.arange(4, dtype=np.int64))
    g = b.dev(np.zeros((4, 11), np.float32))
    tb = lib.dist_grad_views_tmp_bytes(4, V)
    tmp, gp, gi, gd = b.empty((tb // 4,)), b.empty((V, 3, 4)), b.empty((4,)), b.empty((4,))
    pk, pd, pp, pr, pu, pi, pg, pt, st = (b.ptr(intr), b.ptr(dist), b.ptr(poses), b.ptr(rays), b.ptr(used), b.ptr(inds), b.ptr(g),
                                          b.ptr(tmp), b.stream())
    pgp, pgi, pgd = b.ptr(gp), b.ptr(gi), b.ptr(gd)

    def refused(rc, *words):
        msg = lib._dll.nerfhip_last_error().decode()
        assert rc == ERR_ARG and all(w in msg for w in words), (rc, msg, words)

    ok = lambda c=cfg, k=pk, d=pd, v=V, p=pp, vs=16, ld=4, n=4, r=pr: raw_s(C.byref(c) if c else None, k, d, v, p, vs, ld, None, None,  # noqa: E731
                                                                            n, r, None, pu, st)
    assert ok() == 0 and ok(k=None) == 0
    refused(ok(d=None), "select_rays_views_dist", "dist")
    refused(ok(ld=3), "select_rays_views_dist", "pose_ld")
    refused(ok(vs=11), "select_rays_views_dist", "pose_view_stride")
    refused(ok(v=0), "select_rays_views_dist", "num_views")
    refused(ok(c=None), "select_rays_views_dist")
    refused(ok(p=None), "select_rays_views_dist")
    refused(ok(r=None), "select_rays_views_dist")
    okb = lambda c=cfg, k=pk, d=pd, v=V, p=pp, vs=16, ld=4, i=pi, gs=11, t=pt, tbytes=tb, o=pgp, oi=pgi, od=pgd: raw_b(  # noqa: E731
        C.byref(c) if c else None, k, d, v, p, vs, ld, i, 4, pg, None, gs, t, tbytes, o, oi, od, None, st)
    assert okb() == 0 and okb(o=None) == 0 and okb(oi=None) == 0 and okb(od=None) == 0 and okb(k=None) == 0
    assert okb(o=None, oi=None) == 0 and okb(oi=None, od=None) == 0
    refused(okb(d=None), "select_rays_views_dist_bwd", "dist")
    refused(okb(o=None, oi=None, od=None), "select_rays_views_dist_bwd", "g_poses", "g_intr", "g_dist")
    refused(okb(tbytes=tb - 4), "select_rays_views_dist_bwd", "nerfhip_dist_grad_views_tmp_bytes")
    refused(okb(tbytes=lib.intr_grad_views_tmp_bytes(4, V)), "select_rays_views_dist_bwd", "tmp")
    refused(okb(t=None), "select_rays_views_dist_bwd", "tmp")
    refused(okb(ld=3), "select_rays_views_dist_bwd", "pose_ld")
    refused(okb(vs=11), "select_rays_views_dist_bwd", "pose_view_stride")
    refused(okb(v=VC.L_MAX_VIEWS + 1), "select_rays_views_dist_bwd", "num_views")
    refused(okb(gs=8), "select_rays_views_dist_bwd", "g_rays_stride")
    refused(okb(i=None), "select_rays_views_dist_bwd")
    c2w = b.dev(np.eye(4, dtype=np.float32))
    ro, rd = b.empty((H * W, 3)), b.empty((H * W, 3))
    okr = lambda k=pk, d=pd, ld=4, n=H * W: raw_r(H, W, 3.0, k, d, b.ptr(c2w), ld, None, n, b.ptr(ro), b.ptr(rd), st)  # noqa: E731
    assert okr() == 0 and okr(k=None) == 0
    refused(okr(d=None), "ray_bundle_dist", "dist")
    refused(okr(ld=3), "ray_bundle_dist")
    refused(okr(n=3), "ray_bundle_dist", "height*width")
