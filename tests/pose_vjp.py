"""fp64 references and the error bound of the pose VJP (nerfhip_ray_bundle_bwd / nerfhip_select_rays_bwd), shared by
tests/test_pose_grad.py (emulator) and tests/test_gpu_pose.py (MI355X).

Reference value: torch autograd in fp64 through the oracle's get_ray_bundle -> (select) -> ndc_rays -> pack_rays, i.e.
what the reference's own torch code gives a pose that requires grad.

Bound, per entry of the 3 x 4 result, derived from the kernel's arithmetic (csrc/dataio.hip, k_pose_vjp_part / _sum):

    |kernel - exact| <= (D(n) + C_RAY) * 2^-24 * sum_i A_i

* The sum over rays is a tree of fp32 additions of depth D(n): with G = min(ceil(n / 256), 1024) workgroups, a thread adds
  ceil(n / 256 G) ray terms in sequence, a wave butterfly adds 6 levels, the 4 waves of a workgroup 3 more, a lane of the
  final workgroup ceil(G / 64) partials in sequence and a last butterfly 6 levels.  A sum evaluated along a tree of depth D
  is off by at most gamma_D * sum_i |x_i| (Higham, Accuracy and Stability of Numerical Algorithms, 4.2), gamma_D ~ D u.
* Each ray term x_i is itself an fp32 expression of the pose and the cotangents.  Evaluated with the same operations on
  the absolute values of its operands (subtractions as additions: A_i, computed here in fp64) it is off by at most
  C_RAY u A_i, where C_RAY bounds the number of roundings along the longest dependency chain of the per-ray stage:
  camera direction 2, pre-NDC direction 4, t 2, p 2, 1/pz 1, d/d(pz) 6, d/dt 3, d/d(dz) 5, the viewdir normalisation's
  backward 12 (norm 4, u 1, u . g 3, subtract / scale 2, divide 1, add 1), the coarse + fine add 1, the product with the
  camera direction 1 -- 26 on the NDC + viewdirs path (fewer on every other path) -- plus 2 for the fp32 focal length
  and NDC constants the kernel reads against the fp64 ones of the oracle: 28, taken as 32.
  (The abs-evaluation bounds a division's error only while its denominator is not itself the result of cancellation:
  dz ~ -1 and pz = -near hold for the forward-facing cameras of these tests, as for every LLFF scene.)
"""
import math

import numpy as np
import torch

import nerf_oracle as O

U32 = 2.0 ** -24
C_RAY = 32


def wgs(n):
    return 0 if n <= 0 else min(-(-n // 256), 1024)


def reduction_depth(n):
    g = wgs(n)
    if g == 0:
        return 0
    return -(-n // (256 * g)) + 6 + 3 + -(-g // 64) + 6


def bound(n, mag):
    """Per-entry bound (3 x 4 fp64) of the kernel's result for n rays of magnitude sum `mag`."""
    return (reduction_depth(n) + C_RAY) * U32 * mag


def _cam(H, W, focal, rows, cols):
    cols = cols.double()
    rows = rows.double()
    return torch.stack([(cols - W * 0.5) / focal, -(rows - H * 0.5) / focal, -torch.ones_like(cols)], -1)


def pixel_rc(H, W, ids, select):
    ids = torch.as_tensor(ids, dtype=torch.int64)
    return (ids % H, ids // H) if select else (ids // W, ids % W)


def oracle_bundle_vjp(H, W, focal, c2w, pixels, g_o, g_d):
    """fp64 autograd of the oracle's get_ray_bundle (rows of `pixels`, or the whole image) -> 3 x 4."""
    p = torch.as_tensor(np.asarray(c2w)[:3, :4], dtype=torch.float64).clone().requires_grad_(True)
    ro, rd = O.get_ray_bundle(H, W, focal, p)
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    if pixels is not None:
        idx = torch.as_tensor(pixels, dtype=torch.int64)
        ro, rd = ro[idx], rd[idx]
    s = 0.0
    if g_o is not None:
        s = s + (ro * torch.as_tensor(g_o, dtype=torch.float64)).sum()
    if g_d is not None:
        s = s + (rd * torch.as_tensor(g_d, dtype=torch.float64)).sum()
    s.backward()
    return p.grad.numpy()


def oracle_select_vjp(H, W, focal, c2w, inds, g_rays, ndc, view, near=2.0, far=6.0):
    """fp64 autograd of get_ray_bundle -> the rows the select indices address -> ndc_rays(near = 1) -> pack_rays."""
    p = torch.as_tensor(np.asarray(c2w)[:3, :4], dtype=torch.float64).clone().requires_grad_(True)
    ro, rd = O.get_ray_bundle(H, W, focal, p)
    r, c = pixel_rc(H, W, inds, True)
    ro, rd = ro[r, c], rd[r, c]
    src = rd
    if ndc:
        ro, rd = O.ndc_rays(H, W, focal, 1.0, ro, rd)
    rays = O.pack_rays(ro, rd, near, far, src if view else None)
    (rays * torch.as_tensor(g_rays[:, :rays.shape[1]], dtype=torch.float64)).sum().backward()
    return p.grad.numpy()


def magnitude(H, W, focal, c2w, ids, select, g_o=None, g_d=None, g_rays=None, ndc=False, view=False):
    """sum_i A_i (3 x 4 fp64): each ray term evaluated on absolute values (see the module docstring)."""
    c2w = torch.as_tensor(np.asarray(c2w)[:3, :4], dtype=torch.float64)
    R, t = c2w[:, :3].abs(), c2w[:, 3].abs()
    n = len(ids) if ids is not None else H * W
    ids = torch.arange(n) if ids is None else torch.as_tensor(ids, dtype=torch.int64)
    rows, cols = pixel_rc(H, W, ids, select)
    dc = _cam(H, W, focal, rows, cols).abs()
    if not select:
        go = torch.zeros(n, 3, dtype=torch.float64) if g_o is None else torch.as_tensor(g_o, dtype=torch.float64).abs()
        gd = torch.zeros(n, 3, dtype=torch.float64) if g_d is None else torch.as_tensor(g_d, dtype=torch.float64).abs()
    else:
        g = torch.as_tensor(g_rays, dtype=torch.float64).abs()
        d_true = _cam(H, W, focal, rows, cols) @ c2w[:, :3].T
        d = dc @ R.T                                        # |R| |dc|
        o = t.expand(n, 3)
        go, gd = g[:, 0:3], g[:, 3:6]
        if ndc:
            cw, ch, near = abs(-1.0 / (W / (2.0 * focal))), abs(-1.0 / (H / (2.0 * focal))), 1.0
            dz = d_true[:, 2].abs()                        # (|dz| ~ 1: no cancellation, module docstring)
            tt = (near + o[:, 2]) / dz
            px, py = o[:, 0] + tt * d[:, 0], o[:, 1] + tt * d[:, 1]
            ipz = 1.0 / near                               # (pz = -near)
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
    out = torch.zeros(3, 4, dtype=torch.float64)
    out[:, :3] = gd.T @ dc
    out[:, 3] = go.sum(0)
    return out.numpy()


def rodrigues(w):
    """SO(3) exponential of an axis-angle 3-vector (differentiable; small-angle safe)."""
    th2 = (w * w).sum()
    small = th2 <= 1e-12
    th2s = torch.where(small, torch.ones_like(th2), th2)   # (no 0/0 in the branch torch.where does not select: its gradient
    th = torch.sqrt(th2s)                                  # would be NaN too)
    K = torch.zeros(3, 3, dtype=w.dtype, device=w.device)
    K = K + torch.stack([torch.stack([0 * w[0], -w[2], w[1]]), torch.stack([w[2], 0 * w[0], -w[0]]),
                         torch.stack([-w[1], w[0], 0 * w[0]])])
    a = torch.where(small, 1.0 - th2 / 6.0, torch.sin(th) / th)
    b = torch.where(small, 0.5 - th2 / 24.0, (1.0 - torch.cos(th)) / th2s)
    return torch.eye(3, dtype=w.dtype, device=w.device) + a * K + b * (K @ K)


def rot_angle_deg(R):
    c = (np.trace(np.asarray(R, dtype=np.float64)) - 1.0) / 2.0
    return math.degrees(math.acos(max(-1.0, min(1.0, c))))
