"""Cases of the robust photometric loss (include/nerfhip.h nerfhip_robust_loss_fwd_bwd, csrc/reg/robust.hip) and of its cotangent through
the fused backward, shared by the emulator suite (tests/test_robust.py) and the GPU suite (tests/test_gpu_robust.py).  Every case drives
the C ABI through a backend's library handle (tests/backends.py).

The definition is restated here independently of the kernel (robust_rho, robust_reference): the header's table in torch, autograd for
the cotangent, the mask of a trim as a constant.

Bounds of this file, and where they come from:

  spread_cases.held_to_yardstick (SPREAD_YARDSTICK / SPREAD_FLOOR, with their reasons): `loss`, `g_rgb` and `resid_out` may be no further
                    from the fp64 run of the formulas than the SAME formulas run in torch fp32 are, x 2, plus 4 x 2^-24 of the quantity's
                    largest magnitude in the case.  Each output is held on its own.  With a trim, `loss` and `g_rgb` are compared under
                    the kernel's OWN mask (a ray whose residual sits within rounding of tau may fall on either side in another
                    precision); the mask itself is held exactly against the kernel's own residuals: tau is the kk-th smallest of
                    resid_out bit for bit, mask == !(resid_out > tau), kept == count / n.
  render cases      tolerances.py `tf.grad.filtered`, `relu_margin` and `unit.compact_vs_dense`, as matte_cases.py uses them: where the
                    oracle's OWN fp32 autograd is further from its fp64 run than `tf.grad.filtered`, that tensor's bound is 2 x that fp32
                    distance (printed).
"""
import math

import numpy as np
import torch

import nerf_oracle as O
import nerf_pytorch_amd._lib as L
import spread_cases as SC
import tolerances as TL

f32 = np.float32
KINDS = {"l2": 0, "l1": 1, "huber": 2, "charbonnier": 3, "relative": 4}
# (kind, param) of the kernel cases: delta = 0.3 splits uniform differences about in half; the two eps are the papers' orders
KERNEL_KINDS = ((0, 0.0), (1, 0.0), (2, 0.3), (3, 1e-3), (4, 1e-3))
SHAPES_N = (1, 2, 63, 64, 65, 1023, 1025, 3073)   # the wave edges, the block edge, a thread with a ragged last element
STRIDES = (3, 7)
ERR_ARG = -1


# ---- the definition, in torch ----------------------------------------------------------------------------------------------------
def robust_rho(rgb, tgt, kind, param):
    """rho [n, 3] of the header's table, differentiable in rgb, in its dtype (the relative kind's p is held constant)."""
    d = rgb - tgt.detach().to(rgb.dtype)[:, :3]
    a = d.abs()
    if kind == 0:
        return d * d
    if kind == 1:
        return a
    if kind == 2:
        return torch.where(a <= param, d * d, param * (2.0 * a - param))
    if kind == 3:
        return torch.sqrt(d * d + param * param) - param
    if kind == 4:
        return d * d / (rgb.detach() + param) ** 2
    raise ValueError(kind)


def keep_count(keep, n):
    """kk of the header: min(n, max(1, ceil((double)keep * n))) for keep as the float the C call receives."""
    return min(n, max(1, math.ceil(float(f32(keep)) * n)))


def trim_mask(resid, keep):
    """(mask [n] bool, tau) of the header's rule on residuals `resid` (a torch vector): tau the kk-th smallest, m = !(e > tau)."""
    n = resid.shape[0]
    if keep >= 1.0:
        return torch.ones(n, dtype=torch.bool), float("inf")
    tau = torch.kthvalue(resid.detach(), keep_count(keep, n)).values
    return ~(resid.detach() > tau), float(tau)


def robust_loss_torch(rgb, tgt, kind, param, keep=1.0, mask=None):
    """(loss, mask, tau): the robust mean of the definition in rgb's dtype, differentiable in rgb; mask: a given constant mask (else
    the definition's own, from this precision's residuals)."""
    rho = robust_rho(rgb, tgt, kind, param)
    tau = None
    if mask is None:
        mask, tau = trim_mask(rho.sum(dim=1), keep)
    return (rho * mask[:, None].to(rho.dtype)).sum() / (3 * rgb.shape[0]), mask, tau


def robust_reference(rgb, tgt, kind, param, grad_scale, dtype, mask=None):
    """(loss [1], g_rgb [n, 3], resid [n]) of the definition in `dtype` under a given mask (None: no trim)."""
    r = torch.as_tensor(np.asarray(rgb)).to(dtype).requires_grad_(True)
    t = torch.as_tensor(np.asarray(tgt)).to(dtype)
    m = torch.ones(r.shape[0], dtype=torch.bool) if mask is None else torch.as_tensor(np.asarray(mask)).bool()
    loss, _, _ = robust_loss_torch(r, t, kind, param, mask=m)
    g, = torch.autograd.grad(loss * float(grad_scale), r)
    return loss.detach().reshape(1), g, robust_rho(r, t, kind, param).sum(dim=1).detach()


# ---- the kernel through a backend ---------------------------------------------------------------------------------------------------
def robust_loss(b, rgb, tgt, kind, param=0.0, keep=1.0, grad_scale=1.0, want=("g_rgb", "resid", "mask"), raise_on_error=True, n=None,
                stride=None, null=(), tmp="auto", tmp_bytes=None):
    """nerfhip_robust_loss_fwd_bwd on numpy inputs: dict(loss [3], g_rgb [n, 3], resid [n], mask [n] uint8; None where not asked for);
    raise_on_error=False: the return code under "rc", the outputs as the call left them (NaN-filled before).  null: names of arguments
    passed as NULL; tmp: "auto" (a buffer of nerfhip_robust_loss_tmp_bytes(n) bytes when keep < 1), None, or "odd" (misaligned)."""
    nn = rgb.shape[0]
    tgt = np.ascontiguousarray(tgt, f32)
    d = dict(rgb=b.dev(np.ascontiguousarray(rgb, f32)), target=b.dev(tgt), loss_out=b.empty((3,)))
    g_rgb = b.empty((nn, 3)) if "g_rgb" in want else None
    resid = b.empty((nn,)) if "resid" in want else None
    mask = b.dev(np.full(nn, 7, np.uint8)) if "mask" in want else None
    need = b.lib.robust_loss_tmp_bytes(nn)
    assert need == 4 * nn
    buf = b.empty((nn + 2,)) if tmp in ("auto", "odd") and (keep < 1.0 or tmp == "odd") else None
    tptr = None if buf is None else b.ptr(buf) + (1 if tmp == "odd" else 0)
    ptr = lambda k: None if k in null else b.ptr(d[k])  # noqa: E731
    args = (ptr("rgb"), ptr("target"), tgt.shape[1] if stride is None else stride, nn if n is None else n, kind, float(param), float(keep),
            float(grad_scale), b.p(g_rgb), b.p(resid), b.p(mask), ptr("loss_out"), tptr,
            (need if buf is not None else 0) if tmp_bytes is None else tmp_bytes, b.stream())
    out = lambda: dict(loss=b.host(d["loss_out"]), g_rgb=None if g_rgb is None else b.host(g_rgb),  # noqa: E731
                       resid=None if resid is None else b.host(resid), mask=None if mask is None else b.host(mask))
    if not raise_on_error:
        rc = b.lib._dll.nerfhip_robust_loss_fwd_bwd(*args)
        return dict(out(), rc=rc)
    b.lib.robust_loss_fwd_bwd(*args)
    return out()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def kernel_inputs(n, stride, seed, kind, param):
    """rgb in [0, 1) (the relative kind: a fifth of the elements at 1e-4 and below, p near 0), targets in [0, 1); every fifth element
    walks the edges of the kind: d = 0 exactly, d on either side of the parameter (Huber's delta: both branches next to the joint),
    d = 1e-7 x the parameter; target columns beyond 3 are garbage."""
    g = np.random.default_rng(seed)
    rgb = g.random((n, 3)).astype(f32)
    tgt = (g.normal(size=(n, stride)) * 1e3).astype(f32)
    tgt[:, :3] = g.random((n, 3))
    flat_r, q = rgb.reshape(-1), max(param, 1e-3)
    edges = np.array([0.0, q * (1 + 1e-3), -q * (1 - 1e-3), 1e-7 * q, -1e-7 * q], np.float64)
    idx = np.arange(0, 3 * n, 5)
    if kind == 4:
        flat_r[idx[::2]] = (1e-4 * g.random(len(idx[::2]))).astype(f32)
    want = flat_r[idx].astype(np.float64) - edges[(np.arange(len(idx)) + seed) % 5]
    tgt[idx // 3, idx % 3] = want.astype(f32)
    return rgb, tgt


def check_untrimmed(b, n, stride, kind, param, seed, record=None):
    rgb, tgt = kernel_inputs(n, stride, seed, kind, param)
    tag = "kind=%d n=%d stride=%d" % (kind, n, stride)
    gs = 0.37
    l64, g64, e64 = robust_reference(rgb, tgt, kind, param, gs, torch.float64)
    l32, g32, e32 = robust_reference(rgb, tgt, kind, param, gs, torch.float32)
    got = robust_loss(b, rgb, tgt, kind, param, grad_scale=gs)
    assert float(l64) > 0.0 or n <= 2, tag
    if kind == 2 and n >= 63:   # (not vacuous, from the reference alone: both Huber branches are well populated)
        beyond = float((np.abs(rgb.astype(np.float64) - tgt[:, :3].astype(np.float64)) > param).mean())
        assert 0.1 <= beyond <= 0.9, (tag, beyond)
    SC.held_to_yardstick(got["loss"][:1], l64, l32, tag + " loss", record)
    SC.held_to_yardstick(got["g_rgb"], g64, g32, tag + " g_rgb", record)
    SC.held_to_yardstick(got["resid"], e64, e32, tag + " resid", record)
    assert got["loss"][1] == 1.0 and got["loss"][2] == np.inf and (got["mask"] == 1).all(), tag
    # the optional outputs change nothing
    bare = robust_loss(b, rgb, tgt, kind, param, grad_scale=gs, want=())
    only = robust_loss(b, rgb, tgt, kind, param, grad_scale=gs, want=("g_rgb",))
    assert bare["g_rgb"] is None and np.array_equal(bits(bare["loss"]), bits(got["loss"])), tag
    assert np.array_equal(bits(only["g_rgb"]), bits(got["g_rgb"])) and np.array_equal(bits(only["loss"]), bits(got["loss"])), tag


def check_selection(got, n, keep, tag):
    """Check 2 of the trimmed cases, exact, on the kernel's own residuals; -> the mask as bool."""
    resid, mask, loss = got["resid"], got["mask"], got["loss"]
    kk = keep_count(keep, n)
    # (keep == 1 -- 1 / n at n = 1 -- runs no selection and reports +inf)
    tau = np.partition(resid, kk - 1)[kk - 1] if f32(keep) < 1.0 else f32(np.inf)
    assert bits(loss[2:3])[0] == bits(np.array([tau], f32))[0], (tag, loss[2], tau)
    assert np.array_equal(mask, (~(resid > tau)).astype(np.uint8)), tag
    assert bits(loss[1:2])[0] == bits(np.array([mask.sum() / n], f32))[0], (tag, loss[1], mask.sum(), n)
    assert mask.sum() >= kk, tag
    return mask.astype(bool)


def check_trimmed(b, n, stride, kind, param, keep, seed, record=None):
    rgb, tgt = kernel_inputs(n, stride, seed, kind, param)
    tag = "kind=%d n=%d stride=%d keep=%.4f" % (kind, n, stride, keep)
    gs = 0.37
    kk = keep_count(keep, n)
    got = robust_loss(b, rgb, tgt, kind, param, keep=keep, grad_scale=gs)
    # 1. the residuals against the definition
    _, _, e64 = robust_reference(rgb, tgt, kind, param, gs, torch.float64)
    _, _, e32 = robust_reference(rgb, tgt, kind, param, gs, torch.float32)
    SC.held_to_yardstick(got["resid"], e64, e32, tag + " resid", record)
    if 1 < kk < n:   # (not vacuous, from the reference alone: the definition trims a ray and keeps one)
        m64, _ = trim_mask(e64, keep)
        assert 0 < int(m64.sum()) < n, tag
    # 2. the selection, exact, on the kernel's own residuals
    mask = check_selection(got, n, keep, tag)
    assert (1 < kk < n) <= (0 < mask.sum() < n), tag
    # 3. loss and g_rgb against the definition under the kernel's own mask; trimmed rows exact zeros
    l64, g64, _ = robust_reference(rgb, tgt, kind, param, gs, torch.float64, mask)
    l32, g32, _ = robust_reference(rgb, tgt, kind, param, gs, torch.float32, mask)
    SC.held_to_yardstick(got["loss"][:1], l64, l32, tag + " loss", record)
    SC.held_to_yardstick(got["g_rgb"], g64, g32, tag + " g_rgb", record)
    assert not bits(got["g_rgb"][~mask]).any(), tag
    # the optional outputs change nothing
    bare = robust_loss(b, rgb, tgt, kind, param, keep=keep, grad_scale=gs, want=("g_rgb",))
    assert np.array_equal(bits(bare["g_rgb"]), bits(got["g_rgb"])) and np.array_equal(bits(bare["loss"]), bits(got["loss"])), tag


def keeps_of(n):
    return (0.5, 0.8, 1.0 / n) + ((0.999,) if n == 3073 else ())


def case_kernel(b, kind, param, record=None):
    """Every n with both target strides, without a trim and with every keep of the shape."""
    seed = 1000 * kind
    for n in SHAPES_N:
        for stride in STRIDES:
            seed += 1
            check_untrimmed(b, n, stride, kind, param, seed, record)
            for keep in keeps_of(n):
                check_trimmed(b, n, stride, kind, param, keep, seed, record)


def case_ties(b):
    """Duplicated rows are bitwise ties: kept >= kk and every tie at tau is kept; with all residuals equal everything is kept."""
    for kind, param in KERNEL_KINDS:
        for n in (2, 65, 1025):
            rgb, tgt = kernel_inputs(5, 4, 50 + kind, kind, param)
            pick = np.random.default_rng(n).integers(0, 5, n)
            pick[:2] = (0, 0)
            rgb, tgt = rgb[pick], tgt[pick]
            for keep in (0.3, 0.5, 0.8):
                got = robust_loss(b, rgb, tgt, kind, param, keep=keep)
                tag = "ties kind=%d n=%d keep=%.1f" % (kind, n, keep)
                mask = check_selection(got, n, keep, tag)
                tau, resid = got["loss"][2], got["resid"]
                assert len(np.unique(bits(resid))) <= 5 and (resid == tau).sum() >= 2 and mask[resid == tau].all(), tag
                assert not bits(got["g_rgb"][~mask]).any(), tag
            # all residuals equal
            same = robust_loss(b, np.tile(rgb[:1], (n, 1)), np.tile(tgt[:1], (n, 1)), kind, param, keep=0.5)
            assert same["loss"][1] == 1.0 and (same["mask"] == 1).all() and same["loss"][2] == same["resid"][0], (kind, n)


def case_bit_identities(b):
    for n in (1, 64, 65, 1025, 3073):
        for stride in STRIDES:
            rgb, tgt = kernel_inputs(n, stride, 300 + n + stride, 0, 0.0)
            what = (n, stride)
            # kind 0 without a trim is the plain loss's loss word and cotangent
            for gs in (1.0, 0.37):
                got = robust_loss(b, rgb, tgt, 0, grad_scale=gs)
                plain, pg, _ = b.mse_loss(rgb, None, tgt, grad_scale=gs)
                assert bits(got["loss"])[0] == bits(plain)[0] and np.array_equal(bits(got["g_rgb"]), bits(pg)), what
            # Huber with a delta beyond every |d| is kind 0, trimmed or not
            for keep in (1.0, 0.5):
                a, h = robust_loss(b, rgb, tgt, 0, keep=keep), robust_loss(b, rgb, tgt, 2, 1e30, keep=keep)
                assert all(np.array_equal(bits(a[k]), bits(h[k])) for k in ("loss", "g_rgb", "resid")) and np.array_equal(a["mask"], h["mask"]), what
            # grad_scale scales g_rgb only
            for kind, param in KERNEL_KINDS:
                one = robust_loss(b, rgb, tgt, kind, param, keep=0.8)
                two = robust_loss(b, rgb, tgt, kind, param, keep=0.8, grad_scale=2.0)
                assert all(np.array_equal(bits(one[k]), bits(two[k])) for k in ("loss", "resid")) and np.array_equal(one["mask"], two["mask"]), what
                assert np.array_equal(bits(2.0 * one["g_rgb"]), bits(two["g_rgb"])), what


def case_nan(b):
    """One NaN in rgb: the loss is NaN and its ray stays kept; the other rays' g_rgb are those of the run without it under the same mask
    (the clean value of that ray is the batch's largest residual: it sorts last either way, so tau does not move)."""
    for kind, param in KERNEL_KINDS:
        for n in (5, 65, 1025):
            rgb, tgt = kernel_inputs(n, 4, 77 + n, kind, param)
            ray = n // 2
            tgt[ray, :3] = 50.0   # (the largest residual under every kind: |d| = 50, and p + eps = eps for the relative one)
            rgb[ray] = 0.0
            for keep in (1.0, 0.5):
                clean = robust_loss(b, rgb, tgt, kind, param, keep=keep)
                bad = rgb.copy()
                bad[ray, 1] = np.nan
                got = robust_loss(b, bad, tgt, kind, param, keep=keep)
                what = (kind, n, keep)
                assert np.isnan(got["loss"][0]) and np.isnan(got["resid"][ray]) and got["mask"][ray] == 1, what
                assert clean["mask"][ray] == int(keep == 1.0) and np.isfinite(clean["loss"][:2]).all(), what
                others = np.arange(n) != ray
                assert np.array_equal(got["mask"][others], clean["mask"][others]) and bits(got["loss"])[2] == bits(clean["loss"])[2], what
                assert np.array_equal(bits(got["g_rgb"][others]), bits(clean["g_rgb"][others])), what
                assert np.isnan(got["g_rgb"][ray, 1]) and not np.isnan(got["g_rgb"][others]).any(), what
                assert got["loss"][1] == f32((clean["mask"][others].sum() + 1) / n), what


def case_refusals(b):
    """Every refusal returns NERFHIP_ERR_ARG, names its argument and leaves the outputs untouched."""
    rgb, tgt = kernel_inputs(6, 5, 1, 2, 0.3)

    def refused(match, kind=2, param=0.3, **kw):
        got = robust_loss(b, rgb, tgt, kind, param, raise_on_error=False, **kw)
        assert got["rc"] == ERR_ARG and match in b.lib.last_error().decode(), (got["rc"], match, b.lib.last_error())
        assert np.isnan(got["loss"]).all() and np.isnan(got["g_rgb"]).all() and np.isnan(got["resid"]).all() and (got["mask"] == 7).all()

    refused("n must", n=0)
    refused("n must", n=-3)
    refused("n must", n=1 << 31)
    refused("target_stride", stride=2)
    for name in ("rgb", "target", "loss_out"):
        refused(name + " is NULL", null=(name,))
    refused("kind", kind=5)
    refused("kind", kind=-1)
    for kind in (2, 3, 4):
        for bad in (0.0, -0.1, float("nan"), float("inf")):
            refused("param", kind=kind, param=bad)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        refused("keep", keep=bad)
    refused("tmp is NULL", keep=0.5, tmp=None)
    refused("tmp must be aligned", keep=0.5, tmp="odd")
    refused("tmp_bytes", keep=0.5, tmp_bytes=4 * 6 - 1)
    # ... and what is not refused: a parameter the kind does not read, no tmp without a trim
    for kind in (0, 1):
        assert robust_loss(b, rgb, tgt, kind, float("nan"), raise_on_error=False)["rc"] == 0
    assert robust_loss(b, rgb, tgt, 2, 0.3, keep=1.0, tmp=None, raise_on_error=False)["rc"] == 0
    assert robust_loss(b, rgb, tgt, 2, 0.3, keep=0.5, raise_on_error=False)["rc"] == 0


# ---- through the render -------------------------------------------------------------------------------------------------------------
HUBER_DELTA = 0.25   # (random nets against uniform targets: differences on both sides, asserted in the case)


def robust_cotangents(b, out, tgt, kind, param, keep=1.0):
    """The kernel on a render's maps: ((g_rgb_c, g_rgb_f), (result_c, result_f))."""
    c = robust_loss(b, out["rgb_coarse"], tgt, kind, param, keep=keep)
    f = robust_loss(b, out["rgb_fine"], tgt, kind, param, keep=keep)
    return (c["g_rgb"], f["g_rgb"]), (c, f)


def teacher(par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, kind, param, dtype, want_margin=False):
    """The oracle's autograd of both nets' robust means on GIVEN depths in `dtype` (matte_cases.teacher with this file's loss)."""
    cast = lambda d: {k: torch.as_tensor(v).to(dtype) for k, v in d.items()}  # noqa: E731
    pc = {k: v.detach().to(dtype).requires_grad_(True) for k, v in par_c.items()}
    pf = {k: v.detach().to(dtype).requires_grad_(True) for k, v in par_f.items()}
    r = torch.as_tensor(rays).to(dtype)
    w = O.render_at_depths(r, torch.as_tensor(z_c).to(dtype), torch.as_tensor(z_f).to(dtype), pc, pf, cfg, cfg, opt, cast(rand),
                           want_margin=want_margin)
    t = torch.as_tensor(tgt)
    total = robust_loss_torch(w["rgb_coarse"], t, kind, param)[0] + robust_loss_torch(w["rgb_fine"], t, kind, param)[0]
    total.backward()
    beyond = [float(((w["rgb_" + tag].detach() - t.to(dtype)).abs() > param).double().mean()) for tag in ("coarse", "fine")]
    return ({k: v.grad.numpy() for k, v in pc.items()}, {k: v.grad.numpy() for k, v in pf.items()},
            w["relu_margin"].numpy() if want_margin else None, beyond)


def case_param_grads(b, net="w64", arith="fp32", shape=(48, 8, 8), min_decided=0.3, record=None):
    """Parameter gradients of the Huber loss through nerfhip_robust_loss_fwd_bwd + nerfhip_render_bwd_parts against the oracle's fp64
    autograd of the same loss, teacher-forced on the kernels' own depths, on the rays all of whose samples pass `relu_margin`
    (matte_cases.case_param_grads' construction and bound)."""
    tol = TL.bound("tf.grad.filtered", arith)[0]
    kind, param = 2, HUBER_DELTA
    cfg, pc, par_c, _, packed_c = SC.setup(b, net, arith, seed=3)
    _, pf, par_f, _, packed_f = SC.setup(b, net, arith, seed=4)
    n, nc, nf = shape
    _, rays, rand, opt, tgt = SC.render_problem(net, n, nc, nf, seed=33)
    r = SC.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
    z_c, z_f = r.region("z_coarse"), r.region("z_fine")
    margin = teacher(par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, kind, param, torch.float64, want_margin=True)[2]
    keep = margin > TL.bound("relu_margin")
    print("param grads %s %s n=%d: %d of %d rays decided" % (net, arith, n, int(keep.sum()), n))
    assert keep.mean() >= min_decided, (net, n, float(keep.mean()))
    rays, tgt, rand = rays[keep], tgt[keep], {k: np.ascontiguousarray(v[keep]) for k, v in rand.items()}
    r = SC.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
    assert np.array_equal(r.region("z_coarse"), z_c[keep]) and np.array_equal(r.region("z_fine"), z_f[keep])
    g, _ = robust_cotangents(b, r.out, tgt, kind, param)
    got = r.backward(g, entry="parts")
    targs = (par_c, par_f, cfg, rays, z_c[keep], z_f[keep], opt, rand, tgt, kind, param)
    ref_c, ref_f, _, beyond = teacher(*targs, torch.float64)
    r32_c, r32_f, _, _ = teacher(*targs, torch.float32)
    l2_c, l2_f, _, _ = teacher(*targs[:-2], 0, 0.0, torch.float64)
    # not vacuous, from the oracle alone: both Huber branches occur in both nets, and the gradient is not the plain loss's
    assert all(0.05 <= x <= 0.95 for x in beyond), beyond
    for tag, plan, ref, r32, l2 in (("coarse", pc, ref_c, r32_c, l2_c), ("fine", pf, ref_f, r32_f, l2_f)):
        gp = b.unflatten(plan, got["g_params_" + tag])
        moved = max(float(np.abs(v - l2[k]).max()) / float(np.abs(v).max()) for k, v in ref.items())
        assert moved > 10.0 * tol, (tag, moved)
        for k, v in ref.items():
            mag = float(np.abs(v).max())
            err, own = float(np.abs(gp[k] - v).max()) / mag, float(np.abs(r32[k] - v).max()) / mag
            bound = tol if own <= tol else 2.0 * own
            print("param grads %s %s n=%d %s %s: %.3e of max|g| (oracle fp32 vs fp64 %.3e, bound %.1e)" % (net, arith, n, tag, k, err, own, bound))
            if record is not None:
                record.append((net, arith, n, tag, k, err, own, bound))
            assert err <= bound, (net, arith, n, tag, k, err, own, bound)
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


def case_modes(b, net, arith, modes, n=48, nc=8, nf=8, noise=0.6, keep=0.5):
    """Every backward mode against the dense one with trim = 0.5, within `unit.compact_vs_dense` of max|g| per tensor (the bound of
    matte_cases.case_compacted).  From the dense run: every sample of a trimmed ray has a zero d(loss)/d(raw) row, and a kept ray has
    a nonzero one; the modes that walk a list keep fewer samples than the same step untrimmed."""
    ctol = TL.bound("unit.compact_vs_dense", arith)
    kind, param = 2, HUBER_DELTA
    cfg, pc, _, _, packed_c = SC.setup(b, net, arith, seed=3)
    _, pf, _, _, packed_f = SC.setup(b, net, arith, seed=4)
    _, rays, rand, opt, tgt = SC.render_problem(net, n, nc, nf, seed=35, noise=noise)
    res, kept_trim, kept_all = {}, {}, {}
    for mode in (False,) + tuple(modes):
        b.set_compaction(pc, mode)
        b.set_compaction(pf, mode)
        r = SC.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
        if mode is False:
            g, (c, f) = robust_cotangents(b, r.out, tgt, kind, param, keep)
            g_all, _ = robust_cotangents(b, r.out, tgt, kind, param)
            masks = dict(coarse=c["mask"].astype(bool), fine=f["mask"].astype(bool))
            assert all(0 < m.sum() < n for m in masks.values())
        out = {}
        for fine, part, tag in ((True, L.PART_FINE, "fine"), (False, L.PART_COARSE, "coarse")):
            total = n * (nc + (nf if fine else 0))
            listed = mode in (True, "recompute", "fused_compact")
            if listed:   # (the same step untrimmed, first: the trimmed run's rows stay in the workspace)
                r.backward(g_all, entry="parts", parts=part)
                kept_all[(mode, tag)] = r.kept(tag)[0]
            got = r.backward(g, entry="parts", parts=part)
            out["g_params_" + tag] = got["g_params_" + tag]
            rows = r.region("bwd_g_raw_" + tag).reshape(n, -1, 4).any(axis=2)
            if mode is False:
                assert not rows[~masks[tag]].any() and rows[masks[tag]].any(axis=1).all(), tag
            if listed:
                kept, tot = r.kept(tag)
                assert tot == total and kept == int(rows.sum()) and 0 < kept < kept_all[(mode, tag)], (mode, tag, kept, kept_all[(mode, tag)])
        res[mode] = out
    for mode in modes:
        for tag, plan in (("coarse", pc), ("fine", pf)):
            gd, gk = b.unflatten(plan, res[False]["g_params_" + tag]), b.unflatten(plan, res[mode]["g_params_" + tag])
            for k in gd:
                d = float(np.abs(gk[k] - gd[k]).max()) / (float(np.abs(gd[k]).max()) + 1e-30)
                assert np.isfinite(gk[k]).all() and d <= ctol, (net, arith, mode, tag, k, d, ctol)
    for p in (pc, pf):
        b.set_compaction(p, False)
        b.lib.plan_destroy(p)


# ---- the capability run's corruption (shared by scripts/study_robust.py and tests/test_gpu_robust.py) --------------------------------
CORRUPTION_RATE = 0.3
CORRUPTION_SEED = 1234


def corrupt(clean, rate=CORRUPTION_RATE, seed=CORRUPTION_SEED):
    """clean [V, P, 3] (CPU) -> (corrupted, hit [V, P] bool): in each view a fixed random `rate` of the pixels -- an independent draw per
    pixel and per view -- is replaced by a saturated random colour (each channel 0 or 1)."""
    g = torch.Generator().manual_seed(seed)
    hit = torch.rand(clean.shape[:2], generator=g) < rate
    colours = torch.randint(0, 2, clean.shape, generator=g).to(clean.dtype)
    return torch.where(hit[..., None], colours, clean), hit
