"""Cases of the alpha-matte loss (include/nerfhip.h nerfhip_matte_loss_fwd_bwd, csrc/reg/matte.hip) and of its opacity cotangent
through the fused backward (g_acc_coarse / g_acc_fine of nerfhip_render_cotangents), shared by the emulator suite (tests/test_matte.py)
and the GPU suite (tests/test_gpu_matte.py).  Every case drives the C ABI through a backend's library handle (tests/backends.py).

The definition is restated here independently of the kernel (matte_terms): the header's formulas in torch, autograd for the two
cotangents.

Bounds of this file, and where they come from:

  spread_cases.held_to_yardstick (SPREAD_YARDSTICK / SPREAD_FLOOR, with their reasons): the kernel's three loss words, `g_rgb` and
                    `g_acc` may be no further from the fp64 run of the formulas than the SAME formulas run in torch fp32 are, x 2, plus
                    4 x 2^-24 of the quantity's largest magnitude in the case.  Each loss word is held on its own.
  render cases      tolerances.py `tf.grad.filtered`, `relu_margin` and `unit.compact_vs_dense`, and parity_cases.case_ray_grad's
                    distribution bound, as depth_prior_cases.py uses them: where the oracle's OWN fp32 autograd is further from its fp64
                    run than `tf.grad.filtered`, that tensor's bound is 2 x that fp32 distance (printed).
"""
import numpy as np
import torch

import nerf_oracle as O
import nerf_pytorch_amd._lib as L
import occupancy_cases as OC
import spread_cases as SC
import tolerances as TL

f32 = np.float32
EPS = 1e-6
RNG_STREAM = 4   # (nerfhip.h: stream id 4 = background colour)

SHAPES_N = (1, 63, 64, 65, 1023, 1025, 3073)   # the wave edges, the block edge, a thread with a ragged last element
STRIDES = (4, 7)
BACKGROUNDS = ("given", "constant", "random")
ACC_EDGES = (0.0, 1e-7, 0.5, 1.0, 1.0 + 1e-6)   # the entropy clamp acts at both ends
ALPHA_EDGES = (0.0, 1.0, 0.37, -0.1, 1.2)        # (clamped to [0, 1] on read)
BG_CONST = (0.25, 1.0, 0.6)


# ---- the definition, in torch ----------------------------------------------------------------------------------------------------
def matte_terms(rgb, acc, tgt, mode, bg):
    """(photometric, alpha, entropy): the three unscaled means of the header's definition, differentiable in rgb [n, 3] and acc [n], in
    their dtype.  tgt [n, >= 4]; bg [n, 3] (matte mode) or None."""
    n = rgb.shape[0]
    dtype = rgb.dtype
    tgt = tgt.detach().to(dtype)
    C, a = tgt[:, :3], torch.clamp(tgt[:, 3], 0.0, 1.0)   # (a NaN stays a NaN)
    if mode == 0:
        b = bg.detach().to(dtype)
        t = a[:, None] * C + (1.0 - a)[:, None] * b
        p = rgb + (1.0 - acc)[:, None] * b
        photo = ((p - t) ** 2).sum() / (3 * n)
        alpha = ((acc - a) ** 2).sum() / n
    else:
        photo = (a[:, None] * (rgb - C) ** 2).sum() / (3 * n)
        alpha = torch.zeros((), dtype=dtype)
    x = torch.clamp(acc, EPS, 1.0 - EPS)
    ent = -(x * torch.log(x) + (1.0 - x) * torch.log(1.0 - x)).sum() / n
    return photo, alpha, ent


def matte_reference(rgb, acc, tgt, mode, bg, lam, grad_scale, dtype):
    """(loss [3], g_rgb [n, 3], g_acc [n]) of the definition in `dtype`: autograd of grad_scale * (photometric + lam_alpha alpha +
    lam_entropy entropy).  A term whose weight is exactly 0 is left out of the total (not 0 * inf)."""
    r = torch.as_tensor(np.asarray(rgb)).to(dtype).requires_grad_(True)
    a = torch.as_tensor(np.asarray(acc)).to(dtype).requires_grad_(True)
    b = None if bg is None else torch.as_tensor(np.asarray(bg))
    photo, alpha, ent = matte_terms(r, a, torch.as_tensor(np.asarray(tgt)), mode, b)
    total = photo
    if lam[0] != 0.0 and mode == 0:
        total = total + float(lam[0]) * alpha
    if lam[1] != 0.0:
        total = total + float(lam[1]) * ent
    g_r, g_a = torch.autograd.grad(total * float(grad_scale), (r, a), allow_unused=True)
    g_a = torch.zeros_like(a) if g_a is None else g_a
    return torch.stack((photo, alpha, ent)).detach(), g_r, g_a


# ---- the kernel through a backend ---------------------------------------------------------------------------------------------------
def matte_loss(b, rgb, acc, tgt, mode=0, bg=None, bg_random=False, bg_const=(0.0, 0.0, 0.0), seed=0, ray_offset=0, lam=(0.0, 0.0),
               grad_scale=1.0, want_rgb=True, want_acc=True, raise_on_error=True, n=None, stride=None, null=()):
    """nerfhip_matte_loss_fwd_bwd on numpy inputs: (loss [3], g_rgb [n, 3] or None, g_acc [n] or None); raise_on_error=False: the
    return code first, the outputs as the call left them (NaN-filled before).  null: names of arguments passed as NULL."""
    nn = rgb.shape[0]
    tgt = np.ascontiguousarray(tgt, f32)
    d = dict(rgb=b.dev(np.ascontiguousarray(rgb, f32)), acc=b.dev(np.ascontiguousarray(acc, f32)), target=b.dev(tgt), loss_out=b.empty((3,)))
    dbg = b.devopt(bg)
    g_rgb, g_acc = (b.empty((nn, 3)) if want_rgb else None), (b.empty((nn,)) if want_acc else None)
    ptr = lambda k: None if k in null else b.ptr(d[k])  # noqa: E731
    args = (ptr("rgb"), ptr("acc"), ptr("target"), tgt.shape[1] if stride is None else stride, nn if n is None else n, mode, b.p(dbg),
            int(bool(bg_random)), *[float(v) for v in bg_const], seed, ray_offset, float(lam[0]), float(lam[1]), float(grad_scale),
            b.p(g_rgb), b.p(g_acc), ptr("loss_out"), b.stream())
    out = lambda: (b.host(d["loss_out"]), None if g_rgb is None else b.host(g_rgb), None if g_acc is None else b.host(g_acc))  # noqa: E731
    if not raise_on_error:
        return (b.lib._dll.nerfhip_matte_loss_fwd_bwd(*args),) + out()
    b.lib.matte_loss_fwd_bwd(*args)
    return out()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def kernel_inputs(n, stride, seed):
    """rgb in [-0.1, 1.1), acc and alpha random in (0, 1) but for every third ray, which walks ACC_EDGES x ALPHA_EDGES (from a
    seed-dependent start, so that the short cases see different pairs); target columns beyond 3 are garbage."""
    g = np.random.default_rng(seed)
    rgb = (-0.1 + 1.2 * g.random((n, 3))).astype(f32)
    acc = (0.02 + 0.96 * g.random(n)).astype(f32)
    tgt = (g.normal(size=(n, stride)) * 1e3).astype(f32)
    tgt[:, :3] = g.random((n, 3))
    tgt[:, 3] = 0.02 + 0.96 * g.random(n)
    edge = np.arange(n)[::3]
    k = np.arange(len(edge)) + seed
    acc[edge] = np.array(ACC_EDGES, f32)[k % 5]
    tgt[edge, 3] = np.array(ALPHA_EDGES, f32)[(k // 5) % 5]
    bg = g.random((n, 3)).astype(f32)
    return dict(rgb=rgb, acc=acc, tgt=tgt, bg=bg)


def background_of(b, kind, c, n, seed, ray_offset):
    """(the kernel's background arguments, the [n, 3] rows the reference uses)."""
    if kind == "given":
        return dict(bg=c["bg"]), c["bg"]
    if kind == "constant":
        return dict(bg_const=BG_CONST), np.tile(np.array(BG_CONST, f32), (n, 1))
    return dict(bg_random=True, seed=seed, ray_offset=ray_offset), b.rng_fill(0, seed, RNG_STREAM, 3 * ray_offset, 3 * n).reshape(n, 3)


def check_kernel(b, n, stride, mode, bgkind, seed, record=None):
    c = kernel_inputs(n, stride, seed)
    rgb, acc, tgt = c["rgb"], c["acc"], c["tgt"]
    kw, bg = ({}, None) if mode == 1 else background_of(b, bgkind, c, n, 4321 + seed, 17 + seed)
    what = "mode=%d n=%d stride=%d bg=%s" % (mode, n, stride, bgkind if mode == 0 else "-")
    gs = 0.37
    for lam in (((0.3, 0.05), (0.0, 0.0), (0.3, 0.0), (0.0, 0.05)) if mode == 0 else ((0.0, 0.05), (0.0, 0.0))):
        l64, r64, a64 = matte_reference(rgb, acc, tgt, mode, bg, lam, gs, torch.float64)
        l32, r32, a32 = matte_reference(rgb, acc, tgt, mode, bg, lam, gs, torch.float32)
        loss, g_rgb, g_acc = matte_loss(b, rgb, acc, tgt, mode, lam=lam, grad_scale=gs, **kw)
        tag = what + " lam=%s" % (lam,)
        for i, name in enumerate(("photometric", "alpha", "entropy")):
            if mode == 1 and i == 1:
                assert loss[1] == 0.0 and float(l64[1]) == 0.0, tag
                continue
            assert float(l64[i]) > 0.0 or (mode == 1 and n == 1), (tag, name)   # (not vacuous; one ray of weight 0 has no loss)
            SC.held_to_yardstick(loss[i:i + 1], l64[i:i + 1], l32[i:i + 1], tag + " " + name, record)
        assert float(r64.abs().max()) > 0 or (mode == 1 and n == 1), tag
        SC.held_to_yardstick(g_rgb, r64, r32, tag + " g_rgb", record)
        if float(a64.abs().max()) > 0:
            SC.held_to_yardstick(g_acc, a64, a32, tag + " g_acc", record)
        else:   # (weight mode without an entropy term, or with every ray's opacity in the clamp: exact zeros)
            assert mode == 1 and not g_acc.any(), tag
        # where the entropy clamp acted its gradient is exactly 0: with the entropy term alone (weight mode) those rays' g_acc is +-0
        clamped = (acc.astype(np.float64) < EPS) | (acc.astype(np.float64) > 1.0 - EPS)
        if mode == 1:
            assert not g_acc[clamped].any() and not a64.numpy()[clamped].any(), tag
            if lam[1] != 0.0 and n >= 3:
                assert g_acc[~clamped & (acc != 0.5)].all(), tag
        # the single-output calls and a repeat: the combined call's bits
        lo1, r1, none = matte_loss(b, rgb, acc, tgt, mode, lam=lam, grad_scale=gs, want_acc=False, **kw)
        lo2, none2, a2 = matte_loss(b, rgb, acc, tgt, mode, lam=lam, grad_scale=gs, want_rgb=False, **kw)
        lo3, none3, none4 = matte_loss(b, rgb, acc, tgt, mode, lam=lam, grad_scale=gs, want_rgb=False, want_acc=False, **kw)
        assert none is None and none2 is None and none3 is None and none4 is None
        for lo in (lo1, lo2, lo3):
            assert np.array_equal(bits(lo), bits(loss)), tag
        assert np.array_equal(bits(r1), bits(g_rgb)) and np.array_equal(bits(a2), bits(g_acc)), tag
    return c, kw, bg


def case_kernel(b, mode, record=None):
    """Every n with both target strides; matte mode with the three backgrounds."""
    seed = 1000 * mode
    for n in SHAPES_N:
        for stride in STRIDES:
            for bgkind in (BACKGROUNDS if mode == 0 else ("-",)):
                seed += 1
                check_kernel(b, n, stride, mode, bgkind, seed, record)


def case_nan(b):
    """A NaN in rgb and a NaN in alpha propagate to the loss words that read them and to that ray's rows only."""
    for mode in (0, 1):
        for n in (5, 65, 1025):
            c = kernel_inputs(n, 4, 77 + n)
            lam = (0.3 if mode == 0 else 0.0, 0.05)
            ray = n // 2
            for where in ("rgb", "alpha"):
                rgb, tgt = c["rgb"].copy(), c["tgt"].copy()
                if where == "rgb":
                    rgb[ray, 1] = np.nan
                else:
                    tgt[ray, 3] = np.nan
                loss, g_rgb, g_acc = matte_loss(b, rgb, c["acc"], tgt, mode, bg=c["bg"] if mode == 0 else None, lam=lam)
                what = (mode, n, where)
                assert np.isnan(loss[0]) and not np.isnan(loss[2]), what
                assert np.isnan(loss[1]) == (where == "alpha" and mode == 0), what
                others = np.arange(n) != ray
                assert np.isnan(g_rgb[ray]).any() and not np.isnan(g_rgb[others]).any() and not np.isnan(g_acc[others]).any(), what
                if mode == 0:
                    assert np.isnan(g_acc[ray]), what
                    assert np.isnan(g_rgb[ray]).all() == (where == "alpha"), what
                else:   # (weight mode: g_acc is the entropy term alone, which reads neither)
                    assert not np.isnan(g_acc[ray]), what


def case_bit_identities(b):
    for n in (1, 64, 65, 1025, 3073):
        for stride in STRIDES:
            c = kernel_inputs(n, stride, 300 + n + stride)
            rgb, acc, tgt = c["rgb"], c["acc"], c["tgt"]
            what = (n, stride)
            # weight mode with a == 1 everywhere and lam == 0: the plain loss's loss word and cotangent
            ones = tgt.copy()
            ones[:, 3] = 1.0
            for gs in (1.0, 0.37):
                loss, g_rgb, g_acc = matte_loss(b, rgb, acc, ones, 1, grad_scale=gs)
                plain, pg, _ = b.mse_loss(rgb, None, ones, grad_scale=gs)
                assert bits(loss)[0] == bits(plain)[0] and np.array_equal(bits(g_rgb), bits(pg)) and not g_acc.any(), what
            # ... and with a == 0 everywhere: exact zeros
            zeros = tgt.copy()
            zeros[:, 3] = (0.0, -0.1)[n % 2]
            loss, g_rgb, g_acc = matte_loss(b, rgb, acc, zeros, 1)
            assert loss[0] == 0.0 and loss[1] == 0.0 and not g_rgb.any() and not g_acc.any(), what
            # bg_random is the same call with bg = rng_fill's stream-4 draws; a second ray_offset shifts the draws by 3 * offset
            lam, seed = (0.3, 0.05), 99 + n
            for off in (0, 5):
                draws = b.rng_fill(0, seed, RNG_STREAM, 3 * off, 3 * n).reshape(n, 3)
                rnd = matte_loss(b, rgb, acc, tgt, 0, bg_random=True, seed=seed, ray_offset=off, lam=lam)
                giv = matte_loss(b, rgb, acc, tgt, 0, bg=draws, lam=lam)
                for x, y in zip(rnd, giv):
                    assert np.array_equal(bits(x), bits(y)), (what, off)
            long = b.rng_fill(0, seed, RNG_STREAM, 0, 3 * (n + 5))
            assert np.array_equal(bits(long[15:]), bits(draws.reshape(-1))) and not np.array_equal(long[:3 * n], long[15:]), what
            assert long.min() >= 0.0 and long.max() < 1.0
            # a given background outranks bg_random, and bg_random the constant
            both = matte_loss(b, rgb, acc, tgt, 0, bg=draws, bg_random=True, seed=seed + 1, bg_const=BG_CONST, lam=lam)
            assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(both, giv)), what
            # grad_scale scales the cotangents and not the losses
            one = matte_loss(b, rgb, acc, tgt, 0, bg=c["bg"], lam=lam)
            two = matte_loss(b, rgb, acc, tgt, 0, bg=c["bg"], lam=lam, grad_scale=2.0)
            assert np.array_equal(bits(one[0]), bits(two[0])), what
            assert np.array_equal(bits(2.0 * one[1]), bits(two[1])) and np.array_equal(bits(2.0 * one[2]), bits(two[2])), what
            # a term whose weight is exactly 0 contributes nothing: acc = 0 / 1 with lam_entropy = 0 leaves g_acc finite
            assert np.isfinite(matte_loss(b, rgb, acc, tgt, 0, bg=c["bg"], lam=(0.3, 0.0))[2]).all(), what


def case_refusals(b):
    """Every refusal returns NERFHIP_ERR_ARG, names its argument and leaves the outputs untouched."""
    c = kernel_inputs(6, 5, 1)

    def refused(match, mode=0, **kw):
        rc, lo, g_rgb, g_acc = matte_loss(b, c["rgb"], c["acc"], c["tgt"], mode, raise_on_error=False, **kw)
        assert rc == -1 and match in b.lib.last_error().decode(), (rc, match, b.lib.last_error())
        assert np.isnan(lo).all() and np.isnan(g_rgb).all() and np.isnan(g_acc).all()

    refused("n must", n=0)
    refused("n must", n=-3)
    refused("target_stride", stride=3)
    for name in ("rgb", "acc", "target", "loss_out"):
        refused(name + " is NULL", null=(name,))
    refused("mode", mode=2)
    refused("mode", mode=-1)
    for bad in (-0.1, float("nan"), float("inf")):
        refused("lam_alpha", lam=(bad, 0.0))
        refused("lam_entropy", lam=(0.0, bad))
        refused("lam_entropy", mode=1, lam=(0.0, bad))
    refused("lam_alpha", mode=1, lam=(0.1, 0.0))
    rc = matte_loss(b, c["rgb"], c["acc"], c["tgt"], 1, lam=(0.0, 0.1), raise_on_error=False)[0]
    assert rc == 0


# ---- through the render -------------------------------------------------------------------------------------------------------------
RENDER_NETS = (("w64", "fp32"), ("w128", "fp32"), ("w40of64", "f16x3_train"))
RENDER_SHAPES = ((48, 8, 8), (21, 64, 64))
# ((alpha_loss, opacity_entropy) of the coarse net, of the fine net) in the render cases
MATTE_LAM = ((0.5, 0.02), (1.0, 0.01))


def render_targets(n, seed, opaque=False):
    """RGBA targets [n, 4] (a quarter of the rays a = 0, a quarter a = 1, the others fractional; opaque: a = 1 on every ray) and a
    background [n, 3]."""
    g = np.random.default_rng(seed)
    tgt = g.random((n, 4)).astype(f32)
    pick = g.random(n)
    tgt[pick < 0.25, 3], tgt[pick > 0.75, 3] = 0.0, 1.0
    if opaque:
        tgt[:, 3] = 1.0
    return tgt, g.random((n, 3)).astype(f32)


def density_bias_condition(g_raw):
    """sum |d(loss)/d(sigma)| / |sum d(loss)/d(sigma)| over a pass's samples: the one-element gradient of fc_alpha.bias is that sum,
    and a bound relative to max|g| of a tensor says something about rounding only while it does not cancel."""
    gs = g_raw[..., 3].astype(np.float64)
    return float(np.abs(gs).sum() / max(abs(gs.sum()), 1e-300))


def matte_cotangents(b, out, tgt, bg, lam=MATTE_LAM, mode=0):
    """The kernel on a render's maps: ((g_rgb_c, g_rgb_f, g_acc_c, g_acc_f) in backends.RenderSession._cot's order, (loss_c, loss_f))."""
    lc, grc, gac = matte_loss(b, out["rgb_coarse"], out["acc_coarse"], tgt, mode, bg=bg, lam=lam[0])
    lf, grf, gaf = matte_loss(b, out["rgb_fine"], out["acc_fine"], tgt, mode, bg=bg, lam=lam[1])
    return (grc, grf, gac, gaf), (lc, lf)


def oracle_total_loss(w, tgt, bg, lam, mode=0, acc_grad=True):
    """Both nets' photometric + lam_alpha alpha + lam_entropy entropy of an O.render_at_depths result, in its dtype.  acc_grad=False:
    the same value with the accumulated opacity a constant -- the loss whose gradient lacks the g_acc part."""
    total = 0.0
    for tag, (la, lh) in (("coarse", lam[0]), ("fine", lam[1])):
        acc = w["acc_" + tag] if acc_grad else w["acc_" + tag].detach()
        photo, alpha, ent = matte_terms(w["rgb_" + tag], acc, tgt, mode, bg)
        total = total + photo + la * alpha + lh * ent
    return total


def teacher(par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, bg, lam, dtype, wrt_rays=False, want_margin=False, acc_grad=True):
    """spread_cases._teacher with this file's total loss: the oracle's autograd on GIVEN depths in `dtype`."""
    cast = lambda d: {k: torch.as_tensor(v).to(dtype) for k, v in d.items()}  # noqa: E731
    pc = {k: v.detach().to(dtype).requires_grad_(True) for k, v in par_c.items()}
    pf = {k: v.detach().to(dtype).requires_grad_(True) for k, v in par_f.items()}
    r = torch.as_tensor(rays).to(dtype).requires_grad_(wrt_rays)
    zc, zf = torch.as_tensor(z_c).to(dtype), torch.as_tensor(z_f).to(dtype)
    w = O.render_at_depths(r, zc, zf, pc, pf, cfg, cfg, opt, cast(rand), want_margin=want_margin)
    oracle_total_loss(w, torch.as_tensor(tgt), torch.as_tensor(bg), lam, acc_grad=acc_grad).backward()
    return ({k: v.grad.numpy() for k, v in pc.items()}, {k: v.grad.numpy() for k, v in pf.items()},
            r.grad.numpy() if wrt_rays else None, w["relu_margin"].numpy() if want_margin else None)


def case_param_grads(b, net, arith, shapes=RENDER_SHAPES, min_decided=0.3, record=None):
    """Parameter gradients of the matte loss through nerfhip_matte_loss_fwd_bwd + nerfhip_render_bwd_parts (g_rgb and g_acc of both
    nets) against the oracle's fp64 autograd of the same loss, teacher-forced on the kernels' own depths, on the rays all of whose
    samples pass `relu_margin` (depth_prior_cases.case_param_grads' construction and bound)."""
    tol = TL.bound("tf.grad.filtered", arith)[0]
    cfg, pc, par_c, _, packed_c = SC.setup(b, net, arith, seed=3)
    _, pf, par_f, _, packed_f = SC.setup(b, net, arith, seed=4)
    for n, nc, nf in shapes:
        _, rays, rand, opt, _ = SC.render_problem(net, n, nc, nf, seed=33)
        tgt, bg = render_targets(n, seed=61)
        r = SC.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
        z_c, z_f = r.region("z_coarse"), r.region("z_fine")
        margin = teacher(par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, bg, MATTE_LAM, torch.float64, want_margin=True)[3]
        keep = margin > TL.bound("relu_margin")
        print("param grads %s %s n=%d: %d of %d rays decided" % (net, arith, n, int(keep.sum()), n))
        # (a ray is decided when EVERY sample of both passes is: a fraction of the rays is a floor for the short shape only.  min_decided
        # of the rays at 8 + 16 samples is min_decided^(1 / 24) per sample, and that per sample over 64 + 128 samples is
        # min_decided^8 = 7e-5 of the rays: below one ray of 21.  The long shape asks for a ray to compare on; that the comparison is
        # about the opacity cotangent is asserted below, from the oracle)
        assert (keep.mean() >= min_decided) if nc + nf <= 16 else keep.any(), (net, n, float(keep.mean()))
        rays, tgt, bg, rand = rays[keep], tgt[keep], bg[keep], {k: np.ascontiguousarray(v[keep]) for k, v in rand.items()}
        r = SC.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
        assert np.array_equal(r.region("z_coarse"), z_c[keep]) and np.array_equal(r.region("z_fine"), z_f[keep])
        g, _ = matte_cotangents(b, r.out, tgt, bg)
        got = r.backward(g, entry="parts")
        targs = (par_c, par_f, cfg, rays, z_c[keep], z_f[keep], opt, rand, tgt, bg, MATTE_LAM)
        ref_c, ref_f, _, _ = teacher(*targs, torch.float64)
        r32_c, r32_f, _, _ = teacher(*targs, torch.float32)
        no_c, no_f, _, _ = teacher(*targs, torch.float64, acc_grad=False)
        for tag, plan, ref, r32, no in (("coarse", pc, ref_c, r32_c, no_c), ("fine", pf, ref_f, r32_f, no_f)):
            gp = b.unflatten(plan, got["g_params_" + tag])
            # not vacuous, from the oracle alone: the g_acc part moves the net's gradient by far more than the bound
            moved = max(float(np.abs(v - no[k]).max()) / float(np.abs(v).max()) for k, v in ref.items())
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


def case_compacted(b, net, arith, modes, n=48, nc=8, nf=8, noise=0.6, opaque=True):
    """The backward modes with the opacity cotangent: every mode against mode 0 within `unit.compact_vs_dense` of max|g| per tensor (the
    existing bound); `kept` equals the count of nonzero d(loss)/d(raw) rows the compositing backward left.
    The targets are opaque (a = 1 on every ray, the nets' opacity below it: every ray's alpha term pulls the same way).  With mixed
    alphas on random nets the samples' d(loss)/d(sigma) can cancel -- measured on the emulator, w128 at noise 0.6: their sum is 1 / 4900
    of the sum of their magnitudes -- and fc_alpha.bias, a tensor of ONE element, then moves by 2.5e-5 of itself with the order of
    summation while every other tensor stays at 3e-7: a property of those inputs, not of a mode.  The case asserts from the dense run
    that its sums do not cancel (a ratio of at most 4; the MSE cases' own is 1.1 to 2.8).
    opaque=False is the run with mixed alphas (a g_acc of both signs, asserted): every tensor is held to the same bound but the
    tensors of ONE element, whose gradient is a plain sum over the samples: theirs is the bound times the measured ratio of that sum
    (rounding moves a sum by a fraction of the sum of its terms' magnitudes, not of the sum)."""
    ctol = TL.bound("unit.compact_vs_dense", arith)
    cfg, pc, _, _, packed_c = SC.setup(b, net, arith, seed=3)
    _, pf, _, _, packed_f = SC.setup(b, net, arith, seed=4)
    _, rays, rand, opt, _ = SC.render_problem(net, n, nc, nf, seed=35, noise=noise)
    tgt, bg = render_targets(n, seed=63, opaque=opaque)
    res, conds = {}, {}
    for mode in (False,) + tuple(modes):
        b.set_compaction(pc, mode)
        b.set_compaction(pf, mode)
        r = SC.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
        if mode is False:
            g, _ = matte_cotangents(b, r.out, tgt, bg)
            assert g[2].any() and g[3].any()
            assert opaque or all((x > 0).any() and (x < 0).any() for x in g[2:]), "mixed alphas: g_acc of both signs"
        out = {}
        for fine, part, tag in ((True, L.PART_FINE, "fine"), (False, L.PART_COARSE, "coarse")):
            got = r.backward(g, entry="parts", parts=part)
            out["g_params_" + tag] = got["g_params_" + tag]
            nonzero = int(r.region("bwd_g_raw_" + tag).reshape(-1, 4).any(axis=1).sum())
            if mode in (True, "recompute", "fused_compact"):
                kept, total = r.kept(tag)
                assert total == n * (nc + (nf if fine else 0)) and kept == nonzero and 0 < kept < total, (mode, tag, kept, nonzero, total)
            else:
                assert 0 < nonzero < n * (nc + (nf if fine else 0))
            if mode is False:
                cond = density_bias_condition(r.region("bwd_g_raw_" + tag))
                print("backward modes %s %s noise %.1f %s: density-bias sum / magnitudes = 1 / %.2f" % (net, arith, noise, tag, cond))
                assert cond <= 4.0 or not opaque, (net, arith, tag, cond)
                conds[tag] = max(cond, 1.0)
        res[mode] = out
    for mode in modes:
        for tag, plan in (("coarse", pc), ("fine", pf)):
            gd, gk = b.unflatten(plan, res[False]["g_params_" + tag]), b.unflatten(plan, res[mode]["g_params_" + tag])
            for k in gd:
                d = float(np.abs(gk[k] - gd[k]).max()) / (float(np.abs(gd[k]).max()) + 1e-30)
                bound = ctol * conds[tag] if (not opaque and gd[k].size == 1) else ctol
                assert np.isfinite(gk[k]).all() and d <= bound, (net, arith, mode, tag, k, d, bound)
    for p in (pc, pf):
        b.set_compaction(p, False)
        b.lib.plan_destroy(p)


def case_ray_grad(b, net="w128", n=48, nc=8, nf=8):
    """nerfhip_render_bwd_rays with g_rgb and g_acc of the matte loss: d(loss)/d(rays) against the oracle's autograd teacher-forced on
    the kernels' own depths, under parity_cases.case_ray_grad's distribution bound (as spread_cases.case_rays_w); the frozen ray
    gradient (nerfhip_render_grad_rays) gives the same ray gradient within that bound's floor."""
    cfg, pc, par_c, flat_c, packed_c = SC.setup(b, net, "fp32", seed=3)
    _, pf, par_f, flat_f, packed_f = SC.setup(b, net, "fp32", seed=4)
    _, rays, rand, opt, _ = SC.render_problem(net, n, nc, nf, seed=37, noise=0.0)
    tgt, bg = render_targets(n, seed=65)
    r = SC.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
    z_c, z_f = r.region("z_coarse"), r.region("z_fine")
    g, _ = matte_cotangents(b, r.out, tgt, bg)
    got = r.backward(g, entry="rays", params=(flat_c, flat_f))["g_rays"]
    targs = (par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, bg, MATTE_LAM)
    ref = teacher(*targs, torch.float32, wrt_rays=True)[2]
    ref64 = teacher(*targs, torch.float64, wrt_rays=True)[2]
    no64 = teacher(*targs, torch.float64, wrt_rays=True, acc_grad=False)[2]
    assert np.isfinite(ref64).all() and float(np.any(ref64[:, 0:3] != 0.0, axis=1).mean()) >= 0.9
    for lo, hi, what in ((0, 3, "origin"), (3, 6, "direction"), (8, 11, "viewdirs")):
        scale = float(np.abs(ref64[:, lo:hi]).max())
        assert scale > 0.0, what
        # (the g_acc part is in it -- but for the view directions: the density, and so the opacity, does not depend on them)
        assert what == "viewdirs" or float(np.abs(ref64[:, lo:hi] - no64[:, lo:hi]).max()) > 1e-2 * scale, what
        e_hip = np.abs(got[:, lo:hi] - ref[:, lo:hi]).max(axis=1) / scale
        e_yard = np.abs(ref[:, lo:hi] - ref64[:, lo:hi]).max(axis=1) / scale
        print("ray grad %s: median %.3e (oracle fp32 vs fp64 %.3e), beyond 2e-3: %d (%d)" % (what, np.median(e_hip), np.median(e_yard),
                                                                                          (e_hip > 2e-3).sum(), (e_yard > 2e-3).sum()))
        assert np.median(e_hip) <= 3.0 * np.median(e_yard) + 2e-6, what
        assert (e_hip > 2e-3).sum() <= 2 * (e_yard > 2e-3).sum() + 3, what
    assert np.all(got[:, 6:8] == 0.0)
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


def case_culled_step(b, net, arith, outside, n=21, nc=9, nf=6, noise_std=0.3):
    """occupancy_train_cases.case_half_empty with the matte loss: arm A by hand in mode 1 (training forward, the library's own flags,
    the culled rows overwritten with the empty row, compositing again), arm B nerfhip_render_fwd_occ_train in mode 2 (and 4 where the
    plan has it); in both arms nerfhip_matte_loss_fwd_bwd on the maps and nerfhip_render_bwd_parts with g_rgb and g_acc.  The maps and
    the matte cotangents bit-identical, each net's kept count equal, gradients array_equal in mode 2 and within unit.compact_vs_dense
    in mode 4 -- and not the gradients without g_acc."""
    import occupancy_train_cases as OT
    cfg, pc, pf, packed_c, packed_f, modes = OT.nets_and_modes(b, net, arith)
    rays, rnp, _ = OT.half_empty_inputs(cfg, n, nc, nf)
    tgt, bg = render_targets(n, seed=67, opaque=True)   # (case_compacted's reason)
    grid = OC.Grid(b, OT.half_empty_bits(rays, 23), *OC.SCENE_BOX, (8, 8, 16), outside)
    opt = dict(num_coarse=nc, num_fine=nf, perturb=True, white_background=False, noise_std=noise_std)
    rd = np.ascontiguousarray(rays[:, 3:6])
    for p in (pc, pf):
        b.set_compaction(p, True)
    a = OT.Step(b, pc, pf, packed_c, packed_f, rays, opt, rnp)
    for fine, part in ((False, L.PART_COARSE), (True, L.PART_FINE)):
        a.fwd(part)
        tag = "fine" if fine else "coarse"
        z, raw = a.region("z_" + tag), a.region("raw_" + tag)
        fl = OC.occ_mark(b, grid, rays, z).astype(bool)
        assert 0.2 < 1.0 - fl.mean() < 0.8
        raw[~fl] = OC.EMPTY
        a.set_region("raw_" + tag, raw)
        out = b.volume_render_fwd(raw, z, rd, noise_std, rnp["noise_fine" if fine else "noise_coarse"], False)
        for k, v in zip(("rgb", "disp", "acc", None, "depth"), out):
            if k:
                a.set_map(k + "_" + tag, v)
        if not fine:
            a.set_region("weights_coarse", out[3])
    want = a.maps()
    g_a, _ = matte_cotangents(b, want, tgt, bg)
    assert g_a[2].any() and g_a[3].any()
    run = lambda s, g: dict(s.backward(g, entry="parts"), kept_coarse=s.kept("coarse"), kept_fine=s.kept("fine"))  # noqa: E731
    plain = run(a, g_a[:2])
    want.update(run(a, g_a))
    for tag in ("coarse", "fine"):
        assert not np.array_equal(want["g_params_" + tag], plain["g_params_" + tag]), tag
    ctol = TL.bound("unit.compact_vs_dense", arith if arith == "fp32" else "f16x3_train")
    for mode in modes:
        for p in (pc, pf):
            b.set_compaction(p, mode)
        s = OT.Step(b, pc, pf, packed_c, packed_f, rays, opt, rnp)
        s.fwd_occ(grid)
        got = s.maps()
        g, _ = matte_cotangents(b, got, tgt, bg)
        for x, y in zip(g, g_a):
            assert np.array_equal(bits(x), bits(y)), mode
        got.update(run(s, g))
        for tag, plan in (("coarse", pc), ("fine", pf)):
            assert got["kept_" + tag] == want["kept_" + tag], (mode, tag, got["kept_" + tag], want["kept_" + tag])
            gg, w = got["g_params_" + tag], want["g_params_" + tag]
            assert w.any() and np.isfinite(gg).all()
            if mode == "recompute":
                assert np.array_equal(gg, w), (tag, float(np.abs(gg - w).max()))
            else:
                gd, gk = b.unflatten(plan, w), b.unflatten(plan, gg)
                for k in gd:
                    d = float(np.abs(gk[k] - gd[k]).max()) / (float(np.abs(gd[k]).max()) + 1e-30)
                    assert d <= ctol, (mode, tag, k, d, ctol)
    for p in (pc, pf):
        b.lib.plan_destroy(p)
