"""Cases of the ray-weight spread loss (mip-NeRF 360's L_dist; include/nerfhip.h nerfhip_spread_loss, csrc/reg/spread.hip) and of the
weight cotangent through the fused backward (nerfhip_render_bwd_parts_w / nerfhip_render_bwd_rays_w), shared by the emulator suite
(tests/test_spread.py) and the GPU suite (tests/test_gpu_spread.py).  Every case drives the C ABI through a backend's library handle
(tests/backends.py).

The definition is restated here independently of the kernel: the S^2 double sum in torch, with the weights from the oracle's
compositing (O.volume_render) on the same raw rows, depths and noise draws, and autograd for dL/dw.

Bounds of this file, and where they come from:

  SPREAD_YARDSTICK  the kernel's `loss` and `g_weights` may be no further from the fp64 run of that formula than the SAME formula run in
                    fp32 is, x 2 (what tolerances.py allows two fp32 evaluations that do not share their rounding), plus a floor.  The
                    yardstick is the reference's own error, never a measurement of the kernel.
  SPREAD_FLOOR      4 x 2^-24 of the quantity's largest magnitude in the case: the outputs are fp32 (half an ulp each from the final
                    rounding), and the weights the kernel sums are the compositing's fp32 weights (an ulp or two of w from expf and the
                    transmittance product); at S = 1 or 2 the fp32 run of the formula can be exact by accident on a few rays, so x 2 of
                    its error alone is no bound there.  Measured on the wave emulator over every shape and case of KERNEL_KINDS: the
                    kernel's largest error is 2.50 x 2^-24 of that magnitude for `loss` and 1.72 x 2^-24 for `g_weights` (the fp32 run of
                    the formula: up to 4.24 and 6.26 x 2^-24), and the most the kernel exceeds 2 x the formula's error of its own case
                    by -- what the floor has to cover -- is 0.46 x 2^-24 (`loss`, n = 5, S = 129).
"""
import numpy as np
import torch

import backends as BK
import nerf_oracle as O
import nerf_pytorch_amd._lib as L
import occupancy_cases as OC
import parity_cases as P
import tolerances as TL

f32 = np.float32
SPREAD_YARDSTICK = dict(mul=2.0)
SPREAD_FLOOR = 4.0 * 2.0 ** -24

SHAPES_S = (1, 2, 3, 63, 64, 65, 129, 192)
SHAPES_N = (1, 5, 70)
STRIDES = (8, 11)
KERNEL_KINDS = ("noise_draws", "noise_stream", "zero_density", "opaque_first", "tied_depths", "empty_rows", "near_eq_far")


# ---- the definition, in torch ----------------------------------------------------------------------------------------------------
def spread_of_weights(w, z, rays):
    """L [n] of the header's definition for weights w [n, S] (differentiable), depths z and packed rays, in w's dtype: the S^2 sum."""
    dtype = w.dtype
    z, rays = z.detach().to(dtype), rays.detach().to(dtype)
    near, far = rays[:, 6:7], rays[:, 7:8]
    ok = far > near
    inv = torch.where(ok, 1.0 / torch.where(ok, far - near, torch.ones_like(far)), torch.zeros_like(far))
    s = (z - near) * inv
    e = torch.cat((s[:, 1:], torch.clamp(s[:, -1:], min=1.0)), dim=1)
    m, delta = 0.5 * (s + e), e - s
    pair = (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum(dim=(1, 2))
    return (pair + (w * w * delta).sum(dim=1) / 3.0) * ok[:, 0].to(dtype)   # (inv = 0: L = 0 and a zero gradient)


def spread_reference(raw, z, rays, noise_std, noise, dtype, scale=1.0, g_loss=None):
    """(L [n], scale_ray * dL/dw [n, S], w [n, S]) of the header's definition in `dtype`: the weights from the oracle's compositing,
    autograd for dL/dw."""
    raw, z, rays = (torch.as_tensor(a).to(dtype) for a in (raw, z, rays))
    nz = None if noise is None else torch.as_tensor(noise).to(dtype)
    w = O.volume_render(raw, z, rays[:, 3:6], float(noise_std), nz, False)[3].detach().requires_grad_(True)
    loss = spread_of_weights(w, z, rays)
    sr = torch.full_like(loss, float(scale)) if g_loss is None else float(scale) * torch.as_tensor(g_loss).to(dtype)
    g, = torch.autograd.grad((loss * sr).sum(), w)
    return loss.detach(), g, w.detach()


# ---- the kernel through a backend ---------------------------------------------------------------------------------------------------
def spread_loss(b, raw, z, rays, noise_std=0.0, noise=None, seed=0, rng_stream=1, ray_offset=0, scale=1.0, g_loss=None,
                want_loss=True, want_g=True, raise_on_error=True, n=None, s=None, stride=None, null=()):
    """nerfhip_spread_loss on numpy inputs: (loss [n] or None, g_weights [n, S] or None); with raise_on_error=False: (rc, loss, g) with
    the outputs as the call left them (NaN-filled before).  null: names of inputs passed as NULL."""
    nn, ss = z.shape
    n, s, stride = (nn if n is None else n), (ss if s is None else s), (rays.shape[1] if stride is None else stride)
    d = dict(raw=b.dev(np.ascontiguousarray(raw, f32)), z=b.dev(np.ascontiguousarray(z, f32)), rays=b.dev(np.ascontiguousarray(rays, f32)))
    dn, dg = b.devopt(noise), b.devopt(g_loss)
    lo = b.empty((nn,)) if want_loss else None
    gw = b.empty((nn, ss)) if want_g else None
    args = (*[None if k in null else b.ptr(d[k]) for k in ("raw", "z", "rays")], stride, n, s, float(noise_std), b.p(dn), seed, rng_stream,
            ray_offset, float(scale), b.p(dg), b.p(lo), b.p(gw), b.stream())
    if not raise_on_error:
        rc = b.lib._dll.nerfhip_spread_loss(*args)
        return rc, (None if lo is None else b.host(lo)), (None if gw is None else b.host(gw))
    b.lib.spread_loss(*args)
    return (None if lo is None else b.host(lo)), (None if gw is None else b.host(gw))


def kernel_inputs(kind, n, S, stride, seed):
    """One case's inputs and the rays on which the definition is degenerate (exactly zero L and gradient).  sigma is mostly on (a ray
    needs weight to have a spread), a quarter of the samples of rays with S >= 3 sit behind an off ReLU."""
    g = np.random.default_rng(seed)
    rays = g.normal(size=(n, stride)).astype(f32)
    rays[:, 6] = 2.0 + 0.5 * g.random(n)
    rays[:, 7] = 6.0 + 0.5 * g.random(n)
    z = np.sort(rays[:, 6:7] + (rays[:, 7:8] - rays[:, 6:7]) * g.random((n, S)), axis=1).astype(f32)
    raw = (g.normal(size=(n, S, 4)) * 1.5).astype(f32)
    raw[..., 3] = 0.5 + 1.5 * np.abs(raw[..., 3])
    if S >= 3:
        off = g.random((n, S)) < 0.25
        off[:, 0] = False
        raw[..., 3] = np.where(off, -raw[..., 3], raw[..., 3])
    c = dict(raw=raw, z=z, rays=rays, noise_std=0.0, noise=None, seed=0, rng_stream=1, ray_offset=0, degenerate=np.zeros(n, bool))
    if kind == "noise_draws":
        c.update(noise_std=0.3, noise=g.normal(size=(n, S)).astype(f32))
    elif kind == "noise_stream":   # (the reference gets the kernel's own draws from nerfhip_rng_fill: check_kernel)
        c.update(noise_std=0.3, seed=4321 + seed, rng_stream=3, ray_offset=17)
    elif kind == "zero_density":
        raw[0, :, 3] = -np.abs(raw[0, :, 3])
        c["degenerate"][0] = True
    elif kind == "opaque_first":
        raw[0, 0, 3] = 1e4
    elif kind == "tied_depths":   # (runs of equal depths; from S = 3 on also last depths beyond `far`: s_{S-1} > 1, delta_{S-1} = 0)
        z[:] = np.sort(np.floor(z * 4.0) / 4.0 + (0.5 if S >= 3 else 0.0), axis=1)
    elif kind == "empty_rows":
        raw[0] = OC.EMPTY
        c["degenerate"][0] = True
        if S >= 3:
            raw[:, 1::3] = OC.EMPTY
    elif kind == "near_eq_far":
        rays[0, 7] = rays[0, 6]
        c["degenerate"][0] = True
        if n > 1:
            rays[1, 7] = rays[1, 6] - 1.0   # (far < near: inv = 0 as well)
            c["degenerate"][1] = True
    else:
        raise KeyError(kind)
    return c


def err_over(got, ref64):
    return float(np.abs(np.asarray(got, np.float64) - ref64).max())


def held_to_yardstick(got, ref64, ref32, what, record=None):
    """got no further from the fp64 run than the fp32 run of the same formula is, x 2, + SPREAD_FLOOR of the largest magnitude."""
    ref64 = ref64.numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref64)), what
    mag = float(np.abs(ref64).max())
    e_got, e_ref = err_over(got, ref64), err_over(ref32.numpy(), ref64)
    if record is not None and mag > 0:
        record.append((what, e_got / mag * 2.0 ** 24, e_ref / mag * 2.0 ** 24))
    print("%s: kernel %.3e  fp32 formula %.3e  magnitude %.3e" % (what, e_got, e_ref, mag))
    assert e_got <= SPREAD_YARDSTICK["mul"] * e_ref + SPREAD_FLOOR * mag, (what, e_got, e_ref, mag)


def check_kernel(b, kind, n, S, stride, seed, record=None):
    c = kernel_inputs(kind, n, S, stride, seed)
    noise = c["noise"]
    kw = dict(noise_std=c["noise_std"], noise=noise, seed=c["seed"], rng_stream=c["rng_stream"], ray_offset=c["ray_offset"])
    ref_noise = noise
    if kind == "noise_stream":
        ref_noise = b.rng_fill(1, c["seed"], c["rng_stream"], c["ray_offset"] * S, n * S).reshape(n, S)
    g = np.random.default_rng(seed + 1000)
    g_loss = (0.5 + g.random(n)).astype(f32) * np.where(g.random(n) < 0.5, -1.0, 1.0).astype(f32)
    scale = 0.37
    what = "%s n=%d S=%d stride=%d" % (kind, n, S, stride)
    deg = c["degenerate"]
    for gl in (None, g_loss):
        l64, g64, w64 = spread_reference(c["raw"], c["z"], c["rays"], c["noise_std"], ref_noise, torch.float64, scale, gl)
        l32, g32, _ = spread_reference(c["raw"], c["z"], c["rays"], c["noise_std"], ref_noise, torch.float32, scale, gl)
        # not vacuous, from the reference alone: a spread on >= 90 % of the non-degenerate rays, a gradient to compare
        live = ~deg
        if live.any():
            assert float((l64.numpy()[live] > 0).mean()) >= 0.9, (what, l64.numpy()[live])
            assert float(g64.abs().max()) > 0, what
        assert not l64.numpy()[deg].any() and not g64.numpy()[deg].any(), what
        loss, gw = spread_loss(b, c["raw"], c["z"], c["rays"], scale=scale, g_loss=gl, **kw)
        held_to_yardstick(loss, l64, l32, what + " loss", record)
        held_to_yardstick(gw, g64, g32, what + (" g_weights" if gl is None else " g_weights (g_loss)"), record)
        assert not loss[deg].any() and not gw[deg].any(), what   # exactly zero
        # the two single-output calls and a repeat: the combined call's bits
        lo_only, none = spread_loss(b, c["raw"], c["z"], c["rays"], scale=scale, g_loss=gl, want_g=False, **kw)
        none2, g_only = spread_loss(b, c["raw"], c["z"], c["rays"], scale=scale, g_loss=gl, want_loss=False, **kw)
        again = spread_loss(b, c["raw"], c["z"], c["rays"], scale=scale, g_loss=gl, **kw)
        assert none is None and none2 is None
        assert np.array_equal(lo_only, loss) and np.array_equal(g_only, gw), what
        assert np.array_equal(again[0], loss) and np.array_equal(again[1], gw), what
    # the weights the kernel sums are the compositing's own: g_loss = 0 rays and scale = 0 give +-0, and a NaN density propagates
    if kind == "noise_draws" and S >= 2:
        raw = c["raw"].copy()
        raw[0, S // 2, 3] = np.nan
        loss, gw = spread_loss(b, raw, c["z"], c["rays"], **kw)
        assert np.isnan(loss[0]) and np.isnan(gw[0]).any() and not np.isnan(loss[1:]).any() and not np.isnan(gw[1:]).any(), what


def check_kernel_sums(b, kind, n, S, stride, seed):
    """The kernel's sums alone, at any S: with the weights GIVEN -- the library's own compositing weights (nerfhip_volume_render_fwd on
    the same inputs, which the kernel forms bit for bit) -- the S^2 sum in fp64 is exact to ~1e-16, and the kernel's fp64 prefix sums
    must land within the final rounding to fp32 of it: SPREAD_FLOOR of the largest magnitude, no yardstick term.  (Against the oracle's
    own weights a long ray measures the device's expf in alpha = 1 - exp(-sigma dist) at tiny dist, not this kernel.)"""
    c = kernel_inputs(kind, n, S, stride, seed)
    kw = dict(noise_std=c["noise_std"], noise=c["noise"], seed=c["seed"], rng_stream=c["rng_stream"], ray_offset=c["ray_offset"])
    w = b.volume_render_fwd(c["raw"], c["z"], np.ascontiguousarray(c["rays"][:, 3:]), **kw)[3]
    # the S^2 sum in fp64 numpy, a block of rows at a time (S = 8192 fits): A_i = sum_j w_j |m_i - m_j|, L = sum_i w_i A_i + ...,
    # dL/dw_i = 2 A_i + (2/3) w_i delta_i (the S^2 form's own derivative: |m_i - m_j| is symmetric)
    w64, z, rays = w.astype(np.float64), c["z"].astype(np.float64), c["rays"].astype(np.float64)
    sn = (z - rays[:, 6:7]) / (rays[:, 7:8] - rays[:, 6:7])
    en = np.concatenate((sn[:, 1:], np.maximum(sn[:, -1:], 1.0)), axis=1)
    m, delta = 0.5 * (sn + en), en - sn
    A = np.concatenate([(w64[:, None, :] * np.abs(m[:, i:i + 256, None] - m[:, None, :])).sum(axis=2) for i in range(0, S, 256)], axis=1)
    l64, g64 = (w64 * A).sum(axis=1) + (w64 * w64 * delta).sum(axis=1) / 3.0, 2.0 * A + (2.0 / 3.0) * w64 * delta
    loss, gw = spread_loss(b, c["raw"], c["z"], c["rays"], **kw)
    assert float((l64 > 0).mean()) >= 0.9 and float(np.abs(g64).max()) > 0
    for got, ref, what in ((loss, l64, "loss"), (gw, g64, "g_weights")):
        mag = float(np.abs(ref).max())
        e = err_over(got, ref)
        print("%s n=%d S=%d sums %s: %.3e of the magnitude (%.2f x 2^-24)" % (kind, n, S, what, e / mag, e / mag * 2.0 ** 24))
        assert e <= SPREAD_FLOOR * mag, (kind, n, S, what, e, mag)


def case_kernel(b, kind, record=None):
    """Every S with every n; the first kind with both ray strides at each, the others alternating between the two."""
    seed = 100 * KERNEL_KINDS.index(kind)
    for S in SHAPES_S:
        for n in SHAPES_N:
            for stride in (STRIDES if kind == KERNEL_KINDS[0] else STRIDES[seed % 2:seed % 2 + 1]):
                seed += 1
                check_kernel(b, kind, n, S, stride, seed, record)


def case_kernel_refusals(b):
    """Every refusal returns NERFHIP_ERR_ARG and leaves both outputs untouched; n == 0 is OK and launches nothing."""
    c = kernel_inputs("noise_draws", 4, 5, 8, 1)
    base = dict(noise_std=0.0, raise_on_error=False)

    def refused(match, **kw):
        rc, lo, gw = spread_loss(b, c["raw"], c["z"], c["rays"], **dict(base, **kw))
        assert rc == -1 and match in b.lib.last_error().decode(), (rc, b.lib.last_error())
        assert (lo is None or np.isnan(lo).all()) and (gw is None or np.isnan(gw).all())

    refused("NULL", null=("raw",))
    refused("NULL", null=("z",))
    refused("NULL", null=("rays",))
    refused("ray_stride", stride=7)
    refused("samples per ray", s=0)
    refused("samples per ray", s=8193)
    refused("n < 0", n=-1)
    refused("both outputs", want_loss=False, want_g=False)
    rc, lo, gw = spread_loss(b, c["raw"], c["z"], c["rays"], n=0, **base)
    assert rc == 0 and np.isnan(lo).all() and np.isnan(gw).all()
    rc, lo, gw = spread_loss(b, c["raw"], c["z"], c["rays"], n=0, null=("raw", "z", "rays"), **base)
    assert rc == 0


# ---- through the render -------------------------------------------------------------------------------------------------------------
BOTH = L.PART_COARSE | L.PART_FINE
RENDER_NETS = ("w64", "w128", "w256", "w40of64")
RENDER_ARITHS = {"fp32": 0, "f16x3_train": P.F16X3_TRAIN}
RENDER_SHAPES = ((48, 8, 8), (150, 13, 5))
LAMBDA = (0.02, 0.01)   # (coarse, fine) weights of the spread term in the render cases: mip-NeRF 360's 0.01 and twice that


# One training forward of two nets on a backend and the backward entry points over it, with the spread kernel reading the forward's own
# raw rows and depths in the workspace.  layout: 1 (one set of backward buffers per net) or 2 (shared).
RenderW = BK.Rendered


def setup(b, net, arith, seed):
    """occupancy_cases.setup with the training arithmetics of this file."""
    cfg = OC.NETS[net]
    plan, params, flat, packed = P.mlp_setup(b, cfg, seed=seed, precision=RENDER_ARITHS[arith])
    return cfg, plan, params, flat, packed


def render_problem(net, n, nc, nf, seed, noise=0.3, white=False):
    cfg = OC.NETS[net]
    rays, rand = OC.render_inputs(cfg, n, nc, nf, seed)
    tgt = torch.rand(n, 3, generator=P.rng(seed + 1))
    opt = dict(num_coarse=nc, num_fine=nf, perturb=True, lindisp=False, white_background=white, noise_std=noise)
    return cfg, rays.numpy(), {k: v.numpy() for k, v in rand.items()}, opt, tgt.numpy()


def spread_cotangents(r, lam, g_loss=(None, None)):
    """The two passes' weight cotangents of lam_c mean(L_c) + lam_f mean(L_f) over the forward in r's workspace (device), + the losses."""
    lc, gwc = r.spread(False, lam[0] / r.n, g_loss[0])
    lf, gwf = r.spread(True, lam[1] / r.n, g_loss[1])
    return (gwc, gwf), (lc, lf)


def case_w_bits(b, net, arith, layout, shapes=RENDER_SHAPES):
    """nerfhip_render_bwd_parts_w / _rays_w with NULL weight cotangents give the bits of nerfhip_render_bwd_parts / _rays; with the spread
    kernel's g_weights, the d(loss)/d(raw) rows each pass's compositing backward leaves in the workspace are those of a hand-assembled
    nerfhip_volume_render_bwd(..., g_weights, ...) on the same regions, bit for bit -- and are not the rows without the weight cotangent."""
    _, pc, _, _, packed_c = setup(b, net, arith, seed=3)
    _, pf, _, _, packed_f = setup(b, net, arith, seed=4)
    for n, nc, nf in shapes:
        cfg, rays, rand, opt, tgt = render_problem(net, n, nc, nf, seed=31)
        r = RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand, layout)
        _, gc, gf = b.mse_loss(r.out["rgb_coarse"], r.out["rgb_fine"], tgt)
        old = r.backward((gc, gf), entry="parts")
        r.forward()
        new = r.backward((gc, gf), entry="parts_w")
        for k in ("g_params_coarse", "g_params_fine"):
            assert np.array_equal(old[k], new[k]), (net, arith, layout, k)
        r.forward()
        gw, (lc, lf) = spread_cotangents(r, LAMBDA)
        assert (lc > 0).mean() >= 0.9 and (lf > 0).mean() >= 0.9
        rd = np.ascontiguousarray(rays[:, 3:])
        for fine, part, tag, g_rgb, noise in ((True, L.PART_FINE, "fine", gf, rand["noise_fine"]), (False, L.PART_COARSE, "coarse", gc, rand["noise_coarse"])):
            got = r.backward((gc, gf), gw, entry="parts_w", parts=part)
            g_raw = r.region("bwd_g_raw_" + tag)
            args = (r.region("raw_" + tag), r.region("z_" + tag), rd)
            kw = dict(noise_std=opt["noise_std"], noise=noise, white=opt["white_background"])
            want = b.volume_render_bwd(*args, g_rgb, None, None, b.host(gw[1 if fine else 0]), **kw)
            plain = b.volume_render_bwd(*args, g_rgb, None, None, None, **kw)
            assert np.array_equal(g_raw, want), (net, arith, layout, tag, float(np.abs(g_raw - want).max()))
            assert not np.array_equal(want, plain)
            assert not np.array_equal(got["g_params_" + tag], old["g_params_" + tag])
            # the exact-zero claim: a weight cotangent moves no d(loss)/d(raw) row that the colour cotangent alone leaves at zero behind an
            # off ReLU or T = 0 (k_volume_render_bwd's mask and T factors)
            off = (r.region("raw_" + tag)[..., 3] + opt["noise_std"] * noise) <= 0
            assert off.any() and not want[off][:, 3].any()
        # a weight cotangent ALONE runs a pass (no colour cotangent at all)
        r.forward()
        alone = r.backward((None, None), gw, entry="parts_w")
        assert np.isfinite(alone["g_params_fine"]).all() and alone["g_params_fine"].any() and alone["g_params_coarse"].any()
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


def oracle_total_loss(w, z_c, z_f, rays, tgt, lam):
    """MSE terms + lam_c mean(L_c) + lam_f mean(L_f) of an O.render_at_depths result, in its dtype."""
    loss, _, _, _ = O.loss_and_psnr(w["rgb_coarse"], w["rgb_fine"], tgt)
    return (loss + lam[0] * spread_of_weights(w["weights_coarse"], z_c, rays).mean()
            + lam[1] * spread_of_weights(w["weights_fine"], z_f, rays).mean())


def _teacher(par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, lam, dtype, wrt_rays=False, want_margin=False):
    """The oracle's autograd of the total loss on GIVEN depths in `dtype`: ({tensor: grad} coarse, fine, d/d(rays) or None, margin)."""
    cast = lambda d: {k: torch.as_tensor(v).to(dtype) for k, v in d.items()}
    pc = {k: v.detach().to(dtype).requires_grad_(True) for k, v in par_c.items()}
    pf = {k: v.detach().to(dtype).requires_grad_(True) for k, v in par_f.items()}
    r = torch.as_tensor(rays).to(dtype).requires_grad_(wrt_rays)
    zc, zf = torch.as_tensor(z_c).to(dtype), torch.as_tensor(z_f).to(dtype)
    w = O.render_at_depths(r, zc, zf, pc, pf, cfg, cfg, opt, cast(rand), want_margin=want_margin)
    oracle_total_loss(w, zc, zf, r, torch.as_tensor(tgt).to(dtype), lam).backward()
    return ({k: v.grad.numpy() for k, v in pc.items()}, {k: v.grad.numpy() for k, v in pf.items()},
            r.grad.numpy() if wrt_rays else None, w["relu_margin"].numpy() if want_margin else None)


def case_param_grads(b, net, arith, shapes=RENDER_SHAPES, min_decided=0.3):
    """Parameter gradients of MSE + lam * mean(L) through nerfhip_spread_loss + nerfhip_render_bwd_parts_w against the oracle's autograd
    of the same loss, teacher-forced on the kernels' own depths (O.render_at_depths; the spread term restated by spread_of_weights),
    ReLU-margin filtered: the comparison runs on the rays all of whose samples pass tolerances.py `relu_margin` in the oracle's fp64
    forward -- the kernels run on exactly those rays (their rows of the draws: a ray's depths do not depend on the other rays).  Bound:
    `tf.grad.filtered`'s maximum, of max|g| per tensor, imported from tolerances.py."""
    tol = TL.bound("tf.grad.filtered", arith)[0]
    cfg, pc, par_c, _, packed_c = setup(b, net, arith, seed=3)
    _, pf, par_f, _, packed_f = setup(b, net, arith, seed=4)
    for n, nc, nf in shapes:
        _, rays, rand, opt, tgt = render_problem(net, n, nc, nf, seed=33)
        r = RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
        z_c, z_f = r.region("z_coarse"), r.region("z_fine")
        _, _, _, margin = _teacher(par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, LAMBDA, torch.float64, want_margin=True)
        keep = margin > TL.bound("relu_margin")
        assert keep.mean() >= min_decided, (net, n, float(keep.mean()))
        rays, tgt, rand = rays[keep], tgt[keep], {k: np.ascontiguousarray(v[keep]) for k, v in rand.items()}
        r = RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
        assert np.array_equal(r.region("z_coarse"), z_c[keep]) and np.array_equal(r.region("z_fine"), z_f[keep])
        _, gc, gf = b.mse_loss(r.out["rgb_coarse"], r.out["rgb_fine"], tgt)
        gw, _ = spread_cotangents(r, LAMBDA)
        got = r.backward((gc, gf), gw, entry="parts_w")
        ref_c, ref_f, _, _ = _teacher(par_c, par_f, cfg, rays, z_c[keep], z_f[keep], opt, rand, tgt, LAMBDA, torch.float32)
        mse_c, mse_f, _, _ = _teacher(par_c, par_f, cfg, rays, z_c[keep], z_f[keep], opt, rand, tgt, (0.0, 0.0), torch.float32)
        for tag, plan, ref, mse in (("coarse", pc, ref_c, mse_c), ("fine", pf, ref_f, mse_f)):
            g = b.unflatten(plan, got["g_params_" + tag])
            # not vacuous, from the reference alone: the spread term moves the net's gradient by far more than the bound
            moved = max(float(np.abs(v - mse[k]).max()) / float(np.abs(v).max()) for k, v in ref.items())
            assert moved > 10.0 * tol, (tag, moved)
            for k, v in ref.items():
                err = float(np.abs(g[k] - v).max()) / float(np.abs(v).max())
                print("param grads %s %s n=%d %s %s: %.3e of max|g| (bound %.1e)" % (net, arith, n, tag, k, err, tol))
                assert err <= tol, (net, arith, n, tag, k, err, tol)
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


def case_compacted(b, net, arith, modes, n=48, nc=8, nf=8, noise=0.6):
    """The backward modes with a weight cotangent: modes 1, 2 (and 3, 4, 5 where asked) against mode 0 within `unit.compact_vs_dense` of
    max|g| per tensor; `kept` equals the count of nonzero d(loss)/d(raw) rows the compositing backward left -- the exact-zero claim:
    k_volume_render_bwd's mask and T factors leave a row at zero where the ReLU is off or T = 0 whatever g_weights holds.  The zero
    rows are the renderer's own (sigma noise `noise` over the nets' raw densities), as in parity_cases.case_render_compacted; the case
    asserts that some rows are kept and some dropped in both passes."""
    ctol = TL.bound("unit.compact_vs_dense", arith)
    cfg, pc, _, _, packed_c = setup(b, net, arith, seed=3)
    _, pf, _, _, packed_f = setup(b, net, arith, seed=4)
    _, rays, rand, opt, tgt = render_problem(net, n, nc, nf, seed=35, noise=noise)
    res = {}
    for mode in (False,) + tuple(modes):
        b.set_compaction(pc, mode)
        b.set_compaction(pf, mode)
        r = RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
        if mode is False:
            _, gc, gf = b.mse_loss(r.out["rgb_coarse"], r.out["rgb_fine"], tgt)
        gw, _ = spread_cotangents(r, LAMBDA)
        out = {}
        for fine, part, tag in ((True, L.PART_FINE, "fine"), (False, L.PART_COARSE, "coarse")):
            got = r.backward((gc, gf), gw, entry="parts_w", parts=part)
            out["g_params_" + tag] = got["g_params_" + tag]
            nonzero = int(r.region("bwd_g_raw_" + tag).reshape(-1, 4).any(axis=1).sum())
            if mode in (True, "recompute", "fused_compact"):
                kept, total = r.kept(tag)
                assert total == n * (nc + (nf if fine else 0)) and kept == nonzero and 0 < kept < total, (mode, tag, kept, nonzero, total)
            else:
                assert 0 < nonzero < n * (nc + (nf if fine else 0))
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


def case_rays_w(b, net="w128", n=48, nc=8, nf=8):
    """nerfhip_render_bwd_rays_w: d(loss)/d(rays) of MSE + lam * mean(L) against the oracle's autograd teacher-forced on the kernels' own
    depths, under parity_cases.case_ray_grad's distribution bound (median <= 3 x the oracle's own fp32-vs-fp64 median + 2e-6; no more
    rays beyond 2e-3 than 2 x the oracle's + 3); with NULL weight cotangents: nerfhip_render_bwd_rays' bits."""
    cfg, pc, par_c, flat_c, packed_c = setup(b, net, "fp32", seed=3)
    _, pf, par_f, flat_f, packed_f = setup(b, net, "fp32", seed=4)
    _, rays, rand, opt, tgt = render_problem(net, n, nc, nf, seed=37, noise=0.0)
    lam = (0.5, 0.5)   # (a spread term of the MSE terms' size in the ray gradient, so that the comparison is about it)
    r = RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
    z_c, z_f = r.region("z_coarse"), r.region("z_fine")
    _, gc, gf = b.mse_loss(r.out["rgb_coarse"], r.out["rgb_fine"], tgt)
    old = r.backward((gc, gf), entry="rays", params=(flat_c, flat_f))
    r.forward()
    null = r.backward((gc, gf), entry="rays_w", params=(flat_c, flat_f))
    for k in old:
        assert np.array_equal(old[k], null[k]), k
    r.forward()
    gw, _ = spread_cotangents(r, lam)
    got = r.backward((gc, gf), gw, entry="rays_w", params=(flat_c, flat_f))["g_rays"]
    ref = _teacher(par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, lam, torch.float32, wrt_rays=True)[2]
    ref64 = _teacher(par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, lam, torch.float64, wrt_rays=True)[2]
    plain64 = _teacher(par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, (0.0, 0.0), torch.float64, wrt_rays=True)[2]
    assert np.isfinite(ref64).all() and float(np.any(ref64[:, 0:3] != 0.0, axis=1).mean()) >= 0.9
    for lo, hi, what in ((0, 3, "origin"), (3, 6, "direction"), (8, 11, "viewdirs")):
        scale = float(np.abs(ref64[:, lo:hi]).max())
        assert scale > 0.0, what
        # (the spread term is in it -- but for the view directions: the density, and so the weights, do not depend on them)
        assert what == "viewdirs" or float(np.abs(ref64[:, lo:hi] - plain64[:, lo:hi]).max()) > 1e-2 * scale, what
        e_hip = np.abs(got[:, lo:hi] - ref[:, lo:hi]).max(axis=1) / scale
        e_yard = np.abs(ref[:, lo:hi] - ref64[:, lo:hi]).max(axis=1) / scale
        print("rays_w %s: median %.3e (oracle fp32 vs fp64 %.3e), beyond 2e-3: %d (%d)" % (what, np.median(e_hip), np.median(e_yard),
                                                                                        (e_hip > 2e-3).sum(), (e_yard > 2e-3).sum()))
        assert np.median(e_hip) <= 3.0 * np.median(e_yard) + 2e-6, what
        assert (e_hip > 2e-3).sum() <= 2 * (e_yard > 2e-3).sum() + 3, what
    assert np.all(got[:, 6:8] == 0.0)
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


# ---- the culled step of the occupancy grid with a spread term -------------------------------------------------------------------------
def case_culled_step(b, net, arith, outside, n=21, nc=9, nf=6, noise_std=0.3, lam=(0.05, 0.05)):
    """occupancy_train_cases.case_half_empty with a spread term: arm A by hand in mode 1 (training forward, the library's own flags, the
    culled rows overwritten with the empty row, compositing again), arm B nerfhip_render_fwd_occ_train in mode 2 and (where the plan
    has it) 4; in both arms nerfhip_spread_loss over the workspace and nerfhip_render_bwd_parts_w.  By that case's own criteria: the
    weight cotangents bit-identical (the spread kernel reads the same rows), each net's kept count equal, gradients array_equal in mode 2
    and within unit.compact_vs_dense of max|g| per tensor in mode 4 -- and not the gradients without the spread term."""
    import occupancy_train_cases as OT
    cfg, pc, pf, packed_c, packed_f, modes = OT.nets_and_modes(b, net, arith)
    rays, rnp, tgt = OT.half_empty_inputs(cfg, n, nc, nf)
    grid = OC.Grid(b, OT.half_empty_bits(rays, 23), *OC.SCENE_BOX, (8, 8, 16), outside)
    opt = dict(num_coarse=nc, num_fine=nf, perturb=True, white_background=True, noise_std=noise_std)
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
        out = b.volume_render_fwd(raw, z, rd, noise_std, rnp["noise_fine" if fine else "noise_coarse"], True)
        for k, v in zip(("rgb", "disp", "acc", None, "depth"), out):
            if k:
                a.set_map(k + "_" + tag, v)
        if not fine:
            a.set_region("weights_coarse", out[3])
    want = a.maps()
    gw_a, losses = spread_cotangents(a, lam)
    assert all((lo >= 0).all() for lo in losses)
    plain = a.bwd(want["rgb_coarse"] - tgt, want["rgb_fine"] - tgt)
    want.update(a.bwd(want["rgb_coarse"] - tgt, want["rgb_fine"] - tgt, gw_a))
    assert not np.array_equal(want["g_coarse"], plain["g_coarse"]) and not np.array_equal(want["g_fine"], plain["g_fine"])
    assert want["kept_coarse"] == plain["kept_coarse"] and want["kept_fine"] == plain["kept_fine"]   # (a weight cotangent wakes no row)
    ctol = TL.bound("unit.compact_vs_dense", arith if arith == "fp32" else "f16x3_train")
    for mode in modes:
        for p in (pc, pf):
            b.set_compaction(p, mode)
        s = OT.Step(b, pc, pf, packed_c, packed_f, rays, opt, rnp)
        s.fwd_occ(grid)
        got = s.maps()
        gw, losses = spread_cotangents(s, lam)
        assert all((lo >= 0).all() for lo in losses)
        for i in (0, 1):
            assert np.array_equal(b.host(gw[i]), b.host(gw_a[i])), (mode, i)
        got.update(s.bwd(got["rgb_coarse"] - tgt, got["rgb_fine"] - tgt, gw))
        for tag, plan in (("coarse", pc), ("fine", pf)):
            assert got["kept_" + tag] == want["kept_" + tag], (mode, tag, got["kept_" + tag], want["kept_" + tag])
            g, w = got["g_" + tag], want["g_" + tag]
            assert w.any() and np.isfinite(g).all()
            if mode == "recompute":
                assert np.array_equal(g, w), (tag, float(np.abs(g - w).max()))
            else:
                gd, gk = b.unflatten(plan, w), b.unflatten(plan, g)
                for k in gd:
                    d = float(np.abs(gk[k] - gd[k]).max()) / (float(np.abs(gd[k]).max()) + 1e-30)
                    assert d <= ctol, (mode, tag, k, d, ctol)
    for p in (pc, pf):
        b.lib.plan_destroy(p)
