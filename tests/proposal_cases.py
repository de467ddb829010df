"""Cases of the interlevel proposal loss (mip-NeRF 360's L_prop; include/nerfhip.h nerfhip_proposal_loss, csrc/reg/proposal.hip) and of
its coarse weight cotangent through the fused backward, shared by the emulator suite (tests/test_proposal.py) and the GPU suite
(tests/test_gpu_proposal.py).  Every case drives the C ABI through a backend's library handle (tests/backends.py).

The definition is restated here independently of the kernel: torch.searchsorted for lo_i and hi_i, a masked sum for B_i, autograd for
dL/dw^.  The weights it is evaluated on are the LIBRARY'S OWN (nerfhip_volume_render_fwd through the same backend, with the same
noise arguments): the kernel forms exactly those, so what is compared is the kernel's index algebra and sums, not expf.

PROPOSAL_BOUND: each output of the kernel is an fp64 quantity rounded to fp32 once, so |got - ref| <= 2 * 2^-24 * max|ref| of the
case (half an ulp of the largest magnitude; the factor 2 covers the fp64 reassociation of the prefix differences, ~1e-12 here).  It is
derived, not measured.
"""
import numpy as np
import torch

import nerf_oracle as O
import nerf_pytorch_amd._lib as L
import occupancy_cases as OC
import spread_cases as S
import tolerances as TL

f32 = np.float32
PROPOSAL_BOUND = 2.0 * 2.0 ** -24
EPS = 2.0 ** -23
CAP = 4096

SHAPES = ((1, 1), (2, 1), (3, 5), (7, 3), (63, 64), (64, 192), (65, 129), (129, 200))
SHAPES_N = (1, 5, 70)
STRIDES = (8, 11)
KERNEL_KINDS = ("refining", "free", "tied_depths", "last_beyond_far", "noise_draws", "noise_stream", "zero_coarse", "zero_fine",
                "empty_rows", "opaque_first")


# ---- the definition, in torch ----------------------------------------------------------------------------------------------------
def proposal_ranges(z_c, z_f, far):
    """(lo, hi) [n, Sf] int64 of the header's definition, from the depths as they are (fp32 comparisons are exact in any dtype)."""
    ec = torch.cat((z_c, torch.maximum(far, z_c[:, -1:])), dim=1).contiguous()
    ef = torch.cat((z_f, torch.maximum(far, z_f[:, -1:])), dim=1).contiguous()
    Sc = z_c.shape[1]
    lo = torch.searchsorted(ec[:, 1:].contiguous(), ef[:, :-1].contiguous(), right=True).clamp(max=Sc - 1)
    hi = torch.maximum(torch.searchsorted(ec[:, :-1].contiguous(), ef[:, 1:].contiguous(), right=False) - 1, lo)
    return lo, hi


def proposal_of_weights(w_c, w_f, z_c, z_f, rays):
    """L [n] of the header's definition for coarse weights w_c [n, Sc] (differentiable) and fine weights w_f [n, Sf] (a constant of
    the term: detached here), in w_c's dtype."""
    dtype = w_c.dtype
    z_c, z_f, far = z_c.detach().to(dtype), z_f.detach().to(dtype), rays.detach().to(dtype)[:, 7:8]
    w_f = w_f.detach().to(dtype)
    lo, hi = proposal_ranges(z_c, z_f, far)
    j = torch.arange(z_c.shape[1])
    mask = (lo[:, :, None] <= j) & (j <= hi[:, :, None])                      # [n, Sf, Sc]
    B = (mask.to(dtype) * w_c[:, None, :]).sum(dim=2)
    return (torch.clamp(w_f - B, min=0.0) ** 2 / (w_f + EPS)).sum(dim=1)


def proposal_reference(w_c, w_f, z_c, z_f, rays, scale=1.0, g_loss=None):
    """(L [n], scale_ray dL/dw^ [n, Sc]) in fp64 on GIVEN fp32 weights; scale and g_loss as the kernel takes them (fp32 values)."""
    t = lambda a: torch.as_tensor(np.asarray(a, f32)).to(torch.float64)  # noqa: E731
    wc = t(w_c).requires_grad_(True)
    loss = proposal_of_weights(wc, t(w_f), t(z_c), t(z_f), t(rays))
    sr = torch.full_like(loss, float(f32(scale))) if g_loss is None else float(f32(scale)) * t(g_loss)
    g, = torch.autograd.grad((loss * sr).sum(), wc)
    return loss.detach().numpy(), g.numpy()


# ---- the kernel through a backend ---------------------------------------------------------------------------------------------------
INPUTS = ("raw_c", "z_c", "raw_f", "z_f", "rays")


def proposal_loss(b, c, scale=1.0, g_loss=None, want_loss=True, want_g=True, accumulate=False, prefill=None, raise_on_error=True,
                  n=None, sc=None, sf=None, stride=None, null=()):
    """nerfhip_proposal_loss on a case's numpy inputs: (loss [n] or None, g_weights_coarse [n, Sc] or None); with raise_on_error=False:
    (rc, loss, g) with the outputs as the call left them (NaN-filled before, or `prefill` for g).  null: inputs passed as NULL."""
    nn, Sc = c["z_c"].shape
    Sf = c["z_f"].shape[1]
    d = {k: b.dev(np.ascontiguousarray(c[k], f32)) for k in INPUTS}
    dnc, dnf, dg = b.devopt(c["noise_c"]), b.devopt(c["noise_f"]), b.devopt(g_loss)
    lo = b.empty((nn,)) if want_loss else None
    gw = None
    if want_g:
        gw = b.empty((nn, Sc)) if prefill is None else b.dev(np.ascontiguousarray(prefill, f32))
    p = {k: (None if k in null else b.ptr(d[k])) for k in INPUTS}
    args = (p["raw_c"], p["z_c"], Sc if sc is None else sc, p["raw_f"], p["z_f"], Sf if sf is None else sf, p["rays"],
            c["rays"].shape[1] if stride is None else stride, nn if n is None else n, float(c["noise_std"]), b.p(dnc), b.p(dnf),
            c["seed"], c["ray_offset"], float(scale), b.p(dg), b.p(lo), b.p(gw), int(accumulate), b.stream())
    host = lambda a: None if a is None else np.array(b.host(a), copy=True)  # noqa: E731
    if not raise_on_error:
        rc = b.lib._dll.nerfhip_proposal_loss(*args)
        return rc, host(lo), host(gw)
    b.lib.proposal_loss(*args)
    return host(lo), host(gw)


def library_weights(b, c):
    """(w^ [n, Sc], w [n, Sf]): nerfhip_volume_render_fwd's weights of both passes through backend b, with the case's noise arguments
    (streams 1 and 3)."""
    rd = np.ascontiguousarray(c["rays"][:, 3:])
    kw = dict(noise_std=c["noise_std"], seed=c["seed"], ray_offset=c["ray_offset"])
    return (b.volume_render_fwd(c["raw_c"], c["z_c"], rd, noise=c["noise_c"], rng_stream=1, **kw)[3],
            b.volume_render_fwd(c["raw_f"], c["z_f"], rd, noise=c["noise_f"], rng_stream=3, **kw)[3])


def _raw(g, n, S):
    """spread_cases.kernel_inputs' densities: sigma mostly on, a quarter of the samples of rays with S >= 3 behind an off ReLU."""
    raw = (g.normal(size=(n, S, 4)) * 1.5).astype(f32)
    raw[..., 3] = 0.5 + 1.5 * np.abs(raw[..., 3])
    if S >= 3:
        off = g.random((n, S)) < 0.25
        off[:, 0] = False
        raw[..., 3] = np.where(off, -raw[..., 3], raw[..., 3])
    return raw


def kernel_inputs(kind, n, Sc, Sf, stride, seed):
    """One case's inputs.  zero_rays: the rays on which L and the gradient are exactly zero by construction."""
    g = np.random.default_rng(seed)
    rays = g.normal(size=(n, stride)).astype(f32)
    rays[:, 6] = 2.0 + 0.5 * g.random(n)
    rays[:, 7] = 6.0 + 0.5 * g.random(n)
    span = lambda S: (rays[:, 6:7] + (rays[:, 7:8] - rays[:, 6:7]) * g.random((n, S))).astype(f32)  # noqa: E731
    z_c = np.sort(span(Sc), axis=1)
    if kind == "free" or Sf < Sc:      # independent depths (a union needs Sf >= Sc)
        z_f = np.sort(span(Sf), axis=1)
    else:                              # refining: the sorted union of the coarse depths and extra draws inside [z^_0, z^_last]
        extra = np.clip(span(Sf - Sc), z_c[:, :1], z_c[:, -1:])
        z_f = np.sort(np.concatenate((z_c, extra), axis=1), axis=1)
    raw_c, raw_f = _raw(g, n, Sc), _raw(g, n, Sf)
    c = dict(raw_c=raw_c, z_c=z_c, raw_f=raw_f, z_f=z_f, rays=rays, noise_std=0.0, noise_c=None, noise_f=None, seed=0, ray_offset=0,
             zero_rays=np.zeros(n, bool))
    if kind in ("refining", "free"):
        pass
    elif kind == "tied_depths":
        # floor(4 z) / 4 on a random quarter of each pass's samples: runs of equal depths, zero-width intervals and edges that coincide
        # between the passes, next to untied samples.  (Tying EVERY sample leaves 18 distinct depths: at Sc = 65 fewer than 10 % of the
        # coarse intervals have a width, and the condition on the inputs -- built_case -- cannot hold.)
        for z in (z_c, z_f):
            z[:] = np.sort(np.where(g.random(z.shape) < 0.25, np.floor(z * 4.0) / 4.0, z), axis=1)
    elif kind == "last_beyond_far":  # (every other ray: far inside the sampled range, so z_last >= far in both passes)
        rays[::2, 7] = (0.5 * (z_c[::2, 0] + z_c[::2, -1])).astype(f32)
        if n > 2:
            rays[2, 7] = z_f[2, -1]  # (and z_last == far exactly)
    elif kind == "noise_draws":
        c.update(noise_std=0.3, noise_c=g.normal(size=(n, Sc)).astype(f32), noise_f=g.normal(size=(n, Sf)).astype(f32))
    elif kind == "noise_stream":     # (in-kernel draws: the reference weights come from the library with the same key)
        c.update(noise_std=0.3, seed=4321 + seed, ray_offset=17)
    elif kind == "zero_coarse":      # B = 0 on ray 0: the gradient there is -2 w / (w + eps) summed over the overlapping fine samples
        raw_c[0, :, 3] = -np.abs(raw_c[0, :, 3])
    elif kind == "zero_fine":        # w = 0 on ray 0: L = 0 and a zero gradient, exactly
        raw_f[0, :, 3] = -np.abs(raw_f[0, :, 3])
        c["zero_rays"][0] = True
    elif kind == "empty_rows":       # (what the culled step leaves: w = 0 at a culled sample)
        raw_c[0], raw_f[0] = OC.EMPTY, OC.EMPTY
        c["zero_rays"][0] = True
        if Sf >= 3:
            raw_f[:, 1::3] = OC.EMPTY
        if Sc >= 3:
            raw_c[:, 2::3] = OC.EMPTY
    elif kind == "opaque_first":
        raw_c[0, 0, 3] = 1e4
        raw_f[0, 0, 3] = 1e4
    else:
        raise KeyError(kind)
    return c


def built_case(b, kind, n, Sc, Sf, stride, seed):
    """kernel_inputs + the library's weights + the fp64 reference at scale 1 -- and the condition on the inputs, asserted here from the
    reference alone: with Sf >= 3, L > 0 on at least half of the rays that are not zero by construction, and at least 10 % of their
    coarse gradient entries non-zero (a comparison over an all-zero loss shows nothing)."""
    c = kernel_inputs(kind, n, Sc, Sf, stride, seed)
    c["w_c"], c["w_f"] = library_weights(b, c)
    l64, g64 = proposal_reference(c["w_c"], c["w_f"], c["z_c"], c["z_f"], c["rays"])
    live = ~c["zero_rays"]
    assert not l64[~live].any() and not g64[~live].any(), (kind, n, Sc, Sf)
    if Sf >= 3 and live.any():
        assert float((l64[live] > 0).mean()) >= 0.5, (kind, n, Sc, Sf, l64)
        assert float((g64[live] != 0).mean()) >= 0.1, (kind, n, Sc, Sf, float((g64[live] != 0).mean()))
    if kind == "zero_coarse":
        assert not c["w_c"][0].any() and (Sf < 3 or l64[0] > 0)
    return c


def held_to_bound(got, ref, what):
    mag = float(np.abs(ref).max())
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("%s: error %.3e = %.2f x 2^-24 of the magnitude %.3e" % (what, err, err / mag * 2.0 ** 24 if mag else 0.0, mag))
    assert np.isfinite(got).all() and err <= PROPOSAL_BOUND * mag, (what, err, mag)


def check_kernel(b, kind, n, Sc, Sf, stride, seed):
    c = built_case(b, kind, n, Sc, Sf, stride, seed)
    g = np.random.default_rng(seed + 1000)
    g_loss = (0.5 + g.random(n)).astype(f32) * np.where(g.random(n) < 0.5, -1.0, 1.0).astype(f32)
    scale = 0.37
    what = "%s n=%d Sc=%d Sf=%d stride=%d" % (kind, n, Sc, Sf, stride)
    zero = c["zero_rays"]
    for gl in (None, g_loss):
        l64, g64 = proposal_reference(c["w_c"], c["w_f"], c["z_c"], c["z_f"], c["rays"], scale, gl)
        loss, gw = proposal_loss(b, c, scale=scale, g_loss=gl)
        held_to_bound(loss, l64, what + " loss")
        held_to_bound(gw, g64, what + (" g_weights" if gl is None else " g_weights (g_loss)"))
        assert not loss[zero].any() and not gw[zero].any(), what   # exactly zero
        # the two single-output calls and a repeat: the combined call's bits
        lo_only, none = proposal_loss(b, c, scale=scale, g_loss=gl, want_g=False)
        none2, g_only = proposal_loss(b, c, scale=scale, g_loss=gl, want_loss=False)
        again = proposal_loss(b, c, scale=scale, g_loss=gl)
        assert none is None and none2 is None
        assert np.array_equal(lo_only, loss) and np.array_equal(g_only, gw), what
        assert np.array_equal(again[0], loss) and np.array_equal(again[1], gw), what
    if kind == "zero_coarse":   # B = 0 on ray 0: every fine sample contributes -2 w / (w + eps) to the coarse samples it overlaps
        lo, hi = proposal_ranges(*(torch.as_tensor(c[k]) for k in ("z_c", "z_f")), torch.as_tensor(c["rays"][:, 7:8]))
        w = c["w_f"][0].astype(np.float64)
        r = -2.0 * w / (w + EPS)
        want = np.array([r[(lo[0].numpy() <= j) & (j <= hi[0].numpy())].sum() for j in range(Sc)])
        _, gw = proposal_loss(b, c)
        held_to_bound(gw[0], want, what + " ray 0")
    # accumulate: ONE fp32 add onto what the buffer holds
    pre = g.normal(size=(n, Sc)).astype(f32)
    _, plain = proposal_loss(b, c, scale=scale, g_loss=g_loss)
    _, acc = proposal_loss(b, c, scale=scale, g_loss=g_loss, accumulate=True, prefill=pre)
    assert np.array_equal(acc, pre + plain), what
    _, over = proposal_loss(b, c, scale=scale, g_loss=g_loss, prefill=pre)
    assert np.array_equal(over, plain), what
    # NaN in either raw propagates to its ray, and to no other
    if kind == "noise_draws" and Sf >= 2:
        for key, S_ in (("raw_c", Sc), ("raw_f", Sf)):
            bad = dict(c, **{key: c[key].copy()})
            bad[key][0, S_ // 2, 3] = np.nan
            loss, gw = proposal_loss(b, bad)
            assert np.isnan(loss[0]) and not np.isnan(loss[1:]).any() and not np.isnan(gw[1:]).any(), (what, key)
            assert key == "raw_f" or np.isnan(gw[0]).any(), what


def case_kernel(b, kind):
    """Every (Sc, Sf) with every n; the first kind with both ray strides at each, the others alternating between the two."""
    seed = 100 * KERNEL_KINDS.index(kind)
    for Sc, Sf in SHAPES:
        for n in SHAPES_N:
            for stride in (STRIDES if kind == KERNEL_KINDS[0] else STRIDES[seed % 2:seed % 2 + 1]):
                seed += 1
                check_kernel(b, kind, n, Sc, Sf, stride, seed)


def case_kernel_long_rays(b):
    """The cap (Sc + Sf = 4096, split both ways) and many ragged chunks: the binary searches at their full depth."""
    for n, Sc, Sf, seed in ((2, 1000, 3096, 5), (2, 3095, 1001, 6), (3, 64, 2011, 7)):
        c = built_case(b, "refining" if Sf >= Sc else "free", n, Sc, Sf, 8, seed)
        l64, g64 = proposal_reference(c["w_c"], c["w_f"], c["z_c"], c["z_f"], c["rays"])
        loss, gw = proposal_loss(b, c)
        held_to_bound(loss, l64, "long Sc=%d Sf=%d loss" % (Sc, Sf))
        held_to_bound(gw, g64, "long Sc=%d Sf=%d g_weights" % (Sc, Sf))


def case_kernel_refusals(b):
    """Every refusal returns NERFHIP_ERR_ARG and leaves both outputs untouched; n == 0 is OK and launches nothing."""
    c = kernel_inputs("noise_draws", 4, 5, 7, 8, 1)

    def refused(match, **kw):
        rc, lo, gw = proposal_loss(b, c, raise_on_error=False, **kw)
        assert rc == -1 and match in b.lib.last_error().decode(), (rc, b.lib.last_error())
        assert (lo is None or np.isnan(lo).all()) and (gw is None or np.isnan(gw).all())

    for k in INPUTS:
        refused("NULL", null=(k,))
    refused("ray_stride", stride=7)
    refused("at least 1 sample", sc=0)
    refused("at least 1 sample", sf=0)
    refused("at most %d" % CAP, sc=CAP - 6)            # Sc + Sf = CAP + 1
    refused("at most %d" % CAP, sf=CAP - 4)
    refused("at most %d" % CAP, sc=2 ** 31 - 4, sf=8)  # (the sum does not wrap)
    refused("n < 0", n=-1)
    refused("both outputs", want_loss=False, want_g=False)
    rc, lo, gw = proposal_loss(b, c, raise_on_error=False, n=0)
    assert rc == 0 and np.isnan(lo).all() and np.isnan(gw).all()
    rc, _, _ = proposal_loss(b, c, raise_on_error=False, n=0, null=INPUTS)
    assert rc == 0


# ---- through the render -------------------------------------------------------------------------------------------------------------
# One training forward of two nets on a backend (spread_cases' harness: its smallest nets, shapes and problems), nerfhip_proposal_loss
# over both passes' regions of the workspace (RenderCall.proposal), and the _w backward entry points with its cotangent.
LAM = 0.1        # weight of the term on the coarse net: lam * mean_ray(L)
LAM_RAYS = 0.5   # ... in the ray-gradient case (a term of the MSE terms' size in the ray gradient, so that the comparison is about it)


def proposal_cotangent(r, lam, g_loss=None, into=None):
    """(coarse weight cotangent of lam * mean_ray(L) [n, Sc] on the device, per-ray L on the host) over the forward in r's workspace;
    into: a device cotangent to ACCUMULATE onto (the term stacks behind the spread and depth terms)."""
    b = r.b
    lo, dg = b.empty((r.n,)), b.devopt(g_loss)
    gw = b.empty((r.n, r.nc)) if into is None else into
    r.call.proposal(float(lam) / r.n, b.p(dg), b.ptr(lo), b.ptr(gw), into is not None, b.stream())
    return gw, np.array(b.host(lo), copy=True)


def case_render_call(b, net="w64", n=21, nc=9, nf=6):
    """RenderCall.proposal over the workspace is the raw call on those regions, with each pass's own noise draws (and, without draws,
    the in-kernel streams keyed by the call's seed and ray offset): loss and cotangent bit for bit."""
    cfg, pc, _, _, packed_c = S.setup(b, net, "fp32", seed=3)
    _, pf, _, _, packed_f = S.setup(b, net, "fp32", seed=4)
    _, rays, rand, opt, _ = S.render_problem(net, n, nc, nf, seed=39)
    for draws, seed, off in ((rand, 0, 0), ({k: v for k, v in rand.items() if not k.startswith("noise")}, 77, 5)):
        r = S.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, draws, seed=seed, ray_offset=off)
        gw, lo = proposal_cotangent(r, 0.3)
        c = dict(raw_c=r.region("raw_coarse"), z_c=r.region("z_coarse"), raw_f=r.region("raw_fine"), z_f=r.region("z_fine"), rays=rays,
                 noise_std=opt["noise_std"], noise_c=draws.get("noise_coarse"), noise_f=draws.get("noise_fine"), seed=seed, ray_offset=off)
        lo_raw, gw_raw = proposal_loss(b, c, scale=0.3 / n)
        assert (lo > 0).any() and np.array_equal(lo, lo_raw) and np.array_equal(b.host(gw), gw_raw), (seed, off)
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


def _teacher(par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, lam, dtype, wrt_rays=False, want_margin=False, lam_spread=(0.0, 0.0)):
    """The oracle's autograd of MSE terms + lam * mean_ray(L) (+ spread terms) on GIVEN depths in `dtype`: ({tensor: grad} coarse,
    fine, d/d(rays) or None, margin or None, mean L)."""
    cast = lambda d: {k: torch.as_tensor(v).to(dtype) for k, v in d.items()}  # noqa: E731
    pc = {k: v.detach().to(dtype).requires_grad_(True) for k, v in par_c.items()}
    pf = {k: v.detach().to(dtype).requires_grad_(True) for k, v in par_f.items()}
    r = torch.as_tensor(rays).to(dtype).requires_grad_(wrt_rays)
    zc, zf = torch.as_tensor(z_c).to(dtype), torch.as_tensor(z_f).to(dtype)
    w = O.render_at_depths(r, zc, zf, pc, pf, cfg, cfg, opt, cast(rand), want_margin=want_margin)
    Lp = proposal_of_weights(w["weights_coarse"], w["weights_fine"], zc, zf, r).mean()
    total = S.oracle_total_loss(w, zc, zf, r, torch.as_tensor(tgt).to(dtype), lam_spread) + lam * Lp
    total.backward()
    return ({k: v.grad.numpy() for k, v in pc.items()}, {k: v.grad.numpy() for k, v in pf.items()},
            r.grad.numpy() if wrt_rays else None, w["relu_margin"].numpy() if want_margin else None, float(Lp.detach()))


def case_param_grads(b, net, arith, shapes=S.RENDER_SHAPES, min_decided=0.3):
    """Parameter gradients of MSE + LAM * mean(L) through nerfhip_proposal_loss + nerfhip_render_bwd_parts_w against the oracle's
    autograd of the same loss, teacher-forced on the kernels' own depths and ReLU-margin filtered exactly as
    spread_cases.case_param_grads does it; bound: `tf.grad.filtered` of tolerances.py, of max|g| per tensor.  The fine net's gradient is
    the run's without the term, bit for bit; and with a spread term on the coarse net the proposal term ACCUMULATES behind it."""
    tol = TL.bound("tf.grad.filtered", arith)[0]
    cfg, pc, par_c, _, packed_c = S.setup(b, net, arith, seed=3)
    _, pf, par_f, _, packed_f = S.setup(b, net, arith, seed=4)
    for n, nc, nf in shapes:
        _, rays, rand, opt, tgt = S.render_problem(net, n, nc, nf, seed=33)
        r = S.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
        z_c, z_f = r.region("z_coarse"), r.region("z_fine")
        margin = _teacher(par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, LAM, torch.float64, want_margin=True)[3]
        keep = margin > TL.bound("relu_margin")
        assert keep.mean() >= min_decided, (net, n, float(keep.mean()))
        rays, tgt, rand = rays[keep], tgt[keep], {k: np.ascontiguousarray(v[keep]) for k, v in rand.items()}
        z_c, z_f = z_c[keep], z_f[keep]
        r = S.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
        assert np.array_equal(r.region("z_coarse"), z_c) and np.array_equal(r.region("z_fine"), z_f)
        _, gc, gf = b.mse_loss(r.out["rgb_coarse"], r.out["rgb_fine"], tgt)
        plain = r.backward((gc, gf), (None, None), entry="parts_w")
        mse_c, mse_f = _teacher(par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, 0.0, torch.float32)[:2]
        for spread in ((0.0, 0.0), (S.LAMBDA[0], 0.0)):
            r.forward()
            gwc = r.spread(False, spread[0] / r.n)[1] if spread[0] else None
            gwc, lo = proposal_cotangent(r, LAM, into=gwc)
            got = r.backward((gc, gf), (gwc, None), entry="parts_w")
            ref_c, ref_f, _, _, Lp = _teacher(par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, LAM, torch.float32, lam_spread=spread)
            assert (lo > 0).mean() >= 0.5 and abs(float(lo.mean()) - Lp) <= 1e-3 * Lp, (lo.mean(), Lp)
            assert np.array_equal(got["g_params_fine"], plain["g_params_fine"]), (net, arith, n)   # (no gradient to the fine net)
            assert not np.array_equal(got["g_params_coarse"], plain["g_params_coarse"])
            for tag, plan, ref, mse in (("coarse", pc, ref_c, mse_c), ("fine", pf, ref_f, mse_f)):
                g = b.unflatten(plan, got["g_params_" + tag])
                moved = max(float(np.abs(v - mse[k]).max()) / float(np.abs(v).max()) for k, v in ref.items())
                # not vacuous, from the reference alone: the term moves the coarse net's gradient by far more than the bound
                assert moved > 10.0 * tol if tag == "coarse" else moved == 0.0, (tag, moved)
                for k, v in ref.items():
                    err = float(np.abs(g[k] - v).max()) / float(np.abs(v).max())
                    print("param grads %s %s n=%d spread=%g %s %s: %.3e of max|g| (bound %.1e)" % (net, arith, n, spread[0], tag, k, err, tol))
                    assert err <= tol, (net, arith, n, tag, k, err, tol)
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


def case_compacted(b, net, arith, modes, n=48, nc=8, nf=8, noise=0.6):
    """The backward modes with the proposal cotangent on the coarse pass (spread_cases.case_compacted's criteria): every mode against
    mode 0 within `unit.compact_vs_dense` of max|g| per tensor; `kept` equals the count of nonzero d(loss)/d(raw) rows; the fine net's
    gradient is, in every mode, that mode's gradient without the term, bit for bit."""
    ctol = TL.bound("unit.compact_vs_dense", arith)
    cfg, pc, _, _, packed_c = S.setup(b, net, arith, seed=3)
    _, pf, _, _, packed_f = S.setup(b, net, arith, seed=4)
    _, rays, rand, opt, tgt = S.render_problem(net, n, nc, nf, seed=35, noise=noise)
    res = {}
    for mode in (False,) + tuple(modes):
        b.set_compaction(pc, mode)
        b.set_compaction(pf, mode)
        r = S.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
        if mode is False:
            _, gc, gf = b.mse_loss(r.out["rgb_coarse"], r.out["rgb_fine"], tgt)
        plain_f = r.backward((gc, gf), (None, None), entry="parts_w", parts=L.PART_FINE)["g_params_fine"]
        r.forward()
        gwc, lo = proposal_cotangent(r, LAM)
        assert (lo > 0).mean() >= 0.5
        out = {}
        for fine, part, tag in ((True, L.PART_FINE, "fine"), (False, L.PART_COARSE, "coarse")):
            got = r.backward((gc, gf), (gwc, None), entry="parts_w", parts=part)
            out["g_params_" + tag] = got["g_params_" + tag]
            nonzero = int(r.region("bwd_g_raw_" + tag).reshape(-1, 4).any(axis=1).sum())
            total = n * (nc + (nf if fine else 0))
            if mode in (True, "recompute", "fused_compact"):
                assert r.kept(tag) == (nonzero, total) and 0 < nonzero < total, (mode, tag, r.kept(tag), nonzero, total)
            else:
                assert 0 < nonzero < total
        assert np.array_equal(out["g_params_fine"], plain_f), mode
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
    """nerfhip_render_bwd_rays_w with the proposal cotangent: d(loss)/d(rays) of MSE + LAM_RAYS * mean(L) against the oracle's autograd
    teacher-forced on the kernels' own depths, under spread_cases.case_rays_w's (parity_cases.case_ray_grad's) distribution bound."""
    cfg, pc, par_c, flat_c, packed_c = S.setup(b, net, "fp32", seed=3)
    _, pf, par_f, flat_f, packed_f = S.setup(b, net, "fp32", seed=4)
    _, rays, rand, opt, tgt = S.render_problem(net, n, nc, nf, seed=37, noise=0.0)
    r = S.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
    z_c, z_f = r.region("z_coarse"), r.region("z_fine")
    _, gc, gf = b.mse_loss(r.out["rgb_coarse"], r.out["rgb_fine"], tgt)
    gwc, _ = proposal_cotangent(r, LAM_RAYS)
    got = r.backward((gc, gf), (gwc, None), entry="rays_w", params=(flat_c, flat_f))["g_rays"]
    args = (par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt)
    ref = _teacher(*args, LAM_RAYS, torch.float32, wrt_rays=True)[2]
    ref64 = _teacher(*args, LAM_RAYS, torch.float64, wrt_rays=True)[2]
    plain64 = _teacher(*args, 0.0, torch.float64, wrt_rays=True)[2]
    assert np.isfinite(ref64).all() and float(np.any(ref64[:, 0:3] != 0.0, axis=1).mean()) >= 0.9
    for lo, hi, what in ((0, 3, "origin"), (3, 6, "direction"), (8, 11, "viewdirs")):
        scale = float(np.abs(ref64[:, lo:hi]).max())
        assert scale > 0.0, what
        # (the term is in it -- but for the view directions: the density, and so the weights, do not depend on them)
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


# ---- the culled step of the occupancy grid with the proposal term ----------------------------------------------------------------------
def case_culled_step(b, net, arith, outside, n=21, nc=9, nf=6, noise_std=0.3, lam=0.5):
    """spread_cases.case_culled_step with the proposal term in place of the spread terms: arm A by hand in mode 1 (training forward, the
    library's own flags, the culled rows overwritten with the empty row -- so a culled sample's weight is 0 --, compositing again), arm B
    nerfhip_render_fwd_occ_train in mode 2 and (where the plan has it) 4; in both arms nerfhip_proposal_loss over the workspace and
    nerfhip_render_bwd_parts_w.  By that case's criteria: the cotangent and the per-ray loss bit-identical (the kernel reads the same
    rows), each net's kept count equal, gradients array_equal in mode 2 and within unit.compact_vs_dense in mode 4 -- the coarse net's
    not the gradient without the term, the fine net's exactly that."""
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
    gw_a, lo_a = proposal_cotangent(a, lam)
    assert (lo_a >= 0).all() and (lo_a > 0).any()
    plain = a.bwd(want["rgb_coarse"] - tgt, want["rgb_fine"] - tgt)
    want.update(a.bwd(want["rgb_coarse"] - tgt, want["rgb_fine"] - tgt, (gw_a, None)))
    assert not np.array_equal(want["g_coarse"], plain["g_coarse"]) and np.array_equal(want["g_fine"], plain["g_fine"])
    assert want["kept_coarse"] == plain["kept_coarse"] and want["kept_fine"] == plain["kept_fine"]   # (a weight cotangent wakes no row)
    ctol = TL.bound("unit.compact_vs_dense", arith if arith == "fp32" else "f16x3_train")
    for mode in modes:
        for p in (pc, pf):
            b.set_compaction(p, mode)
        s = OT.Step(b, pc, pf, packed_c, packed_f, rays, opt, rnp)
        s.fwd_occ(grid)
        got = s.maps()
        gw, lo = proposal_cotangent(s, lam)
        assert np.array_equal(b.host(gw), b.host(gw_a)) and np.array_equal(lo, lo_a), mode
        got.update(s.bwd(got["rgb_coarse"] - tgt, got["rgb_fine"] - tgt, (gw, None)))
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
