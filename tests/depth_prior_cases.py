"""Cases of the depth priors (DS-NeRF's expected-depth and ray-termination losses; include/nerfhip.h nerfhip_depth_prior_loss,
csrc/reg/depth_prior.hip) and of their weight cotangent through the fused backward, shared by the emulator suite
(tests/test_depth_prior.py) and the GPU suite (tests/test_gpu_depth_prior.py).  Every case drives the C ABI through a backend's library
handle (tests/backends.py); the render cases reuse the helpers of tests/spread_cases.py.

The definition is restated here independently of the kernel (depth_terms_of_weights): the header's formulas in torch, with the weights
from the oracle's compositing (O.volume_render) on the same raw rows, depths and noise draws, and autograd for d/dw.

Bounds of this file, and where they come from:

  SPREAD_YARDSTICK / SPREAD_FLOOR (imported from spread_cases.py, with its reasons): the kernel's `loss` and `g_weights` may be no
                    further from the fp64 run of the formulas than the SAME formulas run in torch fp32 are, x 2, plus a floor of
                    4 x 2^-24 of the quantity's largest magnitude in the case (the outputs are fp32, the weights summed are the
                    compositing's fp32 weights).  `loss` [n, 2] is held as ONE quantity, as the bound is stated: a column of its own
                    is no well-posed comparison for Tm at S = 2, where the last sample's w is close to 1, -log(w + eps) cancels to
                    ~1e-5 and the half-ulp of the compositing's fp32 weight (3e-8, given by the definition) is 2e-3 of the whole
                    column (n = 1, S = 2: kernel 5.8e-8 of a Tm of 2.8e-5; the fp32 formula rounds the same w and lands anywhere
                    within that).  The measured distances are printed by every case (and recorded in DESIGN.md 3.19).
  long rays         with the library's own compositing weights given, the fp64 sums must land within the final rounding of the fp32
                    outputs: SPREAD_FLOOR of the largest magnitude, no yardstick term (spread_cases.check_kernel_sums' reason).
  render cases      tolerances.py `tf.grad.filtered`, `unit.compact_vs_dense`, and parity_cases.case_ray_grad's distribution bound, as
                    in spread_cases.py.  The termination term multiplies by up to 1 / eps = 1e5: where the oracle's OWN fp32 autograd
                    is further from its fp64 run than `tf.grad.filtered`, that case's bound is 2 x that fp32 distance (printed).
"""
import numpy as np
import torch

import nerf_oracle as O
import nerf_pytorch_amd._lib as L
import occupancy_cases as OC
import spread_cases as SC
import tolerances as TL

f32 = np.float32
EPS = 1e-5

SHAPES_S = (1, 2, 63, 64, 65, 129)
SHAPES_N = (1, 5, 70)
STRIDES = (8, 11)
PRIOR_STRIDES = (3, 5)
KERNEL_KINDS = ("noise_draws", "noise_stream", "zero_density", "opaque_first", "tied_depths", "d_outside", "sigma_tiny", "sigma_huge",
                "no_prior")
_SC_KIND = dict(d_outside="noise_draws", sigma_tiny="noise_draws", sigma_huge="noise_draws", no_prior="noise_draws")


# ---- the definition, in torch ----------------------------------------------------------------------------------------------------
def depth_terms_of_weights(w, z, rays, prior):
    """(E [n], Tm [n]) of the header's definition for weights w [n, S] (differentiable), depths z, packed rays and prior rows [n, >=3],
    in w's dtype.  A row with !(c > 0) gives exact zeros whatever its D and sigma hold."""
    dtype = w.dtype
    z, far = z.detach().to(dtype), rays.detach().to(dtype)[:, 7:8]
    p = torch.as_tensor(np.asarray(prior, np.float64)).to(dtype)
    has = p[:, 1] > 0
    one, zero = torch.ones_like(p[:, 0]), torch.zeros_like(p[:, 0])
    D, c, sg = torch.where(has, p[:, 0], zero), torch.where(has, p[:, 1], zero), torch.where(has, p[:, 2], one)
    dhat = (w * z).sum(dim=1)
    E = c * (dhat - D) ** 2
    delta = torch.cat((z[:, 1:] - z[:, :-1], torch.clamp(far - z[:, -1:], min=0.0)), dim=1)
    k = torch.exp(-(z - D[:, None]) ** 2 / (2.0 * sg[:, None] ** 2))
    Tm = c * (-torch.log(w + EPS) * k * delta).sum(dim=1)
    return torch.where(has, E, zero), torch.where(has, Tm, zero)


def depth_reference(raw, z, rays, prior, noise_std, noise, dtype, weights=(1.0, 1.0), scale=1.0, g_loss=None):
    """(loss [n, 2], g_weights [n, S], w [n, S]) of the definition in `dtype`: the weights from the oracle's compositing, autograd for
    d/dw of scale * sum_r (w_expected g_loss[r, 0] E_r + w_termination g_loss[r, 1] Tm_r).  A row without a prior takes no part in the
    sum (its weights may be anything)."""
    raw, z, rays = (torch.as_tensor(a).to(dtype) for a in (raw, z, rays))
    nz = None if noise is None else torch.as_tensor(noise).to(dtype)
    w = O.volume_render(raw, z, rays[:, 3:6], float(noise_std), nz, False)[3].detach().requires_grad_(True)
    E, Tm = depth_terms_of_weights(w, z, rays, prior)
    gl = torch.ones(z.shape[0], 2, dtype=dtype) if g_loss is None else torch.as_tensor(g_loss).to(dtype)
    has = torch.as_tensor(np.asarray(prior)[:, 1] > 0)
    tot = (float(weights[0]) * gl[:, 0] * E + float(weights[1]) * gl[:, 1] * Tm)[has].sum() * float(scale)
    g = torch.autograd.grad(tot, w)[0] if bool(has.any()) else torch.zeros_like(w)
    g = torch.where(has[:, None], g, torch.zeros_like(g))
    return torch.stack((E, Tm), dim=1).detach(), g, w.detach()


# ---- the kernel through a backend ---------------------------------------------------------------------------------------------------
def depth_prior_loss(b, raw, z, rays, prior, inds=None, prior_rows=None, noise_std=0.0, noise=None, seed=0, rng_stream=1, ray_offset=0,
                     weights=(1.0, 1.0), scale=1.0, g_loss=None, want_loss=True, want_g=True, prefill=None, raise_on_error=True, n=None,
                     s=None, stride=None, prior_stride=None, null=()):
    """nerfhip_depth_prior_loss on numpy inputs: (loss [n, 2] or None, g_weights [n, S] or None); prefill: accumulate != 0 into a copy
    of it.  raise_on_error=False: (rc, loss, g) with the outputs as the call left them (NaN-filled before)."""
    nn, ss = z.shape
    n, s, stride = (nn if n is None else n), (ss if s is None else s), (rays.shape[1] if stride is None else stride)
    prior = np.ascontiguousarray(prior, f32)
    d = dict(raw=b.dev(np.ascontiguousarray(raw, f32)), z=b.dev(np.ascontiguousarray(z, f32)), rays=b.dev(np.ascontiguousarray(rays, f32)),
             prior=b.dev(prior))
    dn, dg, di = b.devopt(noise), b.devopt(g_loss), b.devopt(inds, np.int64)
    lo = b.empty((nn, 2)) if want_loss else None
    gw = (b.empty((nn, ss)) if prefill is None else b.dev(np.ascontiguousarray(prefill, f32))) if want_g else None
    args = (*[None if k in null else b.ptr(d[k]) for k in ("raw", "z", "rays")], stride, n, s, float(noise_std), b.p(dn), seed, rng_stream,
            ray_offset, None if "prior" in null else b.ptr(d["prior"]), prior.shape[1] if prior_stride is None else prior_stride, b.p(di),
            prior.shape[0] if prior_rows is None else prior_rows, float(weights[0]), float(weights[1]), float(scale), b.p(dg), b.p(lo),
            b.p(gw), int(prefill is not None), b.stream())
    if not raise_on_error:
        rc = b.lib._dll.nerfhip_depth_prior_loss(*args)
        return rc, (None if lo is None else b.host(lo)), (None if gw is None else b.host(gw))
    b.lib.depth_prior_loss(*args)
    return (None if lo is None else b.host(lo)), (None if gw is None else b.host(gw))


def prior_rows_for(g, kind, z, rays, prior_stride, has):
    """Prior rows [n, prior_stride] of a case: D near a sample of the ray (a prior sits near a surface), c in [0.5, 2), sigma in
    [0.1, 0.5); the rows of ~has cycle through c = 0, c < 0 and c = NaN and carry NaN in D and sigma; columns beyond 2 are garbage."""
    n, S = z.shape
    p = g.normal(size=(n, prior_stride)).astype(f32) * 1e3
    sg = (0.1 + 0.4 * g.random(n)).astype(f32)
    p[:, 0] = z[np.arange(n), g.integers(0, S, n)] + sg * g.normal(size=n).astype(f32) + f32(1e-3)
    p[:, 1] = 0.5 + 1.5 * g.random(n)
    p[:, 2] = sg
    if kind == "d_outside":   # (before `near` on even rays, beyond `far` on odd ones)
        p[:, 0] = np.where(np.arange(n) % 2 == 0, rays[:, 6] - 1.0 - g.random(n), rays[:, 7] + 1.0 + g.random(n))
        p[:, 2] = 0.5 + 0.5 * g.random(n)   # (wide enough that k_i stays a normal fp64 number 6 depth units away)
    elif kind == "sigma_tiny":   # (every k_i underflows: D is no sample's depth -- asserted from the reference)
        p[:, 2] = 1e-20
    elif kind == "sigma_huge":
        p[:, 2] = 1e6
    none = np.flatnonzero(~has)
    p[none, 0], p[none, 2] = np.nan, np.nan
    p[none, 1] = np.array([0.0, -1.0, np.nan], f32)[np.arange(len(none)) % 3]
    return p


def kernel_inputs(kind, n, S, stride, prior_stride, seed):
    """spread_cases.kernel_inputs (raw rows, ascending depths, packed rays, the noise kinds, an all-zero-density ray 0, a ray 0 opaque
    at its first sample, tied depths with -- from S = 3 on -- depths beyond `far`) and the prior rows.  Rays 1, 4, 7, ... have no
    prior; in kind "no_prior" ray 0 has none either."""
    c = SC.kernel_inputs(_SC_KIND.get(kind, kind), n, S, stride, seed)
    g = np.random.default_rng(seed + 5000)
    has = np.arange(n) % 3 != 1
    if kind == "no_prior":
        has[0] = False
    c["has"], c["prior"] = has, prior_rows_for(g, kind, c["z"], c["rays"], prior_stride, has)
    return c


def held(got, ref64, ref32, what, record=None):
    SC.held_to_yardstick(np.asarray(got), ref64, ref32, what, record)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def check_kernel(b, kind, n, S, stride, prior_stride, seed, record=None):
    c = kernel_inputs(kind, n, S, stride, prior_stride, seed)
    raw, z, rays, prior, has = c["raw"], c["z"], c["rays"], c["prior"], c["has"]
    kw = dict(noise_std=c["noise_std"], noise=c["noise"], seed=c["seed"], rng_stream=c["rng_stream"], ray_offset=c["ray_offset"])
    ref_noise = c["noise"]
    if kind == "noise_stream":
        ref_noise = b.rng_fill(1, c["seed"], c["rng_stream"], c["ray_offset"] * S, n * S).reshape(n, S)
    g = np.random.default_rng(seed + 1000)
    g_loss = ((0.5 + g.random((n, 2))) * np.where(g.random((n, 2)) < 0.5, -1.0, 1.0)).astype(f32)
    scale, wts = 0.37, (0.8, 0.05)
    what = "%s n=%d S=%d stride=%d/%d" % (kind, n, S, stride, prior_stride)
    ref = lambda dtype, weights=wts, gl=None: depth_reference(raw, z, rays, prior, c["noise_std"], ref_noise, dtype, weights, scale, gl)  # noqa: E731
    call = lambda **k: depth_prior_loss(b, raw, z, rays, prior, **dict(kw, scale=scale, **k))  # noqa: E731
    for gl in (None, g_loss):
        l64, g64, w64 = ref(torch.float64, gl=gl)
        l32, g32, _ = ref(torch.float32, gl=gl)
        # not vacuous, from the reference alone: an expected-depth loss on >= 90 % of the rays with a prior, a termination loss
        # somewhere (but where every k_i underflows), a gradient to compare; exact zeros on the rays without a prior
        if has.any():
            assert float((l64.numpy()[has, 0] > 0).mean()) >= 0.9, (what, l64.numpy()[has])
            assert (float(l64[:, 1].abs().max()) > 0) == (kind != "sigma_tiny"), (what, l64[:, 1])   # (w + eps > 1: negative)
            assert float(g64.abs().max()) > 0, what
        assert not l64.numpy()[~has].any() and not g64.numpy()[~has].any(), what
        loss, gw = call(weights=wts, g_loss=gl)
        held(loss, l64, l32, what + " loss", record)
        if kind == "sigma_tiny":
            assert not loss[:, 1].any(), what
        if has.any():
            held(gw, g64, g32, what + (" g_weights" if gl is None else " g_weights (g_loss)"), record)
        assert not loss[~has].any() and not gw[~has].any(), what   # exactly zero
        # the two single-output calls and a repeat: the combined call's bits
        lo_only, none = call(weights=wts, g_loss=gl, want_g=False)
        none2, g_only = call(weights=wts, g_loss=gl, want_loss=False)
        again = call(weights=wts, g_loss=gl)
        assert none is None and none2 is None
        assert np.array_equal(bits(lo_only), bits(loss)) and np.array_equal(bits(g_only), bits(gw)), what
        assert np.array_equal(bits(again[0]), bits(loss)) and np.array_equal(bits(again[1]), bits(gw)), what
    loss, gw = call(weights=wts, g_loss=g_loss)
    # each term alone: the other's weight exactly 0
    for weights, tag in (((wts[0], 0.0), "E alone"), ((0.0, wts[1]), "Tm alone")):
        _, g64, _ = ref(torch.float64, weights, g_loss)
        _, g32, _ = ref(torch.float32, weights, g_loss)
        lo1, g1 = call(weights=weights, g_loss=g_loss)
        assert np.array_equal(bits(lo1), bits(loss)), what   # (the losses are unscaled and unweighted)
        if tag == "Tm alone" and kind == "sigma_tiny":
            assert not g64.numpy().any() and not g1.any(), what
        elif has.any():
            held(g1, g64, g32, what + " g_weights " + tag, record)
        if tag == "E alone" and kind == "sigma_tiny":   # every k_i underflows: the gradient is exactly the E part
            assert np.array_equal(bits(g1), bits(gw)), what
    # accumulate: one fp32 add onto what the buffer holds; the rows of rays without a prior keep their bits
    pre = (g.normal(size=gw.shape) * np.abs(gw).max()).astype(f32)
    pre[:, 0] = -0.0
    _, acc = call(weights=wts, g_loss=g_loss, prefill=pre)
    assert np.array_equal(bits(acc[has]), bits(pre[has] + gw[has])) and np.array_equal(bits(acc[~has]), bits(pre[~has])), what
    # inds: permuted and repeated rows of a longer table give the bits of the call with the rows gathered on the host; -1 and
    # prior_rows are rows without a prior
    rows = 2 * n + 3
    table = prior_rows_for(g, "noise_draws", z[np.arange(rows) % n], rays[np.arange(rows) % n], prior_stride, np.arange(rows) % 4 != 2)
    inds = g.integers(0, rows, n).astype(np.int64)
    if n >= 5:
        inds[1], inds[2], inds[3] = inds[0], -1, rows
    else:
        inds[0] = (-1, rows)[seed % 2]
    gathered = table[np.clip(inds, 0, rows - 1)].copy()
    gathered[(inds < 0) | (inds >= rows)] = (np.nan, 0.0, np.nan) + (0.0,) * (prior_stride - 3)
    via = depth_prior_loss(b, raw, z, rays, table, inds=inds, weights=wts, scale=scale, g_loss=g_loss, **kw)
    host = depth_prior_loss(b, raw, z, rays, gathered, weights=wts, scale=scale, g_loss=g_loss, **kw)
    assert np.array_equal(bits(via[0]), bits(host[0])) and np.array_equal(bits(via[1]), bits(host[1])), what
    out = (inds < 0) | (inds >= rows)
    assert not via[0][out].any() and not via[1][out].any(), what
    _, acc = depth_prior_loss(b, raw, z, rays, table, inds=inds, weights=wts, scale=scale, g_loss=g_loss, prefill=pre, **kw)
    assert np.array_equal(bits(acc[out]), bits(pre[out])), what
    # a NaN density propagates on a ray with a prior, and not onto its neighbours
    if kind == "noise_draws" and S >= 2:
        rawn = raw.copy()
        rawn[0, S // 2, 3] = np.nan
        loss, gw = depth_prior_loss(b, rawn, z, rays, prior, weights=wts, **kw)
        assert has[0] and np.isnan(loss[0]).all() and np.isnan(gw[0]).any(), what
        assert not np.isnan(loss[1:]).any() and not np.isnan(gw[1:]).any(), what


def check_kernel_sums(b, kind, n, S, stride, seed):
    """The kernel's sums alone, at any S: with the weights GIVEN -- the library's own compositing weights (nerfhip_volume_render_fwd on
    the same inputs, which the kernel forms bit for bit) -- the header's closed forms in fp64 numpy are exact to ~1e-16, and the
    kernel's fp64 sums must land within the final rounding to fp32 of them (spread_cases.check_kernel_sums' reason: against the
    oracle's own weights a long ray measures the device's expf at tiny dist, not this kernel)."""
    c = kernel_inputs(kind, n, S, stride, 3, seed)
    kw = dict(noise_std=c["noise_std"], noise=c["noise"], seed=c["seed"], rng_stream=c["rng_stream"], ray_offset=c["ray_offset"])
    w = b.volume_render_fwd(c["raw"], c["z"], np.ascontiguousarray(c["rays"][:, 3:]), **kw)[3].astype(np.float64)
    z, rays, p, has = c["z"].astype(np.float64), c["rays"].astype(np.float64), c["prior"].astype(np.float64), c["has"]
    D, cw, sg = (np.where(has, p[:, k], v)[:, None] for k, v in ((0, 0.0), (1, 0.0), (2, 1.0)))
    delta = np.concatenate((np.diff(z, axis=1), np.maximum(rays[:, 7:8] - z[:, -1:], 0.0)), axis=1)
    k = np.exp(-(z - D) ** 2 / (2.0 * sg ** 2))
    dhat = (w * z).sum(axis=1, keepdims=True)
    l64 = np.concatenate((cw * (dhat - D) ** 2, cw * (-np.log(w + EPS) * k * delta).sum(axis=1, keepdims=True)), axis=1)
    wts = (0.8, 0.05)
    g64 = wts[0] * 2.0 * cw * (dhat - D) * z - wts[1] * cw * k * delta / (w + EPS)
    assert has.any() and (l64[has] > 0).all() and float(np.abs(g64).max()) > 0
    loss, gw = depth_prior_loss(b, c["raw"], c["z"], c["rays"], c["prior"], weights=wts, **kw)
    for got, ref, what in ((loss[:, 0], l64[:, 0], "E"), (loss[:, 1], l64[:, 1], "Tm"), (gw, g64, "g_weights")):
        mag = float(np.abs(ref).max())
        e = SC.err_over(got, ref)
        print("%s n=%d S=%d sums %s: %.3e of the magnitude (%.2f x 2^-24)" % (kind, n, S, what, e / mag, e / mag * 2.0 ** 24))
        assert e <= SC.SPREAD_FLOOR * mag, (kind, n, S, what, e, mag)


def case_kernel(b, kind, record=None):
    """Every S with every n; the first kind with both ray strides at each, the others alternating; the prior stride alternates."""
    seed = 100 * KERNEL_KINDS.index(kind)
    for S in SHAPES_S:
        for n in SHAPES_N:
            for stride in (STRIDES if kind == KERNEL_KINDS[0] else STRIDES[seed % 2:seed % 2 + 1]):
                seed += 1
                check_kernel(b, kind, n, S, stride, PRIOR_STRIDES[(seed // 2) % 2], seed, record)


def case_kernel_refusals(b):
    """Every refusal returns NERFHIP_ERR_ARG and leaves both outputs untouched; n == 0 is OK and launches nothing."""
    c = kernel_inputs("noise_draws", 4, 5, 8, 3, 1)
    base = dict(noise_std=0.0, raise_on_error=False)

    def refused(match, **kw):
        rc, lo, gw = depth_prior_loss(b, c["raw"], c["z"], c["rays"], c["prior"], **dict(base, **kw))
        assert rc == -1 and match in b.lib.last_error().decode(), (rc, b.lib.last_error())
        assert (lo is None or np.isnan(lo).all()) and (gw is None or np.isnan(gw).all())

    for name in ("raw", "z", "rays", "prior"):
        refused("NULL", null=(name,))
    refused("ray_stride", stride=7)
    refused("prior_stride", prior_stride=2)
    refused("prior_rows", prior_rows=-1)
    refused("samples per ray", s=0)
    refused("samples per ray", s=8193)
    refused("n < 0", n=-1)
    refused("both outputs", want_loss=False, want_g=False)
    rc, lo, gw = depth_prior_loss(b, c["raw"], c["z"], c["rays"], c["prior"], n=0, **base)
    assert rc == 0 and np.isnan(lo).all() and np.isnan(gw).all()
    rc, lo, gw = depth_prior_loss(b, c["raw"], c["z"], c["rays"], c["prior"], n=0, null=("raw", "z", "rays", "prior"), **base)
    assert rc == 0


# ---- through the render -------------------------------------------------------------------------------------------------------------
RENDER_NETS, RENDER_ARITHS, RENDER_SHAPES = SC.RENDER_NETS, SC.RENDER_ARITHS, SC.RENDER_SHAPES
# ((a, b) of the coarse net, (a, b) of the fine net): weights of the expected-depth and termination terms in the render cases
DEPTH_W = ((0.05, 0.02), (0.1, 0.01))


def render_prior(rays, seed, frac=1.0 / 3.0):
    """Prior rows [n, 3] for the rays of a render case: about `frac` of them (at least two) with D in the middle 60 % of [near, far],
    c in [0.5, 1.5), sigma = 5 % of far - near; the others c = 0 with NaN in D and sigma."""
    g = np.random.default_rng(seed)
    n = rays.shape[0]
    near, far = rays[:, 6], rays[:, 7]
    has = g.random(n) < frac
    has[:2] = True
    p = np.full((n, 3), np.nan, f32)
    p[:, 1] = 0.0
    p[has, 0] = (near + (0.2 + 0.6 * g.random(n)) * (far - near))[has]
    p[has, 1] = (0.5 + g.random(n))[has]
    p[has, 2] = (0.05 * (far - near))[has]
    return p


def depth_prior_on(r, fine, prior, weights, scale=1.0, g_loss=None, inds=None, into=None, want_g=True):
    """nerfhip_depth_prior_loss over the pass's regions of a RenderSession's workspace (RenderCall.depth_prior) -> (loss host [n, 2],
    g_weights device [n, S] or None); into: a device weight cotangent to accumulate into (what the spread launch wrote)."""
    b = r.b
    prior = np.ascontiguousarray(prior, f32)
    dp, di, dg = b.dev(prior), b.devopt(inds, np.int64), b.devopt(g_loss)
    lo = b.empty((r.n, 2))
    gw = into if into is not None else (b.empty((r.n, r.nc + (r.nf if fine else 0))) if want_g else None)
    r.call.depth_prior(fine, b.ptr(dp), prior.shape[1], b.p(di), prior.shape[0], float(weights[0]), float(weights[1]), float(scale),
                       b.p(dg), b.ptr(lo), b.p(gw), into is not None, b.stream())
    return b.host(lo), gw


def depth_cotangents(r, prior, dw=DEPTH_W):
    """The two passes' weight cotangents of a mean(E) + b mean(Tm) per net over the forward in r's workspace (device), + the losses."""
    lc, gwc = depth_prior_on(r, False, prior, dw[0], 1.0 / r.n)
    lf, gwf = depth_prior_on(r, True, prior, dw[1], 1.0 / r.n)
    return (gwc, gwf), (lc, lf)


def oracle_total_loss(w, z_c, z_f, rays, tgt, prior, dw):
    """MSE terms + a mean(E) + b mean(Tm) of each pass of an O.render_at_depths result, in its dtype (means over ALL rays)."""
    loss, _, _, _ = O.loss_and_psnr(w["rgb_coarse"], w["rgb_fine"], tgt)
    for key, zz, (a, bb) in (("weights_coarse", z_c, dw[0]), ("weights_fine", z_f, dw[1])):
        E, Tm = depth_terms_of_weights(w[key], zz, rays, prior)
        loss = loss + a * E.mean() + bb * Tm.mean()
    return loss


def teacher(par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, prior, dw, dtype, wrt_rays=False, want_margin=False):
    """spread_cases._teacher with this file's total loss: the oracle's autograd on GIVEN depths in `dtype`."""
    cast = lambda d: {k: torch.as_tensor(v).to(dtype) for k, v in d.items()}  # noqa: E731
    pc = {k: v.detach().to(dtype).requires_grad_(True) for k, v in par_c.items()}
    pf = {k: v.detach().to(dtype).requires_grad_(True) for k, v in par_f.items()}
    r = torch.as_tensor(rays).to(dtype).requires_grad_(wrt_rays)
    zc, zf = torch.as_tensor(z_c).to(dtype), torch.as_tensor(z_f).to(dtype)
    w = O.render_at_depths(r, zc, zf, pc, pf, cfg, cfg, opt, cast(rand), want_margin=want_margin)
    oracle_total_loss(w, zc, zf, r, torch.as_tensor(tgt).to(dtype), prior, dw).backward()
    return ({k: v.grad.numpy() for k, v in pc.items()}, {k: v.grad.numpy() for k, v in pf.items()},
            r.grad.numpy() if wrt_rays else None, w["relu_margin"].numpy() if want_margin else None)


def case_param_grads(b, net, arith, shapes=RENDER_SHAPES, min_decided=0.3, record=None):
    """Parameter gradients of MSE + a mean(E) + b mean(Tm) through nerfhip_depth_prior_loss + nerfhip_render_bwd_parts_w against the
    oracle's fp64 autograd of the same loss, teacher-forced on the kernels' own depths, on the rays all of whose samples pass
    `relu_margin` (spread_cases.case_param_grads' construction).  Bound: `tf.grad.filtered`'s maximum of max|g| per tensor -- or, for a
    tensor on which the oracle's own fp32 autograd is further than that from its fp64 run, 2 x that fp32 distance (both printed)."""
    tol = TL.bound("tf.grad.filtered", arith)[0]
    cfg, pc, par_c, _, packed_c = SC.setup(b, net, arith, seed=3)
    _, pf, par_f, _, packed_f = SC.setup(b, net, arith, seed=4)
    for n, nc, nf in shapes:
        _, rays, rand, opt, tgt = SC.render_problem(net, n, nc, nf, seed=33)
        prior = render_prior(rays, seed=41)
        r = SC.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
        z_c, z_f = r.region("z_coarse"), r.region("z_fine")
        margin = teacher(par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, prior, DEPTH_W, torch.float64, want_margin=True)[3]
        keep = margin > TL.bound("relu_margin")
        assert keep.mean() >= min_decided, (net, n, float(keep.mean()))
        rays, tgt, prior, rand = rays[keep], tgt[keep], prior[keep], {k: np.ascontiguousarray(v[keep]) for k, v in rand.items()}
        assert 0 < (prior[:, 1] > 0).sum() < len(prior)
        r = SC.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
        assert np.array_equal(r.region("z_coarse"), z_c[keep]) and np.array_equal(r.region("z_fine"), z_f[keep])
        _, gc, gf = b.mse_loss(r.out["rgb_coarse"], r.out["rgb_fine"], tgt)
        gw, _ = depth_cotangents(r, prior)
        got = r.backward((gc, gf), gw, entry="parts_w")
        targs = (par_c, par_f, cfg, rays, z_c[keep], z_f[keep], opt, rand, tgt, prior)
        ref_c, ref_f, _, _ = teacher(*targs, DEPTH_W, torch.float64)
        r32_c, r32_f, _, _ = teacher(*targs, DEPTH_W, torch.float32)
        mse_c, mse_f, _, _ = teacher(*targs, ((0.0, 0.0), (0.0, 0.0)), torch.float64)
        for tag, plan, ref, r32, mse in (("coarse", pc, ref_c, r32_c, mse_c), ("fine", pf, ref_f, r32_f, mse_f)):
            g = b.unflatten(plan, got["g_params_" + tag])
            # not vacuous, from the reference alone: the depth terms move the net's gradient by far more than the bound
            moved = max(float(np.abs(v - mse[k]).max()) / float(np.abs(v).max()) for k, v in ref.items())
            assert moved > 10.0 * tol, (tag, moved)
            for k, v in ref.items():
                mag = float(np.abs(v).max())
                err, own = float(np.abs(g[k] - v).max()) / mag, float(np.abs(r32[k] - v).max()) / mag
                bound = tol if own <= tol else 2.0 * own
                print("param grads %s %s n=%d %s %s: %.3e of max|g| (oracle fp32 vs fp64 %.3e, bound %.1e)" % (net, arith, n, tag, k, err, own, bound))
                if record is not None:
                    record.append((net, arith, n, tag, k, err, own, bound))
                assert err <= bound, (net, arith, n, tag, k, err, own, bound)
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


def case_compacted(b, net, arith, modes, n=48, nc=8, nf=8, noise=0.6):
    """spread_cases.case_compacted with the depth priors' cotangent: the modes against mode 0 within `unit.compact_vs_dense` of max|g|
    per tensor; `kept` equals the count of nonzero d(loss)/d(raw) rows the compositing backward left."""
    ctol = TL.bound("unit.compact_vs_dense", arith)
    cfg, pc, _, _, packed_c = SC.setup(b, net, arith, seed=3)
    _, pf, _, _, packed_f = SC.setup(b, net, arith, seed=4)
    _, rays, rand, opt, tgt = SC.render_problem(net, n, nc, nf, seed=35, noise=noise)
    prior = render_prior(rays, seed=43)
    res = {}
    for mode in (False,) + tuple(modes):
        b.set_compaction(pc, mode)
        b.set_compaction(pf, mode)
        r = SC.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
        if mode is False:
            _, gc, gf = b.mse_loss(r.out["rgb_coarse"], r.out["rgb_fine"], tgt)
        gw, _ = depth_cotangents(r, prior)
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
    """nerfhip_render_bwd_rays_w with both terms: d(loss)/d(rays) against the oracle's autograd teacher-forced on the kernels' own
    depths, under parity_cases.case_ray_grad's distribution bound (as spread_cases.case_rays_w)."""
    cfg, pc, par_c, flat_c, packed_c = SC.setup(b, net, "fp32", seed=3)
    _, pf, par_f, flat_f, packed_f = SC.setup(b, net, "fp32", seed=4)
    _, rays, rand, opt, tgt = SC.render_problem(net, n, nc, nf, seed=37, noise=0.0)
    prior = render_prior(rays, seed=45)
    r = SC.RenderW(b, pc, pf, packed_c, packed_f, rays, opt, rand)
    z_c, z_f = r.region("z_coarse"), r.region("z_fine")
    _, gc, gf = b.mse_loss(r.out["rgb_coarse"], r.out["rgb_fine"], tgt)
    gw, _ = depth_cotangents(r, prior)
    got = r.backward((gc, gf), gw, entry="rays_w", params=(flat_c, flat_f))["g_rays"]
    targs = (par_c, par_f, cfg, rays, z_c, z_f, opt, rand, tgt, prior)
    ref = teacher(*targs, DEPTH_W, torch.float32, wrt_rays=True)[2]
    ref64 = teacher(*targs, DEPTH_W, torch.float64, wrt_rays=True)[2]
    plain64 = teacher(*targs, ((0.0, 0.0), (0.0, 0.0)), torch.float64, wrt_rays=True)[2]
    assert np.isfinite(ref64).all() and float(np.any(ref64[:, 0:3] != 0.0, axis=1).mean()) >= 0.9
    for lo, hi, what in ((0, 3, "origin"), (3, 6, "direction"), (8, 11, "viewdirs")):
        scale = float(np.abs(ref64[:, lo:hi]).max())
        assert scale > 0.0, what
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


def case_culled_step(b, net, arith, outside, n=21, nc=9, nf=6, noise_std=0.3):
    """spread_cases.case_culled_step with the depth priors' cotangent: arm A by hand in mode 1, arm B nerfhip_render_fwd_occ_train in
    mode 2 (and 4 where the plan has it); by that case's criteria -- the weight cotangents bit-identical, each net's kept count equal,
    gradients array_equal in mode 2 and within unit.compact_vs_dense in mode 4, and not the gradients without the depth terms --, and
    the d(loss)/d(raw) rows of culled samples exactly zero."""
    import occupancy_train_cases as OT
    cfg, pc, pf, packed_c, packed_f, modes = OT.nets_and_modes(b, net, arith)
    rays, rnp, tgt = OT.half_empty_inputs(cfg, n, nc, nf)
    prior = render_prior(rays, seed=47, frac=0.6)
    grid = OC.Grid(b, OT.half_empty_bits(rays, 23), *OC.SCENE_BOX, (8, 8, 16), outside)
    opt = dict(num_coarse=nc, num_fine=nf, perturb=True, white_background=True, noise_std=noise_std)
    rd = np.ascontiguousarray(rays[:, 3:6])
    for p in (pc, pf):
        b.set_compaction(p, True)
    a = OT.Step(b, pc, pf, packed_c, packed_f, rays, opt, rnp)
    culled = {}
    for fine, part in ((False, L.PART_COARSE), (True, L.PART_FINE)):
        a.fwd(part)
        tag = "fine" if fine else "coarse"
        z, raw = a.region("z_" + tag), a.region("raw_" + tag)
        fl = OC.occ_mark(b, grid, rays, z).astype(bool)
        assert 0.2 < 1.0 - fl.mean() < 0.8
        culled[tag] = ~fl
        raw[~fl] = OC.EMPTY
        a.set_region("raw_" + tag, raw)
        out = b.volume_render_fwd(raw, z, rd, noise_std, rnp["noise_fine" if fine else "noise_coarse"], True)
        for k, v in zip(("rgb", "disp", "acc", None, "depth"), out):
            if k:
                a.set_map(k + "_" + tag, v)
        if not fine:
            a.set_region("weights_coarse", out[3])
    want = a.maps()
    gw_a, losses = depth_cotangents(a, prior)
    assert all(np.isfinite(lo).all() and lo.any() for lo in losses)
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
        gw, _ = depth_cotangents(s, prior)
        for i in (0, 1):
            assert np.array_equal(b.host(gw[i]), b.host(gw_a[i])), (mode, i)
        got.update(s.bwd(got["rgb_coarse"] - tgt, got["rgb_fine"] - tgt, gw))
        for tag, plan in (("coarse", pc), ("fine", pf)):
            g_raw = s.region("bwd_g_raw_" + tag)
            assert culled[tag].any() and not g_raw[culled[tag]].any(), (mode, tag)   # rows of culled samples stay exactly zero
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
