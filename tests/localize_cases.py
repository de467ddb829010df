"""Cases of the frozen ray gradient (nerfhip_render_grad_rays / nerfhip_render_grad_rays_tmp_bytes, include/nerfhip.h; csrc/nh_raygrad.h),
written once against a backend of tests/backends.py: tests/test_localize.py runs them on the wave emulator, tests/test_gpu_localize.py
on the product library.

1. against the oracle: the construction and the distribution test of parity_cases.case_ray_grad -- per column block the median error
   against the oracle's fp32 autograd <= 3 x the median of the oracle's own fp32-vs-fp64 error + 2e-6, rays beyond 2e-3 <= 2 x the
   oracle's own count + 3, columns 6-7 exactly zero (the bound nerfhip_render_bwd_rays is held to, for the reason given there);
2. against the path it stands in for (nerfhip_render_bwd_rays on the same build and inputs): the d(pre-activation) images are the same,
   the two differ in summation order and in the grouping of the encoding's VJP only: per column block the median over rays of
   |new - old| / max|ref64| <= 3 x the same oracle median + 2e-6;
3. on the bits: backward modes, repeated calls, parts, workspace layouts, an open encoding window;
4. refusals.
The oracle's references are computed once per problem and shared by 1 and 2 (and by both backends of one session).
The emulator suite runs the GPU suite's geometries at ray counts it can walk in seconds (5 .. 12 rays): there 1 and 2 check the index
algebra (a wrong column, unit or row is an error of order one); a median over so few rays says little about the distribution, and the
oracle bound carries its meaning at the GPU suite's sizes only.
"""
import ctypes as C

import numpy as np
import torch

import nerf_oracle as O
import nerf_pytorch_amd._lib as L
import parity_cases as PC
import window_cases as WC

BOTH = L.PART_COARSE | L.PART_FINE


# ---- the launches -----------------------------------------------------------------------------------------------------------------
class Rendered:
    """A training forward of two plans whose workspace stays, so that any number of backwards can run over it.
    layout: 1 (one set of backward buffers per net) or 2 (shared: calls carry NERFHIP_PART_SHARED_BWD)."""

    def __init__(self, b, pc, pf, packed_c, packed_f, rays, opt, rand=None, layout=1, seed=0, ray_offset=0):
        rand = rand or {}
        self.b, self.pc, self.pf, self.packed_c, self.packed_f = b, pc, pf, packed_c, packed_f
        self.n, self.stride = rays.shape
        n, nc, nf = self.n, opt["num_coarse"], opt["num_fine"]
        self.nc, self.nf, self.layout, self.seed, self.ray_offset = nc, nf, layout, seed, ray_offset
        self.cfg = L.RenderCfg(nc, nf, int(bool(opt.get("perturb", True))), int(bool(opt.get("lindisp", False))),
                               int(bool(opt.get("white_background", False))), float(opt.get("noise_std", 0.0)), self.stride)
        self.rays = b.dev(np.ascontiguousarray(rays, np.float32))
        t_vals, u_det = b.dev(b._linspace01(nc)), b.dev(b._linspace01(nf))
        self._keep = [b.devopt(rand.get(k)) for k in ("t_rand", "noise_coarse", "u", "noise_fine")]
        self.rr = L.RenderRand(*[b.p(k) for k in self._keep])
        names = ("rgb_coarse", "disp_coarse", "acc_coarse", "depth_coarse", "rgb_fine", "disp_fine", "acc_fine", "depth_fine")
        bufs = {k: b.empty((n, 3) if k.startswith("rgb") else (n,)) for k in names}
        ro = L.RenderOut(*[b.ptr(bufs[k]) for k in names])
        self.wsb = b.lib.render_workspace_bytes(pc, pf, C.byref(self.cfg), n, layout)
        assert self.wsb >= 0, b.lib.last_error()
        self.ws = b.empty((self.wsb // 4 + 1,))
        b.lib.render_fwd(pc, pf, C.byref(self.cfg), b.ptr(self.rays), n, b.ptr(packed_c), b.ptr(packed_f), b.ptr(t_vals), b.ptr(u_det),
                         C.byref(self.rr), seed, ray_offset, C.byref(ro), b.ptr(self.ws), self.wsb, layout, b.stream())
        self.out = {k: b.host(v) for k, v in bufs.items()}

    def mse_cotangents(self, target):
        _, gc, gf = self.b.mse_loss(self.out["rgb_coarse"], self.out["rgb_fine"], np.ascontiguousarray(target, np.float32))
        return gc, gf

    def _head(self):
        b = self.b
        return (self.pc, self.pf, C.byref(self.cfg), b.ptr(self.rays), self.n, b.ptr(self.packed_c), b.ptr(self.packed_f), C.byref(self.rr),
                self.seed, self.ray_offset)

    def grad_rays(self, g, params, parts=BOTH):
        """nerfhip_render_grad_rays -> g_rays (host)."""
        b = self.b
        gc, gf, fc, ff = b.dev(g[0]), b.dev(g[1]), b.dev(params[0]), b.dev(params[1])
        tb = b.lib.render_grad_rays_tmp_bytes(self.pc, self.pf, C.byref(self.cfg), self.n)
        assert tb >= 0
        tmp, g_rays = b.empty((tb // 4 + 4,)), b.empty((self.n, self.stride))
        cot = L.RenderCotangents(b.ptr(gc), None, None, b.ptr(gf), None, None)
        b.lib.render_grad_rays(*self._head(), C.byref(cot), b.ptr(self.ws), self.wsb, parts | (L.PART_SHARED_BWD if self.layout == 2 else 0),
                               b.ptr(fc), b.ptr(ff), b.ptr(tmp), tb, b.ptr(g_rays), b.stream())
        return b.host(g_rays)

    def bwd_rays(self, g, params):
        """nerfhip_render_bwd_rays (the trainable path: parameter gradients too) -> g_rays (host)."""
        b = self.b
        gc, gf, fc, ff = b.dev(g[0]), b.dev(g[1]), b.dev(params[0]), b.dev(params[1])
        gpc, gpf = b.empty((b.lib.plan_num_params(self.pc),)), b.empty((b.lib.plan_num_params(self.pf),))
        tb = b.lib.render_bwd_rays_tmp_bytes(self.pc, self.pf, C.byref(self.cfg), self.n)
        tmp, g_rays = b.empty((tb // 4 + 1,)), b.empty((self.n, self.stride))
        cot = L.RenderCotangents(b.ptr(gc), None, None, b.ptr(gf), None, None)
        b.lib.render_bwd_rays(*self._head(), C.byref(cot), b.ptr(self.ws), self.wsb, b.ptr(gpc), b.ptr(gpf),
                              BOTH | (L.PART_SHARED_BWD if self.layout == 2 else 0), b.ptr(fc), b.ptr(ff), b.ptr(tmp), tb, b.ptr(g_rays), b.stream())
        return b.host(g_rays)

    def kept(self, fine=True):
        """(kept, total) sample points of the last compacted backward of one net (layout 1)."""
        b = self.b
        assert self.layout == 1
        plan, samples = (self.pf, self.nc + self.nf) if fine else (self.pc, self.nc)
        off, nb = C.c_int64(), C.c_int64()
        b.lib.render_workspace_region(self.pc, self.pf, C.byref(self.cfg), self.n, 1, b"bwd_scratch_fine" if fine else b"bwd_scratch_coarse",
                                      C.byref(off), C.byref(nb))
        so = b.lib.plan_bwd_stats_offset(plan, self.n * samples)
        w = b.host(self.ws[(off.value + so) // 4:(off.value + so) // 4 + 2])
        return tuple(int(v) for v in np.ascontiguousarray(w).view(np.int32))


# ---- the problems -------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def problem(name, n, nc, nf, seed=61, white=False, noise=0.0):
    """parity_cases.case_ray_grad's construction, and the oracle's fp32 / fp64 ray gradients of it (computed once)."""
    key = (name, n, nc, nf, seed, white, noise)
    if key in _ORACLE:
        return _ORACLE[key]
    cfg = PC.MLP_GEOMETRIES[name]
    gen = PC.rng(seed)
    par_c, par_f = O.init_params(cfg, seed=seed + 1), O.init_params(cfg, seed=seed + 2)
    ro = torch.tensor([0.2, -0.1, 4.0]).expand(n, 3) + 0.05 * torch.randn(n, 3, generator=gen)
    rd = torch.randn(n, 3, generator=gen) * 0.3
    rd[:, 2] = -1.0
    view = cfg["use_viewdirs"]
    rays = O.pack_rays(ro, rd, 2.0, 6.0, rd if view else None).requires_grad_(True)
    rand = dict(t_rand=torch.rand(n, nc, generator=gen), noise_coarse=torch.randn(n, nc, generator=gen),
                u=torch.rand(n, nf, generator=gen), noise_fine=torch.randn(n, nc + nf, generator=gen))
    opt = dict(num_coarse=nc, num_fine=nf, perturb=True, lindisp=False, white_background=white, noise_std=noise)
    tgt = torch.rand(n, 3, generator=gen)
    want = O.render_rays(rays, par_c, par_f, cfg, cfg, opt, rand)
    loss, _, _, _ = O.loss_and_psnr(want["rgb_coarse"], want["rgb_fine"], tgt)
    loss.backward()
    r64 = rays.detach().double().requires_grad_(True)
    w64 = O.render_rays(r64, {k: v.double() for k, v in par_c.items()}, {k: v.double() for k, v in par_f.items()}, cfg, cfg, opt,
                        {k: v.double() for k, v in rand.items()})
    l64, _, _, _ = O.loss_and_psnr(w64["rgb_coarse"], w64["rgb_fine"], tgt.double())
    l64.backward()
    pr = dict(cfg=cfg, view=view, par_c=par_c, par_f=par_f, rays=rays.detach().numpy(), rand={k: v.numpy() for k, v in rand.items()}, opt=opt,
              tgt=tgt.numpy(), ref=rays.grad.numpy(), ref64=r64.grad.numpy(), results={})
    _ORACLE[key] = pr
    return pr


def plans(b, pr, mode=False, precision=0):
    out = []
    for par in (pr["par_c"], pr["par_f"]):
        plan = b.make_plan(pr["cfg"], precision)
        flat = b.flatten_params(plan, {k: v.numpy() for k, v in par.items()})
        b.set_compaction(plan, mode)
        out.append((plan, flat, b.pack(plan, flat)))
    return out


def blocks(view):
    return ((0, 3, "origin"), (3, 6, "direction")) + (((8, 11, "viewdirs"),) if view else ())


def both_paths(b, pr, mode=False, precision=0):
    """(new, old): g_rays of nerfhip_render_grad_rays and of nerfhip_render_bwd_rays on the same forward (once per backend and problem)."""
    key = (b.name, mode, precision)
    if key not in pr["results"]:
        (pc, fc, kc), (pf, ff, kf) = plans(b, pr, mode, precision)
        r = Rendered(b, pc, pf, kc, kf, pr["rays"], pr["opt"], pr["rand"])
        g = r.mse_cotangents(pr["tgt"])
        pr["results"][key] = (r.grad_rays(g, (fc, ff)), r.bwd_rays(g, (fc, ff)))
        b.lib.plan_destroy(pc)
        b.lib.plan_destroy(pf)
    return pr["results"][key]


# ---- 1 / 2 --------------------------------------------------------------------------------------------------------------------------
def case_vs_oracle(b, name, n, nc=16, nf=16, mode=False, precision=0, **kw):
    pr = problem(name, n, nc, nf, **kw)
    got, _ = both_paths(b, pr, mode, precision)
    ref, ref64 = pr["ref"], pr["ref64"]
    rec = {}
    for lo, hi, what in blocks(pr["view"]):
        scale = float(np.abs(ref64[:, lo:hi]).max()) + 1e-30
        e_hip = np.abs(got[:, lo:hi] - ref[:, lo:hi]).max(axis=1) / scale
        e_yard = np.abs(ref[:, lo:hi] - ref64[:, lo:hi]).max(axis=1) / scale
        rec[what] = dict(hip_median=float(np.median(e_hip)), yard_median=float(np.median(e_yard)), hip_over=int((e_hip > 2e-3).sum()),
                         yard_over=int((e_yard > 2e-3).sum()))
        print("LOCALIZE oracle %s n%d %s %s: %s" % (name, n, b.name, what, rec[what]))
        assert np.median(e_hip) <= 3.0 * np.median(e_yard) + 2e-6, (what, rec[what])
        assert (e_hip > 2e-3).sum() <= 2 * (e_yard > 2e-3).sum() + 3, (what, rec[what])
    PC.note("grad_rays_%s_n%d_%s_p%d_%s" % (name, n, mode, precision, b.name), **{"%s_%s" % (w_, k): v for w_, d in rec.items() for k, v in d.items()})
    assert np.all(got[:, 6:8] == 0.0)


def case_vs_trainable_path(b, name, n, nc=16, nf=16, mode=False, precision=0, **kw):
    pr = problem(name, n, nc, nf, **kw)
    new, old = both_paths(b, pr, mode, precision)
    ref, ref64 = pr["ref"], pr["ref64"]
    rec = {}
    for lo, hi, what in blocks(pr["view"]):
        scale = float(np.abs(ref64[:, lo:hi]).max()) + 1e-30
        d = np.abs(new[:, lo:hi].astype(np.float64) - old[:, lo:hi]).max(axis=1) / scale
        e_yard = np.abs(ref[:, lo:hi] - ref64[:, lo:hi]).max(axis=1) / scale
        rec[what + "_new_vs_old_median"], rec[what + "_yard_median"] = float(np.median(d)), float(np.median(e_yard))
        print("LOCALIZE new-vs-old %s n%d %s %s: median %.3e (yardstick %.3e), max %.3e" % (name, n, b.name, what, np.median(d), np.median(e_yard), d.max()))
    PC.note("grad_rays_vs_bwd_rays_%s_n%d_%s_p%d_%s" % (name, n, mode, precision, b.name), **rec)
    for _, _, what in blocks(pr["view"]):
        assert rec[what + "_new_vs_old_median"] <= 3.0 * rec[what + "_yard_median"] + 2e-6, (what, rec)
    assert np.array_equal(new[:, 6:8], old[:, 6:8])


# ---- 3: on the bits -----------------------------------------------------------------------------------------------------------------
def _zero_fraction_inputs(pr, which):
    """Parameters and a cotangent mask for a zero fraction of the d(raw output) rows near 0 ("none": every density pre-activation
    pushed positive, every ray's cotangent kept), near one half and above ("half": the plain nets -- the samples whose density
    pre-activation is negative are single zero rows -- and every other ray's cotangent zeroed: whole rays) or 1 ("all")."""
    par_c, par_f = dict(pr["par_c"]), dict(pr["par_f"])
    n = pr["rays"].shape[0]
    mask = np.ones((n, 1), np.float32)
    if which == "none":
        for par in (par_c, par_f):
            k = [k for k in par if "alpha" in k and k.endswith("bias")]
            assert len(k) == 1, list(par)
            par[k[0]] = par[k[0]] + 3.0
    elif which == "half":
        mask[::2] = 0.0
    else:
        mask[:] = 0.0
    return dict(pr, par_c=par_c, par_f=par_f), mask


def case_modes_give_the_same_bits(b, name="default4x128", n=13, nc=8, nf=8, modes=(False, True, "recompute"), noise=0.3):
    pr0 = problem(name, n, nc, nf, noise=noise)
    for which, lo, hi in (("none", 0.0, 0.05), ("half", 0.45, 0.95), ("all", 1.0, 1.0)):
        pr, mask = _zero_fraction_inputs(pr0, which)
        got = {}
        for mode in modes:
            (pc, fc, kc), (pf, ff, kf) = plans(b, pr, mode)
            r = Rendered(b, pc, pf, kc, kf, pr["rays"], pr["opt"], pr["rand"])
            gc, gf = r.mse_cotangents(pr["tgt"])
            g = (gc * mask, gf * mask)
            got[mode] = r.grad_rays(g, (fc, ff))
            again = r.grad_rays(g, (fc, ff))                      # (two calls over one forward)
            assert np.array_equal(WC.bits(again), WC.bits(got[mode])), (which, mode)
            if b.lib.plan_bwd_compaction(pf) in (1, 2):
                kept, total = r.kept()
                frac = 1.0 - kept / float(total)
                PC.note("grad_rays_modes_%s_%s" % (name, b.name), **{"zero_fraction_" + which: frac})
                assert total == n * (nc + nf) and lo <= frac <= hi, (which, kept, total)
            b.lib.plan_destroy(pc)
            b.lib.plan_destroy(pf)
        assert np.isfinite(got[modes[0]]).all()
        for mode in modes[1:]:
            assert np.array_equal(got[mode], got[modes[0]]), (which, mode, float(np.abs(got[mode] - got[modes[0]]).max()))
        if which == "all":
            assert not got[modes[0]].any()
        else:
            assert np.abs(got[modes[0]][:, :6]).max() > 0.0
            if which == "half":   # (a ray whose cotangents are zero has no gradient; the others have one)
                assert not got[modes[0]][::2].any() and got[modes[0]][1::2, :6].any(axis=1).all()


def case_parts_layouts_window(b, name="default4x128", n=13, nc=8, nf=8, mode=True):
    pr = problem(name, n, nc, nf, noise=0.3)
    (pc, fc, kc), (pf, ff, kf) = plans(b, pr, mode)
    r = Rendered(b, pc, pf, kc, kf, pr["rays"], pr["opt"], pr["rand"])
    g = r.mse_cotangents(pr["tgt"])
    whole = r.grad_rays(g, (fc, ff))
    # the fine pass and the coarse pass by themselves (each the first pass of its call: it overwrites), added as the engine's pose VJP
    # adds its two buffers, are the one call's "overwrite, then accumulate"
    fine, coarse = r.grad_rays(g, (fc, ff), L.PART_FINE), r.grad_rays(g, (fc, ff), L.PART_COARSE)
    assert np.isfinite(fine).all() and np.isfinite(coarse).all() and fine[:, :6].any() and coarse[:, :6].any()
    assert np.array_equal(WC.bits(fine + coarse), WC.bits(whole))
    # one shared set of backward buffers
    r2 = Rendered(b, pc, pf, kc, kf, pr["rays"], pr["opt"], pr["rand"], layout=2)
    assert np.array_equal(WC.bits(r2.grad_rays(r2.mse_cotangents(pr["tgt"]), (fc, ff))), WC.bits(whole))
    # an open encoding window: theta_eff is theta
    codes = WC.window_index(b, pc)
    lx, ld = WC.bands_of(pr["cfg"])
    w = WC.window_struct(pr["cfg"], float(lx), float(ld))
    ec, ef = WC.window_params(b, fc, codes, w), WC.window_params(b, ff, codes, w)
    r3 = Rendered(b, pc, pf, b.pack(pc, ec), b.pack(pf, ef), pr["rays"], pr["opt"], pr["rand"])
    assert np.array_equal(WC.bits(r3.grad_rays(r3.mse_cotangents(pr["tgt"]), (ec, ef))), WC.bits(whole))
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


# ---- 4: refusals ----------------------------------------------------------------------------------------------------------------------
def case_refusals(b, name="default4x128", n=5, nc=8, nf=8):
    pr = problem(name, n, nc, nf)
    (pc, fc, kc), (pf, ff, kf) = plans(b, pr)
    r = Rendered(b, pc, pf, kc, kf, pr["rays"], pr["opt"], pr["rand"])
    gc, gf = (b.dev(v) for v in r.mse_cotangents(pr["tgt"]))
    dfc, dff = b.dev(fc), b.dev(ff)
    raw, err = b.lib._dll.nerfhip_render_grad_rays, b.lib._dll.nerfhip_last_error
    tb = b.lib.render_grad_rays_tmp_bytes(pc, pf, C.byref(r.cfg), n)
    assert tb > 0 and b.lib.render_grad_rays_tmp_bytes(pc, pf, C.byref(r.cfg), 0) >= 0 and b.lib.render_grad_rays_tmp_bytes(pc, pf, C.byref(r.cfg), -1) == -1
    tmp, g_rays = b.empty((tb // 4 + 4,)), b.empty((n, r.stride))
    cot = L.RenderCotangents(b.ptr(gc), None, None, b.ptr(gf), None, None)

    def call(parts=BOTH, params=(b.ptr(dfc), b.ptr(dff)), tmp_p=b.ptr(tmp), tmp_b=tb, out=b.ptr(g_rays), plans_=(pc, pf), packs=(kc, kf), rays_n=n):
        head = (plans_[0], plans_[1], C.byref(r.cfg), b.ptr(r.rays), rays_n, b.ptr(packs[0]), b.ptr(packs[1]), C.byref(r.rr), 0, 0)
        return raw(*head, C.byref(cot), b.ptr(r.ws), r.wsb, parts, params[0], params[1], tmp_p, tmp_b, out, b.stream())

    assert call() == 0
    for kw, msg in ((dict(out=None), b"g_rays is NULL"), (dict(tmp_p=None), b"tmp is NULL"), (dict(params=(None, b.ptr(dff))), b"params"),
                    (dict(params=(b.ptr(dfc), None)), b"params"), (dict(tmp_b=tb - 1), b"bytes of tmp"), (dict(parts=0), b"parts"),
                    (dict(parts=L.PART_SHARED_BWD), b"parts"), (dict(parts=8), b"parts")):
        assert call(**kw) == -1 and msg in err(), (kw, err())
    assert call(rays_n=0) == 0 and call(rays_n=0, out=None, tmp_p=None) == 0          # (empty: nothing to launch)
    # an fp16 inference-only plan has no backward
    (qc, gc_flat, qkc), (qf, gf_flat, qkf) = plans(b, pr, precision=PC.F16X3)
    assert call(plans_=(qc, qf), packs=(qkc, qkf)) == -1 and b"inference-only" in err(), err()
    for p in (pc, pf, qc, qf):
        b.lib.plan_destroy(p)
