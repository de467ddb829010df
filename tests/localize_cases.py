"""Cases of the frozen ray gradient (nerfhip_render_grad_rays / nerfhip_render_grad_rays_tmp_bytes, include/nerfhip.h; csrc/nh_raygrad.h),
written once against a backend of tests/backends.py: tests/test_localize.py runs them on the wave emulator, tests/test_gpu_localize.py
on the product library.

0. teacher-forced, EVERY ray (case_teacher_forced): both chains -- nerfhip_render_grad_rays and nerfhip_render_bwd_rays over one forward --
   against the oracle's autograd in fp64 on the depths that forward's kernels produced, held constant (O.render_at_depths: no stratified
   draw, no sampler between the two, so none of the chaos 1 has to allow for).  Per column block, of max|ref64|: the LARGEST error over the
   rays whose ReLU branches round-off cannot decide (O.mlp_relu_margin in fp64 at every coarse and fine sample above unit.mlp_bwd's margin)
   <= 2 x the oracle's own fp32 run's largest over those rays + 2e-6 (tolerances.py: unit.ray_grad.tf_fp64_yardstick), and the two chains
   within 1 x that + 2e-6 of each other on ALL rays (unit.ray_grad.new_vs_old: they share every branch).  With the colour cotangents, or
   with all six (ALL_COT: acc and depth of both passes drive g_norm and the depth-weighted sums).  Nothing is compared before the
   reference alone has shown that there is something to compare: a scale in every block, a gradient on >= 90 % of the rays, and the
   filter leaving at least DECIDED_GPU / DECIDED_EMU of them;
1. against the oracle END TO END: the construction and the distribution test of parity_cases.case_ray_grad -- per column block the median
   error against the oracle's fp32 autograd <= 3 x the median of the oracle's own fp32-vs-fp64 error + 2e-6, rays beyond 2e-3 <= 2 x the
   oracle's own count + 3, columns 6-7 exactly zero (the bound nerfhip_render_bwd_rays is held to, for the reason given there: the sampler
   and the ReLU branches make a few per cent of the rays chaotic).  A claim about the distribution: an error in fewer than half of the
   rays, or one below 2e-3 in all of them, passes it -- 0 is what looks at those;
2. against the path it stands in for (nerfhip_render_bwd_rays on the same build and inputs): the d(pre-activation) images are the same,
   the two differ in summation order and in the grouping of the encoding's VJP only: per column block the median over rays of
   |new - old| / max|ref64| <= 3 x the same oracle median + 2e-6, and the maximum over all rays under unit.ray_grad.new_vs_old with the
   teacher-forced yardstick of 0 on this forward's depths;
3. on the bits: backward modes, repeated calls, parts, workspace layouts, an open encoding window;
4. refusals.
The oracle's references are computed once per problem and shared by 0, 1 and 2 (and by both backends of one session).
The emulator suite runs the GPU suite's geometries at ray counts it can walk in seconds (5 .. 12 rays): there 0 checks every ray it has,
1 and 2 check the index algebra (a wrong column, unit or row is an error of order one); a median over so few rays says little about the
distribution, and 1's bound carries its meaning at the GPU suite's sizes only.
"""
import ctypes as C

import numpy as np
import torch

import backends as BK
import nerf_oracle as O
import nerf_pytorch_amd._lib as L
import parity_cases as PC
import tolerances as TL
import window_cases as WC

BOTH = L.PART_COARSE | L.PART_FINE


# ---- the launches -----------------------------------------------------------------------------------------------------------------
class Rendered(BK.Rendered):
    """A training forward of two plans whose workspace stays, so that any number of backwards can run over it (backends.RenderSession:
    grad_rays, backward, region, kept), and the cotangents of this file's losses.
    layout: 1 (one set of backward buffers per net) or 2 (shared: calls carry NERFHIP_PART_SHARED_BWD)."""

    def mse_cotangents(self, target):
        _, gc, gf = self.b.mse_loss(self.out["rgb_coarse"], self.out["rgb_fine"], np.ascontiguousarray(target, np.float32))
        return gc, gf

    def all_cotangents(self, target):
        """The six cotangents of the summed colour mse + ALL_COT's terms, formed on the host from this forward's outputs:
        (g_rgb_coarse, g_rgb_fine, g_acc_coarse, g_acc_fine, g_depth_coarse, g_depth_fine)."""
        gc, gf = self.mse_cotangents(target)
        n, one = np.float32(self.n), np.ones(self.n, np.float32)
        return (gc, gf, np.float32(2.0 * ALL_COT["acc_coarse"]) * self.out["acc_coarse"] / n, np.float32(2.0 * ALL_COT["acc_fine"]) * self.out["acc_fine"] / n,
                np.float32(ALL_COT["depth_coarse"]) * one / n, np.float32(ALL_COT["depth_fine"]) * one / n)

    def bwd_rays(self, g, params):
        """nerfhip_render_bwd_rays (the trainable path: parameter gradients too) -> g_rays (host).  g: as grad_rays."""
        return self.backward(g, entry="rays", params=params)["g_rays"]


# ---- the problems -------------------------------------------------------------------------------------------------------------------
_ORACLE = {}
# the "all cotangents" loss: the summed colour mse + these multiples of mean(acc^2) and mean(depth) of either pass
ALL_COT = dict(acc_fine=0.3, acc_coarse=0.2, depth_fine=0.1, depth_coarse=0.05)
NONZERO_SHARE = 0.9        # of the rays have a gradient in the reference, or a comparison over "the rays" compares zeros
DECIDED_GPU, DECIDED_EMU = (0.5, 16), (0.3, 3)     # (share, count) of the rays the ReLU filter must leave a teacher-forced case


def problem(name, n, nc, nf, seed=61, white=False, noise=0.0):
    """parity_cases.case_ray_grad's construction (the oracle's gradients of it: oracle_grads, teacher_forced)."""
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
    rays = O.pack_rays(ro, rd, 2.0, 6.0, rd if view else None)
    rand = dict(t_rand=torch.rand(n, nc, generator=gen), noise_coarse=torch.randn(n, nc, generator=gen),
                u=torch.rand(n, nf, generator=gen), noise_fine=torch.randn(n, nc + nf, generator=gen))
    opt = dict(num_coarse=nc, num_fine=nf, perturb=True, lindisp=False, white_background=white, noise_std=noise)
    tgt = torch.rand(n, 3, generator=gen)
    pr = dict(name=name, cfg=cfg, view=view, par_c=par_c, par_f=par_f, rays=rays.numpy(), rand={k: v.numpy() for k, v in rand.items()}, opt=opt,
              tgt=tgt.numpy(), results={}, tf={})
    _ORACLE[key] = pr
    return pr


def _as(pr, dtype):
    cast = lambda d: {k: torch.from_numpy(np.asarray(v)).to(dtype) if not torch.is_tensor(v) else v.to(dtype) for k, v in d.items()}
    return cast(pr["par_c"]), cast(pr["par_f"]), cast(pr["rand"]), torch.from_numpy(pr["tgt"]).to(dtype)


def oracle_grads(pr):
    """(ref, ref64): the oracle's END-TO-END fp32 and fp64 autograd w.r.t. the rays (its own depths, its sampler in the graph's path), once."""
    if "ref" not in pr:
        for key, dtype in (("ref", torch.float32), ("ref64", torch.float64)):
            par_c, par_f, rand, tgt = _as(pr, dtype)
            rays = torch.from_numpy(pr["rays"]).to(dtype).requires_grad_(True)
            want = O.render_rays(rays, par_c, par_f, pr["cfg"], pr["cfg"], pr["opt"], rand)
            loss, _, _, _ = O.loss_and_psnr(want["rgb_coarse"], want["rgb_fine"], tgt)
            loss.backward()
            pr[key] = rays.grad.numpy()
    return pr["ref"], pr["ref64"]


def nonvacuous(ref64, view, what):
    """Computed from the reference alone: every block has a scale, and NONZERO_SHARE of the rays a gradient.  -> {block: scale}."""
    share = float(np.any(ref64[:, 0:3] != 0.0, axis=1).mean())
    assert np.isfinite(ref64).all() and share >= NONZERO_SHARE, "%s: %.2f of the rays have a gradient in the fp64 reference" % (what, share)
    scales = {}
    for lo, hi, blk in blocks(view):
        scales[blk] = float(np.abs(ref64[:, lo:hi]).max())
        assert scales[blk] > 0.0, "%s: the fp64 reference has no %s gradient" % (what, blk)
    return scales


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


def both_paths(b, pr, mode=False, precision=0, allcot=False):
    """One forward, both backwards over it (once per backend and problem): dict(new = g_rays of nerfhip_render_grad_rays, old = of
    nerfhip_render_bwd_rays, z_coarse, z_fine = the depths the forward's kernels produced)."""
    key = (b.name, mode, precision, allcot)
    if key not in pr["results"]:
        (pc, fc, kc), (pf, ff, kf) = plans(b, pr, mode, precision)
        r = Rendered(b, pc, pf, kc, kf, pr["rays"], pr["opt"], pr["rand"])
        z_c, z_f = r.region("z_coarse"), r.region("z_fine")
        g = r.all_cotangents(pr["tgt"]) if allcot else r.mse_cotangents(pr["tgt"])
        pr["results"][key] = dict(new=r.grad_rays(g, (fc, ff)), old=r.bwd_rays(g, (fc, ff)), z_coarse=z_c, z_fine=z_f)
        b.lib.plan_destroy(pc)
        b.lib.plan_destroy(pf)
    return pr["results"][key]


def teacher_forced(b, pr, mode=False, precision=0, allcot=False):
    """The oracle's autograd w.r.t. the rays on the KERNEL's depths (both_paths' z_coarse / z_fine, constants: O.render_at_depths), in
    fp64 and in fp32, and per ray the smallest ReLU margin (fp64) over its samples of both passes: dict(ref64, ref32, margin), once."""
    key = (b.name, mode, precision, allcot)
    if key not in pr["tf"]:
        res = both_paths(b, pr, mode, precision, allcot)
        nc, nf = pr["opt"]["num_coarse"], pr["opt"]["num_fine"]
        assert res["z_coarse"].shape == (pr["rays"].shape[0], nc) and res["z_fine"].shape == (pr["rays"].shape[0], nc + nf)
        assert np.isfinite(res["z_fine"]).all() and np.all(np.diff(res["z_fine"], axis=1) >= 0.0)
        out = {}
        for tag, dtype in (("ref64", torch.float64), ("ref32", torch.float32)):
            par_c, par_f, rand, tgt = _as(pr, dtype)
            rays = torch.from_numpy(pr["rays"]).to(dtype).requires_grad_(True)
            z_c, z_f = torch.from_numpy(res["z_coarse"]).to(dtype), torch.from_numpy(res["z_fine"]).to(dtype)
            w = O.render_at_depths(rays, z_c, z_f, par_c, par_f, pr["cfg"], pr["cfg"], pr["opt"], rand, want_margin=dtype == torch.float64)
            loss, _, _, _ = O.loss_and_psnr(w["rgb_coarse"], w["rgb_fine"], tgt)
            if allcot:
                loss = loss + sum(c * ((w[k] ** 2).mean() if k.startswith("acc") else w[k].mean()) for k, c in ALL_COT.items())
            loss.backward()
            out[tag] = rays.grad.numpy()
            if "relu_margin" in w:
                out["margin"] = w["relu_margin"].numpy()
        pr["tf"][key] = out
    return pr["tf"][key]


def _tf_errors(tf, view, decided, **got):
    """Per block: scale = max|ref64| over all rays; per ray e_x = max|x - ref64| / scale for x = ref32 and every array of `got`."""
    out = {}
    for lo, hi, what in blocks(view):
        scale = float(np.abs(tf["ref64"][:, lo:hi]).max())
        e = {k: np.abs(v[:, lo:hi].astype(np.float64) - tf["ref64"][:, lo:hi]).max(axis=1) / scale for k, v in dict(got, ref32=tf["ref32"]).items()}
        out[what] = dict(scale=scale, e=e, yard=float(e["ref32"][decided].max()) if decided.any() else 0.0)
    return out


# ---- 0: teacher-forced, every ray ---------------------------------------------------------------------------------------------------
def case_teacher_forced(b, name, n, nc=16, nf=16, mode=False, precision=0, allcot=False, floor=DECIDED_GPU, **kw):
    """Both chains on the depths their own forward produced, against the oracle's fp64 autograd on those depths, ray for ray: the largest
    error over the rays whose ReLU branches round-off cannot decide is at most unit.ray_grad.tf_fp64_yardstick of the oracle's own fp32
    run's; the two chains (same d(pre-activation) images, same branches) are unit.ray_grad.new_vs_old apart on EVERY ray.
    n = 1: the filter may leave nothing; the bounds against fp64 then hold for nobody, and new-vs-old is asserted alone."""
    pr = problem(name, n, nc, nf, **kw)
    res, tf = both_paths(b, pr, mode, precision, allcot), teacher_forced(b, pr, mode, precision, allcot)
    new, old = res["new"], res["old"]
    case = "tf_ray_grad_%s_n%d_%d+%d_%s_p%d%s_%s" % (name, n, nc, nf, mode, precision, "_allcot" if allcot else "", b.name)
    # not vacuous: from the reference alone, before anything is compared
    nonvacuous(tf["ref64"], pr["view"], case)
    decided = tf["margin"] > TL.bound("unit.mlp_bwd")["margin"]
    share = float(decided.mean())
    PC.note(case, decided_share=share, rays=n)
    if n > 1:
        assert share >= floor[0] and int(decided.sum()) >= floor[1], "%s: the ReLU filter leaves %d of %d rays" % (case, int(decided.sum()), n)
    form, pair = TL.bound("unit.ray_grad.tf_fp64_yardstick"), TL.bound("unit.ray_grad.new_vs_old")
    err = _tf_errors(tf, pr["view"], decided, new=new, old=old)
    fails = []
    for lo, hi, what in blocks(pr["view"]):
        e, scale, yard = err[what]["e"], err[what]["scale"], err[what]["yard"]
        d = np.abs(new[:, lo:hi].astype(np.float64) - old[:, lo:hi]).max(axis=1) / scale
        rec = dict(scale=scale, new_vs_old_max=float(d.max()), e_ref32_max=yard, e_ref32_median=float(np.median(e["ref32"])))
        for k in ("new", "old"):
            if decided.any():
                rec["e_%s_max" % k] = float(e[k][decided].max())
            rec["e_%s_median" % k] = float(np.median(e[k]))
            rec["e_%s_max_all_rays" % k] = float(e[k].max())
        print("LOCALIZE teacher-forced %s %s: %s" % (case, what, rec))
        PC.note(case, **{"%s_%s" % (what, k): v for k, v in rec.items()})
        for k in ("new", "old"):
            if decided.any() and not TL.within(rec["e_%s_max" % k], yard, form):
                fails.append((what, k, "ray %d" % int(np.flatnonzero(decided)[e[k][decided].argmax()]), rec["e_%s_max" % k], yard))
        if not TL.within(rec["new_vs_old_max"], yard, pair):
            fails.append((what, "new vs old", "ray %d" % int(d.argmax()), rec["new_vs_old_max"], yard))
    assert not fails, (case, fails)
    assert np.all(new[:, 6:8] == 0.0) and np.all(old[:, 6:8] == 0.0)
    assert np.isfinite(new).all() and np.isfinite(old).all()


# ---- 1 / 2 --------------------------------------------------------------------------------------------------------------------------
def case_vs_oracle(b, name, n, nc=16, nf=16, mode=False, precision=0, **kw):
    pr = problem(name, n, nc, nf, **kw)
    got = both_paths(b, pr, mode, precision)["new"]
    ref, ref64 = oracle_grads(pr)
    scales = nonvacuous(ref64, pr["view"], "%s n%d" % (name, n))
    rec = {}
    for lo, hi, what in blocks(pr["view"]):
        scale = scales[what]
        e_hip = np.abs(got[:, lo:hi] - ref[:, lo:hi]).max(axis=1) / scale
        e_yard = np.abs(ref[:, lo:hi] - ref64[:, lo:hi]).max(axis=1) / scale
        rec[what] = dict(hip_median=float(np.median(e_hip)), yard_median=float(np.median(e_yard)), hip_over=int((e_hip > 2e-3).sum()),
                         yard_over=int((e_yard > 2e-3).sum()), hip_max=float(e_hip.max()), yard_max=float(e_yard.max()))
        print("LOCALIZE oracle %s n%d %s %s: %s" % (name, n, b.name, what, rec[what]))
        assert np.median(e_hip) <= 3.0 * np.median(e_yard) + 2e-6, (what, rec[what])
        assert (e_hip > 2e-3).sum() <= 2 * (e_yard > 2e-3).sum() + 3, (what, rec[what])
    PC.note("grad_rays_%s_n%d_%s_p%d_%s" % (name, n, mode, precision, b.name), **{"%s_%s" % (w_, k): v for w_, d in rec.items() for k, v in d.items()})
    assert np.all(got[:, 6:8] == 0.0)


def case_vs_trainable_path(b, name, n, nc=16, nf=16, mode=False, precision=0, **kw):
    pr = problem(name, n, nc, nf, **kw)
    res = both_paths(b, pr, mode, precision)
    new, old = res["new"], res["old"]
    ref, ref64 = oracle_grads(pr)
    scales = nonvacuous(ref64, pr["view"], "%s n%d" % (name, n))
    # the teacher-forced yardstick of case_teacher_forced, on this forward's depths (no floor on the decided rays here: fewer of them
    # make the yardstick smaller, never larger; with none it is 0 and the bound is the form's `add`)
    tf = teacher_forced(b, pr, mode, precision)
    decided = tf["margin"] > TL.bound("unit.mlp_bwd")["margin"]
    err = _tf_errors(tf, pr["view"], decided)
    rec = {}
    for lo, hi, what in blocks(pr["view"]):
        scale = scales[what]
        d = np.abs(new[:, lo:hi].astype(np.float64) - old[:, lo:hi]).max(axis=1) / scale
        e_yard = np.abs(ref[:, lo:hi] - ref64[:, lo:hi]).max(axis=1) / scale
        rec[what + "_new_vs_old_median"], rec[what + "_yard_median"] = float(np.median(d)), float(np.median(e_yard))
        # (the maximum over the teacher-forced scale, the one its yardstick is relative to)
        rec[what + "_new_vs_old_max"] = float(d.max() * scale / err[what]["scale"]) if err[what]["scale"] > 0.0 else float("inf")
        rec[what + "_tf_yard_max"] = err[what]["yard"]
        print("LOCALIZE new-vs-old %s n%d %s %s: median %.3e (yardstick %.3e), max %.3e (teacher-forced yardstick %.3e)"
              % (name, n, b.name, what, np.median(d), np.median(e_yard), rec[what + "_new_vs_old_max"], err[what]["yard"]))
    PC.note("grad_rays_vs_bwd_rays_%s_n%d_%s_p%d_%s" % (name, n, mode, precision, b.name), decided_share=float(decided.mean()), **rec)
    for _, _, what in blocks(pr["view"]):
        assert rec[what + "_new_vs_old_median"] <= 3.0 * rec[what + "_yard_median"] + 2e-6, (what, rec)
        assert TL.within(rec[what + "_new_vs_old_max"], rec[what + "_tf_yard_max"], TL.bound("unit.ray_grad.new_vs_old")), (what, rec)
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
                kept, total = r.kept("fine")
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
    cot, rr = L.RenderCotangents(b.ptr(gc), None, None, b.ptr(gf), None, None), L.RenderRand(*r.call.rand)

    def call(parts=BOTH, params=(b.ptr(dfc), b.ptr(dff)), tmp_p=b.ptr(tmp), tmp_b=tb, out=b.ptr(g_rays), plans_=(pc, pf), packs=(kc, kf), rays_n=n):
        head = (plans_[0], plans_[1], C.byref(r.cfg), r.call.rays, rays_n, b.ptr(packs[0]), b.ptr(packs[1]), C.byref(rr), 0, 0)
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
