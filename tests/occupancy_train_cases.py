"""Cases of the occupancy grid in training (include/nerfhip.h "occupancy grid in training"; fused.hip nerfhip_render_fwd_occ_train,
csrc/occ/occ_train.hip), shared by the emulator suite (tests/test_occupancy_train.py) and the GPU suite
(tests/test_gpu_occupancy_train.py).  Every case drives the C ABI through a backend's library handle (tests/backends.py) and compares
with the library's own dense entry points or with numpy -- exactly, wherever the header promises bits."""
import ctypes as C

import numpy as np

import backends as BK
import nerf_pytorch_amd._lib as L
import occupancy_cases as OC
import parity_cases as P
import tolerances as TL

f32 = np.float32
MAPS = OC.MAPS
PRECISIONS = {"fp32": 0, "f16x3_train": P.F16X3_TRAIN}
ONES = 0xFFFFFFFF


def setup(b, net, arith, seed):
    cfg = OC.NETS[net]
    plan, params, _, packed = P.mlp_setup(b, cfg, seed=seed, precision=PRECISIONS[arith])
    return cfg, plan, params, packed


def has_mode(b, plan, mode):
    """Whether nerfhip_plan_set_bwd_compaction(plan, mode) is accepted (the fused modes: plans with a resident image only)."""
    cur = b.lib.plan_bwd_compaction(plan)
    ok = b.lib._dll.nerfhip_plan_set_bwd_compaction(plan, mode) == 0
    b.lib.plan_set_bwd_compaction(plan, cur)
    return ok


class Step(BK.RenderSession):
    """One training step's buffers on a backend, layout 1 (one set of backward buffers per net): the forward entry points write into
    ONE workspace and ONE set of maps, whose regions can be read and overwritten between the calls (backends.RenderSession)."""
    fwd = BK.RenderSession.forward

    def fwd_occ(self, grid_c, grid_f=OC.SAME, parts=3, training=None, tmp_words=None, check=True):
        """nerfhip_render_fwd_occ_train; returns the code (check=False: a refusal is the caller's to look at, from a raw call)."""
        if check:
            return self.forward_occ(grid_c, grid_f, parts, tmp_words)
        return self.refused_forward_occ("render_fwd_occ_train", grid_c, grid_f, parts, training, tmp_words)

    def bwd(self, g_c, g_f, gw=None):
        """nerfhip_render_bwd_parts (gw, the two device weight cotangents: _parts_w) of both nets on the step's workspace: the two flat
        gradients and each net's {kept, total}."""
        r = self.backward((g_c, g_f), gw, entry="parts" if gw is None else "parts_w")
        out = dict(g_coarse=r["g_params_coarse"], g_fine=r["g_params_fine"])
        for name, plan in (("coarse", self.pc), ("fine", self.pf)):
            if plan is not None and self.b.lib.plan_bwd_compaction(plan) in (1, 2, 4):
                out["kept_" + name] = self.kept(name)
        return out


def same(a, b_, what):
    assert np.array_equal(a, b_, equal_nan=True), (what, float(np.nanmax(np.abs(np.asarray(a, np.float64) - b_))))


def nets_and_modes(b, net, arith):
    """The two plans of a case and the culled-step modes they have: 2 always, 4 where the plan carries a resident image."""
    cfg, pc, _, packed_c = setup(b, net, arith, seed=3)
    _, pf, _, packed_f = setup(b, net, arith, seed=4)
    modes = ["recompute"] + (["fused_compact"] if has_mode(b, pc, 4) else [])
    return cfg, pc, pf, packed_c, packed_f, modes


# ---- 1. an all-ones grid is the recomputing step, bit for bit ---------------------------------------------------------------
def case_all_ones(b, net, arith, n=19, nc=8, nf=5):
    """Arm A: nerfhip_render_fwd_parts(training = 1) + nerfhip_render_bwd_parts with both plans in mode 2 (and in mode 4 where the plan
    has it: w64 / w40of64 in fp32 carry a resident image); arm B: nerfhip_render_fwd_occ_train through an all-ones grid with
    outside = 1 + the same backward.  The eight maps, both raw regions, z_fine, both flat gradients and the backward's statistics are
    the same bits; the grid's counts are {M, M}."""
    cfg, pc, pf, packed_c, packed_f, modes = nets_and_modes(b, net, arith)
    rays, rand = OC.render_inputs(cfg, n, nc, nf, seed=21)
    rnp = {k: v.numpy() for k, v in rand.items()}
    tgt = np.random.default_rng(5).random((n, 3)).astype(f32)
    grid = OC.Grid(b, np.full(4 * 4 * 4 // 32, ONES, np.uint32), *OC.SCENE_BOX, (4, 4, 4), 1)
    opt = dict(num_coarse=nc, num_fine=nf, perturb=True, white_background=True, noise_std=0.4)
    for mode in modes:
        for p in (pc, pf):
            b.set_compaction(p, mode)
        arms = []
        for culled in (False, True):
            s = Step(b, pc, pf, packed_c, packed_f, rays.numpy(), opt, rnp)
            if culled:
                s.fwd_occ(grid)
                assert s.counts() == (n * nc, n * nc, n * (nc + nf), n * (nc + nf)), s.counts()
            else:
                s.fwd()
            m = s.maps()
            m.update({k: s.region(k) for k in ("raw_coarse", "raw_fine", "z_fine")})
            m.update(s.bwd(m["rgb_coarse"] - tgt, m["rgb_fine"] - tgt))
            arms.append(m)
        for k in arms[0]:
            same(np.asarray(arms[1][k]), np.asarray(arms[0][k]), "all-ones %s %s %s %s" % (net, arith, mode, k))
        assert arms[0]["g_coarse"].any() and arms[0]["g_fine"].any()
    for p in (pc, pf):
        b.lib.plan_destroy(p)


# ---- 2. a half-empty grid is the substituted dense arm -----------------------------------------------------------------------
def half_empty_inputs(cfg, n, nc, nf, seed=22):
    """Rays, draws and target of the half-empty cases: OC.render_inputs with three rays of their own -- ray 0 wholly outside the scene
    box (culled or kept as `outside` says), rays 1 and 2 inside it, more than four cells apart at every depth: the grid
    generator below sets every cell ray 1 can cross and clears every cell ray 2 can cross."""
    rays, rand = OC.render_inputs(cfg, n, nc, nf, seed=seed)
    rays = rays.numpy().copy()
    rays[0, 0] += 40.0   # (x = 40: outside [-1.5, 1.5] at every depth)
    for i, o, d in ((1, (0.6, 0.5, 4.0), (0.1, 0.1, -1.0)), (2, (-0.6, -0.5, 4.0), (-0.1, -0.1, -1.0))):
        rays[i, 0:3], rays[i, 3:6] = o, d
        if cfg["use_viewdirs"]:
            rays[i, 8:11] = np.asarray(d, f32) / f32(np.linalg.norm(d))
    tgt = np.random.default_rng(seed + 1).random((n, 3)).astype(f32)
    return rays, {k: v.numpy() for k, v in rand.items()}, tgt


def half_empty_bits(rays, seed, res=(8, 8, 16)):
    """Random bits over OC.SCENE_BOX; every cell ray 2 can cross at depths 2 .. 6 (and its neighbours along every axis: a sample an
    ulp across a face stays in a cleared cell) cleared, then every such cell of ray 1 set."""
    g = np.random.default_rng(seed)
    bits = g.integers(0, 1 << 32, size=res[0] * res[1] * res[2] // 32, dtype=np.uint64).astype(np.uint32)
    cells = OC.unpack_bits(bits, res).copy()
    lo, hi = np.asarray(OC.SCENE_BOX[0], np.float64), np.asarray(OC.SCENE_BOX[1], np.float64)
    z = np.linspace(2.0, 6.0, 4001)
    for ray, value in ((2, False), (1, True)):
        p = rays[ray, None, 0:3].astype(np.float64) + rays[ray, None, 3:6].astype(np.float64) * z[:, None]
        i = np.floor((p - lo) / (hi - lo) * np.asarray(res)).astype(np.int64)
        assert np.all((i >= 0) & (i < np.asarray(res)))   # (the ray stays inside the box)
        for d in (-1, 0, 1):
            for ax in range(3):
                j = i.copy()
                j[:, ax] = np.clip(j[:, ax] + d, 0, res[ax] - 1)
                cells[j[:, 2], j[:, 1], j[:, 0]] = value
    return OC.pack_bits(cells)


def case_half_empty(b, net, arith, outside, n=21, nc=9, nf=6, noise_std=0.3):
    """Arm A, by hand, both plans in mode 1: the coarse training forward, the library's own flags (nerfhip_occ_mark on the workspace's
    z_coarse), the culled samples' rows of raw_coarse overwritten with the empty row, nerfhip_volume_render_fwd again into the maps and
    weights_coarse, then the same for the fine pass (parts = FINE), cotangents rgb - target, nerfhip_render_bwd_parts.  Arm B:
    nerfhip_render_fwd_occ_train + the same backward, in mode 2 and (where the plan has it) mode 4.  Maps, z_fine and both raw regions
    bit-identical; each net's backward kept count equals arm A's and is <= the grid's kept count; gradients array_equal in mode 2
    (the suite holds mode 2 to mode 1 bit for bit: parity_cases.case_render_compacted), within unit.compact_vs_dense of max|g| per
    tensor in mode 4 (the fused kernel k_bwd64r sums in another order).  White background, caller-given draws, sigma noise on."""
    cfg, pc, pf, packed_c, packed_f, modes = nets_and_modes(b, net, arith)
    rays, rnp, tgt = half_empty_inputs(cfg, n, nc, nf)
    grid = OC.Grid(b, half_empty_bits(rays, 23), *OC.SCENE_BOX, (8, 8, 16), outside)
    opt = dict(num_coarse=nc, num_fine=nf, perturb=True, white_background=True, noise_std=noise_std)
    rd = np.ascontiguousarray(rays[:, 3:6])
    # arm A
    for p in (pc, pf):
        b.set_compaction(p, True)
    a = Step(b, pc, pf, packed_c, packed_f, rays, opt, rnp)
    flags = {}
    for fine, part in ((False, L.PART_COARSE), (True, L.PART_FINE)):
        a.fwd(part)
        tag = "fine" if fine else "coarse"
        z, raw = a.region("z_" + tag), a.region("raw_" + tag)
        fl = OC.occ_mark(b, grid, rays, z).astype(bool)
        raw[~fl] = OC.EMPTY
        a.set_region("raw_" + tag, raw)
        out = b.volume_render_fwd(raw, z, rd, noise_std, rnp["noise_fine" if fine else "noise_coarse"], True)
        for k, v in zip(("rgb", "disp", "acc", None, "depth"), out):
            if k:
                a.set_map(k + "_" + tag, v)
        if not fine:
            a.set_region("weights_coarse", out[3])
        flags[tag] = fl
    want = a.maps()
    want.update({k: a.region(k) for k in ("raw_coarse", "raw_fine", "z_fine")})
    want.update(a.bwd(want["rgb_coarse"] - tgt, want["rgb_fine"] - tgt))
    # the generator's own promises
    for tag, fl in flags.items():
        culled = 1.0 - fl.mean()
        assert 0.2 < culled < 0.8, (tag, culled)
        assert fl[1].all() and not fl[2].any() and fl[0].all() == bool(outside) and fl[0].any() == bool(outside), (tag, outside)
    ctol = TL.bound("unit.compact_vs_dense", arith if arith == "fp32" else "f16x3_train")
    for mode in modes:
        for p in (pc, pf):
            b.set_compaction(p, mode)
        s = Step(b, pc, pf, packed_c, packed_f, rays, opt, rnp)
        s.fwd_occ(grid)
        got = s.maps()
        got.update({k: s.region(k) for k in ("raw_coarse", "raw_fine", "z_fine")})
        got.update(s.bwd(got["rgb_coarse"] - tgt, got["rgb_fine"] - tgt))
        kc, tc, kf, tf = s.counts()
        assert (kc, tc, kf, tf) == (int(flags["coarse"].sum()), n * nc, int(flags["fine"].sum()), n * (nc + nf))
        for k in MAPS + ("raw_coarse", "raw_fine", "z_fine"):
            same(got[k], want[k], "half-empty %s %s" % (mode, k))
        for tag, kept_occ in (("coarse", kc), ("fine", kf)):
            assert got["kept_" + tag] == want["kept_" + tag], (mode, tag, got["kept_" + tag], want["kept_" + tag])
            assert 0 < got["kept_" + tag][0] <= kept_occ
            g, w = got["g_" + tag], want["g_" + tag]
            assert w.any() and np.isfinite(g).all()
            if mode == "recompute":
                assert np.array_equal(g, w), (tag, float(np.abs(g - w).max()))
            else:
                plan = pc if tag == "coarse" else pf
                gd, gk = b.unflatten(plan, w), b.unflatten(plan, g)
                for k in gd:
                    d = float(np.abs(gk[k] - gd[k]).max()) / (float(np.abs(gd[k]).max()) + 1e-30)
                    print("half-empty %s %s %s %s: %.3e of max|g| (bound %.1e)" % (net, mode, tag, k, d, ctol))
                    assert d <= ctol, (mode, tag, k, d, ctol)
    for p in (pc, pf):
        b.lib.plan_destroy(p)


# ---- 3. an all-zero grid ------------------------------------------------------------------------------------------------------
def case_all_zero(b, net, arith, n=7, nc=8, nf=5):
    """Nothing is kept: rgb is the background, both gradients are exactly zero in every entry, the grid's kept and the backward's
    kept are 0, and nothing is non-finite except the reference's own NaN disparity of a ray without weight."""
    cfg, pc, pf, packed_c, packed_f, modes = nets_and_modes(b, net, arith)
    rays, rand = OC.render_inputs(cfg, n, nc, nf, seed=24)
    rnp = {k: v.numpy() for k, v in rand.items()}
    tgt = np.random.default_rng(6).random((n, 3)).astype(f32)
    grid = OC.Grid(b, np.zeros(2, np.uint32), *OC.SCENE_BOX, (4, 4, 4), 0)
    for mode in modes:
        for p in (pc, pf):
            b.set_compaction(p, mode)
        for white in (False, True):
            opt = dict(num_coarse=nc, num_fine=nf, perturb=True, white_background=white, noise_std=0.5)
            s = Step(b, pc, pf, packed_c, packed_f, rays.numpy(), opt, rnp)
            s.fwd_occ(grid)
            assert s.counts() == (0, n * nc, 0, n * (nc + nf))
            m = s.maps()
            for k in ("rgb_coarse", "rgb_fine"):
                assert np.array_equal(m[k], np.full((n, 3), 1.0 if white else 0.0, f32)), k
            for k in ("acc_coarse", "acc_fine", "depth_coarse", "depth_fine"):
                assert np.array_equal(m[k], np.zeros(n, f32)), k
            assert np.isnan(m["disp_coarse"]).all() and np.isnan(m["disp_fine"]).all()
            assert np.isfinite(s.region("weights_coarse")).all() and np.isfinite(s.region("z_fine")).all()
            r = s.bwd(m["rgb_coarse"] - tgt, m["rgb_fine"] - tgt)
            for tag, total in (("coarse", n * nc), ("fine", n * (nc + nf))):
                assert r["kept_" + tag] == (0, total), (mode, tag, r["kept_" + tag])
                assert r["g_" + tag].shape[0] > 0 and not r["g_" + tag].any() and np.isfinite(r["g_" + tag]).all(), (mode, tag)
    for p in (pc, pf):
        b.lib.plan_destroy(p)


# ---- 4. the density kernels against numpy, exact ------------------------------------------------------------------------------
BOX = ((-1.0, -0.5, 0.25), (1.5, 1.0, 2.0))


def density_update(b, plan, packed, grid, dens, decay, k, seed, first, count, check=True, tb=None):
    need = b.lib.occ_update_tmp_bytes(count)
    tmp = b.empty((max(need, 256) // 4,))
    fn = b.lib.occ_density_update if check else b.lib._dll.nerfhip_occ_density_update
    rc = fn(plan, b.p(packed), C.byref(grid.c) if grid is not None else None, b.p(dens), C.c_float(decay), k, seed, first, count,
            b.ptr(tmp), need if tb is None else tb, b.stream())
    return rc, b.host(tmp)


def initial_density(ncells, seed):
    g = np.random.default_rng(seed)
    d = (g.random(ncells) ** 4 * 3.0).astype(f32)
    d[0], d[1], d[2] = 0.0, 1e-40, 1e30   # (zero, an fp32 denormal, a huge value)
    d[ncells - 1] = 1e-42
    return d


def case_density_update(b, net, arith, res, ranges, seed=77, nan_weights=False):
    """dens against np.maximum(f32(dens * decay), relu(raw[3])) bit for bit, raw from the call's own kept tmp; cells outside the range
    untouched; probe rows equal nerfhip_occ_update's for the same pass and seed.  nan_weights: every weight NaN -> every raw[3] NaN ->
    dens * decay stays."""
    cfg = OC.NETS[net]
    plan, params, _, packed = P.mlp_setup(b, cfg, seed=9, precision=PRECISIONS[arith])
    if nan_weights:
        packed = b.dev(np.full(np.asarray(b.host(packed)).shape, np.nan, f32))
    ncells = res[0] * res[1] * res[2]
    grid = OC.Grid(b, np.zeros(ncells // 32, np.uint32), *BOX, res, 0)
    grid.c.bits = None   # (the density update neither reads nor writes the bits)
    for decay in (0.0, 0.95, 1.0):
        host = initial_density(ncells, seed)
        dens = b.dev(host)
        for k, (first, count) in enumerate(ranges):
            pas = 1 + k
            _, tmp = density_update(b, plan, packed, grid, dens, decay, pas, seed, first, count)
            r_off, z_off, raw_off = OC.update_layout(count)
            raw3 = np.asarray(tmp[raw_off:raw_off + 4 * count]).reshape(count, 4)[:, 3]
            assert np.isnan(raw3).all() if nan_weights else np.isfinite(raw3).all()
            want = host.copy()
            with np.errstate(invalid="ignore"):
                s = np.where(raw3 > 0, raw3, f32(0.0)).astype(f32)
            want[first:first + count] = np.maximum((host[first:first + count] * f32(decay)).astype(f32), s)
            got = np.array(b.host(dens), copy=True)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (res, decay, first, count, np.flatnonzero(got != want)[:4])
            host = want
            # the probes are nerfhip_occ_update's
            ref_grid = OC.Grid(b, np.zeros(ncells // 32, np.uint32), *BOX, res, 0)
            ref = OC.occ_update(b, plan, packed, ref_grid, 0.5, pas, seed, first, count)
            assert np.array_equal(np.asarray(ref[:11 * count]), np.asarray(tmp[:11 * count]))
            assert np.array_equal(np.asarray(ref[raw_off:raw_off + 4 * count]), np.asarray(tmp[raw_off:raw_off + 4 * count]), equal_nan=True)
            if not nan_weights and decay == 0.0:
                assert (s > 0).any() and (s == 0).any()   # (both branches of the relu)
    b.lib.plan_destroy(plan)


def np_threshold(dens, tau):
    return min(f32(tau), f32(np.asarray(dens, np.float64).sum() / dens.size))


def bits_case(res, seed, tau_below_mean):
    """dens and tau of a density_bits case; asserts (on the CPU) that no cell lies within 2 ulp of the threshold."""
    ncells = res[0] * res[1] * res[2]
    dens = initial_density(ncells, seed)
    dens[2] = 7.0   # (no 1e30: it would be the whole mean)
    mean = float(np.asarray(dens, np.float64).mean())
    tau = mean * (0.5 if tau_below_mean else 3.0)
    thr = np_threshold(dens, tau)
    assert (thr == f32(tau)) == tau_below_mean
    near = np.abs(dens.astype(np.float64) - float(thr)) <= 2 * np.spacing(thr)
    assert not near.any()
    assert 0 < (dens > thr).mean() < 1
    return dens, tau, thr


def density_bits(b, dens, res, tau, check=True, tmp_bytes=None, bits=None):
    r = (C.c_int * 3)(*res)
    need = b.lib.occ_density_bits_tmp_bytes(r)
    tmp = b.empty((max(need, 256) // 4,))
    out = b.dev(np.full(max(res[0] * res[1] * res[2] // 32, 1), 0x5A5A5A5A, np.int32)) if bits is None else bits
    fn = b.lib.occ_density_bits if check else b.lib._dll.nerfhip_occ_density_bits
    rc = fn(b.p(dens), r, C.c_float(tau), b.p(out), b.ptr(tmp), need if tmp_bytes is None else tmp_bytes, b.stream())
    return rc, np.array(b.host(out), copy=True), np.array(b.host(tmp), copy=True)


def case_density_bits(b, res):
    ncells = res[0] * res[1] * res[2]
    for below in (True, False):
        dens, tau, thr = bits_case(res, 31, below)
        _, words, tmp = density_bits(b, b.dev(dens), res, tau)
        got_thr = np.asarray(tmp[:1]).view(f32)[0]
        assert abs(float(got_thr) - float(thr)) <= float(np.spacing(thr)), (res, below, got_thr, thr)
        assert np.array_equal(OC.unpack_bits(words, res).reshape(-1), dens > thr), (res, below)
    _, words, tmp = density_bits(b, b.dev(np.zeros(ncells, f32)), res, 0.01)
    assert not np.asarray(words).any() and np.asarray(tmp[:1]).view(f32)[0] == 0.0


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def case_refusals(b):
    cfg, plan, _, packed = OC.setup(b, "w128", "fp32")
    rays, rand = OC.render_inputs(cfg, 4, 8, 4, seed=1)
    rays = rays.numpy()
    opt = dict(num_coarse=8, num_fine=4, perturb=False)
    ok = OC.Grid(b, np.full(2, ONES, np.uint32), *OC.SCENE_BOX, (4, 4, 4), 1)
    b.set_compaction(plan, "recompute")

    def refused(match, pc=plan, pf=plan, packed_=packed, **kw):
        kw.setdefault("grid_c", ok)
        s = Step(b, pc, pf, packed_, packed_, rays, opt)
        rc = s.fwd_occ(check=False, **kw)
        assert rc == -1 and match in b.lib.last_error().decode(), (rc, b.lib.last_error())
        assert all(np.isnan(v).all() for v in s.maps().values()) and (np.asarray(b.host(s.tmp)).view(np.int32) == -7).all()
        assert np.isnan(np.asarray(b.host(s.ws))).all()   # (nothing launched: the workspace is untouched too)

    # the entry point works at all with these inputs
    s = Step(b, plan, plan, packed, packed, rays, opt)
    assert s.fwd_occ(ok) == 0 and s.counts() == (32, 32, 48, 48)
    refused("training must be 1", training=0)
    refused("training must be 1", training=3)
    refused("grid_coarse is NULL", grid_c=None, grid_f=ok)
    refused("grid_fine is NULL", grid_f=None)
    refused("parts must be", parts=0)
    bad = lambda **kw: OC.Grid(b, np.full(2, ONES, np.uint32), kw.get("lo", OC.SCENE_BOX[0]), kw.get("hi", OC.SCENE_BOX[1]), (4, 4, 4), 1)
    g = bad()
    g.c.res = (C.c_int * 3)(513, 4, 4)
    refused("each axis must be", grid_c=g)
    g.c.res = (C.c_int * 3)(3, 3, 3)
    refused("multiple of 32", grid_c=g)
    refused("hi > lo", grid_c=bad(hi=(1.5, -1.5, 3.0)))
    refused("tmp too small", tmp_words=20)
    g = bad()
    g.c.bits = None
    refused("no bits", grid_c=g)
    # the modes whose training forward leaves a stash; the message names the modes that work
    for mode in (0, 1):
        b.lib.plan_set_bwd_compaction(plan, mode)
        refused("modes 2 (recompute), 3 (fused) and 4 (fused over the list)")
    b.set_compaction(plan, "recompute")
    _, p64, _, packed64 = OC.setup(b, "w64", "fp32")
    b.lib.plan_set_bwd_compaction(p64, 5)
    refused("modes 2 (recompute), 3 (fused) and 4 (fused over the list)", pc=p64, pf=p64, packed_=packed64)
    b.lib.plan_set_bwd_compaction(p64, 3)   # (mode 3 is accepted: correct, though it saves no backward work)
    s = Step(b, p64, p64, packed64, packed64, rays, opt)
    assert s.fwd_occ(ok) == 0
    b.lib.plan_destroy(p64)
    # an inference-only plan
    _, pinf, _, packed_inf = OC.setup(b, "w128", "f16x3")
    assert b.lib._dll.nerfhip_plan_set_bwd_compaction(pinf, 2) == 0
    refused("modes 2 (recompute), 3 (fused) and 4 (fused over the list)", pc=pinf, pf=pinf, packed_=packed_inf)
    b.lib.plan_destroy(pinf)
    # plans the listed kernels do not cover
    p2, _, _, packed2 = P.mlp_setup(b, P.MLP_GEOMETRIES["wide3x512_skip2"], seed=1)
    b.lib.plan_set_bwd_compaction(p2, 2)
    refused("render without an occupancy grid", pc=p2, pf=p2, packed_=packed2)
    b.lib.plan_destroy(p2)
    # M beyond the recomputing flow's limit (ceil(M / 128) * 128 * 1024 >= 2^32: the flow falls back to the dense row), and M >= 2^31, which that limit covers
    # (no buffer is touched before the refusal: the pointers only have to be non-NULL)
    one = b.dev(np.zeros(64, f32))
    ro = L.RenderOut(*[None] * 8)
    for big, match in ((L.RenderCfg(1 << 11, 0, 0, 0, 0, 0.0, 11), "modes 2 (recompute)"), (L.RenderCfg(1 << 15, 1 << 15, 0, 0, 0, 0.0, 11), "too many sample points")):
        rc = b.lib._dll.nerfhip_render_fwd_occ_train(plan, plan, C.byref(big), b.ptr(one), 1 << 15 if big.num_fine else 1 << 11, b.ptr(packed),
                                                     b.ptr(packed), b.ptr(one), b.ptr(one), None, 0, 0, C.byref(ro), b.ptr(one), 1 << 62, 1,
                                                     3, C.byref(ok.c), C.byref(ok.c), b.ptr(one), 1 << 62, b.stream())
        assert rc == -1 and match in b.lib.last_error().decode(), b.lib.last_error()
    # nerfhip_render_fwd_occ keeps refusing training != 0
    rc, maps, _ = OC.render_occ(b, plan, plan, packed, packed, rays, opt, ok, raise_on_error=False, training=1)
    assert rc == -1 and "inference render only" in b.lib.last_error().decode()
    # ---- the density entry points
    res = (4, 4, 4)
    grid = OC.Grid(b, np.zeros(2, np.uint32), *BOX, res, 0)
    poison = np.full(64, 3.25, f32)

    def upd_refused(match, dens="own", g=grid, decay=0.5, k=1, first=0, count=32, tb=None, plan_=plan, packed_=packed):
        d = b.dev(poison) if dens == "own" else dens
        rc, tmp = density_update(b, plan_, packed_, g, d, decay, k, 0, first, count, check=False, tb=tb)
        assert rc == -1 and match in b.lib.last_error().decode(), (rc, b.lib.last_error())
        assert np.isnan(np.asarray(tmp)).all() and (d is None or np.array_equal(b.host(d), poison))

    g = OC.Grid(b, np.zeros(2, np.uint32), *BOX, res, 0)
    g.c.res = (C.c_int * 3)(0, 4, 4)
    upd_refused("each axis must be", g=g)
    g.c.res = (C.c_int * 3)(3, 3, 3)
    upd_refused("multiple of 32", g=g)
    upd_refused("hi > lo", g=OC.Grid(b, np.zeros(2, np.uint32), BOX[0], (1.5, -0.5, 2.0), res, 0))
    upd_refused("grid is NULL", g=None)
    for first, count in ((16, 32), (0, 48), (32, 64), (-32, 32)):
        upd_refused("multiples of 32", first=first, count=count)
    upd_refused("pass must be", k=4096)
    upd_refused("pass must be", k=-1)
    for decay in (-0.01, 1.01, float("nan"), float("inf")):
        upd_refused("decay must lie in [0, 1]", decay=decay)
    upd_refused("dens is NULL", dens=None)
    upd_refused("plan / packed is NULL", plan_=None)
    upd_refused("plan / packed is NULL", packed_=None)
    upd_refused("tmp too small", tb=100)

    def bits_refused(match, dens="own", r=res, tau=0.01, tmp_bytes=None, null_bits=False):
        d = b.dev(poison) if dens == "own" else dens
        out = b.dev(np.full(2, 0x5A5A5A5A, np.int32))
        rr = (C.c_int * 3)(*r) if r is not None else None
        tmp = b.empty((256,))
        rc = b.lib._dll.nerfhip_occ_density_bits(b.p(d), rr, C.c_float(tau), None if null_bits else b.ptr(out), b.ptr(tmp),
                                                 1024 if tmp_bytes is None else tmp_bytes, b.stream())
        assert rc == -1 and match in b.lib.last_error().decode(), (rc, b.lib.last_error())
        assert (np.asarray(b.host(out)) == 0x5A5A5A5A).all() and np.isnan(np.asarray(b.host(tmp))).all()

    bits_refused("each axis must be", r=(4, 4, 513))
    bits_refused("multiple of 32", r=(3, 3, 3))
    bits_refused("res is NULL", r=None)
    bits_refused("tau is NaN", tau=float("nan"))
    bits_refused("is NULL", dens=None)
    bits_refused("is NULL", null_bits=True)
    bits_refused("tmp too small", tmp_bytes=256)
    assert b.lib.occ_density_bits_tmp_bytes(None) == -1 and b.lib.occ_density_bits_tmp_bytes((C.c_int * 3)(4, 4, 4)) == 512
    b.lib.plan_destroy(plan)


# ---- 7. capability (GPU; the engine and the Python surface) -----------------------------------------------------------------------
CAP_ANGLES = (0.0, 20.0, 40.0, 60.0, 80.0, 100.0)   # degrees about the scene's up axis (world z) from the fixture pose
CAP_HELD_OUT = 3


def teacher_views(s):
    """The six teacher views of the capability test, rendered once per session from the fixture nets (dense render, 64 x 64, 64 + 64
    samples, white background): packed rays (6, 4096, 11) and rgb_fine (6, 4096, 3)."""
    import torch
    if "teacher" in s:
        return s["teacher"]
    N = s["N"]
    rays, rgb = [], []
    for deg in CAP_ANGLES:
        a = np.deg2rad(deg)
        rot = torch.tensor([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32,
                           device=s["dev"])
        pose = s["pose"].clone()
        pose[:3, :4] = rot[:3, :3] @ pose[:3, :4]
        pix = torch.arange(s["H"] * s["W"], dtype=torch.int64, device=s["dev"])
        ro, rd = N.get_rays_at_pixels(s["H"], s["W"], s["focal"], pose[:3, :4].contiguous(), pix)
        rays.append(N.pack_rays(ro, rd, s["opts"], s["H"], s["W"], s["focal"]))
        with torch.no_grad():
            out, _ = N.render_pose_rows(s["H"], s["W"], s["focal"], pose, s["mc"], s["mf"], s["opts"],
                                        N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True))
        rgb.append(out[3].reshape(-1, 3).contiguous())
    s["teacher"] = (torch.stack(rays), torch.stack(rgb))
    return s["teacher"]


def capability(s, seed, with_grid, steps=400, n_rays=1024, warmup=100, every=16, lr=5e-3, noise_std=1.0):
    """One arm of the capability test: two 4 x 64 students from `seed`, `steps` steps of `n_rays` rays drawn (from the same seed) from
    the five training views; the held-out view's PSNR of the student's dense render against the teacher."""
    import torch
    N = s["N"]
    rays, rgb = teacher_views(s)
    train = [i for i in range(len(CAP_ANGLES)) if i != CAP_HELD_OUT]
    pool_r, pool_t = rays[train].reshape(-1, rays.shape[-1]), rgb[train].reshape(-1, 3)
    torch.manual_seed(seed)
    cfg = dict(num_layers=4, hidden_size=64, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    mc, mf = N.FlexibleNeRFModel(**cfg).to(s["dev"]), N.FlexibleNeRFModel(**cfg).to(s["dev"])
    grid = N.OccupancyGrid.for_training(((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)), resolution=64, device=s["dev"]) if with_grid else None
    eng = N.TrainEngine(mc, mf, 64, 64, perturb=True, white_background=True, noise_std=noise_std, lr=lr, seed=seed, occupancy=grid,
                        occupancy_warmup=warmup, occupancy_every=every)
    picks = torch.randint(0, pool_r.shape[0], (steps, n_rays), generator=torch.Generator().manual_seed(seed)).to(s["dev"])
    losses = torch.zeros(steps, device=s["dev"])
    for i in range(steps):
        idx = picks[i]
        losses[i] = eng.step(pool_r[idx].contiguous(), pool_t[idx].contiguous())[2]
    rec = dict(finite=bool(torch.isfinite(losses).all().item()), final_loss=float(losses[-20:].mean().item()))
    with torch.no_grad():
        out = N.predict_and_render_radiance(rays[CAP_HELD_OUT], mc, mf, s["opts"], mode="validation",
                                            encode_position_fn=N.get_embedding_function(10, True, True),
                                            encode_direction_fn=N.get_embedding_function(4, True, True))
    mse = float(((out[3] - rgb[CAP_HELD_OUT]).double() ** 2).mean().item())
    rec["psnr"] = float(-10.0 * np.log10(max(mse, 1e-30)))
    if with_grid:
        kc, tc, kf, tf = eng.occupancy_counts.tolist()
        rec.update(kept_coarse=kc / tc, kept_fine=kf / tf, occupied_fraction=grid.occupied_fraction(), updates=grid.update_count,
                   modes=[mc.backward_compaction, mf.backward_compaction])
    return rec
