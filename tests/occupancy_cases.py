"""Cases of the occupancy grid (include/nerfhip.h "occupancy grid"; csrc/occ/occupancy.hip, the LIST forward kernels, fused.hip
nerfhip_render_fwd_occ), shared by the emulator suite (tests/test_occupancy.py) and the GPU suite (tests/test_gpu_occupancy.py).
Every case drives the C ABI through a backend's library handle (tests/backends.py) and compares with a numpy restatement or with
the library's own dense entry points -- exactly, wherever the header promises bits."""
import ctypes as C

import numpy as np
import torch

import backends as BK
import nerf_oracle as O
import nerf_pytorch_amd._lib as L
import parity_cases as P
import tolerances as TL
from backends import model_cfg

f32 = np.float32
EMPTY = np.array([0.0, 0.0, 0.0, L.OCC_EMPTY_RAW], f32)
PRECISIONS = {"fp32": 0, "f16x3": P.F16X3}
# 2-layer nets at the three kernel widths + one padded width (40 of 64); the 64-wide fp32 plans carry a resident image (k_fwd64r
# renders them densely: the listed forward must reproduce ITS bits with the general kernel)
NETS = {"w64": model_cfg(2, 64, 4, 6, 2), "w128": model_cfg(2, 128, 4, 10, 4), "w256": model_cfg(2, 256, 4, 4, 2),
        "w40of64": model_cfg(2, 40, 4, 5, 3), "novw128": model_cfg(2, 128, 4, 6, 0, use_viewdirs=False)}


# ---- numpy restatement of the header -----------------------------------------------------------------------------------
def np_points(rays, z):
    """ro + rd * z in fp32: one multiply, one add (what the kernels compute with -ffp-contract=off)."""
    rays, z = np.asarray(rays, f32), np.asarray(z, f32)
    return rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]


def np_mark(rays, z, bits, lo, hi, res, outside, want_near=False):
    """flags [n, S] of the header's cell rule; want_near: also the samples within 4 ulp (of the coordinate's magnitude, scaled by
    inv) of a cell face or box face, which an fma-contracted ro + rd * z may put on the other side."""
    lo, hi, res = np.asarray(lo, f32), np.asarray(hi, f32), np.asarray(res, np.int64)
    inv = (res.astype(f32) / (hi - lo)).astype(f32)
    p = np_points(rays, z)
    with np.errstate(invalid="ignore", over="ignore"):
        f = ((p - lo) * inv).astype(f32)
        t = np.floor(f)
        inside = np.all((t >= 0) & (t < res.astype(f32)), axis=-1)
    nan = np.isnan(p).any(axis=-1)
    i = np.where(inside[..., None], np.nan_to_num(t), 0).astype(np.int64)
    b = (i[..., 2] * res[1] + i[..., 1]) * res[0] + i[..., 0]
    occ = (np.asarray(bits, np.uint32)[b >> 5] >> (b & 31).astype(np.uint32)) & 1
    flags = np.where(nan, 1, np.where(inside, occ, int(bool(outside)))).astype(np.uint8)
    if not want_near:
        return flags
    rays = np.asarray(rays, f32)
    mag = np.abs(rays[:, None, 0:3]) + np.abs(rays[:, None, 3:6] * np.asarray(z, f32)[:, :, None]) + np.abs(lo)
    with np.errstate(invalid="ignore"):
        tol = 4.0 * 2.0 ** -23 * mag.astype(np.float64) * inv
        near = (np.abs(f.astype(np.float64) - np.rint(f.astype(np.float64))) <= tol).any(axis=-1)
    return flags, near & ~nan


def np_dilate(cells):
    """cells [rz, ry, rx] bool: set if the cell or one of its six face neighbours is set; no wrap."""
    out = cells.copy()
    out[1:] |= cells[:-1]
    out[:-1] |= cells[1:]
    out[:, 1:] |= cells[:, :-1]
    out[:, :-1] |= cells[:, 1:]
    out[:, :, 1:] |= cells[:, :, :-1]
    out[:, :, :-1] |= cells[:, :, 1:]
    return out


def pack_bits(cells):
    """bool cells in bit-index order -> uint32 words."""
    flat = np.asarray(cells, bool).reshape(-1)
    assert flat.size % 32 == 0
    return (flat.reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def unpack_bits(words, res):
    w = np.asarray(words).view(np.uint32)
    return (((w[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)).reshape(res[2], res[1], res[0])


# ---- plumbing ----------------------------------------------------------------------------------------------------------
class Grid:
    """A grid on a backend's device: keeps the device bits alive next to the host struct."""

    def __init__(self, b, bits, lo, hi, res, outside):
        self.bits = np.ascontiguousarray(bits, np.uint32)
        self.lo, self.hi, self.res, self.outside = tuple(lo), tuple(hi), tuple(int(r) for r in res), int(outside)
        self.dev = b.dev(self.bits.view(np.int32))
        self.c = L.OccGrid(b.ptr(self.dev), (C.c_float * 3)(*self.lo), (C.c_float * 3)(*self.hi), (C.c_int * 3)(*self.res), self.outside)


def random_rays(n, lo, hi, seed, view=True):
    """Packed ray rows whose samples (z in [near, far] = [0.1, 2]) land inside the box and beyond every one of its faces."""
    g = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    ext = hi - lo
    rays = np.zeros((n, 11 if view else 8), f32)
    rays[:, 0:3] = g.uniform(lo - 0.4 * ext, hi + 0.4 * ext, (n, 3))
    rays[:, 3:6] = g.normal(0.0, 0.35, (n, 3)) * ext
    rays[:, 6], rays[:, 7] = 0.1, 2.0
    if view:
        v = g.normal(size=(n, 3))
        rays[:, 8:11] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return rays


def occ_mark(b, grid, rays, z):
    n, S = z.shape
    dr, dz = b.dev(np.ascontiguousarray(rays, f32)), b.dev(np.ascontiguousarray(z, f32))
    flags = b.empty((n * S,), np.uint8)
    b.lib.occ_mark(b.ptr(dr), rays.shape[1], n, b.ptr(dz), S, C.byref(grid.c), b.ptr(flags), b.stream())
    return b.host(flags).reshape(n, S)


SAME = BK.SAME


def render_occ(b, plan_c, plan_f, packed_c, packed_f, rays, opt, grid_c, grid_f=SAME, rand=None, parts=3, ws=None,
               raise_on_error=True, training=0, tmp_words=None):
    """nerfhip_render_fwd_occ as Backend.render drives nerfhip_render_fwd (backends.RenderSession in the inference layout).  Returns the
    eight maps, the four count words, the regions the passes left in the workspace and the last pass's list."""
    s = BK.RenderSession(b, plan_c, plan_f, packed_c, packed_f, rays, opt, rand, 0, ws=ws)
    n, nc, nf = s.n, s.nc, s.nf
    if not raise_on_error:  # (a refusal: the return code of a raw call, and what the call left in its outputs)
        rc = s.refused_forward_occ("render_fwd_occ", grid_c, grid_f, parts, training, tmp_words)
        return rc, s.maps(), b.host(s.tmp)
    s.forward_occ(grid_c, grid_f, parts, tmp_words)
    out = s.maps()
    t = np.ascontiguousarray(b.host(s.tmp)).view(np.int32)
    out["counts"] = s.counts()
    m_max = n * (nc + nf)
    c_words = 16 * (-(-(-(-m_max // 2048)) // 16))
    last_kept = out["counts"][2] if (nf > 0 and parts & 2) else out["counts"][0]
    out["list"] = t[16 + c_words:16 + c_words + last_kept].copy()
    out["list_padding"] = t[16 + c_words + last_kept:16 + c_words + ((last_kept + 127) & ~127)].copy()
    for name in ("z_coarse", "raw_coarse", "weights_coarse") + (("z_fine", "raw_fine") if nf > 0 else ()):
        out[name] = s.region(name)
    return out


def setup(b, net, arith, seed=3):
    cfg = NETS[net]
    plan, params, _, packed = P.mlp_setup(b, cfg, seed=seed, precision=PRECISIONS[arith])
    return cfg, plan, params, packed


# ---- 1. mark against numpy ----------------------------------------------------------------------------------------------
MARK_GRIDS = [((1, 1, 32), 0), ((4, 8, 16), 1), ((64, 64, 64), 0), ((512, 2, 2), 1), ((4, 8, 16), 0), ((64, 64, 64), 1)]


def mark_case(res, outside, seed, n=37, S=13):
    g = np.random.default_rng(seed)
    lo, hi = (-1.0, -0.5, 0.25), (1.5, 1.0, 2.0)
    bits = g.integers(0, 1 << 32, size=res[0] * res[1] * res[2] // 32, dtype=np.uint64).astype(np.uint32)
    rays = random_rays(n, lo, hi, seed + 1)
    z = np.sort(g.uniform(0.1, 2.0, (n, S)).astype(f32), axis=1)
    rays[3, 0] = np.nan  # (a NaN point counts as occupied)
    want, near = np_mark(rays, z, bits, lo, hi, res, outside, want_near=True)
    # the generator's own promises (checked on the CPU): every face has samples on both sides; the reference alone leaves out < 1 %
    p = np_points(rays, z)
    for a in range(3):
        assert (p[..., a] < lo[a]).any() and (p[..., a] > hi[a]).any() and ((p[..., a] > lo[a]) & (p[..., a] < hi[a])).any()
    assert near.mean() < 0.01, near.mean()
    assert want[3].all() and 0 < want[~near].mean() < 1
    return dict(lo=lo, hi=hi, res=res, outside=outside, bits=bits, rays=rays, z=z, want=want, near=near)


def case_mark(b, res, outside, seed=11):
    c = mark_case(res, outside, seed)
    grid = Grid(b, c["bits"], c["lo"], c["hi"], res, outside)
    got = occ_mark(b, grid, c["rays"], c["z"])
    assert set(np.unique(got)) <= {0, 1}
    bad = (got != c["want"]) & ~c["near"]
    assert not bad.any(), (res, outside, int(bad.sum()), np.argwhere(bad)[:4])


# ---- 2. listed forward, exact -------------------------------------------------------------------------------------------
def box_rays(n, kept_rays, view, seed):
    """Rays that stand still (direction 0): the first kept_rays origins inside the unit box, the others far outside it -- against an
    all-ones grid with outside = 0 exactly kept_rays * S samples are kept, whatever the depths."""
    g = np.random.default_rng(seed)
    rays = np.zeros((n, 11 if view else 8), f32)
    rays[:, 0:3] = g.uniform(0.1, 0.9, (n, 3))
    rays[kept_rays:, 0:3] += 5.0
    rays[:, 6], rays[:, 7] = 2.0, 6.0
    if view:
        v = g.normal(size=(n, 3))
        rays[:, 8:11] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return rays


def case_listed_forward(b, net, arith, shapes=None):
    """Coarse pass alone (the list it leaves is the one read back): every kept row equals the dense forward's, every culled row is the
    empty row, kept == the set flags, the list is ascending and padded with sample 0.  Shapes: the list ends at 0, at a workgroup
    boundary (128 kept slots: a boundary for the 4-wave and the 8-wave kernels alike), inside a workgroup with S no multiple of 16,
    and a random half-empty grid over more than one workgroup."""
    cfg, plan, _, packed = setup(b, net, arith)
    view = bool(cfg["use_viewdirs"])
    ones = np.full(1, 0xFFFFFFFF, np.uint32)
    for n, S, kept_rays in shapes or ((5, 8, 0), (20, 8, 16), (9, 13, 5), (1, 3, 1)):
        rays = box_rays(n, kept_rays, view, seed=n)
        grid = Grid(b, ones, (0, 0, 0), (1, 1, 1), (1, 1, 32), 0)
        _check_listed(b, plan, packed, rays, S, grid, expect_kept=kept_rays * S)
    rays = random_rays(23, (-1, -1, -1), (1, 1, 1), seed=5, view=view)
    g = np.random.default_rng(6)
    grid = Grid(b, g.integers(0, 1 << 32, size=4 * 8 * 16 // 32, dtype=np.uint64).astype(np.uint32), (-1, -1, -1), (1, 1, 1), (4, 8, 16), 0)
    _check_listed(b, plan, packed, rays, 13, grid)
    b.lib.plan_destroy(plan)


def _check_listed(b, plan, packed, rays, S, grid, expect_kept=None):
    opt = dict(num_coarse=S, num_fine=0, perturb=False)
    dense = b.render(plan, None, packed, None, rays, opt, want_regions=("raw_coarse", "z_coarse"))
    got = render_occ(b, plan, None, packed, None, rays, opt, grid, parts=1)
    assert np.array_equal(got["z_coarse"], dense["z_coarse"])
    flags = occ_mark(b, grid, rays, got["z_coarse"]).astype(bool)
    kept, total = got["counts"][:2]
    assert total == flags.size and kept == int(flags.sum()), (kept, total, int(flags.sum()))
    assert expect_kept is None or kept == expect_kept, (kept, expect_kept)
    assert got["counts"][2:] == (-7, -7)  # (the fine pass did not run: its pair is untouched)
    assert np.array_equal(got["list"], np.flatnonzero(flags.reshape(-1))) and not got["list_padding"].any()
    raw, want = got["raw_coarse"], dense["raw_coarse"]
    assert np.array_equal(raw[flags], want[flags]), float(np.abs(raw[flags] - want[flags]).max())
    assert np.array_equal(raw[~flags], np.broadcast_to(EMPTY, raw[~flags].shape))
    # ... and the compositing behind it is the ordinary one on those rows
    rgb = b.volume_render_fwd(raw, got["z_coarse"], np.ascontiguousarray(rays[:, 3:6]))[0]
    assert np.array_equal(rgb, got["rgb_coarse"])


# ---- 3. render ----------------------------------------------------------------------------------------------------------
MAPS = ("rgb_coarse", "disp_coarse", "acc_coarse", "depth_coarse", "rgb_fine", "disp_fine", "acc_fine", "depth_fine")


def same(a, b_, what):
    assert np.array_equal(a, b_, equal_nan=True), (what, float(np.nanmax(np.abs(np.asarray(a, np.float64) - b_))))


def render_inputs(cfg, n, nc, nf, seed):
    gen = P.rng(seed)
    ro = torch.tensor([0.2, -0.1, 4.0]).expand(n, 3) + 0.05 * torch.randn(n, 3, generator=gen)
    rd = torch.randn(n, 3, generator=gen) * 0.3
    rd[:, 2] = -1.0
    rays = O.pack_rays(ro, rd, 2.0, 6.0, rd if cfg["use_viewdirs"] else None)
    rand = dict(t_rand=torch.rand(n, nc, generator=gen), noise_coarse=torch.randn(n, nc, generator=gen),
                u=torch.rand(n, nf, generator=gen), noise_fine=torch.randn(n, nc + nf, generator=gen))
    return rays, rand


SCENE_BOX = ((-1.5, -1.5, -3.0), (1.5, 1.5, 3.0))  # around the samples of render_inputs (origin z ~ 4, direction z = -1, depths 2 .. 6)


def case_render_all_ones(b, net, arith, n=19, nc=8, nf=5):
    """An all-ones grid with outside = 1 culls nothing: every map of nerfhip_render_fwd_occ equals nerfhip_render_fwd's bit for bit --
    both parts in one call and one after the other, white background on and off, with the sigma noise on."""
    cfg, pc, _, packed_c = setup(b, net, arith, seed=3)
    _, pf, _, packed_f = setup(b, net, arith, seed=4)
    rays, rand = render_inputs(cfg, n, nc, nf, seed=21)
    rnp = {k: v.numpy() for k, v in rand.items()}
    grid = Grid(b, np.full(4 * 4 * 4 // 32, 0xFFFFFFFF, np.uint32), *SCENE_BOX, (4, 4, 4), 1)
    for white in (False, True):
        opt = dict(num_coarse=nc, num_fine=nf, perturb=True, white_background=white, noise_std=0.4)
        dense = b.render(pc, pf, packed_c, packed_f, rays.numpy(), opt, rnp, want_regions=("raw_coarse", "raw_fine", "z_fine"))
        got = render_occ(b, pc, pf, packed_c, packed_f, rays.numpy(), opt, grid, rand=rnp)
        assert got["counts"] == (n * nc, n * nc, n * (nc + nf), n * (nc + nf))
        for k in MAPS + ("raw_coarse", "raw_fine", "z_fine"):
            same(got[k], dense[k], "all-ones %s white=%s" % (k, white))
        # the two parts one after the other, on one workspace
        ws = b.empty((BK.RenderCall.workspace_bytes(b.lib, pc, pf, L.RenderCfg(nc, nf, 1, 0, int(white), 0.4, rays.shape[1]), n, 0) // 4 + 1,))
        first = render_occ(b, pc, pf, packed_c, packed_f, rays.numpy(), opt, grid, rand=rnp, parts=1, ws=ws)
        second = render_occ(b, pc, pf, packed_c, packed_f, rays.numpy(), opt, grid, rand=rnp, parts=2, ws=ws)
        for k in MAPS[:4]:
            same(first[k], dense[k], "parts=1 " + k)
        for k in MAPS[4:]:
            same(second[k], dense[k], "parts=2 " + k)
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


def half_grid(b, seed, outside=0):
    g = np.random.default_rng(seed)
    return Grid(b, g.integers(0, 1 << 32, size=8 * 8 * 16 // 32, dtype=np.uint64).astype(np.uint32), *SCENE_BOX, (8, 8, 16), outside)


def oracle_masked(rays, rand, par_c, par_f, cfg, opt, flags_c, flags_f):
    """The oracle's render with the rows of the masked samples replaced by the empty row (the masks are GIVEN: the library's own)."""
    ro, rd = rays[..., :3], rays[..., 3:6]
    z = O.stratified_z(rays[..., 6:7], rays[..., 7:8], opt["num_coarse"], False, True, rand["t_rand"])
    empty = torch.from_numpy(EMPTY)
    raw_c = O.run_network(par_c, ro[..., None, :] + rd[..., None, :] * z[..., :, None], rays, cfg)
    raw_c = torch.where(torch.from_numpy(flags_c)[..., None], raw_c, empty)
    rgb_c, _, acc_c, w_c, _ = O.volume_render(raw_c, z, rd, opt["noise_std"], rand["noise_coarse"], opt["white_background"])
    _, z_f = O.hierarchical_z(z, w_c, opt["num_fine"], det=False, u=rand["u"])
    raw_f = O.run_network(par_f, ro[..., None, :] + rd[..., None, :] * z_f[..., :, None], rays, cfg)
    raw_f = torch.where(torch.from_numpy(flags_f)[..., None], raw_f, empty)
    rgb_f, _, acc_f, _, _ = O.volume_render(raw_f, z_f, rd, opt["noise_std"], rand["noise_fine"], opt["white_background"])
    return dict(rgb_coarse=rgb_c.numpy(), acc_coarse=acc_c.numpy(), rgb_fine=rgb_f.numpy(), acc_fine=acc_f.numpy())


def case_render_half_empty(b, net, arith, n=21, nc=9, nf=6, white=True):
    """A random half-empty grid: the maps are what the library's own nerfhip_volume_render_fwd / nerfhip_hierarchical_z make of the
    masked raw rows the passes left in the workspace (bit for bit), the masked rows are the empty row, the kept coarse rows the dense
    render's -- and the colour maps are within the fused render's rgb bound (tests/tolerances.py e2e.rgb_fine: the 1e-4 that
    parity_cases.case_render_vs_oracle holds the unit render cases to) of the CPU oracle given the same masks."""
    cfg, pc, par_c, packed_c = setup(b, net, arith, seed=3)
    _, pf, par_f, packed_f = setup(b, net, arith, seed=4)
    rays, rand = render_inputs(cfg, n, nc, nf, seed=22)
    rnp = {k: v.numpy() for k, v in rand.items()}
    grid = half_grid(b, 23)
    opt = dict(num_coarse=nc, num_fine=nf, perturb=True, white_background=white, noise_std=0.3)
    got = render_occ(b, pc, pf, packed_c, packed_f, rays.numpy(), opt, grid, rand=rnp)
    dense = b.render(pc, pf, packed_c, packed_f, rays.numpy(), opt, rnp, want_regions=("raw_coarse",))
    rd = np.ascontiguousarray(rays.numpy()[:, 3:6])
    fc = occ_mark(b, grid, rays.numpy(), got["z_coarse"]).astype(bool)
    ff = occ_mark(b, grid, rays.numpy(), got["z_fine"]).astype(bool)
    assert got["counts"] == (int(fc.sum()), fc.size, int(ff.sum()), ff.size)
    assert 0.2 < fc.mean() < 0.8 and 0.2 < ff.mean() < 0.8
    assert np.array_equal(got["list"], np.flatnonzero(ff.reshape(-1)))
    assert np.array_equal(got["raw_coarse"][fc], dense["raw_coarse"][fc])
    for raw, flags in ((got["raw_coarse"], fc), (got["raw_fine"], ff)):
        assert np.array_equal(raw[~flags], np.broadcast_to(EMPTY, raw[~flags].shape))
        assert not (raw[flags][:, 3] == EMPTY[3]).any() and not np.isnan(raw).any()
    rc = b.volume_render_fwd(got["raw_coarse"], got["z_coarse"], rd, 0.3, rnp["noise_coarse"], white)
    for k, v in zip(("rgb_coarse", "disp_coarse", "acc_coarse", "weights_coarse", "depth_coarse"), rc):
        same(got[k], v, "half-empty " + k)
    _, z_f = b.hierarchical_z(got["z_coarse"], rc[3], nf, u=rnp["u"])
    same(got["z_fine"], z_f, "half-empty z_fine")
    rf = b.volume_render_fwd(got["raw_fine"], z_f, rd, 0.3, rnp["noise_fine"], white)
    for k, v in zip(("rgb_fine", "disp_fine", "acc_fine", None, "depth_fine"), rf):
        if k:
            same(got[k], v, "half-empty " + k)
    want = oracle_masked(rays, rand, par_c, par_f, cfg, opt, fc, ff)
    tol = TL.bound("e2e.rgb_fine")[0]
    P.close(got["rgb_coarse"], want["rgb_coarse"], tol, what="half-empty rgb_coarse vs oracle")
    P.close(got["rgb_fine"], want["rgb_fine"], tol, what="half-empty rgb_fine vs oracle")
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


def case_render_all_zero(b, net, arith, n=7, nc=8, nf=5):
    """An all-zero grid with outside = 0: nothing is kept, rgb is exactly the background, acc and depth are exactly 0, and none of
    them is NaN.  The disparity maps are the one exception, and it is asserted as such: the disparity of a ray without any weight is
    the reference's own 0 / 0 (nerf/volume_rendering_utils.py:46-48), as in the dense render of empty space -- the compositing kernel
    is the unchanged one -- so disp is NaN exactly where acc == 0, here on every ray."""
    cfg, pc, _, packed_c = setup(b, net, arith, seed=3)
    _, pf, _, packed_f = setup(b, net, arith, seed=4)
    rays, rand = render_inputs(cfg, n, nc, nf, seed=24)
    rnp = {k: v.numpy() for k, v in rand.items()}
    grid = Grid(b, np.zeros(2, np.uint32), *SCENE_BOX, (4, 4, 4), 0)
    for white in (False, True):
        opt = dict(num_coarse=nc, num_fine=nf, perturb=True, white_background=white, noise_std=0.5)
        got = render_occ(b, pc, pf, packed_c, packed_f, rays.numpy(), opt, grid, rand=rnp)
        assert got["counts"] == (0, n * nc, 0, n * (nc + nf)) and got["list"].size == 0
        for k in ("rgb_coarse", "rgb_fine"):
            assert np.array_equal(got[k], np.full((n, 3), 1.0 if white else 0.0, f32)), k
        for k in ("acc_coarse", "acc_fine", "depth_coarse", "depth_fine"):
            assert np.array_equal(got[k], np.zeros(n, f32)), k
        assert not np.isnan(got["weights_coarse"]).any() and not np.isnan(got["z_fine"]).any()
        for d, a in (("disp_coarse", "acc_coarse"), ("disp_fine", "acc_fine")):
            assert np.array_equal(np.isnan(got[d]), got[a] == 0) and np.isnan(got[d]).all(), d
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


# ---- 4. update and dilate -----------------------------------------------------------------------------------------------
def update_layout(cells):
    """(rows, depths, raw) float offsets inside nerfhip_occ_update's tmp."""
    a = lambda v: (v + 255) & ~255
    return 0, a(cells * 44) // 4, (a(cells * 44) + a(cells * 4)) // 4


def occ_update(b, plan, packed, grid, tau, k, seed, first, count):
    tb = b.lib.occ_update_tmp_bytes(count)
    tmp = b.empty((tb // 4,))
    b.lib.occ_update(plan, b.ptr(packed), C.byref(grid.c), float(tau), k, seed, first, count, b.ptr(tmp), tb, b.stream())
    return b.host(tmp)


def case_update(b, net, arith, res=(4, 6, 8), passes=3, seed=77):
    cfg, plan, _, packed = setup(b, net, arith, seed=9)
    lo, hi = (-1.0, -0.5, 0.25), (1.5, 1.0, 2.0)
    ncells = res[0] * res[1] * res[2]
    grid = Grid(b, np.zeros(ncells // 32, np.uint32), lo, hi, res, 0)
    cell = ((np.asarray(hi, f32) - np.asarray(lo, f32)) / np.asarray(res, f32)).astype(f32)
    ids = np.arange(ncells)
    ijk = np.stack((ids % res[0], (ids // res[0]) % res[1], ids // (res[0] * res[1])), axis=1)
    dx, dd = O.model_dims(cfg)
    r_off, z_off, raw_off = update_layout(ncells)
    want_bits = np.zeros(ncells, bool)
    tau = None
    for k in range(passes):
        # (tau: the median density of the centre probes, so that about half the cells are set -- fixed before any bit is looked at)
        if k == 0:
            t0 = occ_update(b, plan, packed, Grid(b, np.zeros(ncells // 32, np.uint32), lo, hi, res, 0), 1e30, 0, seed, 0, ncells)
            tau = float(np.median(t0[raw_off:raw_off + 4 * ncells].reshape(-1, 4)[:, 3]))
        tmp = occ_update(b, plan, packed, grid, tau, k, seed, 0, ncells)
        rows = tmp[r_off:r_off + 11 * ncells].reshape(ncells, 11)
        u = np.full((ncells, 3), 0.5, f32) if k == 0 else b.rng_fill(0, seed, L.OCC_RNG_STREAM, 3 * k * ncells, 3 * ncells).reshape(ncells, 3)
        probe = np.asarray(lo, np.float64) + (ijk + u.astype(np.float64)) * cell
        assert np.abs(rows[:, 0:3] - probe).max() <= 1e-6 * float(np.max(np.asarray(hi) - np.asarray(lo)))
        assert np.array_equal(rows[:, 3:], np.broadcast_to(np.array([0, 0, 0, 0, 0, 0, 0, 1], f32), (ncells, 8)))
        assert not tmp[z_off:z_off + ncells].any()
        raw = tmp[raw_off:raw_off + 4 * ncells].reshape(ncells, 4)
        # raw[3] from nerfhip_mlp_fwd on exactly the read-back rows, encoded as the fused-input forward encodes them: the kernels'
        # own arithmetic both times (bit for bit)
        x = np.concatenate([b.positional_encoding(rows[:, 0:3], O.frequency_bands(cfg["num_encoding_fn_xyz"], cfg["log_sampling_xyz"]).numpy(),
                                                  cfg["include_input_xyz"])] +
                           ([b.positional_encoding(rows[:, 8:11], O.frequency_bands(cfg["num_encoding_fn_dir"], cfg["log_sampling_dir"]).numpy(),
                                                   cfg["include_input_dir"])] if cfg["use_viewdirs"] else []), axis=1)
        assert x.shape[1] == dx + dd
        ref, _ = b.mlp_fwd(plan, packed, x)
        assert np.array_equal(raw[:, 3] > tau, ref[:, 3] > tau), (k, float(np.abs(raw - ref).max()))
        P.close(raw, ref, *TL.bound("unit.mlp_fwd"), what="probe raw rows vs nerfhip_mlp_fwd")
        want_bits |= ref[:, 3] > tau
        assert np.array_equal(unpack_bits(b.host(grid.dev), res).reshape(-1), want_bits), k
    assert 0.1 < want_bits.mean() < 0.9
    # chunked updates give the same bits as one call
    for chunk in (32, 96):
        g2 = Grid(b, np.zeros(ncells // 32, np.uint32), lo, hi, res, 0)
        for k in range(passes):
            for first in range(0, ncells, chunk):
                occ_update(b, plan, packed, g2, tau, k, seed, first, min(chunk, ncells - first))
        assert np.array_equal(b.host(g2.dev), b.host(grid.dev)), chunk
    b.lib.plan_destroy(plan)


def case_dilate(b):
    g = np.random.default_rng(5)
    for res in ((4, 8, 16), (32, 1, 1), (1, 1, 32), (2, 16, 3), (33, 4, 8)):
        cells = g.random((res[2], res[1], res[0])) < 0.06
        cells[0, 0, 0] = cells[-1, -1, -1] = True  # set cells on the box faces: nothing wraps around
        cells[0, -1, 0] = cells[-1, 0, -1] = True
        din = b.dev(pack_bits(cells).view(np.int32))
        dout = b.dev(np.full(cells.size // 32, -1, np.int32))
        b.lib.occ_dilate(b.ptr(din), b.ptr(dout), (C.c_int * 3)(*res), b.stream())
        assert np.array_equal(unpack_bits(b.host(dout), res), np_dilate(cells)), res
        assert np.array_equal(b.host(din), pack_bits(cells).view(np.int32))


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def case_refusals(b):
    cfg, plan, _, packed = setup(b, "w128", "fp32")
    rays, rand = render_inputs(cfg, 4, 8, 4, seed=1)
    rays = rays.numpy()
    opt = dict(num_coarse=8, num_fine=4, perturb=False)
    ok = Grid(b, np.full(2, 0xFFFFFFFF, np.uint32), *SCENE_BOX, (4, 4, 4), 1)

    def refused(match, **kw):
        kw.setdefault("grid_c", ok)
        rc, maps, tmp = render_occ(b, plan, plan, packed, packed, rays, opt, raise_on_error=False, **kw)
        assert rc == -1 and match in b.lib.last_error().decode(), (rc, b.lib.last_error())
        assert all(np.isnan(v).all() for v in maps.values()) and (np.asarray(tmp).view(np.int32) == -7).all()  # outputs untouched

    refused("inference render only", training=1)
    refused("inference render only", training=2)
    refused("grid_coarse is NULL", grid_c=None, grid_f=ok)
    refused("grid_fine is NULL", grid_f=None)
    refused("grid_fine is NULL", grid_c=None, grid_f=None, parts=2)
    bad = lambda **kw: Grid(b, np.full(2, 0xFFFFFFFF, np.uint32), kw.get("lo", SCENE_BOX[0]), kw.get("hi", SCENE_BOX[1]), (4, 4, 4), 1)
    g = bad()
    g.c.res = (C.c_int * 3)(0, 4, 4)
    refused("each axis must be", grid_c=g)
    g.c.res = (C.c_int * 3)(513, 4, 4)
    refused("each axis must be", grid_c=g)
    g.c.res = (C.c_int * 3)(3, 3, 3)
    refused("multiple of 32", grid_c=g)
    refused("hi > lo", grid_c=bad(hi=(1.5, -1.5, 3.0)))
    refused("hi > lo", grid_f=bad(lo=(1.5, -1.5, -3.0)))
    refused("tmp too small", tmp_words=20)
    g = bad()
    g.c.bits = None
    refused("no bits", grid_c=g)
    # plans the listed kernels do not cover
    for name in ("wide3x512_skip2", "L12_4x128"):
        p2, _, _, packed2 = P.mlp_setup(b, P.MLP_GEOMETRIES[name], seed=1)
        rc, maps, tmp = render_occ(b, p2, p2, packed2, packed2, rays, opt, ok, raise_on_error=False)
        assert rc == -1 and "render without an occupancy grid" in b.lib.last_error().decode(), b.lib.last_error()
        assert all(np.isnan(v).all() for v in maps.values()) and (np.asarray(tmp).view(np.int32) == -7).all()
        b.lib.plan_destroy(p2)
    # M >= 2^31 (no buffer is touched before the refusal: the pointers only have to be non-NULL)
    big = L.RenderCfg(1 << 15, 1 << 15, 0, 0, 0, 0.0, 11)
    ro = L.RenderOut(*[None] * 8)
    one = b.dev(np.zeros(64, f32))
    rc = b.lib._dll.nerfhip_render_fwd_occ(plan, plan, C.byref(big), b.ptr(one), 1 << 15, b.ptr(packed), b.ptr(packed), b.ptr(one), b.ptr(one),
                                           None, 0, 0, C.byref(ro), b.ptr(one), 1 << 62, 0, 3, C.byref(ok.c), C.byref(ok.c), b.ptr(one),
                                           1 << 62, b.stream())
    assert rc == -1 and "2^31" in b.lib.last_error().decode(), b.lib.last_error()
    # the unit entries
    z = np.zeros((4, 8), f32)
    flags = b.dev(np.full(32, 9, np.uint8))
    g = bad()
    g.c.res = (C.c_int * 3)(3, 3, 3)
    dr, dz = b.dev(rays), b.dev(z)
    assert b.lib._dll.nerfhip_occ_mark(b.ptr(dr), 11, 4, b.ptr(dz), 8, C.byref(g.c), b.ptr(flags), b.stream()) == -1
    assert (b.host(flags) == 9).all()
    bits = b.dev(np.full(2, 5, np.int32))
    out = b.dev(np.full(2, 6, np.int32))
    assert b.lib._dll.nerfhip_occ_dilate(b.ptr(bits), b.ptr(bits), (C.c_int * 3)(4, 4, 4), b.stream()) == -1
    assert b.lib._dll.nerfhip_occ_dilate(b.ptr(bits), b.ptr(out), (C.c_int * 3)(4, 4, 5), b.stream()) == -1
    assert (b.host(out) == 6).all() and (b.host(bits) == 5).all()
    tmp = b.dev(np.zeros(4096, f32))
    upd = lambda first, count, tb=16384, k=0: b.lib._dll.nerfhip_occ_update(plan, b.ptr(packed), C.byref(ok.c), C.c_float(0.0), k, 0, first, count,
                                                                            b.ptr(tmp), tb, b.stream())
    assert upd(16, 32) == -1 and upd(0, 48) == -1 and upd(32, 64) == -1 and upd(0, 64, tb=100) == -1 and upd(0, 32, k=-1) == -1
    assert not b.host(tmp).any() and (np.asarray(b.host(ok.dev)).view(np.uint32) == 0xFFFFFFFF).all()
    b.lib.plan_destroy(plan)
