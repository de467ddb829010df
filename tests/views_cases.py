"""Cases of the multi-view ray batch (nerfhip_select_rays_views / nerfhip_select_rays_views_bwd), written once against a backend
of tests/backends.py: tests/test_views.py runs them on the wave emulator, tests/test_gpu_views.py on the product library.

Every comparison with the single-view entry points is on the bits (the contract of include/nerfhip.h); the fp64 reference and the
error bound of the VJP are those of tests/pose_vjp.py with n = the number of rays of the view.  The single-view and the cached
entry points run the views kernels (one selection kernel, one sum kernel): their own edges are pinned here as well.
"""
import ctypes as C

import numpy as np
import torch

import pose_vjp as P

ERR_ARG = -1  # NERFHIP_ERR_ARG


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pose(seed, llff=False):
    rng = np.random.default_rng(seed)
    R = P.rodrigues(torch.tensor(rng.normal(size=3) * 0.2, dtype=torch.float64)).numpy()
    c2w = np.zeros((4, 4), dtype=np.float32)
    c2w[:3, :3] = R
    c2w[:3, 3] = rng.normal(size=3) * 0.5 + np.array([0.0, 0.0, 3.0])
    if llff:  # an LLFF-style camera: in front of the scene, looking down -z, near plane at z = -1
        c2w[:3, 3] = np.array([0.1, -0.05, 0.2], dtype=np.float32) + rng.normal(size=3).astype(np.float32) * 0.02
    c2w[3, 3] = 1.0
    return c2w


def cfg_of(b, H, W, focal, ndc, view, channels=3, seed=0, step=0, first=0):
    return b._select_cfg(H, W, focal, 2.0, 6.0, view, ndc, channels, seed, step, first)


def pose_table(poses, layout):
    """(host float32 array, view stride, row stride) holding `poses` [V, 4, 4]: contiguous [V, 4, 4], or the [V, 3, 4] blocks
    embedded in a NaN-filled table with view stride 20 and row stride 5."""
    V = len(poses)
    if layout == "4x4":
        return np.ascontiguousarray(poses, dtype=np.float32), 16, 4
    assert layout == "embedded"
    t = np.full((V, 20), np.nan, dtype=np.float32)
    for v in range(V):
        for r in range(3):
            t[v, 5 * r:5 * r + 4] = poses[v][r, :4]
    return t, 20, 5


def select_views(b, cfg, table, vstride, ld, V, images, n, inds=None):
    use_view, ch = bool(cfg.use_viewdirs), cfg.channels
    dp, di, dn = b.dev(table), b.devopt(images), b.devopt(inds, np.int64)
    rays, tgt, used = b.empty((n, 11 if use_view else 8)), b.empty((n, ch)), b.empty((n,), np.int64)
    b.lib.select_rays_views(C.byref(cfg), V, b.ptr(dp), vstride, ld, b.p(di), b.p(dn), n, b.ptr(rays),
                            b.ptr(tgt) if images is not None else None, b.ptr(used), b.stream())
    return b.host(rays), (b.host(tgt) if images is not None else None), b.host(used)


def select_one(b, cfg, c2w, image, inds):
    n = len(inds)
    dc, di, dn = b.dev(np.ascontiguousarray(c2w, np.float32)), b.devopt(image), b.dev(np.ascontiguousarray(inds, np.int64))
    rays, tgt, used = b.empty((n, 11 if cfg.use_viewdirs else 8)), b.empty((n, cfg.channels)), b.empty((n,), np.int64)
    b.lib.select_rays(C.byref(cfg), b.ptr(dc), c2w.shape[1], b.p(di), b.ptr(dn), n, b.ptr(rays),
                      b.ptr(tgt) if image is not None else None, b.ptr(used), b.stream())
    return b.host(rays), (b.host(tgt) if image is not None else None)


def case_selection(b, ndc, view, channels, layout):
    """V=3, H=5, W=7 (non-square: a swapped row / col convention shows): the whole population drawn once."""
    V, H, W = 3, 5, 7
    focal = float(np.float32(6.3))
    rng = np.random.default_rng(11 + (channels or 0))
    poses = np.stack([pose(20 + v, llff=ndc) for v in range(V)])
    images = rng.random((V, H, W, channels), dtype=np.float32) if channels else None
    cfg = cfg_of(b, H, W, focal, ndc, view, channels or 3, seed=5, step=2, first=0)
    table, vs, ld = pose_table(poses, layout)
    n = V * H * W
    rays, tgt, used = select_views(b, cfg, table, vs, ld, V, images, n)
    assert sorted(used.tolist()) == list(range(n))
    assert np.all(np.isfinite(rays))
    for v in range(V):
        rows = np.nonzero(used // (H * W) == v)[0]
        assert len(rows) == H * W
        k = used[rows] % (H * W)
        want_rays, want_tgt = select_one(b, cfg, poses[v], images[v] if channels else None, k)
        assert np.array_equal(bits(rays[rows]), bits(want_rays)), (v, "rays")
        if channels:
            assert np.array_equal(bits(tgt[rows]), bits(want_tgt)), (v, "target")
            r, c = k % H, k // H  # (the convention itself, not only agreement with the single-view kernel)
            assert np.array_equal(tgt[rows], images[v][r, c])
    assert tgt is not None or not channels


def case_single_view_is_select_rays(b, ndc, view, channels):
    """nerfhip_select_rays is the V = 1 case of nerfhip_select_rays_views: the same rays, targets and indices on the bits."""
    H, W, n = 20, 16, 64
    focal = float(np.float32(17.5))
    c2w = pose(3, llff=ndc)
    img = np.random.default_rng(1).random((H, W, channels), dtype=np.float32) if channels else None
    cfg = cfg_of(b, H, W, focal, ndc, view, channels or 3, seed=11, step=3, first=64)
    rays, tgt, used = select_views(b, cfg, c2w[None], 16, 4, 1, img[None] if channels else None, n)
    r1, t1, u1 = b.select_rays(H, W, focal, c2w, img, n, 2.0, 6.0, use_viewdirs=view, ndc=ndc, seed=11, step=3, first=64)
    assert np.all(np.isfinite(rays)) and rays.shape == (n, 11 if view else 8)
    assert np.array_equal(used, u1) and np.array_equal(bits(rays), bits(r1))
    assert (tgt is None and t1 is None) if not channels else np.array_equal(bits(tgt), bits(t1))


def case_single_view_row_stride(b):
    """The single-view entry points at a row stride other than 4: the pose embedded in a NaN-filled buffer with c2w_ld = 5 gives the
    bits of the contiguous 4 x 4 pose, forward and backward (H=5, W=7, every pixel once, by explicit indices)."""
    H, W = 5, 7
    focal = float(np.float32(6.3))
    rng = np.random.default_rng(17)
    inds = rng.permutation(H * W).astype(np.int64)
    img = rng.random((H, W, 3), dtype=np.float32)
    g = rng.normal(size=(H * W, 11)).astype(np.float32)
    for ndc in (False, True):
        c2w = pose(5, llff=ndc)
        wide = np.full((3, 5), np.nan, dtype=np.float32)   # (select_one / one_bwd pass shape[1] as c2w_ld)
        wide[:, :4] = c2w[:3, :4]
        cfg = cfg_of(b, H, W, focal, ndc, True)
        rays, tgt = select_one(b, cfg, c2w, img, inds)
        rays5, tgt5 = select_one(b, cfg, wide, img, inds)
        assert np.all(np.isfinite(rays))
        assert np.array_equal(bits(rays), bits(rays5)) and np.array_equal(bits(tgt), bits(tgt5))
        got, got5 = one_bwd(b, cfg, c2w, inds, g, None, 11), one_bwd(b, cfg, wide, inds, g, None, 11)
        assert np.all(np.isfinite(got)) and np.array_equal(bits(got), bits(got5))


def case_cached_rows_are_select_rays_rows(b, view):
    """The cached branch of the selection kernel: the rows of the stored bundle (nerfhip_ray_bundle: pixel row * W + col) are, bit for
    bit, the rows nerfhip_select_rays generates at the transposed index convention (k -> row k % H, col k / H); no NDC."""
    H, W = 5, 7
    focal = float(np.float32(6.3))
    rng = np.random.default_rng(23)
    c2w = pose(5)
    img = rng.random((H, W, 3), dtype=np.float32)
    k = rng.permutation(H * W).astype(np.int64)
    ro, rd = b.ray_bundle(H, W, focal, c2w)
    cached = (k % H) * W + k // H
    rays_c, tgt_c, used_c = b.select_cached_rays(H, W, focal, ro, rd, np.ascontiguousarray(img.reshape(-1, 3)), H * W, 2.0, 6.0,
                                                 inds=cached, use_viewdirs=view)
    rays, tgt = select_one(b, cfg_of(b, H, W, focal, False, view), c2w, img, k)
    assert np.array_equal(used_c, cached) and np.all(np.isfinite(rays_c))
    assert np.array_equal(bits(rays_c), bits(rays)) and np.array_equal(bits(tgt_c), bits(tgt))


def case_explicit_indices_and_rank_slices(b):
    V, H, W = 3, 5, 7
    focal = float(np.float32(6.3))
    poses = np.stack([pose(20 + v) for v in range(V)])
    img = np.random.default_rng(2).random((V, H, W, 3), dtype=np.float32)
    cfg = cfg_of(b, H, W, focal, False, True, 3, seed=9, step=1, first=0)
    inds = np.array([104, 0, 35, 34, 70, 69, 36, 36], dtype=np.int64)  # (first / last of every view; a repeat)
    rays, tgt, used = select_views(b, cfg, poses, 16, 4, V, img, len(inds), inds)
    assert np.array_equal(used, inds)
    for i, g in enumerate(inds):
        v, k = int(g) // (H * W), int(g) % (H * W)
        wr, wt = select_one(b, cfg, poses[v], img[v], np.array([k]))
        assert np.array_equal(bits(rays[i:i + 1]), bits(wr)) and np.array_equal(bits(tgt[i:i + 1]), bits(wt))
    # two ranks: disjoint slices of one permutation
    n = 40
    u0 = select_views(b, cfg, poses, 16, 4, V, img, n)[2]
    cfg1 = cfg_of(b, H, W, focal, False, True, 3, seed=9, step=1, first=n)
    u1 = select_views(b, cfg1, poses, 16, 4, V, img, n)[2]
    assert len(set(u0.tolist()) | set(u1.tolist())) == 2 * n
    assert max(u0.max(), u1.max()) < V * H * W and min(u0.min(), u1.min()) >= 0


# ---- the VJP ------------------------------------------------------------------------------------------------------------------
VH, VW, VV = 27, 35, 4
VFOCAL = float(np.float32(31.7))


def views_bwd(b, cfg, table, vstride, ld, V, inds, g, g2, stride, tmp_slack=0):
    n = len(inds)
    tb = b.lib.pose_grad_views_tmp_bytes(n, V)
    assert tb >= 0
    tmp = b.empty((max(tb // 4, 1) + tmp_slack,))
    out = b.empty((V, 3, 4))
    dp, dn = b.dev(table), b.dev(np.ascontiguousarray(inds, np.int64))
    dg, dg2 = b.devopt(g), b.devopt(g2)
    b.lib.select_rays_views_bwd(C.byref(cfg), V, b.ptr(dp), vstride, ld, b.ptr(dn), n, b.p(dg), b.p(dg2), stride, b.ptr(tmp), tb,
                                b.ptr(out), b.stream())
    return b.host(out)


def one_bwd(b, cfg, c2w, inds, g, g2, stride):
    n = len(inds)
    tb = b.lib.pose_grad_tmp_bytes(n)
    tmp, out = b.empty((max(tb // 4, 1),)), b.empty((3, 4))
    dc, dn = b.dev(np.ascontiguousarray(c2w, np.float32)), b.dev(np.ascontiguousarray(inds, np.int64))
    dg, dg2 = b.devopt(g), b.devopt(g2)
    b.lib.select_rays_bwd(C.byref(cfg), b.ptr(dc), c2w.shape[1], b.ptr(dn), n, b.p(dg), b.p(dg2), stride, b.ptr(tmp), tb,
                          b.ptr(out), b.stream())
    return b.host(out)


def vjp_batch(which, rng):
    """Global indices of the batch: (a) 333 rays over views 0, 1, 3 -- view 2 gets none; (b) 700 rays, 600 of them in view 1 (several
    partials: G(600) = 3)."""
    hw = VH * VW
    if which == "a":
        views = rng.choice([0, 1, 3], size=333)
    else:
        views = np.concatenate([np.full(600, 1), rng.choice([0, 2, 3], size=100)])
        views = views[rng.permutation(700)]
    return views.astype(np.int64) * hw + rng.integers(0, hw, size=len(views))


def case_vjp(b, which, ndc, view, two):
    rng = np.random.default_rng(31 + ord(which) + 2 * ndc + 4 * view + 8 * two)
    V, H, W, focal, hw = VV, VH, VW, VFOCAL, VH * VW
    poses = np.stack([pose(40 + v, llff=ndc) for v in range(V)])
    cfg = cfg_of(b, H, W, focal, ndc, view)
    stride = 12 if view else 9           # (a row stride wider than the row: the padding columns are never read)
    inds = vjp_batch(which, rng)
    n = len(inds)
    g = rng.normal(size=(n, stride)).astype(np.float32)
    g2 = rng.normal(size=(n, stride)).astype(np.float32) if two else None
    got = views_bwd(b, cfg, poses, 16, 4, V, inds, g, g2, stride)
    assert got.shape == (V, 3, 4) and np.all(np.isfinite(got))
    gsum = g.astype(np.float64) + (g2.astype(np.float64) if two else 0.0)
    gmag = np.abs(g.astype(np.float64)) + (np.abs(g2.astype(np.float64)) if two else 0.0)
    vid = inds // hw
    for v in range(V):
        rows = np.nonzero(vid == v)[0]        # (ascending batch position)
        nv = len(rows)
        if nv == 0:
            assert which == "a" and v == 2
            assert np.array_equal(bits(got[v]), np.zeros((3, 4), np.uint32))  # exact +0 over the NaN pre-fill
            continue
        k = inds[rows] - v * hw
        single = one_bwd(b, cfg, poses[v], k, np.ascontiguousarray(g[rows]), np.ascontiguousarray(g2[rows]) if two else None, stride)
        assert np.array_equal(bits(got[v]), bits(single)), (which, v, nv)
        want = P.oracle_select_vjp(H, W, focal, poses[v], k, gsum[rows], ndc, view)
        mag = P.magnitude(H, W, focal, poses[v], k, True, g_rays=gmag[rows], ndc=ndc, view=view)
        bound = P.bound(nv, mag)
        err = np.abs(got[v].astype(np.float64) - want)
        assert np.all(err <= bound), (which, v, float((err / np.maximum(bound, 1e-300)).max()))
    if which == "b":
        assert P.wgs(int((vid == 1).sum())) == 3
    again = views_bwd(b, cfg, poses, 16, 4, V, inds, g, g2, stride, tmp_slack=7)
    assert np.array_equal(bits(got), bits(again))
    if two:  # the two inputs are added row by row first: swapping them gives the same bits (IEEE addition commutes)
        assert np.array_equal(bits(got), bits(views_bwd(b, cfg, poses, 16, 4, V, inds, g2, g, stride)))
    # another interleaving of the views that keeps each view's internal order: the same bits
    keys = rng.random(n)
    perm = np.empty(n, dtype=np.int64)
    order = np.argsort(keys, kind="stable")           # target slots in a random order ...
    slot_view = vid[order]                            # ... hand view labels round: slot j takes the next ray of view slot_view[j]
    for v in range(V):
        perm[np.nonzero(slot_view == v)[0]] = np.nonzero(vid == v)[0]
    assert sorted(perm.tolist()) == list(range(n)) and not np.array_equal(perm, np.arange(n))
    shuffled = views_bwd(b, cfg, poses, 16, 4, V, inds[perm], np.ascontiguousarray(g[perm]),
                         np.ascontiguousarray(g2[perm]) if two else None, stride)
    assert np.array_equal(bits(got), bits(shuffled))
    # the embedded [V, 3, 4] table gives the same bits as the contiguous one
    table, vs, ld = pose_table(poses, "embedded")
    assert np.array_equal(bits(got), bits(views_bwd(b, cfg, table, vs, ld, V, inds, g, g2, stride)))


def case_single_view_vjp_sum_edges(b, n):
    """The sum kernel's single-view form at its edges -- n = 1 (one partial), 257 (two), 256 * 64 + 1 (65 partials: one more than a
    wave has lanes, so the lane-strided loop takes a second trip): within the fp64 bound, and the bits of the views form at V = 1."""
    rng = np.random.default_rng(53 + n)
    H, W, focal = VH, VW, VFOCAL
    c2w = pose(44, llff=True)
    cfg = cfg_of(b, H, W, focal, True, True)
    inds = rng.integers(0, H * W, size=n).astype(np.int64)
    g = rng.normal(size=(n, 11)).astype(np.float32)
    assert P.wgs(n) == {1: 1, 257: 2, 16385: 65}[n]
    got = one_bwd(b, cfg, c2w, inds, g, None, 11)
    assert np.all(np.isfinite(got))
    assert np.array_equal(bits(got), bits(views_bwd(b, cfg, c2w[None], 16, 4, 1, inds, g, None, 11)[0]))
    want = P.oracle_select_vjp(H, W, focal, c2w, inds, g.astype(np.float64), True, True)
    bound = P.bound(n, P.magnitude(H, W, focal, c2w, inds, True, g_rays=np.abs(g.astype(np.float64)), ndc=True, view=True))
    err = np.abs(got.astype(np.float64) - want)
    print("single-view VJP, n = %d: worst error / bound = %.3f" % (n, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound), (n, float((err / np.maximum(bound, 1e-300)).max()))


def case_vjp_no_rays(b):
    lib = b.lib
    assert lib.pose_grad_views_tmp_bytes(0, 5) == 0
    assert lib.pose_grad_views_tmp_bytes(-1, 5) == -1
    assert lib.pose_grad_views_tmp_bytes(700, 4) == 4 * (12 * (700 // 256 + 4) + 2 * 4 + 700)
    cfg = cfg_of(b, VH, VW, VFOCAL, False, True)
    poses = np.stack([pose(v) for v in range(5)])
    out = b.empty((5, 3, 4))
    dp = b.dev(poses)
    lib.select_rays_views_bwd(C.byref(cfg), 5, b.ptr(dp), 16, 4, None, 0, None, None, 11, None, 0, b.ptr(out), b.stream())
    assert np.array_equal(bits(b.host(out)), np.zeros((5, 3, 4), np.uint32))


def case_refusals(b):
    lib = b.lib
    V, H, W = 3, 4, 4
    raw_s, raw_b = lib._dll.nerfhip_select_rays_views, lib._dll.nerfhip_select_rays_views_bwd
    cfg = cfg_of(b, H, W, 3.0, False, True)
    poses = b.dev(np.stack([np.eye(4, dtype=np.float32)] * V))
    rays, used = b.empty((4, 11)), b.empty((4,), np.int64)
    inds = b.dev(np.arange(4, dtype=np.int64))
    g = b.dev(np.zeros((4, 11), np.float32))
    tb = lib.pose_grad_views_tmp_bytes(4, V)
    tmp, out = b.empty((tb // 4,)), b.empty((V, 3, 4))
    pp, pr, pu, pi, pg, pt, po, st = (b.ptr(poses), b.ptr(rays), b.ptr(used), b.ptr(inds), b.ptr(g), b.ptr(tmp), b.ptr(out),
                                      b.stream())
    ok = lambda c=cfg, v=V, p=pp, vs=16, ld=4, n=4, r=pr: raw_s(C.byref(c) if c else None, v, p, vs, ld, None, None, n, r, None,  # noqa: E731
                                                                pu, st)
    assert ok() == 0
    bad = [ok(c=None), ok(p=None), ok(r=None), ok(v=0), ok(v=-2), ok(ld=3), ok(vs=11), ok(vs=13, ld=5),
           ok(v=L_MAX_VIEWS + 1),
           ok(c=cfg_of(b, 400, 400, 3.0, False, True), v=30000),                       # population 4.8e9 > 2^32
           ok(n=V * H * W + 1), ok(c=cfg_of(b, H, W, 3.0, False, True, first=V * H * W - 3))]  # first + n beyond the population
    assert all(rc == ERR_ARG for rc in bad), bad
    assert lib._dll.nerfhip_last_error()
    okb = lambda c=cfg, v=V, p=pp, vs=16, ld=4, i=pi, gs=11, t=pt, tbytes=tb, o=po: raw_b(  # noqa: E731
        C.byref(c) if c else None, v, p, vs, ld, i, 4, pg, None, gs, t, tbytes, o, st)
    assert okb() == 0
    bad = [okb(c=None), okb(p=None), okb(o=None), okb(v=0), okb(ld=3), okb(vs=11), okb(i=None), okb(gs=8), okb(tbytes=tb - 4),
           okb(t=None), okb(c=cfg_of(b, 400, 400, 3.0, False, True), v=30000)]
    assert all(rc == ERR_ARG for rc in bad), bad
    assert lib._dll.nerfhip_last_error()
    assert lib.pose_grad_views_tmp_bytes(4, 0) == -1 and lib.pose_grad_views_tmp_bytes(4, L_MAX_VIEWS + 1) == -1


L_MAX_VIEWS = 65536  # NERFHIP_MAX_VIEWS
