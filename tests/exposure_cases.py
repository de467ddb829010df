"""Cases of the per-view exposure (nerfhip_mse_loss_views_fwd_bwd, nerfhip_exposure_bwd, nerfhip_exposure_grad_tmp_bytes), written
once against a backend of tests/backends.py: tests/test_exposure.py runs them on the wave emulator, tests/test_gpu_exposure.py on
the product library.

Definitions (include/nerfhip.h): expo [V][6], row v = (s_r, s_g, s_b, b_r, b_g, b_b); ray i belongs to view inds[i] // hw; its
corrected prediction is p' = exp(s) p + b per channel, alike for the coarse and the fine rgb; the loss is mse(p', t) per net, the
cotangents carry k = 2 / (3 n) * grad_scale.  An index outside [0, V hw) is the identity in the loss and dropped from the table
gradient.

Reference value (local to this file): torch fp64 autograd of exactly these formulas (`loss64`, `oracle`), fed the fp32 values the
kernels read.  `case_reference_against_itself` holds it to central differences.

Bounds, counted from the operation order written next to the kernels (csrc/elementwise.hip: mse_loss_body; csrc/dataio.hip:
k_expo_part).  u = 2^-24; every operation below is one fp32 rounding, relative to its own result.

* An entry of g_rgb = (d k) e.  e = (float)exp((double)s): 1 (the fp64 exp's own error is 2^-29 of that).  q = e p: e's 1 + 1 = 2,
  relative to |e||p|.  q + b: 1, relative to at most |e||p| + |b|; the subtraction of t: 1, relative to at most
  |e||p| + |b| + |t| =: M.  So d is off by at most (2 + 1 + 1) u M = 4 u M.  k = 2 / (float)(3 n) * grad_scale: the conversion
  1, the division 1, the product 1: 3.  d k: 1.  The product with e: e's 1 + 1 = 2.  C_RGB = 4 + 3 + 1 + 2 = 10:
      |g_rgb - exact| <= C_RGB u k M |e|.
* An entry of g_expo, row v: a sum over the n_v rays of view v along the pose VJP's tree (tests/pose_vjp.py: reduction_depth), so
      |g_expo - exact| <= (D(n_v) + C_EXPO) u sum_i A_i,
  A_i the ray's term on absolute values: for an s column k M |e||p| (coarse) + the same on the fine rgb, for a b column k M
  (+ the fine one).  The longest chain of a term is the s column's (d k) q: d 4, k 3, the product 1, q 2, the product 1: 11 (the b
  column's d k has 8).  Per ray the thread adds the coarse term and then the fine term: one addition more per ray than the tree of
  D(n) counts; a thread holds ceil(n_v / (256 G(n_v))) = 1 ray while n_v <= 2^18 (every case here; `expo_bound` asserts it), so
  that is one level more: C_EXPO = 11 + 1 = 12.
* The loss words: the `tiny.loss` bound of tests/tolerances.py per net (the mse of an rgb map against its target) and `e2e.loss`
  for their sum.

Every gradient batch is drawn (`batch`) with |s| <= 0.5, |b| <= 0.1, rgb and targets in [0, 1], from the first seed at which
-- by the reference alone -- every exact entry of g_expo of a view with rays is at least 100 times its bound
(`case_batches_are_well_conditioned` asserts that on the CPU for every batch the cases use).
"""
import numpy as np
import torch

import pose_vjp as P
import tolerances as T

ERR_ARG = -1  # NERFHIP_ERR_ARG
U32 = 2.0 ** -24
C_RGB, C_EXPO = 10, 12
MAX_VIEWS = 65536  # NERFHIP_MAX_VIEWS
HW = 400           # height * width of the cases' views


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


# ---- the fp64 restatement -------------------------------------------------------------------------------------------------------
def rows_of(inds, hw, table):
    """(valid [n], s [n, 3], b [n, 3]) of each ray (torch fp64; zeros for an index of no view)."""
    inds = torch.as_tensor(np.asarray(inds), dtype=torch.int64)
    V = table.shape[0]
    valid = (inds >= 0) & (inds < V * hw)
    row = table[torch.where(valid, inds // hw, torch.zeros_like(inds))]
    row = torch.where(valid[:, None], row, torch.zeros_like(row))
    return valid, row[:, :3], row[:, 3:]


def loss64(rc, rf, tgt, inds, hw, table):
    """(coarse_mse, fine_mse) in torch fp64; rf may be None (then fine_mse is 0)."""
    _, s, b = rows_of(inds, hw, table)
    t = tgt[:, :3]
    lc = ((torch.exp(s) * rc + b - t) ** 2).mean()
    lf = ((torch.exp(s) * rf + b - t) ** 2).mean() if rf is not None else torch.zeros((), dtype=torch.float64)
    return lc, lf


def oracle(rc, rf, tgt, inds, hw, table, gs=1.0):
    """dict(loss [3], g_c, g_f, g_expo) by fp64 autograd; the gradients are those of grad_scale * (coarse_mse + fine_mse)."""
    leaf = lambda a: None if a is None else torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    c, f, tab = leaf(rc), leaf(rf), leaf(table)
    lc, lf = loss64(c, f, torch.as_tensor(np.asarray(tgt, np.float64)), inds, hw, tab)
    if len(np.asarray(rc)):
        ((lc + lf) * float(gs)).backward()
    z = lambda t: None if t is None else (t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape)))  # noqa: E731
    lc, lf = float(lc.detach()), float(lf.detach())
    return dict(loss=np.array([lc, lf, lc + lf]), g_c=z(c), g_f=z(f), g_expo=z(tab))


def magnitudes(rc, rf, tgt, inds, hw, table, gs=1.0):
    """(M_c |e| k [n, 3], M_f |e| k [n, 3] or None, sum_i A_i [V, 6], rays per view [V]) in numpy fp64."""
    table = np.asarray(table, np.float64)
    n, V = len(inds), table.shape[0]
    valid, s, b = (t.numpy() for t in rows_of(inds, hw, torch.as_tensor(table)))
    e, t = np.exp(s), np.abs(np.asarray(tgt, np.float64)[:, :3])
    k = 2.0 / (3.0 * max(n, 1)) * float(gs)
    vid = np.where(valid, np.asarray(inds) // hw, -1)
    a_sum, per_rgb = np.zeros((V, 6)), []
    for r in (rc, rf):
        if r is None:
            per_rgb.append(None)
            continue
        q = e * np.abs(np.asarray(r, np.float64))
        m = q + np.abs(b) + t
        per_rgb.append(k * m * e)
        for v in range(V):
            a_sum[v, :3] += (k * m * q)[vid == v].sum(0)
            a_sum[v, 3:] += (k * m)[vid == v].sum(0)
    return per_rgb[0], per_rgb[1], a_sum, np.array([(vid == v).sum() for v in range(V)])


def expo_bound(n_views_rays, a_sum):
    """[V, 6]: (D(n_v) + C_EXPO) u sum_i A_i."""
    assert int(np.max(n_views_rays, initial=0)) <= 1 << 18   # (one ray per thread: the module docstring's count of C_EXPO)
    depth = np.array([P.reduction_depth(int(nv)) for nv in n_views_rays], np.float64)
    return (depth[:, None] + C_EXPO) * U32 * a_sum


# ---- batches ---------------------------------------------------------------------------------------------------------------------
def view_ids(n, V, rng, kind):
    if kind == "one":                  # all rays in one view
        return np.zeros(n, np.int64)
    if kind == "gap" and V >= 3:       # view 1 has no ray
        return rng.choice(np.array([v for v in range(V) if v != 1]), size=n).astype(np.int64)
    return rng.integers(0, V, size=n).astype(np.int64)


def draw(n, V, fine, stride, seed, kind):
    rng = np.random.default_rng(seed)
    vid = view_ids(n, V, rng, kind)
    inds = vid * HW + rng.integers(0, HW, size=n)
    table = np.concatenate([rng.uniform(-0.5, 0.5, (V, 3)), rng.uniform(-0.1, 0.1, (V, 3))], -1).astype(np.float32)
    rc = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    rf = rng.uniform(0, 1, (n, 3)).astype(np.float32) if fine else None
    tgt = rng.uniform(0, 1, (n, stride)).astype(np.float32)
    return dict(rc=rc, rf=rf, tgt=tgt, inds=inds.astype(np.int64), table=table, V=V, n=n)


def conditioning(c, gs=1.0):
    """min over the entries of views with rays of |exact g_expo| / bound, by the reference alone."""
    ref = oracle(c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"], gs)
    _, _, a_sum, nv = magnitudes(c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"], gs)
    bound = expo_bound(nv, a_sum)
    has = nv > 0
    return float((np.abs(ref["g_expo"])[has] / bound[has]).min()) if has.any() else np.inf


_BATCHES = {}


def batch(n, V, fine, stride, kind=None):
    """The case's batch: the first seed whose exact g_expo is >= 100 x its bound in every entry of a view with rays (at both
    grad_scale values: the ratio does not depend on it)."""
    kind = kind or ("gap" if V >= 3 and n > 1 else "any")
    key = (n, V, bool(fine), stride, kind)
    if key not in _BATCHES:
        for seed in range(1000, 1200):
            c = draw(n, V, fine, stride, seed + 7 * n + V, kind)
            if conditioning(c) >= 100.0:
                _BATCHES[key] = c
                break
        else:
            raise AssertionError("no well-conditioned batch for %r" % (key,))
    return _BATCHES[key]


GRID = [(n, V, stride, fine) for n in (1, 63, 256, 257, 700) for V in (1, 3) for stride in (3, 4) for fine in (False, True)]
GRID_IDS = ["n%d-V%d-stride%d-%s" % (n, V, s, "fine" if f else "coarse") for n, V, s, f in GRID]
BIG = [(4096, 100, 3, True, "any"), (700, 1, 3, True, "one")]
BIG_IDS = ["4096-rays-100-views", "700-rays-one-view"]


# ---- the entry points on numpy arrays -------------------------------------------------------------------------------------------
def loss_views(b, rc, rf, tgt, inds, hw, table, gs=1.0):
    """(loss [3], g_c, g_f or None) of nerfhip_mse_loss_views_fwd_bwd."""
    n = rc.shape[0]
    dc, df, dt = b.dev(f32(rc)), b.devopt(rf), b.dev(f32(tgt))
    di, dx = b.dev(np.ascontiguousarray(inds, np.int64)), b.dev(f32(table))
    gc, gf, lo = b.empty((n, 3)), (b.empty((n, 3)) if rf is not None else None), b.empty((3,))
    b.lib.mse_loss_views_fwd_bwd(b.ptr(dc), b.p(df), b.ptr(dt), tgt.shape[1], n, float(gs), b.ptr(di), hw, b.ptr(dx), table.shape[0],
                                 b.ptr(gc), b.p(gf), b.ptr(lo), b.stream())
    return b.host(lo), b.host(gc), (b.host(gf) if gf is not None else None)


def expo_bwd(b, rc, rf, tgt, inds, hw, table, gs=1.0, mask=None, tmp_slack=0):
    """g_expo [V, 6] of nerfhip_exposure_bwd."""
    n, V = rc.shape[0], table.shape[0]
    tb = b.lib.exposure_grad_tmp_bytes(n, V)
    assert tb == 4 * (6 * (n // 256 + V) + 2 * V + n)
    tmp, out = b.empty((tb // 4 + tmp_slack,)), b.empty((V, 6))
    dc, df, dt = b.dev(f32(rc)), b.devopt(rf), b.dev(f32(tgt))
    di, dx, dm = b.dev(np.ascontiguousarray(inds, np.int64)), b.dev(f32(table)), b.devopt(mask, np.uint8)
    b.lib.exposure_bwd(b.ptr(dc) if n else None, b.p(df) if n else None, b.ptr(dt) if n else None, tgt.shape[1], n, float(gs),
                       b.ptr(di) if n else None, hw, b.ptr(dx), V, b.p(dm), b.ptr(tmp), tb, b.ptr(out), b.stream())
    return b.host(out)


# ---- 1. the reference alone (CPU only: no backend) -----------------------------------------------------------------------------------
def case_reference_against_itself(fine):
    """Central differences in fp64, relative 1e-6 of the largest entry, on every entry of g_expo and on the rgb entries of a few rays."""
    c = draw(40, 3, fine, 4, 5, "gap")
    c["inds"][3] = -5              # (an index of no view: identity, dropped)
    c["inds"][7] = 3 * HW
    gs = 0.75
    ref = oracle(c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"], gs)
    tgt = torch.as_tensor(c["tgt"].astype(np.float64))

    def loss(table, rc, rf):
        with torch.no_grad():
            lc, lf = loss64(torch.as_tensor(rc), None if rf is None else torch.as_tensor(rf), tgt, c["inds"], HW, torch.as_tensor(table))
            return float(lc + lf) * gs
    base = [c["table"].astype(np.float64), c["rc"].astype(np.float64), None if not fine else c["rf"].astype(np.float64)]
    h = 1e-6
    for which, grad in ((0, ref["g_expo"]), (1, ref["g_c"]), (2, ref["g_f"])):
        if base[which] is None:
            continue
        scale = float(np.abs(grad).max())
        flat_n = base[which].size
        for j in (range(flat_n) if which == 0 else range(0, flat_n, 7)):
            args = [a if a is None else a.copy() for a in base]
            args[which].reshape(-1)[j] += h
            up = loss(*args)
            args[which].reshape(-1)[j] -= 2 * h
            fd = (up - loss(*args)) / (2 * h)
            assert abs(fd - grad.reshape(-1)[j]) <= 1e-6 * scale + 1e-9, (which, j, fd, grad.reshape(-1)[j])
    assert not ref["g_expo"][1].any()                     # the view without a ray


def case_batches_are_well_conditioned():
    for n, V, stride, fine in GRID:
        assert conditioning(batch(n, V, fine, stride)) >= 100.0
    for n, V, stride, fine, kind in BIG:
        assert conditioning(batch(n, V, fine, stride, kind)) >= 100.0
    c = batch(700, 3, True, 3)
    assert not (c["inds"] // HW == 1).any() and c["table"].dtype == np.float32
    for c in _BATCHES.values():
        t = c["table"]
        assert np.abs(t[:, :3]).max() <= 0.5 and np.abs(t[:, 3:]).max() <= 0.1
        assert min(c["rc"].min(), c["tgt"].min()) >= 0.0 and max(c["rc"].max(), c["tgt"].max()) <= 1.0


# ---- 2. loss and cotangents against fp64 ---------------------------------------------------------------------------------------------
def case_loss_fp64(b, n, V, stride, fine, gs):
    c = batch(n, V, fine, stride)
    ref = oracle(c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"], gs)
    lo, gc, gf = loss_views(b, c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"], gs)
    mc, mf, _, _ = magnitudes(c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"], gs)
    err = np.abs(lo.astype(np.float64) - ref["loss"])
    print("loss words off by", err, "of", ref["loss"])
    assert err[0] <= T.bound("tiny.loss") and err[1] <= T.bound("tiny.loss") and err[2] <= T.bound("e2e.loss")
    if not fine:
        assert lo[1] == 0.0
    for got, want, mag in ((gc, ref["g_c"], mc), (gf, ref["g_f"], mf)):
        if want is None:
            continue
        bound = C_RGB * U32 * mag
        ratio = float((np.abs(got.astype(np.float64) - want) / bound).max())
        print("g_rgb worst error / bound", ratio)
        assert ratio <= 1.0, ratio


# ---- 3. the table gradient against fp64 ------------------------------------------------------------------------------------------------
def case_grad_fp64(b, n, V, stride, fine, gs, kind=None):
    c = batch(n, V, fine, stride, kind)
    ref = oracle(c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"], gs)
    got = expo_bwd(b, c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"], gs)
    _, _, a_sum, nv = magnitudes(c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"], gs)
    bound = expo_bound(nv, a_sum)
    assert not got[nv == 0].any() and bits(got[nv == 0]).max(initial=0) == 0   # (a view without a ray: exact +0)
    has = nv > 0
    ratio = float((np.abs(got.astype(np.float64) - ref["g_expo"])[has] / bound[has]).max())
    print("g_expo worst error / bound", ratio, "smallest |exact| / bound", float((np.abs(ref["g_expo"])[has] / bound[has]).min()))
    assert ratio <= 1.0, ratio


# ---- 4. the zero table is the plain loss, bit for bit ----------------------------------------------------------------------------------
def case_zero_table_bits(b, n, V, stride, fine, gs):
    c = batch(n, V, fine, stride)
    zero = np.zeros((V, 6), np.float32)
    lo, gc, gf = loss_views(b, c["rc"], c["rf"], c["tgt"], c["inds"], HW, zero, gs)
    lo0, gc0, gf0 = b.mse_loss(c["rc"], c["rf"], c["tgt"], gs)
    assert np.array_equal(lo, lo0) and np.array_equal(bits(lo), bits(lo0))
    assert np.array_equal(gc, gc0)
    if fine:
        assert np.array_equal(gf, gf0)


# ---- 5. the order of the views in the batch, and run-to-run ----------------------------------------------------------------------------
def case_view_order_bits(b):
    c = batch(700, 3, True, 3)
    first = expo_bwd(b, c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"])
    again = expo_bwd(b, c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"])
    assert np.array_equal(bits(first), bits(again))
    vid = c["inds"] // HW
    orders = [np.argsort(vid, kind="stable"), np.argsort(-vid, kind="stable")]   # the views one after the other, either way round
    rng = np.random.default_rng(3)
    slots = rng.permutation(len(vid))                                            # another random interleaving: each view keeps its order
    order = np.empty(len(vid), np.int64)
    pos = {v: list(np.flatnonzero(vid == v)) for v in np.unique(vid)}
    for j, v in enumerate(vid[slots]):
        order[j] = pos[v].pop(0)
    orders.append(order)
    for o in orders:
        assert sorted(o.tolist()) == list(range(len(vid)))
        for v in np.unique(vid):
            assert np.all(np.diff(o[vid[o] == v]) > 0)     # (each view's rays keep their order)
        got = expo_bwd(b, c["rc"][o], c["rf"][o], c["tgt"][o], c["inds"][o], HW, c["table"])
        assert np.array_equal(bits(got), bits(first))
    assert not np.array_equal(orders[0], np.arange(len(vid)))


# ---- 6. the mask --------------------------------------------------------------------------------------------------------------------
def masks(V):
    rng = np.random.default_rng(11)
    anchor = np.ones((V, 6), np.uint8)
    anchor[0] = 0
    gain = np.tile(np.array([1, 1, 1, 0, 0, 0], np.uint8), (V, 1))
    both = gain.copy()
    both[0] = 0
    return {"anchor": anchor, "gain": gain, "gain+anchor": both, "none": np.zeros((V, 6), np.uint8),
            "random": (rng.random((V, 6)) < 0.5).astype(np.uint8), "all": np.ones((V, 6), np.uint8)}


MASKS = ["anchor", "gain", "gain+anchor", "none", "random", "all"]


def case_mask(b, name):
    c = batch(257, 3, True, 3, "any")
    mask = masks(3)[name]
    full = expo_bwd(b, c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"])
    got = expo_bwd(b, c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"], mask=mask)
    assert np.all(bits(got)[mask == 0] == 0)                                   # exact +0
    assert np.array_equal(bits(got)[mask != 0], bits(full)[mask != 0])
    assert np.all(full != 0)
    # 20 Adam steps on the masked gradient never move a masked entry
    p, m, v = c["table"].reshape(-1).copy(), np.zeros(18, np.float32), np.zeros(18, np.float32)
    for step in range(1, 21):
        g = expo_bwd(b, c["rc"], c["rf"], c["tgt"], c["inds"], HW, p.reshape(3, 6), mask=mask)
        p, m, v = b.adam_step(p, g.reshape(-1), m, v, 1e-2, step)
    still = mask.reshape(-1) == 0
    assert np.array_equal(bits(p)[still], bits(c["table"].reshape(-1))[still])
    assert np.all(bits(p)[~still] != bits(c["table"].reshape(-1))[~still])


# ---- 7. edges ----------------------------------------------------------------------------------------------------------------------
def case_edges(b):
    V = 3
    table = batch(63, 3, True, 3)["table"]
    e = np.zeros((0, 3), np.float32)
    got = expo_bwd(b, e, e, e, np.zeros(0, np.int64), HW, table)
    assert got.shape == (V, 6) and bits(got).max() == 0                        # n = 0: exact zeros
    c = draw(300, V, True, 4, 77, "any")
    out = np.array([0, 5, 17, 120, 256, 299])
    c["inds"][out] = [-1, V * HW, -(1 << 40), 1 << 40, V * HW + 3, -HW]
    # the loss: a ray of no view is the identity
    lo, gc, gf = loss_views(b, c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"])
    lo0, gc0, gf0 = b.mse_loss(c["rc"], c["rf"], c["tgt"])
    assert np.array_equal(gc[out], gc0[out]) and np.array_equal(gf[out], gf0[out])
    ref = oracle(c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"])
    assert np.all(np.abs(lo.astype(np.float64) - ref["loss"])[:2] <= T.bound("tiny.loss"))
    none = np.full(300, V * HW, np.int64)
    lo, gc, gf = loss_views(b, c["rc"], c["rf"], c["tgt"], none, HW, c["table"])
    assert np.array_equal(bits(lo), bits(lo0)) and np.array_equal(gc, gc0) and np.array_equal(gf, gf0)
    # the gradient: dropped -- the bits of the batch without them ... at the same n (k carries n): against fp64, and all dropped: zeros
    got = expo_bwd(b, c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"])
    _, _, a_sum, nv = magnitudes(c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"])
    assert int(nv.sum()) == 300 - len(out)
    assert np.all(np.abs(got.astype(np.float64) - ref["g_expo"]) <= expo_bound(nv, a_sum))
    moved = dict(c, rc=c["rc"].copy(), rf=c["rf"].copy())
    moved["rc"][out] += 0.25                                                    # what a dropped ray holds does not matter
    moved["rf"][out] -= 0.25
    assert np.array_equal(bits(expo_bwd(b, moved["rc"], moved["rf"], c["tgt"], c["inds"], HW, c["table"])), bits(got))
    assert bits(expo_bwd(b, c["rc"], c["rf"], c["tgt"], none, HW, c["table"])).max() == 0


def case_many_indices_of_no_view(b):
    """256 or more indices below 0 and 256 or more at or above V hw in one batch: the indices below 0 count as "less" for every
    view in the grouping, so view 0's first slot is above 0 and the workgroups below it belong to no view; they must leave without
    reading the list (whose head the grouping never writes: the scratch starts poisoned -- NaN words, as int32 far outside the
    batch).  The gradient is held to fp64 on the rays that are left, several partials in one view among them."""
    V, n = 3, 1500
    c = draw(n, V, True, 3, 91, "any")
    rng = np.random.default_rng(5)
    where = rng.permutation(n)
    below, above = where[:300], where[300:620]
    c["inds"][below] = -1 - rng.integers(0, 1 << 40, size=len(below))
    c["inds"][above] = V * HW + rng.integers(0, 1 << 40, size=len(above))
    c["inds"][where[620:1300]] = 2 * HW + rng.integers(0, HW, size=680)          # (view 2: 680 rays, three partials)
    assert int((c["inds"] < 0).sum()) >= 256 and int((c["inds"] >= V * HW).sum()) >= 256
    ref = oracle(c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"])
    _, _, a_sum, nv = magnitudes(c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"])
    assert int(nv.sum()) == n - 620 and int(nv.min()) > 0 and int(nv[2]) > 512
    bound = expo_bound(nv, a_sum)
    assert float((np.abs(ref["g_expo"]) / bound).min()) >= 100.0                # (by the reference alone)
    got = expo_bwd(b, c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"])     # (b.empty: the scratch is NaN-filled)
    ratio = float((np.abs(got.astype(np.float64) - ref["g_expo"]) / bound).max())
    print("g_expo worst error / bound", ratio)
    assert ratio <= 1.0, ratio
    # what the dropped rays hold does not matter, and the loss treats them as the identity
    moved = c["rc"].copy()
    moved[np.concatenate([below, above])] += 0.5
    assert np.array_equal(bits(expo_bwd(b, moved, c["rf"], c["tgt"], c["inds"], HW, c["table"])), bits(got))
    lo, gc, gf = loss_views(b, c["rc"], c["rf"], c["tgt"], c["inds"], HW, c["table"])
    assert np.all(np.abs(lo.astype(np.float64) - ref["loss"])[:2] <= T.bound("tiny.loss"))
    _, gc0, _ = b.mse_loss(c["rc"], c["rf"], c["tgt"])
    drop = np.concatenate([below, above])
    assert np.array_equal(gc[drop], gc0[drop])


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def case_refusals(b):
    lib = b.lib
    raw_l, raw_b = lib._dll.nerfhip_mse_loss_views_fwd_bwd, lib._dll.nerfhip_exposure_bwd
    n, V = 8, 3
    c = draw(n, V, True, 3, 1, "any")
    rc, rf, tgt, inds, tab = (b.dev(c[k]) for k in ("rc", "rf", "tgt", "inds", "table"))
    gc, gf, lo, ge = b.empty((n, 3)), b.empty((n, 3)), b.empty((3,)), b.empty((V, 6))
    tb = lib.exposure_grad_tmp_bytes(n, V)
    tmp = b.empty((tb // 4,))
    st = b.stream()
    P_ = b.ptr

    def okl(c_=P_(rc), t=P_(tgt), ts=3, n_=n, i=P_(inds), hw=HW, x=P_(tab), v=V, lo_=P_(lo)):
        return raw_l(c_, P_(rf), t, ts, n_, 1.0, i, hw, x, v, P_(gc), P_(gf), lo_, st)
    assert okl() == 0
    bad = [okl(c_=None), okl(t=None), okl(ts=2), okl(n_=0), okl(n_=-1), okl(n_=1 << 31), okl(i=None), okl(hw=0), okl(hw=-4), okl(x=None),
           okl(v=0), okl(v=-1), okl(v=MAX_VIEWS + 1), okl(hw=(1 << 32) // 3 + 1), okl(lo_=None)]
    assert all(r == ERR_ARG for r in bad), bad
    assert lib._dll.nerfhip_last_error()

    def okb(c_=P_(rc), t=P_(tgt), ts=3, n_=n, i=P_(inds), hw=HW, x=P_(tab), v=V, tm=P_(tmp), tbytes=tb, o=P_(ge)):
        return raw_b(c_, P_(rf), t, ts, n_, 1.0, i, hw, x, v, None, tm, tbytes, o, st)
    assert okb() == 0
    bad = [okb(c_=None), okb(t=None), okb(ts=2), okb(n_=-1), okb(n_=1 << 31), okb(i=None), okb(hw=0), okb(x=None), okb(v=0),
           okb(v=MAX_VIEWS + 1), okb(hw=(1 << 32) // 3 + 1), okb(tm=None), okb(tbytes=tb - 4), okb(tbytes=0), okb(o=None)]
    assert all(r == ERR_ARG for r in bad), bad
    assert okb(tbytes=tb - 4) == ERR_ARG and b"nerfhip_exposure_grad_tmp_bytes" in lib.last_error()
    f = lib.exposure_grad_tmp_bytes
    assert f(-1, 3) == -1 and f(1 << 31, 3) == -1 and f(4, 0) == -1 and f(4, MAX_VIEWS + 1) == -1
    assert f(0, 5) == 4 * (6 * 5 + 10) and f(700, 3) == 4 * (6 * (2 + 3) + 6 + 700)
