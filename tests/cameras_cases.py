"""Cases of the camera table (nerfhip_pose_table_fwd / nerfhip_pose_table_bwd: poses[v] = base[v] Exp(xi[v]) and its VJP), written
once against a backend of tests/backends.py: tests/test_cameras.py runs them on the wave emulator, tests/test_gpu_cameras.py on the
product library.

Reference value: fp64, base64 @ torch.linalg.matrix_exp(hat4(xi64)) -- the matrix exponential of the 4 x 4 twist matrix shares no
formula with the kernel's closed form / series; gradients and Jacobians are fp64 autograd through the same expression.

Forward bound, per entry:   |poses - exact| <= C_F * 2^-24 * M,   M = |base| |Exp| evaluated on absolute values:
    M_R = |Rb| (I + |A| |W| + |B| (|w| |w|^T + x I)),   M_t = |tb| + |Rb| (I + |B| |W| + |C| (|w| |w|^T + x I)) |v|.
C_F, counted along the kernel's longest chain (csrc/dataio.hip, k_pose_table_fwd).  The kernel's arithmetic between its fp32 inputs
and its fp32 outputs runs in fp64, so an fp64 operation contributes 2^-53 and only these fp32-sized terms are left (in units of
u = 2^-24, relative to the term of M they sit on):
    x < 10 (series branch, every |w| <= pi):   the final rounding to fp32 (one rounding: at most u)                   1
    x >= 10 (closed form):  s = sin(th / 2), c = cos(th / 2) from nh_sincos (sincosf) of the fp32 head of th / 2, corrected to first
        order for the fp64 tail (the correction's own error is of second order).  sincosf is assumed good to 2 ulp = 4 u (HIP
        documents 1 ulp for sincosf; glibc's is below 1):
            A = 2 s c / th              two sincosf factors                                                             8
            B = 2 s^2 / x               two sincosf factors                                                             8
            C = (1 - A) / x             A's absolute error 8 u |A| over 1 - A, |A| <= 1 / th <= 0.32:  8 * 0.32 / 0.68  3.8
        every term of M carries at most one of A, B, C, so                                                              8
        the final rounding                                                                                              1
    fp64 dust (some 40 operations at 2^-53, also across the cancellation-free sums of M)                              < 0.5
    C_F = 10.
R^T R - I is held, per entry, to the same C_F * 2^-24 * M_R.  (The count above is not specific to the threshold: |A| <= 1 / th holds
for every x >= 10, and the head / tail split of th / 2 keeps s and c relatively accurate at any multiple of pi, so
case_forward_wrapped holds twists that wrap well past the threshold -- th up to 100, 2 pi, 2 pi +- 1e-3, 4 pi -- to the same C_F.)
A view whose twist is exactly zero gets its base bit for bit.

VJP bound, per entry:   |g_xi - g64| <= C_G * 2^-24 * sum_ij |d pose_ij / d xi_k| |g_ij|   (the TRUE Jacobian, fp64 autograd).
The kernel computes g_xi in fp64 from fp32 inputs, so
    x < 10:   the final rounding 1 (of |g_xi| <= the sum above) + fp64 dust                                              2
    x >= 10:  g_xi is linear in the six coefficients A, B, C and dA/dx = -(B - C) / 2, dB/dx = -(C - 2 c4) / 2,
        dC/dx = -(c4 - 3 c5) / 2 (c4 = (1/2 - B) / x, c5 = (1/6 - C) / x).  The closed-form rows of these tests sit within two fp32
        steps of th^2 = 10 (every other twist of the list is in the series branch), where A = -0.0066, B = 0.2, C = 0.1007,
        c4 = 0.03, c5 = 0.0066: absolute errors 0.05 u (A), 1.6 u (B), 0.005 u (C), 0.16 u (c4), 0.0005 u (c5), hence relative
        errors 8 (A), 8 (B), 0.1 (C), 16 (dA/dx = -0.0497), 8 (dB/dx = -0.0203), 16 (dC/dx = -0.0051): at most 16 u per coefficient.
        The coefficient terms of one Jacobian column do not all share a sign; their absolute sum is taken as at most 4 times the
        true |J| |g| sum (the terms are O(1) each and the right Jacobian of SO(3) has no singular value below 2 / pi up to |w| = pi,
        so a column cannot cancel to nothing):  16 * 4 = 64, + the final rounding 1 + dust                              66
    C_G = 66.
    This closed-form count covers the threshold rows only, and its factor 4 is an assumption about them, not a count: further out the
    derivative coefficients pass through zeros (dA/dx at tan th = th, th = 4.49), where no relative error per coefficient holds, so
    no C_G against the true |J| |g| is claimed for twists that wrap well past th^2 = 10; their forward is checked (above).
The test asserts C_F <= 64 and C_G <= 128.
"""
import functools

import numpy as np
import torch

import views_cases as VC

ERR_ARG = -1            # NERFHIP_ERR_ARG
U32 = 2.0 ** -24
C_F = 10
C_G = 66
SERIES_BELOW = 10.0     # csrc/dataio.hip PT_SERIES_BELOW: the threshold on th^2 = |w|^2 (as the kernel sums it, in fp64)
VIEW_COUNTS = (1, 2, 65, 300)
bits = VC.bits


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _x_of(w):
    """|w|^2 as the kernel sums it: fp64 products of the fp32 entries, left to right."""
    return (float(w[0]) * float(w[0]) + float(w[1]) * float(w[1])) + float(w[2]) * float(w[2])


def _step(w, outwards):
    """w with its largest entry moved one fp32 value away from zero (outwards = +1) or towards it (-1)."""
    out = np.array(w, dtype=np.float32)
    i = int(np.argmax(np.abs(out)))
    out[i] = np.nextafter(out[i], np.float32(outwards * np.sign(out[i]) * np.inf))
    return out


def _threshold_pair(w):
    """w (fp32, |w|^2 just below the threshold): moves its largest entry outwards one fp32 value at a time until |w|^2 crosses the
    threshold; returns the last twist below and the first one at or above -- fp32 neighbours either side of the branch."""
    w = np.array(w, dtype=np.float32)
    assert _x_of(w) < SERIES_BELOW
    for _ in range(100000):
        up = _step(w, +1)
        if _x_of(up) >= SERIES_BELOW:
            return w, up
        w = up
    raise AssertionError("the start is too far below the threshold")


def twists(V, seed=5):
    """(V, 6) fp32 twists [w, v], translation parts of size ~1.  The first rows are the special angles (V = 1, 2 take the first one /
    two: th = 0 with v != 0, and th = pi - 1e-3); the rest are angles uniform in (0, pi) about random axes."""
    rng = np.random.default_rng(seed)

    def axis():
        a = rng.normal(size=3)
        return a / np.linalg.norm(a)

    def v():
        return rng.normal(size=3)

    root = np.sqrt(SERIES_BELOW)
    lo, hi = _threshold_pair(np.float32((root * (1.0 - 2e-6)) * axis()))
    alo, ahi = _threshold_pair(np.float32([root * (1.0 - 2e-6), 0.0, 0.0]))
    rows = [
        np.concatenate([np.zeros(3), v()]),                          # th = 0 exactly, v != 0
        np.concatenate([(np.pi - 1e-3) * axis(), v()]),              # th = pi - 1e-3
        np.concatenate([1e-8 * axis(), v()]),
        np.zeros(6),                                                 # w = 0 and v = 0
        np.concatenate([lo, v()]), np.concatenate([hi, v()]),        # the fp32 neighbours either side of the series threshold ...
        np.concatenate([_step(lo, -1), v()]), np.concatenate([_step(hi, +1), v()]),   # ... and the next ones out
        np.concatenate([1e-4 * axis(), v()]),
        np.concatenate([1e-2 * axis(), v()]),
        np.concatenate([0.3 * axis(), v()]),
        np.concatenate([3.0 * axis(), v()]),
        np.concatenate([alo, v()]), np.concatenate([ahi, v()]),      # the threshold again, w along one axis (most Jacobian entries 0)
        np.concatenate([[0.0, 0.0, np.pi - 1e-3], v()]),             # th = pi - 1e-3 along one axis: R's off-diagonal A-terms ~ 1e-3
        np.concatenate([[0.0, 1e-8, 0.0], np.zeros(3)]),             # th = 1e-8, v = 0
    ]
    while len(rows) < V:
        rows.append(np.concatenate([rng.uniform(0.0, np.pi) * axis(), v()]))
    xi = np.ascontiguousarray(np.stack(rows[:V]), dtype=np.float32)
    if V >= 16:
        x = np.array([_x_of(r) for r in xi])
        assert (x[[4, 6, 12]] < SERIES_BELOW).all() and (x[[5, 7, 13]] >= SERIES_BELOW).all()
        assert not xi[3].any() and not xi[0, :3].any() and xi[0, 3:].all()
    return xi


def hat4(xi):
    """(V, 4, 4) twist matrices [[hat(w), v], [0, 0]] of (V, 6) twists (torch, differentiable)."""
    w0, w1, w2, v0, v1, v2 = xi.unbind(-1)
    z = torch.zeros_like(w0)
    return torch.stack([torch.stack([z, -w2, w1, v0], -1), torch.stack([w2, z, -w0, v1], -1), torch.stack([-w1, w0, z, v2], -1),
                        torch.stack([z, z, z, z], -1)], -2)


def exact_poses(base64, xi64):
    """(V, 3, 4) fp64: base @ expm(hat4(xi)), base the (V, 3, 4) blocks completed by the row 0 0 0 1."""
    V = xi64.shape[0]
    b4 = torch.zeros(V, 4, 4, dtype=torch.float64)
    b4[:, :3, :4] = base64
    b4[:, 3, 3] = 1.0
    return (b4 @ torch.linalg.matrix_exp(hat4(xi64)))[:, :3, :4]


def _abc(x):
    """A, B, C of th^2 = x in fp64 (series below 1e-4; the closed forms lose at most 1e-8 of themselves above)."""
    x = np.asarray(x, dtype=np.float64)
    th = np.sqrt(np.maximum(x, 1e-300))
    small = x < 1e-4
    a = np.where(small, 1 - x / 6 + x * x / 120, np.sin(th) / th)
    b = np.where(small, 0.5 - x / 24 + x * x / 720, (1 - np.cos(th)) / np.maximum(x, 1e-300))
    c = np.where(small, 1 / 6 - x / 120 + x * x / 5040, (th - np.sin(th)) / np.maximum(x, 1e-300) / th)
    return a, b, c


def magnitude(base64, xi64):
    """M (V, 3, 4): base @ Exp(xi) evaluated on absolute values, subtractions taken as additions (the module docstring)."""
    base64, xi64 = np.asarray(base64), np.asarray(xi64)
    w, v = np.abs(xi64[:, :3]), np.abs(xi64[:, 3:])
    x = (xi64[:, :3] ** 2).sum(-1)
    a, b, c = (np.abs(t)[:, None, None] for t in _abc(x))
    eye = np.eye(3)[None]
    aw = np.zeros((len(x), 3, 3))
    aw[:, 0, 1] = aw[:, 1, 0] = w[:, 2]
    aw[:, 0, 2] = aw[:, 2, 0] = w[:, 1]
    aw[:, 1, 2] = aw[:, 2, 1] = w[:, 0]
    w2 = w[:, :, None] * w[:, None, :] + x[:, None, None] * eye
    rb = np.abs(base64[:, :, :3])
    m = np.empty((len(x), 3, 4))
    m[:, :, :3] = rb @ (eye + a * aw + b * w2)
    m[:, :, 3] = np.abs(base64[:, :, 3]) + (rb @ ((eye + b * aw + c * w2) @ v[:, :, None]))[:, :, 0]
    return m


@functools.lru_cache(maxsize=None)
def reference(V):
    """Inputs and fp64 references of a table of V views, computed once and shared (read-only) by the cases: base poses (V, 4, 4)
    fp32, twists, cotangents N(0, 1), exact poses, M, the exact g_xi and sum_ij |J_ijk| |g_ij|."""
    base = np.stack([VC.pose(60 + v) for v in range(V)])
    xi = twists(V)
    g = np.random.default_rng(17).normal(size=(V, 3, 4)).astype(np.float32)
    b64 = torch.from_numpy(base[:, :3, :4].astype(np.float64))
    x64 = torch.from_numpy(xi.astype(np.float64)).requires_grad_(True)
    g64 = torch.from_numpy(g.astype(np.float64))
    want = exact_poses(b64, x64)
    (want * g64).sum().backward()
    # pose[v] depends on xi[v] alone: the Jacobian of the sum over views holds every view's own 12 x 6 block
    jac = torch.autograd.functional.jacobian(lambda t: exact_poses(b64, t).sum(0), x64.detach())   # (3, 4, V, 6)
    jmag = (jac.abs() * g64.abs().permute(1, 2, 0)[..., None]).sum((0, 1)).numpy()
    out = dict(base=base, xi=xi, g=g, want=want.detach().numpy(), M=magnitude(b64.numpy(), xi.astype(np.float64)),
               g_xi=x64.grad.numpy(), jmag=jmag)
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- the launches ---------------------------------------------------------------------------------------------------------------
def table_fwd(b, xi, table, vstride, ld, V):
    dx, dt, out = b.dev(np.array(xi)), b.dev(np.array(table)), b.empty((V, 3, 4))   # (copies: the shared reference stays read-only)
    b.lib.pose_table_fwd(b.ptr(dx), b.ptr(dt), vstride, ld, V, b.ptr(out), b.stream())
    return b.host(out)


def table_bwd(b, xi, table, vstride, ld, V, g, active=None):
    dx, dt, dg, out = b.dev(np.array(xi)), b.dev(np.array(table)), b.dev(np.array(g)), b.empty((V, 6))
    da = None if active is None else b.dev(np.ascontiguousarray(active, dtype=np.uint8))
    b.lib.pose_table_bwd(b.ptr(dx), b.ptr(dt), vstride, ld, V, b.ptr(dg), b.p(da), b.ptr(out), b.stream())
    return b.host(out)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def case_forward(b, V, layout="4x4"):
    assert C_F <= 64
    r = reference(V)
    table, vs, ld = VC.pose_table(r["base"], layout)
    got = table_fwd(b, r["xi"], table, vs, ld, V)
    assert got.shape == (V, 3, 4) and got.dtype == np.float32 and np.all(np.isfinite(got))
    err, bound = np.abs(got.astype(np.float64) - r["want"]), C_F * U32 * r["M"]
    worst = float((err / bound).max())
    print("CAMERAS forward V=%d %s %s: worst |err| / (C_F u M) = %.3f (C_F = %d)" % (V, layout, b.name, worst, C_F))
    assert np.all(err <= bound), (V, worst, int(np.argmax((err / bound).reshape(V, -1).max(1))))
    # R^T R - I: within the same per-entry bound
    R = got[:, :, :3].astype(np.float64)
    defect = np.abs(np.transpose(R, (0, 2, 1)) @ R - np.eye(3)[None])
    assert np.all(defect <= bound[:, :, :3]), (V, float((defect / bound[:, :, :3]).max()))
    # a zero twist: the base, bit for bit
    zero = np.nonzero(~r["xi"].any(1))[0]
    assert V < 16 or len(zero) == 1
    for v in zero:
        assert np.array_equal(bits(got[v]), bits(r["base"][v][:3, :4])), v


def case_forward_wrapped(b):
    """Twists that wrap round, well inside the closed-form branch: the forward bound with the same C_F (module docstring)."""
    rng = np.random.default_rng(23)
    thetas = [3.2, 4.49, 5.0, 2 * np.pi - 1e-3, 2 * np.pi, 2 * np.pi + 1e-3, 9.0, 4 * np.pi, 20.0, 100.0]
    rows = []
    for k, th in enumerate(thetas):
        a = rng.normal(size=3) if k % 3 else np.eye(3)[k % 3 if k < 3 else (k // 3) % 3]
        rows.append(np.concatenate([th * a / np.linalg.norm(a), rng.normal(size=3)]))
    xi = np.ascontiguousarray(np.stack(rows), dtype=np.float32)
    V = len(xi)
    assert all(_x_of(r) >= SERIES_BELOW for r in xi)
    base = np.stack([VC.pose(90 + v) for v in range(V)])
    b64 = base[:, :3, :4].astype(np.float64)
    want = exact_poses(torch.from_numpy(b64), torch.from_numpy(xi.astype(np.float64))).numpy()
    got = table_fwd(b, xi, base, 16, 4, V)
    err, bound = np.abs(got.astype(np.float64) - want), C_F * U32 * magnitude(b64, xi.astype(np.float64))
    print("CAMERAS forward wrapped %s: worst |err| / (C_F u M) = %.3f (C_F = %d)" % (b.name, float((err / bound).max()), C_F))
    assert np.all(np.isfinite(got)) and np.all(err <= bound), float((err / bound).max())


def case_vjp(b, V, layout="4x4"):
    assert C_G <= 128
    r = reference(V)
    table, vs, ld = VC.pose_table(r["base"], layout)
    got = table_bwd(b, r["xi"], table, vs, ld, V, r["g"])
    assert got.shape == (V, 6) and np.all(np.isfinite(got))   # (th = 0 and th = 1e-8 included: no NaN)
    err = np.abs(got.astype(np.float64) - r["g_xi"])
    assert np.all(r["jmag"] > 0)
    ratio = err / (U32 * r["jmag"])
    closed = np.array([_x_of(row) >= SERIES_BELOW for row in r["xi"]])
    print("CAMERAS vjp V=%d %s %s: worst |err| / (u sum |J| |g|) = %.3f in the series branch, %.3f in the closed form (C_G = %d)"
          % (V, layout, b.name, float(ratio[~closed].max()), float(ratio[closed].max()) if closed.any() else 0.0, C_G))
    assert np.all(ratio <= C_G), (V, float(ratio.max()), int(np.argmax(ratio.max(1))))


def case_active(b):
    """Inactive views: exact zeros (their g_poses rows, NaN here, are not read); the others: the bits of the unmasked call."""
    V = 65
    r = reference(V)
    table, vs, ld = VC.pose_table(r["base"], "4x4")
    full = table_bwd(b, r["xi"], table, vs, ld, V, r["g"])
    active = np.random.default_rng(3).random(V) < 0.6
    active[[0, 64]] = [False, True]
    g = r["g"].copy()
    g[~active] = np.nan
    got = table_bwd(b, r["xi"], table, vs, ld, V, g, active)
    assert np.array_equal(bits(got[~active]), np.zeros((int((~active).sum()), 6), np.uint32))
    assert np.array_equal(bits(got[active]), bits(full[active]))
    all_on = table_bwd(b, r["xi"], table, vs, ld, V, r["g"], np.ones(V, np.uint8))
    assert np.array_equal(bits(all_on), bits(full))


def case_refusals(b):
    lib = b.lib
    V = 3
    raw_f, raw_b = lib._dll.nerfhip_pose_table_fwd, lib._dll.nerfhip_pose_table_bwd
    xi, base = b.dev(np.zeros((V, 6), np.float32)), b.dev(np.stack([np.eye(4, dtype=np.float32)] * V))
    poses, g, gx = b.empty((V, 3, 4)), b.dev(np.zeros((V, 3, 4), np.float32)), b.empty((V, 6))
    px, pb, pp, pg, pgx, st = b.ptr(xi), b.ptr(base), b.ptr(poses), b.ptr(g), b.ptr(gx), b.stream()
    okf = lambda x=px, bb=pb, vs=16, ld=4, v=V, o=pp: raw_f(x, bb, vs, ld, v, o, st)  # noqa: E731
    assert okf() == 0
    bad = [okf(v=0), okf(v=VC.L_MAX_VIEWS + 1), okf(ld=3), okf(vs=11), okf(vs=13, ld=5), okf(x=None), okf(bb=None), okf(o=None)]
    assert all(rc == ERR_ARG for rc in bad), bad
    assert lib._dll.nerfhip_last_error()
    okb = lambda x=px, bb=pb, vs=16, ld=4, v=V, gg=pg, o=pgx: raw_b(x, bb, vs, ld, v, gg, None, o, st)  # noqa: E731
    assert okb() == 0
    bad = [okb(v=0), okb(v=VC.L_MAX_VIEWS + 1), okb(ld=3), okb(vs=11), okb(vs=13, ld=5), okb(x=None), okb(bb=None), okb(gg=None),
           okb(o=None)]
    assert all(rc == ERR_ARG for rc in bad), bad
    assert lib._dll.nerfhip_last_error()
    assert okf(v=1, vs=0) == 0   # (one view: the view stride is not read)
