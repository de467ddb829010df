"""Cases of the coarse-to-fine encoding window (nerfhip_plan_window_index / nerfhip_window_params / nerfhip_window_grads, include/nerfhip.h),
written once against a backend of tests/backends.py: tests/test_window.py runs them on the wave emulator, tests/test_gpu_window.py
on the product library.

The yardstick is the oracle's model (oracle/nerf_oracle.py) behind a wrapper that multiplies its ENCODED INPUT by the column weights
(`windowed`, `windowed_oracle`): that wrapper is the definition of the feature -- band k of an encoding, its six columns sin(3), cos(3)
of frequency k, times w_k(alpha) = (1 - cos(pi clamp(alpha - k, 0, 1))) / 2 evaluated in fp64 and rounded once to fp32; the
include_input columns pass.  It shares nothing with the code under test, which never touches an encoding: it multiplies weight columns.

Bounds: the table's own entries (tests/tolerances.py) -- unit.mlp_fwd, unit.mlp_bwd (with its ReLU-margin filter), unit.mlp_input_grad
for the MLP cases; the fused render is held to what tests/parity_cases.py holds the unwindowed render to (coarse maps 1e-5, fine colour
the north-star 1e-4, coarse-net gradients unit.render_grad.coarse_fp64_yardstick, fine-net gradients unit.render_grad.fine_sanity, ray
gradients the distribution test of case_ray_grad).  Everything that is a product by 0 or 1, or the elementwise kernels against numpy's
fp32 multiply, is compared on the bits.
"""
import contextlib
import ctypes as C

import numpy as np
import torch

import nerf_oracle as O
import nerf_pytorch_amd._lib as L
import parity_cases as PC
import tolerances as TL
from backends import model_cfg

GEOMETRIES = {
    "fern4x64": model_cfg(4, 64, 4, 6, 4),
    "northstar8x256_skip4": model_cfg(8, 256, 4, 10, 4),
    "L11_novw3x64_skip1": model_cfg(3, 64, 1, 11, 0, use_viewdirs=False),
    "noinput3x128_skip2": model_cfg(3, 128, 2, 5, 3, include_input_xyz=False, include_input_dir=False),
    "narrow4x40_skip2": model_cfg(4, 40, 2, 4, 2),
}
TWO_LAYER_40 = model_cfg(2, 40, 4, 4, 2)
SKIP8x128 = model_cfg(8, 128, 4, 10, 4)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def band_weights(alpha, bands):
    """w_k(alpha), k < bands: fp64, rounded once to fp32."""
    k = np.arange(bands, dtype=np.float64)
    return (0.5 * (1.0 - np.cos(np.pi * np.clip(float(alpha) - k, 0.0, 1.0)))).astype(np.float32)


def bands_of(cfg):
    return cfg["num_encoding_fn_xyz"], (cfg["num_encoding_fn_dir"] if cfg["use_viewdirs"] else 0)


def window_struct(cfg, alpha_xyz, alpha_dir):
    w = L.Window()
    lx, ld = bands_of(cfg)
    for field, vals in ((w.xyz, band_weights(alpha_xyz, lx)), (w.dir, band_weights(alpha_dir, ld))):
        for k in range(len(field)):
            field[k] = float(vals[k]) if k < len(vals) else 1.0
    return w


def lut(cfg, alpha_xyz, alpha_dir):
    """fp32[27]: the weight of every code (0: 1.0 -- never multiplied)."""
    lx, ld = bands_of(cfg)
    t = np.ones(27, np.float32)
    t[1:1 + lx] = band_weights(alpha_xyz, lx)
    t[17:17 + ld] = band_weights(alpha_dir, ld)
    return t


def column_weights(cfg, alpha_xyz, alpha_dir):
    """fp32[dim_xyz + dim_dir]: what the wrapper multiplies the encoded input by (nerf/nerf_helpers.py:130-157: [x], then per
    frequency sin(3), cos(3))."""
    lx, ld = bands_of(cfg)
    cols = []
    for inc, w in ((cfg["include_input_xyz"], band_weights(alpha_xyz, lx)), (cfg["include_input_dir"] and cfg["use_viewdirs"], band_weights(alpha_dir, ld))):
        cols += [np.ones(3 if inc else 0, np.float32), np.repeat(w, 6)]
    out = np.concatenate(cols)
    assert out.size == sum(O.model_dims(cfg))
    return out


def windowed(params, x, cfg, colw):
    """The windowed net: the oracle's forward on the encoded input times the column weights."""
    return O.mlp_forward(params, x * torch.as_tensor(colw, dtype=x.dtype), cfg)


@contextlib.contextmanager
def windowed_oracle(colw):
    """The oracle's render with every net's encoded input multiplied by the column weights (run_network calls mlp_forward)."""
    plain = O.mlp_forward
    O.mlp_forward = lambda params, x, cfg: plain(params, x * torch.as_tensor(colw, dtype=x.dtype), cfg)
    try:
        yield
    finally:
        O.mlp_forward = plain


def expected_codes(b, plan, cfg):
    """The code table restated from nerfhip_plan_tensor_info."""
    lx, ld = bands_of(cfg)
    dx, dd = O.model_dims(cfg)
    codes = np.zeros(b.lib.plan_num_params(plan), np.uint8)
    counts = {}
    for name, off, rows, cols in b.tensor_table(plan):
        if name == "layer1.weight" or (name.startswith("layers_xyz.") and name.endswith(".weight") and cols == cfg["hidden_size"] + dx):
            enc, inc, first, nb = dx, cfg["include_input_xyz"], 1, lx
        elif name == "layers_dir.0.weight":
            enc, inc, first, nb = dd, cfg["include_input_dir"], 17, ld
        else:
            continue
        t = codes[off:off + rows * cols].reshape(rows, cols)
        base = cols - enc + (3 if inc else 0)
        for k in range(nb):
            t[:, base + 6 * k:base + 6 * k + 6] = first + k
            counts[(name, first + k)] = rows * 6
    return codes, counts


# ---- the launches -----------------------------------------------------------------------------------------------------------------
def window_index(b, plan):
    t = np.full(b.lib.plan_num_params(plan), 255, np.uint8)
    b.lib.plan_window_index(plan, t.ctypes.data)
    return t


def window_params(b, flat, codes, w, keep_dev=False):
    dp, dc, out = b.dev(np.array(flat, np.float32)), b.dev(np.array(codes, np.uint8)), b.empty((flat.size,))
    b.lib.window_params(b.ptr(dp), b.ptr(dc), flat.size, C.byref(w), b.ptr(out), b.stream())
    return b.host(out)


def window_grads(b, g, codes, w):
    dg, dc = b.dev(np.array(g, np.float32)), b.dev(np.array(codes, np.uint8))
    b.lib.window_grads(b.ptr(dg), b.ptr(dc), g.size, C.byref(w), b.stream())
    return b.host(dg)


def pack_of(b, plan, flat):
    return b.pack(plan, np.ascontiguousarray(flat, np.float32))


# ---- 1: the code table ------------------------------------------------------------------------------------------------------------
def case_code_table(b, name):
    cfg = GEOMETRIES[name]
    plan = b.make_plan(cfg)
    got = window_index(b, plan)
    want, counts = expected_codes(b, plan, cfg)
    assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:8])
    lx, ld = bands_of(cfg)
    assert set(np.unique(got)) == {0} | set(range(1, 1 + lx)) | set(range(17, 17 + ld))
    for name_t, off, rows, cols in b.tensor_table(plan):
        seg = got[off:off + rows * max(cols, 1)]
        for code in np.unique(seg[seg > 0]):
            assert int((seg == code).sum()) == rows * 6 == counts[(name_t, int(code))], (name_t, code)
        if cols == 0:
            assert not seg.any(), name_t
    b.lib.plan_destroy(plan)


# ---- 2: the kernels, on the bits ----------------------------------------------------------------------------------------------------
def alphas_of(bands):
    return (-1.0, 0.0, 0.5, 1.0, 2.25, float(bands), float(bands) + 1.0)


def case_kernels_bit_exact(b):
    cfg = TWO_LAYER_40
    plan = b.make_plan(cfg)
    codes = window_index(b, plan)
    n = codes.size
    assert n % 256 != 0
    rs = np.random.RandomState(7)
    flat = rs.standard_normal(n).astype(np.float32)
    flat[::97] = 0.0
    lx, ld = bands_of(cfg)
    for ax, ad in zip(alphas_of(lx), alphas_of(ld)):
        w, t = window_struct(cfg, ax, ad), lut(cfg, ax, ad)
        want = flat * t[codes]          # numpy fp32: one IEEE multiply per entry (x * 1.0f is x)
        for m in (n, n - 1, n - 2, n - 3, 255, 3, 1):    # whole quads, every tail length, less than one workgroup, less than one quad
            got = window_params(b, flat[:m], codes[:m], w)
            assert np.array_equal(bits(got), bits(want[:m])), ("params", ax, ad, m)
            got = window_grads(b, flat[:m], codes[:m], w)
            assert np.array_equal(bits(got), bits(want[:m])), ("grads", ax, ad, m)
        closed = t[codes] == 0.0
        assert closed.any() == (ax < lx or ad < ld)
        assert not window_grads(b, flat, codes, w)[closed].any()
    # buffers that do not start on a 16-byte boundary (a net's slice of a gradient vector covering two nets): the entry-by-entry path
    w, t = window_struct(cfg, 2.25, 0.5), lut(cfg, 2.25, 0.5)
    for shift in (1, 2, 3):
        dp, dc, out = b.dev(flat), b.dev(codes), b.empty((n,))
        m = n - shift
        b.lib.window_params(b.ptr(dp) + 4 * shift, b.ptr(dc) + shift, m, C.byref(w), b.ptr(out) + 4 * shift, b.stream())
        got = b.host(out)
        assert np.array_equal(bits(got[shift:]), bits(flat[shift:] * t[codes[shift:]])) and np.isnan(got[:shift]).all(), shift
        b.lib.window_grads(b.ptr(dp) + 4 * shift, b.ptr(dc) + shift, m, C.byref(w), b.stream())
        got = b.host(dp)
        assert np.array_equal(bits(got[shift:]), bits(flat[shift:] * t[codes[shift:]])) and np.array_equal(bits(got[:shift]), bits(flat[:shift])), shift
    # a code above 26 is not a band: the entry passes
    odd = codes.copy()
    odd[:8] = [27, 255, 100, 26, 17, 16, 1, 0]
    got = window_params(b, flat, odd, w)
    t2 = np.ones(256, np.float32)
    t2[:27] = t
    assert np.array_equal(bits(got), bits(flat * t2[odd]))
    b.lib.plan_destroy(plan)


def case_refusals(b):
    raw_p, raw_g = b.lib._dll.nerfhip_window_params, b.lib._dll.nerfhip_window_grads
    w = window_struct(TWO_LAYER_40, 1.0, 1.0)
    x, c, o = b.dev(np.zeros(8, np.float32)), b.dev(np.zeros(8, np.uint8)), b.empty((8,))
    px, pc, po, st = b.ptr(x), b.ptr(c), b.ptr(o), b.stream()
    assert raw_p(px, pc, 8, C.byref(w), po, st) == 0 and raw_g(px, pc, 8, C.byref(w), st) == 0
    bad = [raw_p(None, pc, 8, C.byref(w), po, st), raw_p(px, None, 8, C.byref(w), po, st), raw_p(px, pc, 8, None, po, st),
           raw_p(px, pc, 8, C.byref(w), None, st), raw_p(px, pc, 8, C.byref(w), px, st), raw_p(px, pc, -1, C.byref(w), po, st),
           raw_g(None, pc, 8, C.byref(w), st), raw_g(px, None, 8, C.byref(w), st), raw_g(px, pc, 8, None, st), raw_g(px, pc, -1, C.byref(w), st)]
    assert all(rc == -1 for rc in bad), bad
    assert b"bad arguments" in b.lib._dll.nerfhip_last_error()
    assert raw_p(None, None, 0, None, None, st) == 0 and raw_g(None, None, 0, None, st) == 0     # (empty: nothing to launch)
    plan = b.make_plan(TWO_LAYER_40)
    assert b.lib._dll.nerfhip_plan_window_index(plan, None) == -1 and b.lib._dll.nerfhip_plan_window_index(None, None) == -1
    b.lib.plan_destroy(plan)


# ---- 3 / 4: open windows and 0 / 1 windows on the bits ----------------------------------------------------------------------------
def _setup(b, cfg, seed, precision=0):
    plan, params, flat, _ = PC.mlp_setup(b, cfg, seed=seed, precision=precision)
    return plan, params, flat, window_index(b, plan)


def case_open_window_is_no_window(b, name="narrow4x40_skip2", m=70):
    cfg = GEOMETRIES[name]
    plan, params, flat, codes = _setup(b, cfg, 51)
    lx, ld = bands_of(cfg)
    dx, dd = O.model_dims(cfg)
    gen = PC.rng(52)
    x, go = torch.randn(m, dx + dd, generator=gen).numpy(), torch.randn(m, 4, generator=gen).numpy()
    packed = pack_of(b, plan, flat)
    y0, stash = b.mlp_fwd(plan, packed, x, want_stash=True)
    g0 = b.mlp_bwd(plan, packed, go, stash)
    for ax, ad in ((lx, ld), (lx + 1.0, ld + 3.5)):
        w = window_struct(cfg, ax, ad)
        eff = window_params(b, flat, codes, w)
        assert np.array_equal(bits(eff), bits(flat))
        packed_w = pack_of(b, plan, eff)
        assert np.array_equal(bits(b.host(packed_w)), bits(b.host(packed)))
        y1, stash1 = b.mlp_fwd(plan, packed_w, x, want_stash=True)
        g1 = window_grads(b, b.mlp_bwd(plan, packed_w, go, stash1), codes, w)
        assert np.array_equal(bits(y1), bits(y0)) and np.array_equal(bits(g1), bits(g0))
    b.lib.plan_destroy(plan)


def case_integer_alpha_is_zeroed_columns(b, name="narrow4x40_skip2", m=70):
    cfg = GEOMETRIES[name]
    plan, params, flat, codes = _setup(b, cfg, 53)
    dx, dd = O.model_dims(cfg)
    x = torch.randn(m, dx + dd, generator=PC.rng(54)).numpy()
    for ax, ad in ((2.0, 1.0), (0.0, 0.0), (1.0, 2.0)):
        w, t = window_struct(cfg, ax, ad), lut(cfg, ax, ad)
        assert set(np.unique(t)) <= {0.0, 1.0}
        zeroed = flat.copy()
        zeroed[t[codes] == 0.0] = 0.0
        y_w, _ = b.mlp_fwd(plan, pack_of(b, plan, window_params(b, flat, codes, w)), x)
        y_z, _ = b.mlp_fwd(plan, pack_of(b, plan, zeroed), x)
        assert np.array_equal(bits(y_w), bits(y_z)), (ax, ad)
        # ... and it is the wrapper's net
        want = windowed({k: v.double() for k, v in params.items()}, torch.from_numpy(x).double(), cfg, column_weights(cfg, ax, ad).astype(np.float64)).numpy()
        PC.close(y_w, want, *TL.bound("unit.mlp_fwd"), what="integer alpha %s" % name)
    b.lib.plan_destroy(plan)


# ---- 5 / 6: fractional windows against the fp64 wrapper ---------------------------------------------------------------------------
FRACTIONAL = {"fern4x64": (2.6, 1.3), "skip8x128": (4.25, 2.5)}


def _cfg_of(name):
    return SKIP8x128 if name == "skip8x128" else GEOMETRIES[name]


def case_forward_fractional(b, name, precision=0, m=256):
    cfg = _cfg_of(name)
    ax, ad = FRACTIONAL[name]
    plan, params, flat, codes = _setup(b, cfg, 55, precision)
    dx, dd = O.model_dims(cfg)
    x = torch.randn(m, dx + dd, generator=PC.rng(56))
    colw = column_weights(cfg, ax, ad).astype(np.float64)
    want = windowed({k: v.double() for k, v in params.items()}, x.double(), cfg, colw).numpy()
    plain = O.mlp_forward({k: v.double() for k, v in params.items()}, x.double(), cfg).numpy()
    assert float(np.abs(want - plain).max()) > 1e-2          # (the window is not a no-op on this input)
    got, _ = b.mlp_fwd(plan, pack_of(b, plan, window_params(b, flat, codes, window_struct(cfg, ax, ad))), x.numpy())
    print("WINDOW forward %s p%d %s: max |err| %.3e" % (name, precision, b.name, float(np.abs(got - want).max())))
    PC.close(got, want, *TL.bound("unit.mlp_fwd", PC.ARITH_NAME[precision]), what="windowed mlp fwd %s p%d" % (name, precision))
    b.lib.plan_destroy(plan)


def case_backward_fractional(b, name, m=150):
    cfg = _cfg_of(name)
    ax, ad = FRACTIONAL[name]
    # (a second window with closed bands: 0 < alpha < bands on both encodings, so that some gradients must be exact zeros)
    for ax, ad in ((ax, ad), (1.5, 0.5)):
        plan, params, flat, codes = _setup(b, cfg, 57)
        dx, dd = O.model_dims(cfg)
        gen = PC.rng(58)
        x, go = torch.randn(m, dx + dd, generator=gen), torch.randn(m, 4, generator=gen)
        colw32 = column_weights(cfg, ax, ad)
        mb = TL.bound("unit.mlp_bwd")
        keep = O.mlp_relu_margin(params, x * torch.from_numpy(colw32), cfg) > mb["margin"]     # (the filter of case_mlp_backward, on the windowed net)
        x, go = x[keep].contiguous(), go[keep].contiguous()
        assert x.shape[0] >= 0.9 * m, (x.shape[0], m)
        p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
        x64 = x.double().requires_grad_(True)
        (windowed(p64, x64, cfg, colw32.astype(np.float64)) * go.double()).sum().backward()
        w, t = window_struct(cfg, ax, ad), lut(cfg, ax, ad)
        eff = window_params(b, flat, codes, w)
        packed = pack_of(b, plan, eff)
        _, stash = b.mlp_fwd(plan, packed, x.numpy(), want_stash=True)
        gflat, gx = b.mlp_bwd(plan, packed, go.numpy(), stash, flat_for_input_grad=eff)
        gflat = window_grads(b, gflat, codes, w)
        closed = t[codes] == 0.0
        assert closed.any() and not gflat[closed].any()
        worst = 0.0
        for k, g in b.unflatten(plan, gflat).items():
            ref = p64[k].grad.numpy()
            scale = float(np.abs(ref).max()) + 1e-12
            worst = max(worst, float(np.abs(g - ref).max()) / scale)
            PC.close(g, ref, mb["tol"] * scale + 1e-7, 10 * mb["tol"], what="windowed mlp bwd %s %s" % (name, k))
        ref = x64.grad.numpy()
        tol = TL.bound("unit.mlp_input_grad")
        print("WINDOW backward %s alpha (%.2f, %.2f) %s: worst parameter gradient error %.3e of max|g|, input gradient %.3e"
              % (name, ax, ad, b.name, worst, float(np.abs(gx - ref).max()) / float(np.abs(ref).max())))
        PC.close(gx, ref, tol * float(np.abs(ref).max()) + 1e-7, 10 * tol, what="windowed mlp input grad " + name)
        # the columns of a closed band carry no input gradient either: W_eff^T g is the gradient w.r.t. the UNWINDOWED encoding
        assert not gx[:, colw32 == 0.0].any()
        b.lib.plan_destroy(plan)


# ---- 7: the fused render ----------------------------------------------------------------------------------------------------------
def case_render(b, mode=None, n=48, nc=8, nf=8, seed=71):
    """render_fwd colour maps and render_bwd_rays (parameter and ray gradients) of two windowed 4 x 64 nets against the fp64 oracle
    render with wrapped models.  mode: None (the plans' dense backward) or a backward mode of backends.set_compaction."""
    cfg = GEOMETRIES["fern4x64"]
    ax, ad = FRACTIONAL["fern4x64"]
    gen = PC.rng(seed)
    pc, par_c, flat_c, codes = _setup(b, cfg, seed + 1)
    pf, par_f, flat_f, _ = _setup(b, cfg, seed + 2)
    if mode is not None:
        b.set_compaction(pc, mode), b.set_compaction(pf, mode)
    ro = torch.tensor([0.2, -0.1, 4.0]).expand(n, 3) + 0.05 * torch.randn(n, 3, generator=gen)
    rd = torch.randn(n, 3, generator=gen) * 0.3
    rd[:, 2] = -1.0
    rays = O.pack_rays(ro, rd, 2.0, 6.0, rd)
    rand = dict(t_rand=torch.rand(n, nc, generator=gen), noise_coarse=torch.randn(n, nc, generator=gen),
                u=torch.rand(n, nf, generator=gen), noise_fine=torch.randn(n, nc + nf, generator=gen))
    opt = dict(num_coarse=nc, num_fine=nf, perturb=True, lindisp=False, white_background=False, noise_std=0.0)
    tgt = torch.rand(n, 3, generator=gen)
    colw = column_weights(cfg, ax, ad)
    res = {}
    for dt in (torch.float32, torch.float64):
        r = rays.detach().to(dt).requires_grad_(True)
        qc = {k: v.detach().to(dt).requires_grad_(True) for k, v in par_c.items()}
        qf = {k: v.detach().to(dt).requires_grad_(True) for k, v in par_f.items()}
        with windowed_oracle(colw.astype(np.float64 if dt == torch.float64 else np.float32)):
            out = O.render_rays(r, qc, qf, cfg, cfg, opt, {k: v.to(dt) for k, v in rand.items()})
        loss, _, _, _ = O.loss_and_psnr(out["rgb_coarse"], out["rgb_fine"], tgt.to(dt))
        loss.backward()
        res[dt] = dict(out={k: out[k].detach().numpy() for k in ("rgb_coarse", "rgb_fine")}, g_rays=r.grad.numpy(),
                       gc={k: v.grad.numpy() for k, v in qc.items()}, gf={k: v.grad.numpy() for k, v in qf.items()})
    r32, r64 = res[torch.float32], res[torch.float64]
    w = window_struct(cfg, ax, ad)
    eff_c, eff_f = window_params(b, flat_c, codes, w), window_params(b, flat_f, codes, w)
    packed_c, packed_f = pack_of(b, pc, eff_c), pack_of(b, pf, eff_f)
    rnp = {k: v.numpy() for k, v in rand.items()}
    cot = lambda o: b.mse_loss(o["rgb_coarse"], o["rgb_fine"], tgt.numpy())[1:]  # noqa: E731
    out = b.render(pc, pf, packed_c, packed_f, rays.numpy(), opt, rnp, training=True, g_rgb=cot, ray_grad_params=(eff_c, eff_f))
    tag = "%s %s" % (mode or "dense", b.name)
    print("WINDOW render %s: rgb_coarse %.3e, rgb_fine %.3e from the fp64 wrapper" % (
        tag, float(np.abs(out["rgb_coarse"] - r64["out"]["rgb_coarse"]).max()), float(np.abs(out["rgb_fine"] - r64["out"]["rgb_fine"]).max())))
    PC.close(out["rgb_coarse"], r64["out"]["rgb_coarse"], TL.bound("e2e.coarse_maps.max"), what="windowed render rgb_coarse " + tag)
    PC.close(out["rgb_fine"], r64["out"]["rgb_fine"], TL.bound("e2e.rgb_fine")[0], what="windowed render rgb_fine " + tag)
    # parameter gradients: coarse net against the fp64 yardstick, fine net (behind the sampler) the sanity cap of the unwindowed cases
    gpc = b.unflatten(pc, window_grads(b, out["g_params_coarse"], codes, w))
    gpf = b.unflatten(pf, window_grads(b, out["g_params_fine"], codes, w))
    form = TL.bound("unit.render_grad.coarse_fp64_yardstick")
    for k, v in gpc.items():
        ref = r64["gc"][k]
        scale = float(np.abs(ref).max()) + 1e-30
        e_hip = float(np.abs(np.asarray(v, np.float64) - ref).max()) / scale
        e_t32 = float(np.abs(r32["gc"][k].astype(np.float64) - ref).max()) / scale
        assert TL.within(e_hip, e_t32, form), (tag, k, e_hip, e_t32)
    for k, v in gpf.items():
        PC.grad_close(v, r32["gf"][k], TL.bound("unit.render_grad.fine_sanity"), "windowed render grad fine %s %s" % (k, tag),
                      "window_render_%s" % tag.replace(" ", "_"), "g_params_fine")
    # ray gradients: the distribution test of parity_cases.case_ray_grad (the oracle's own fp32 run against its fp64 run is the yardstick)
    got, ref, ref64 = out["g_rays"], r32["g_rays"], r64["g_rays"]
    for lo, hi, what in ((0, 3, "origin"), (3, 6, "direction"), (8, 11, "viewdirs")):
        scale = float(np.abs(ref64[:, lo:hi]).max()) + 1e-30
        e_hip = np.abs(got[:, lo:hi] - ref[:, lo:hi]).max(axis=1) / scale
        e_yard = np.abs(ref[:, lo:hi] - ref64[:, lo:hi]).max(axis=1) / scale
        print("WINDOW render %s ray gradient %s: median %.3e (yardstick %.3e), beyond 2e-3: %d (%d)"
              % (tag, what, float(np.median(e_hip)), float(np.median(e_yard)), int((e_hip > 2e-3).sum()), int((e_yard > 2e-3).sum())))
        assert np.median(e_hip) <= 3.0 * np.median(e_yard) + 2e-6, (tag, what)
        assert (e_hip > 2e-3).sum() <= 2 * (e_yard > 2e-3).sum() + 3, (tag, what)
    assert np.all(got[:, 6:8] == 0.0)
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)
