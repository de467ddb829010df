"""Parity cases shared by the emulator suite (CPU, `-m "not gpu"`) and the GPU suite (`-m gpu`).

Each case feeds identical seeded inputs (and identical random draws) to a backend (tests/backends.py) and to the
oracle (oracle/nerf_oracle.py, pinned against the real reference by tests/test_oracle.py), and compares.

Tolerances (fp32): elementwise geometry is bit-exact or within 1 ulp; anything through sin/cos/exp within 2e-6;
MLP outputs within 2e-5 (different fp32 summation order than torch's GEMM); rendered rgb/depth within 1e-4 abs (the
north-star bar, BASELINE.json); inverse-CDF indices exact for a given (cdf, u).
"""
import ast
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import nerf_oracle as O
import nerf_pytorch_amd._lib as L
import tolerances as TL
from backends import ROOT, model_cfg
from conftest import gold


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def close(a, b, atol, rtol=0.0, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what + ": NaN masks differ"
    err = np.abs(np.nan_to_num(a) - np.nan_to_num(b))
    lim = atol + rtol * np.abs(np.nan_to_num(b))
    assert np.all(err <= lim), "%s: max err %.3e (limit %.3e)" % (what, float(err.max()), float(lim.flat[err.argmax()]))


def rng(seed):
    return torch.Generator().manual_seed(seed)


# measured quantities the cases want on record next to their bounds (the GPU session writes them to
# gpurun_out/parity_small_cases.json -> profiles/): {case: {quantity: value}}
RECORD = {}


def note(case, **kv):
    RECORD.setdefault(case, {}).update({k: (float(v) if not isinstance(v, (int, str)) else v) for k, v in kv.items()})


def grad_close(got, ref, max_rel, what, case, key):
    """Gradient tensor against the reference's: |got - ref| <= max_rel * max|ref| (+ 5e-4 |ref| elementwise); the
    measured worst ratio goes on record."""
    scale = float(np.abs(ref).max()) + 1e-12
    worst = float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max()) / scale
    prev = RECORD.get(case, {}).get(key, 0.0)
    note(case, **{key: max(prev, worst)})
    close(got, ref, max_rel * scale + 1e-9, 5e-4, what=what)


# ---- geometry ----------------------------------------------------------------------------------------------------------
def case_rays(b):
    g = gold("helpers.npz")
    ro, rd = b.ray_bundle(5, 7, 3.3, g["rb_c2w"])
    close(rd.reshape(5, 7, 3), g["rb_rd"], 1e-6, what="ray_bundle rd")
    close(ro.reshape(5, 7, 3), g["rb_ro"], 0, what="ray_bundle ro")
    pix = np.array([0, 3, 319, 160, 7], np.int64)
    ro2, rd2 = b.ray_bundle(20, 16, 555.5555 / 20, g["rb2_c2w"], pix)
    close(rd2, g["rb2_rd"].reshape(-1, 3)[pix], 1e-6, what="ray_bundle pixels")
    no, nd = b.ndc_rays(378, 504, 407.5, 1.0, g["ndc_o"], g["ndc_d"])
    close(no, g["ndc_out_o"], 1e-6, 1e-6, what="ndc o")
    close(nd, g["ndc_out_d"], 1e-6, 1e-6, what="ndc d")
    rays = b.pack_rays(g["ndc_o"], g["ndc_d"], 2.0, 6.0, g["ndc_d"])
    want = O.pack_rays(T(g["ndc_o"]), T(g["ndc_d"]), 2.0, 6.0, T(g["ndc_d"])).numpy()
    close(rays, want, 1e-7, what="pack_rays")
    rays8 = b.pack_rays(g["ndc_o"], g["ndc_d"], 0.0, 1.0, None)
    close(rays8, O.pack_rays(T(g["ndc_o"]), T(g["ndc_d"]), 0.0, 1.0, None).numpy(), 0, what="pack_rays (no viewdirs)")


def case_posenc(b):
    g = gold("helpers.npz")
    x = g["pe_x"]
    close(b.positional_encoding(x, O.frequency_bands(10).numpy(), True), g["pe_L10"], 2e-6, what="posenc L10")
    close(b.positional_encoding(x, O.frequency_bands(4).numpy(), True), g["pe_L4"], 2e-6, what="posenc L4")
    close(b.positional_encoding(x, O.frequency_bands(6).numpy(), False), g["pe_L6_noinput"], 2e-6, what="posenc noinput")
    close(b.positional_encoding(x, O.frequency_bands(3, False).numpy(), True), g["pe_L3_linear"], 2e-6, what="posenc lin")
    close(b.positional_encoding(x, np.zeros(0, np.float32), True), g["pe_L0"], 0, what="posenc L0")


def case_stratified(b):
    gen = rng(3)
    n, nc = 7, 64
    rays = torch.zeros(n, 11)
    rays[:, 6] = 2.0 + torch.rand(n, generator=gen)
    rays[:, 7] = 6.0 + torch.rand(n, generator=gen)
    tr = torch.rand(n, nc, generator=gen)
    tv = torch.linspace(0, 1, nc).numpy()
    for lindisp in (False, True):
        for perturb in (False, True):
            want = O.stratified_z(rays[:, 6:7], rays[:, 7:8], nc, lindisp, perturb, tr).numpy()
            got = b.stratified_z(rays.numpy(), tv, lindisp, perturb, tr.numpy() if perturb else None)
            close(got, want, 0, what="stratified lindisp=%s perturb=%s" % (lindisp, perturb))
    # production RNG: the kernel's own draws are the ones rng_fill reports (stream 0, element = ray*nc + s)
    draws = b.rng_fill(0, 99, 0, 5 * nc, n * nc).reshape(n, nc)
    assert draws.min() >= 0.0 and draws.max() < 1.0
    got = b.stratified_z(rays.numpy(), tv, False, True, None, seed=99, ray_offset=5)
    want = O.stratified_z(rays[:, 6:7], rays[:, 7:8], nc, False, True, T(draws)).numpy()
    close(got, want, 0, what="stratified internal rng")


def case_cumprod(b):
    g = gold("helpers.npz")
    close(b.cumprod_exclusive(g["cp_x"]), g["cp_y"], 0, 2e-7, what="cumprod_exclusive")
    close(b.cumprod_exclusive(np.array([[1, 2, 3, 4]], np.float32)), [[1, 1, 2, 6]], 0, what="KAT1")
    x = (torch.rand(3, 200, generator=rng(5)) * 0.2 + 0.9).numpy()
    close(b.cumprod_exclusive(x), O.cumprod_exclusive(T(x)).numpy(), 0, 2e-7, what="cumprod 200")


# ---- compositing -------------------------------------------------------------------------------------------------------
def case_volume_render(b):
    g = gold("helpers.npz")
    names = ("rgb", "disp", "acc", "weights", "depth")
    r1 = b.volume_render_fwd(g["vr_raw"], g["vr_z"], g["vr_rd"], 0.7, g["vr_noise"], True)
    r2 = b.volume_render_fwd(g["vr_raw"], g["vr_z"], g["vr_rd"], 0.0, None, False)
    for i, n in enumerate(names):
        close(r1[i], g["vr1_" + n], 2e-6, 2e-6, what="render1 " + n)
        close(r2[i], g["vr2_" + n], 2e-6, 2e-6, what="render2 " + n)
    r3 = b.volume_render_fwd(g["vr3_raw"], g["vr_z"], g["vr_rd"])
    close(r3[1], g["vr3_disp"], 2e-6, 2e-6, what="NaN disparity")  # NaN mask must match
    raw = np.array([[[0., 0, 0, 1], [1, -1, 2, .5], [0, 0, 0, -1], [3, 3, 3, 2]]], np.float32)
    k = b.volume_render_fwd(raw, np.array([[2., 3, 4, 6]], np.float32), np.array([[0., 0, -2]], np.float32), white=True)
    close(k[3], [[0.8646647, 0.0855482, 0, 0.0497871]], 1e-6, what="KAT4 weights")
    close(k[0], [[0.5422990, 0.5027657, 0.5551088]], 1e-6, what="KAT4 rgb")
    close(k[4], [2.2846966], 1e-6, what="KAT4 depth")
    close(k[1], [0.4376949], 1e-6, what="KAT4 disp")
    # 192 samples (3 chunks of 64) incl. ray stride 11 as the fused path passes it
    gen = rng(8)
    n, s = 5, 192
    raw = (torch.randn(n, s, 4, generator=gen) * 1.5)
    z = torch.sort(torch.rand(n, s, generator=gen) * 4 + 2, -1)[0]
    rays = torch.randn(n, 11, generator=gen)
    nz = torch.randn(n, s, generator=gen)
    want = O.volume_render(raw, z, rays[:, 3:6], 0.2, nz, False)
    got = b.volume_render_fwd(raw.numpy(), z.numpy(), rays.numpy()[:, 3:], 0.2, nz.numpy(), False)
    for i, nme in enumerate(names):
        close(got[i], want[i].numpy(), 2e-6, 2e-6, what="render192 " + nme)


def case_volume_render_bwd(b):
    gen = rng(9)
    for (n, s, white, std) in ((4, 64, False, 0.0), (3, 192, True, 0.5), (2, 40, True, 0.0)):
        raw = (torch.randn(n, s, 4, generator=gen) * 1.5).requires_grad_(True)
        z = torch.sort(torch.rand(n, s, generator=gen) * 4 + 2, -1)[0]
        rd = torch.randn(n, 3, generator=gen)
        nz = torch.randn(n, s, generator=gen)
        g_rgb, g_depth, g_acc = torch.randn(n, 3, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        g_w = torch.randn(n, s, generator=gen)
        rgb, disp, acc, w, depth = O.volume_render(raw, z, rd, std, nz, white)
        ((rgb * g_rgb).sum() + (depth * g_depth).sum() + (acc * g_acc).sum() + (w * g_w).sum()).backward()
        got = b.volume_render_bwd(raw.detach().numpy(), z.numpy(), rd.numpy(), g_rgb.numpy(), g_depth.numpy(),
                                  g_acc.numpy(), g_w.numpy(), std, nz.numpy(), white)
        close(got, raw.grad.numpy(), 2e-6, 2e-4, what="render bwd n=%d s=%d" % (n, s))
        raw.grad = None
        rgb = O.volume_render(raw, z, rd, std, nz, white)[0]
        (rgb * g_rgb).sum().backward()
        got = b.volume_render_bwd(raw.detach().numpy(), z.numpy(), rd.numpy(), g_rgb.numpy(), None, None, None, std,
                                  nz.numpy(), white)
        close(got, raw.grad.numpy(), 2e-6, 2e-4, what="render bwd (rgb only)")


# ---- sampling ----------------------------------------------------------------------------------------------------------
_C_ORACLE = None


def c_oracle():
    global _C_ORACLE
    if _C_ORACLE is None:
        out = os.path.join(ROOT, "oracle", "_build")
        os.makedirs(out, exist_ok=True)
        so = os.path.join(out, "libcdf_oracle.so")
        src = os.path.join(ROOT, "oracle", "cdf_oracle.c")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
        _C_ORACLE = C.CDLL(so)
    return _C_ORACLE


def run_c_oracle(bins, w, u):
    n, nb = bins.shape
    nf = u.shape[1]
    s, i, c = np.empty((n, nf), np.float32), np.empty((n, nf), np.int64), np.empty((n, nb), np.float32)
    bins, w, u = (np.ascontiguousarray(a, np.float32) for a in (bins, w, u))
    c_oracle().oracle_sample_pdf(C.c_void_p(bins.ctypes.data), C.c_void_p(w.ctypes.data), C.c_int64(n), C.c_int(nb),
                                 C.c_void_p(u.ctypes.data), C.c_int(nf), C.c_void_p(s.ctypes.data),
                                 C.c_void_p(i.ctypes.data), C.c_void_p(c.ctypes.data))
    return s, i, c


def case_sample_pdf(b):
    g = gold("helpers.npz")
    bins, w, u = g["sp_bins"], g["sp_w"], g["sp_u"]
    s, inds, cdf = b.sample_pdf(bins, w, 128, u=u)
    # (1) the declared-order contract: kernel == C restatement, bit for bit
    cs, ci, cc = run_c_oracle(bins, w, u)
    assert np.array_equal(cdf, cc), "cdf differs from the C restatement"
    assert np.array_equal(inds, ci), "searchsorted indices differ from the C restatement"
    assert np.array_equal(s, cs), "samples differ from the C restatement"
    # (2) indices are exactly torch.searchsorted(right=True) of the kernel's own cdf
    ti = torch.searchsorted(T(cdf), T(u), right=True).numpy()
    assert np.array_equal(inds, ti)
    # (3) vs the reference: identical except where a 1-ulp cdf difference flips an index
    _, oi, oc = O.sample_pdf(T(bins), T(w), 128, u=T(u), return_aux=True)
    close(cdf, oc.numpy(), 2.5e-7, what="cdf vs torch")
    # Measured: 0 flipped indices of 1,408 here and 0 of 524,288 on a 4096-ray batch (test_gpu_fullsize.py), although 41 %
    # of the CDF entries differ from torch's by one ulp (torch.sum's vectorised fp32 cascade vs the declared sequential
    # order): a flip needs u within an ulp of a CDF entry, ~4e-6 per index and ulp.  The kernel equals the C
    # restatement bit for bit, so this count is deterministic: none is allowed.
    nflip = int((inds != oi.numpy()).sum())
    note("sample_pdf_golden_%s" % b.name, indices=int(inds.size), flipped_vs_torch=nflip,
         cdf_entries_differing_from_torch=float((cdf != oc.numpy()).mean()), cdf_max_abs_diff=float(np.abs(cdf - oc.numpy()).max()))
    assert nflip == 0, nflip
    same = inds == oi.numpy()
    close(s[same], g["sp_rand"][same], 1e-5, what="samples vs reference")
    sd, _, _ = b.sample_pdf(bins, w, 128, det=True)
    close(sd, g["sp_det"], 1e-5, what="det samples vs reference")
    k, ki, _ = b.sample_pdf(np.array([[1, 2, 3, 4]], np.float32), np.array([[1, 0, 3]], np.float32), 5, det=True)
    close(k, [[1.0, 1.9999975, 3.3333306, 3.6666653, 4.0]], 1e-6, what="KAT5")
    assert ki[0, -1] == 4  # u = 1.0 lands past the last cdf entry
    # KAT8 tie behaviour through the kernel: cdf [0,.2,.2,.7,1] <- weights chosen so that pdf reproduces it
    gen = rng(21)
    z = torch.sort(torch.rand(6, 64, generator=gen) * 4 + 2, -1)[0]
    wf = torch.rand(6, 64, generator=gen) ** 3
    uu = torch.rand(6, 128, generator=gen)
    zs_want, zf_want = O.hierarchical_z(z, wf, 128, det=False, u=uu)
    zs, zf = b.hierarchical_z(z.numpy(), wf.numpy(), 128, u=uu.numpy())
    assert np.all(np.diff(zf, axis=-1) >= 0), "z_fine not sorted"
    close(zs, zs_want.numpy(), 1e-5, what="hierarchical samples")
    close(zf, zf_want.numpy(), 1e-5, what="hierarchical merged")
    zs2, zf2 = b.hierarchical_z(z.numpy(), wf.numpy(), 64, det=True)
    zs_w2, zf_w2 = O.hierarchical_z(z, wf, 64, det=True)
    close(zf2, zf_w2.numpy(), 1e-5, what="hierarchical det")


# ---- MLP ---------------------------------------------------------------------------------------------------------------
def mlp_setup(b, cfg, seed, precision=0, w_gain=1.0):
    plan = b.make_plan(cfg, precision)
    params = O.init_params(cfg, seed=seed)
    if w_gain != 1.0:  # (weights w_gain times torch's default init: activations and gradients grow by that factor per layer)
        params = {k: (v * w_gain if k.endswith("weight") else v) for k, v in params.items()}
    flat = b.flatten_params(plan, {k: v.numpy() for k, v in params.items()})
    packed = b.pack(plan, flat)
    return plan, params, flat, packed


def case_ndc_rays_bwd(b, n=300):
    """nerfhip_ndc_rays_bwd against autograd through the oracle's ndc_rays (nerf/nerf_helpers.py:170-197), fp32 and fp64."""
    gen = rng(77)
    H, W, focal = 378, 504, 407.5
    ro = (torch.tensor([0.1, -0.2, 0.3]).expand(n, 3) + 0.2 * torch.randn(n, 3, generator=gen)).contiguous()
    rd = torch.randn(n, 3, generator=gen) * 0.4
    rd[:, 2] = -1.0 - 0.3 * torch.rand(n, generator=gen)
    g_oo, g_od = torch.randn(n, 3, generator=gen), torch.randn(n, 3, generator=gen)
    res = {}
    for dt in (torch.float32, torch.float64):
        o, d = ro.detach().clone().to(dt).requires_grad_(True), rd.detach().clone().to(dt).requires_grad_(True)
        oo, od = O.ndc_rays(H, W, focal, 1.0, o, d)
        ((oo * g_oo.to(dt)).sum() + (od * g_od.to(dt)).sum()).backward()
        res[dt] = (o.grad.double().numpy(), d.grad.double().numpy())
    got = b.ndc_rays_bwd(H, W, focal, 1.0, ro.numpy(), rd.numpy(), g_oo.numpy(), g_od.numpy())
    for name, g, r32, r64 in zip(("g_rays_o", "g_rays_d"), got, res[torch.float32], res[torch.float64]):
        scale = np.abs(r64).max(axis=1, keepdims=True) + 1e-30
        e_hip, e_ref = float((np.abs(g - r64) / scale).max()), float((np.abs(r32 - r64) / scale).max())
        note("ndc_rays_bwd_%s" % b.name, **{name + "_hip_vs_fp64": e_hip, name + "_oracle_fp32_vs_fp64": e_ref})
        assert e_hip <= 4.0 * e_ref + 2e-6, (name, e_hip, e_ref)
    # empty input
    z = np.zeros((0, 3), np.float32)
    assert b.ndc_rays_bwd(H, W, focal, 1.0, z, z, z, z)[0].shape == (0, 3)


MLP_GEOMETRIES = {
    "default4x128": model_cfg(4, 128, 4, 10, 4),
    "deep8x128_skip4": model_cfg(8, 128, 4, 10, 4),
    "fern8x128_skip3_L6": model_cfg(8, 128, 3, 6, 4),
    "novw4x128": model_cfg(4, 128, 4, 10, 4, use_viewdirs=False),
    "two_layer_L4_L2": model_cfg(2, 128, 4, 4, 2),
    "one_layer": model_cfg(1, 128, 4, 10, 4),
    "one_layer_novw_256": model_cfg(1, 256, 4, 3, 0, use_viewdirs=False),
    "sixteen_layers_skip5": model_cfg(16, 128, 5, 10, 4),
    "skip_every_layer_256": model_cfg(3, 256, 1, 2, 1),
    # 35 weight-gradient jobs: the job tables of wgrad.hip used to hold 32
    "sixteen_layers_skip1": model_cfg(16, 128, 1, 10, 4),
    "twenty_layers_skip7": model_cfg(20, 128, 7, 6, 2),
    "noinput_linear": model_cfg(3, 128, 2, 5, 3, include_input_xyz=False, include_input_dir=False,
                                log_sampling_xyz=False),
    "northstar8x256": model_cfg(8, 256, 4, 10, 4),
    # the 64-wide kernel instances: config/llff.yml:49,74 and pretrained/{fern,hotdog}-lowres/config.yml:19,31
    "llff4x64_skip3_L6": model_cfg(4, 64, 3, 6, 4),
    "deep8x64_skip4": model_cfg(8, 64, 4, 10, 4),
    "novw3x64_skip1": model_cfg(3, 64, 1, 10, 0, use_viewdirs=False),
    "one_layer_64": model_cfg(1, 64, 4, 4, 2),
    # ... and the other instantiations of the fused backward of 64-wide nets (csrc/mlp64r.hip: one kernel per layer count 1..4)
    "two_layer_64": model_cfg(2, 64, 4, 10, 4),
    "three_layer_48": model_cfg(3, 48, 4, 6, 2),
    # hidden_size in (256, 512]: the 512-wide instances (one wave per SIMD, accumulators in AGPRs), split weight-gradient jobs
    "wide3x512_skip2": model_cfg(3, 512, 2, 10, 4),
    "wide2x320": model_cfg(2, 320, 4, 6, 2),
    "novw2x512": model_cfg(2, 512, 4, 4, 0, use_viewdirs=False),
    # other hidden sizes ride zero-padded on the next kernel width (plan.cpp build_specs16)
    "narrow3x40": model_cfg(3, 40, 2, 4, 2),
    "odd5x99_skip2": model_cfg(5, 99, 2, 10, 4),
    "wide3x200_skip1": model_cfg(3, 200, 1, 6, 3),
    "novw2x130": model_cfg(2, 130, 4, 5, 0, use_viewdirs=False),
    # more frequencies than the reference's configs use (nerf/models.py:198-201 takes any): the forward kernel's extended
    # encoding registers (128 + 64 stash slot rows instead of 64 + 32; four / two B tiles in the encoding-column jobs)
    "L12_4x128": model_cfg(4, 128, 4, 12, 4),
    "L16_Ld6_8x256": model_cfg(8, 256, 4, 16, 6),
    "L11_novw3x64_skip1": model_cfg(3, 64, 1, 11, 0, use_viewdirs=False),
    "L12_Ld10_2x512": model_cfg(2, 512, 4, 12, 10),
    "Ld5_4x128_skip2": model_cfg(4, 128, 2, 10, 5),
}
EXT_GEOMETRIES = ("L12_4x128", "L16_Ld6_8x256", "L11_novw3x64_skip1", "L12_Ld10_2x512", "Ld5_4x128_skip2")


def exact_rows(params, cfg, rows, gen, margin):
    """EXACTLY `rows` input rows for a gradient comparison: a pool of 1.3 x rows + 64 draws, `unit.mlp_bwd`'s margin filter
    (O.mlp_relu_margin: rows whose ReLU branches round-off cannot decide), the first `rows` survivors.  The filter is per row, so a
    prefix of the result is what a smaller request over the same pool would have kept.  The pool must suffice: never a skip."""
    dx, dd = O.model_dims(cfg)
    x = torch.randn(int(1.3 * rows) + 64, dx + dd, generator=gen)
    x = x[O.mlp_relu_margin(params, x, cfg) > margin]
    assert x.shape[0] >= rows, "the pool left %d of the %d rows asked for" % (x.shape[0], rows)
    return x[:rows].contiguous()


def case_mlp_forward(b, names=None, m=70, precision=0):
    """precision: 0 (the fp32 kernels) or an fp16-piece plan, at the same bound (the stash-free forward of a training plan is its
    inference forward)."""
    for name in names or MLP_GEOMETRIES:
        cfg = MLP_GEOMETRIES[name]
        plan, params, flat, packed = mlp_setup(b, cfg, seed=31, precision=precision)
        dx, dd = O.model_dims(cfg)
        x = torch.randn(m, dx + dd, generator=rng(32))
        want = O.mlp_forward(params, x, cfg).numpy()
        got, _ = b.mlp_fwd(plan, packed, x.numpy())
        close(got, want, *TL.bound("unit.mlp_fwd", ARITH_NAME[precision]), what="mlp fwd %s m=%d" % (name, m))
        b.lib.plan_destroy(plan)


F16X3, F16X3_FWD, F16X3_FWD_DGRAD, F16X3_TRAIN = 5, 6, 7, 8    # NERFHIP_PRECISION_*: the fp16-piece plans (fp32-grade products)
ARITH_NAME = {0: "fp32", F16X3: "f16x3", F16X3_FWD: "f16x3_fwd", F16X3_FWD_DGRAD: "f16x3_fwd_dgrad", F16X3_TRAIN: "f16x3_train"}
F16X3_GEOMETRIES = ("default4x128", "northstar8x256", "fern8x128_skip3_L6", "novw4x128", "two_layer_L4_L2", "one_layer",
                    "one_layer_novw_256", "skip_every_layer_256", "noinput_linear", "odd5x99_skip2", "wide3x200_skip1",
                    "novw2x130", "llff4x64_skip3_L6", "deep8x64_skip4", "novw3x64_skip1", "one_layer_64", "narrow3x40")


def case_mlp_forward_f16x3(b, names=None, m=70, precision=F16X3):
    """The fp16-piece inference forward (mlp_f16w.hip) against the oracle's fp32 forward AND its fp64 forward: the fp32 kernels' own
    bound against the former, an fp32-sized distance from the latter (tests/tolerances.py); what the case pins besides is the index
    algebra -- unit permutation, slot map, chunking, bias rows, skip / head / direction layers -- where any slip is an O(1) error."""
    for name in names or F16X3_GEOMETRIES:
        cfg = MLP_GEOMETRIES[name]
        plan, params, flat, packed = mlp_setup(b, cfg, seed=31, precision=precision)
        dx, dd = O.model_dims(cfg)
        x = torch.randn(m, dx + dd, generator=rng(32))
        want = O.mlp_forward(params, x, cfg).numpy()
        want64 = O.mlp_forward({k: v.double() for k, v in params.items()}, x.double(), cfg).numpy()
        got, _ = b.mlp_fwd(plan, packed, x.numpy())
        scale = float(np.abs(want64).max())
        err = float(np.abs(got - want64).max()) / scale
        note("mlp_fwd_f16x3_%s_%s" % (name, b.name), max_err_over_scale=err,
             fp32_oracle_err_over_scale=float(np.abs(want - want64).max()) / scale)
        # (the distance from the fp64 forward must be what an fp32 evaluation's is -- torch's own is 1-4e-7)
        assert err < TL.bound("unit.mlp_fwd.vs_fp64_over_scale", "f16x3"), (name, err)
        close(got, want, *TL.bound("unit.mlp_fwd", "f16x3"), what="mlp fwd f16x3 " + name)  # (the fp32 kernels' own bound: case_mlp_forward)
        # a training forward (stash) and a backward are refused
        with pytest.raises(L.NerfHipError, match="inference-only"):
            b.mlp_fwd(plan, packed, x.numpy(), want_stash=True)
        b.lib.plan_destroy(plan)
    with pytest.raises(L.NerfHipError, match="plans need"):
        b.make_plan(MLP_GEOMETRIES["wide3x512_skip2"], precision)     # (512-wide nets run fp32)
    with pytest.raises(L.NerfHipError, match="plans need"):
        b.make_plan(MLP_GEOMETRIES["L12_4x128"], precision)           # (more than 10 xyz frequencies: the fp32 kernels' extended slots)
    # (values 1 .. 4 named round 3's bf16-piece plans: removed, refused with a message)
    for removed in (1, 2, 3, 4):
        with pytest.raises(L.NerfHipError, match="removed in round 5"):
            b.make_plan(MLP_GEOMETRIES["default4x128"], removed)


def case_mlp_golden(b):
    g = gold("mlp_forward.npz")
    geo = {"a": (8, 128, 4, 10, 4, True), "b": (8, 128, 3, 6, 4, True), "c": (6, 128, 2, 10, 4, True),
           "d": (4, 128, 4, 10, 4, False), "e": (2, 128, 4, 4, 2, True)}
    for tag, (L, W, sk, lx, ld, view) in geo.items():
        cfg = model_cfg(L, W, sk, lx, ld, use_viewdirs=view)
        plan, params, flat, packed = mlp_setup(b, cfg, seed=100 + ord(tag))
        got, _ = b.mlp_fwd(plan, packed, g["x_" + tag])
        close(got, g["y_" + tag], 2e-5, 2e-5, what="mlp golden " + tag)
        b.lib.plan_destroy(plan)


def case_mlp_backward(b, names=None, m=150, precision=0, g_scale=1.0, w_gain=1.0, rows=None):
    """Teacher-forced MLP backward against the oracle's autograd, every parameter tensor.  precision: 0 (the fp32 kernels) or an
    fp16-piece training plan (F16X3_FWD: the training forward on fp16 pieces -- its stash: slots in ITS order, fp32 rows as it
    computed them, ReLU masks in the data-gradient kernel's lane layout --, _FWD_DGRAD, _TRAIN) under the SAME margin and bound.
    rows: the kernels see EXACTLY that many rows (exact_rows) instead of whatever the filter leaves of m."""
    mb = TL.bound("unit.mlp_bwd", ARITH_NAME[precision])
    margin, tol = mb["margin"], mb["tol"]
    for name in names or ("default4x128", "deep8x128_skip4", "fern8x128_skip3_L6", "novw4x128"):
        cfg = MLP_GEOMETRIES[name]
        plan, params, flat, packed = mlp_setup(b, cfg, seed=41, precision=precision, w_gain=w_gain)
        dx, dd = O.model_dims(cfg)
        gen = rng(42)
        if rows is not None:
            x = exact_rows(params, cfg, rows, gen, margin)
            go = torch.randn(rows, 4, generator=gen) * g_scale
        else:
            x = torch.randn(m, dx + dd, generator=gen)
            go = torch.randn(m, 4, generator=gen) * g_scale  # (g_scale: cotangents as small as a 4096-ray mean's -- the fp16 chain's scaling)
            # rows with a ReLU input within 1e-6 (relative) of zero are dropped: their branch is decided by fp32 round-off, the
            # kernel's k-ordered sums and torch's GEMM may disagree, and ONE such unit moves the gradient by 1e-2 of max|g|
            # (seen on MI355X and on the emulator alike: sample 136 of seed 42 for the 3x512 net, pre-activation 3.7e-9)
            keep = O.mlp_relu_margin(params, x, cfg) > margin
            x, go = x[keep].contiguous(), go[keep].contiguous()
            assert x.shape[0] >= 0.9 * m, (x.shape[0], m)   # (8x256: 2,300 units per row)
        p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        (O.mlp_forward(p, x, cfg) * go).sum().backward()
        got_y, stash = b.mlp_fwd(plan, packed, x.numpy(), want_stash=True)
        gflat = b.mlp_bwd(plan, packed, go.numpy(), stash)
        grads = b.unflatten(plan, gflat)
        if rows is not None:  # (on record: the largest error of the launch, of max|g| per tensor)
            note("mlp_bwd_exact_rows_%s_%s" % (ARITH_NAME[precision], b.name), **{"%s rows=%d" % (name, rows): max(
                float(np.abs(grads[k] - v.grad.numpy()).max()) / (float(np.abs(v.grad.numpy()).max()) + 1e-12) for k, v in p.items())})
        for k, v in p.items():
            ref = v.grad.numpy()
            scale = float(np.abs(ref).max()) + 1e-12
            close(grads[k], ref, tol * scale + 1e-7 * g_scale, 10 * tol, what="mlp bwd %s %s" % (name, k))
        b.lib.plan_destroy(plan)


def kept_count_patterns(rows, kept_counts, strided=(33, 129)):
    """Masks of `rows` cotangent rows with EXACTLY k non-zero rows, for every k: the first k rows, the last k rows and, for the k in
    `strided`, every (rows // k)-th row -- the kept count of a compacted backward on, one below and one above its 32-row tiles
    (ceil(kept / 32)) and 128-row groups ((slots + 127) >> 7), dense at either end of the batch and gathered from all over it."""
    out = []
    for k in kept_counts:
        assert 0 < k <= rows, (k, rows)
        first, last, every = (torch.zeros(rows, dtype=torch.bool) for _ in range(3))
        first[:k] = True
        last[rows - k:] = True
        out += [("kept %d, the first rows" % k, first), ("kept %d, the last rows" % k, last)]
        if k in strided:
            every[torch.arange(k) * (rows // k)] = True
            out.append(("kept %d, every %d-th row" % (k, rows // k), every))
    assert all(int(on.sum()) == int(what.split()[1].rstrip(",")) for what, on in out)
    return out


def case_mlp_backward_compacted(b, names=None, m=300, precision=0, fractions=(0.0, 0.45, 0.85, 1.0), g_scale=1.0, rows=None,
                                kept_counts=()):
    """The compacted backward (nerfhip_plan_set_bwd_compaction; csrc/compact.hip) against the dense one of the same plan and against the
    oracle's autograd.  d(raw output) rows are zeroed at random at the given fractions -- what relu(sigma + noise)
    (nerf/volume_rendering_utils.py:38) does to the cotangents of a training batch: 0 (nothing to drop), in between (ragged last tile,
    gathered rows), 1 (every row zero: the gradient is exactly zero) --; also a batch whose ONLY non-zero row is the last sample.
    Compacted == dense up to the rounding of another split-K partition (`unit.compact_vs_dense`, of max|g| per tensor); the count the
    library reports is the number of non-zero rows; d(loss)/d(x) comes out the same with zero rows for the dropped samples.
    rows: EXACTLY that many rows (exact_rows) instead of what the filter leaves of m; kept_counts: besides, patterns with exactly k
    non-zero rows for each k (kept_count_patterns) under the same assertions."""
    mb = TL.bound("unit.mlp_bwd", ARITH_NAME[precision])
    margin, tol = mb["margin"], mb["tol"]
    ctol = TL.bound("unit.compact_vs_dense", ARITH_NAME[precision])
    for name in names or ("default4x128", "fern8x128_skip3_L6", "novw4x128"):
        cfg = MLP_GEOMETRIES[name]
        plan, params, flat, packed = mlp_setup(b, cfg, seed=47, precision=precision)
        dx, dd = O.model_dims(cfg)
        gen = rng(48)
        if rows is not None:
            x = exact_rows(params, cfg, rows, gen, margin)
            mm = rows
        else:
            x = torch.randn(m, dx + dd, generator=gen)
            keep = O.mlp_relu_margin(params, x, cfg) > margin
            x = x[keep].contiguous()
            mm = x.shape[0]
            assert mm >= 0.9 * m
        go_full = torch.randn(mm, 4, generator=gen) * g_scale
        patterns = []
        for fr in fractions:
            on = (torch.rand(mm, generator=gen) >= fr) if 0.0 < fr < 1.0 else torch.full((mm,), fr == 0.0)
            patterns.append(("zero fraction %.2f" % fr, on))
        last = torch.zeros(mm, dtype=torch.bool)
        last[-1] = True
        patterns.append(("only the last sample", last))
        patterns += kept_count_patterns(mm, kept_counts)
        _, stash = b.mlp_fwd(plan, packed, x.numpy(), want_stash=True)
        for what, on in patterns:
            go = go_full * on[:, None].float()
            p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
            xr = x.clone().requires_grad_(True)
            (O.mlp_forward(p, xr, cfg) * go).sum().backward()
            b.set_compaction(plan, False)
            dense, gx_dense = b.mlp_bwd(plan, packed, go.numpy(), stash, flat_for_input_grad=flat)
            b.set_compaction(plan, True)
            comp, stats = b.mlp_bwd(plan, packed, go.numpy(), stash, want_stats=True)
            _, gx_comp = b.mlp_bwd(plan, packed, go.numpy(), stash, flat_for_input_grad=flat)
            assert stats == (int(on.sum()), mm), (name, what, stats, int(on.sum()), mm)
            assert np.isfinite(comp).all(), (name, what)
            if not bool(on.any()):
                assert not comp.any() and not gx_comp.any(), (name, what)  # (every term dropped: exactly zero)
            gd, gc = b.unflatten(plan, dense), b.unflatten(plan, comp)
            worst = 0.0
            for k, v in p.items():
                ref = v.grad.numpy()
                scale = float(np.abs(ref).max()) + 1e-12
                close(gc[k], ref, tol * scale + 1e-7 * g_scale, 10 * tol, what="compacted mlp bwd %s %s %s" % (name, what, k))
                d = float(np.abs(gc[k] - gd[k]).max()) / (float(np.abs(gd[k]).max()) + 1e-30)
                worst = max(worst, d)
                assert d <= ctol, ("compacted vs dense", name, what, k, d, ctol)
            # d(loss)/d(x): per-sample chains, no sum over samples -- identical rows, zero rows where the cotangent is zero
            sx = float(np.abs(gx_dense).max()) + 1e-30
            assert float(np.abs(gx_comp - gx_dense).max()) <= 1e-6 * sx, (name, what)
            assert not gx_comp[~on.numpy()].any(), (name, what)
            note("compact_vs_dense_%s_%s" % (ARITH_NAME[precision], b.name), **{"%s | %s" % (name, what): worst})
        b.set_compaction(plan, False)
        b.lib.plan_destroy(plan)


def case_render_compacted(b, cfg, n, nc, nf, precision=0, seed=9, white=False, noise=0.3, tag="", fused=False):
    """The fused render's backward in its three modes on one batch -- dense, compacted (stash rows gathered), compacted + recomputed
    (nerfhip_plan_set_bwd_compaction(plan, 2): stash-free training forward, the backward re-runs the forward for the listed samples) --
    with the renderer's OWN cotangents: the rows dropped are those relu(sigma + noise) and the transmittance zero
    (nerf/volume_rendering_utils.py:38-42).  Outputs bit-identical in all modes (the stash-free forward is the same kernel without its
    stores); gradients of both nets within `unit.compact_vs_dense` of the dense ones; kept + dropped = all samples, and some of each.
    fused: also the modes of the fused backward of 64-wide nets (3 / 4 / 5, csrc/mlp64r.hip: one persistent kernel, no
    d(pre-activation) images) -- over every sample with the forward recomputed, over the same list, and over every sample with the
    chain's registers read back from the register-image stash the training forward left (5: the SAME arithmetic as 3 on the same
    values -- its gradient equals mode 3's bit for bit)."""
    gen = rng(seed)
    pc, par_c, _, packed_c = mlp_setup(b, cfg, seed=seed + 1, precision=precision)
    pf, par_f, _, packed_f = mlp_setup(b, cfg, seed=seed + 2, precision=precision)
    ro = torch.tensor([0.2, -0.1, 4.0]).expand(n, 3) + 0.05 * torch.randn(n, 3, generator=gen)
    rd = torch.randn(n, 3, generator=gen) * 0.3
    rd[:, 2] = -1.0
    rays = O.pack_rays(ro, rd, 2.0, 6.0, rd if cfg["use_viewdirs"] else None).numpy()
    rnp = dict(t_rand=torch.rand(n, nc, generator=gen).numpy(), noise_coarse=torch.randn(n, nc, generator=gen).numpy(),
               u=torch.rand(n, nf, generator=gen).numpy(), noise_fine=torch.randn(n, nc + nf, generator=gen).numpy())
    opt = dict(num_coarse=nc, num_fine=nf, perturb=True, lindisp=False, white_background=white, noise_std=noise)
    tgt = torch.rand(n, 3, generator=gen).numpy()
    ctol = TL.bound("unit.compact_vs_dense", ARITH_NAME[precision])
    res = {}
    modes = (False, True, "recompute") + (("fused", "fused_compact", "fused_stash") if fused else ())
    for mode in modes:
        b.set_compaction(pc, mode)
        b.set_compaction(pf, mode)
        fwd = b.render(pc, pf, packed_c, packed_f, rays, opt, rnp, training=True)
        if mode is False:
            _, gc, gf = b.mse_loss(fwd["rgb_coarse"], fwd["rgb_fine"], tgt)
        res[mode] = b.render(pc, pf, packed_c, packed_f, rays, opt, rnp, training=True, g_rgb=(gc, gf))
    dense = res[False]
    for mode in modes[1:]:
        r = res[mode]
        for k in ("rgb_coarse", "acc_coarse", "depth_coarse", "disp_coarse", "rgb_fine", "acc_fine", "depth_fine", "disp_fine"):
            assert np.array_equal(r[k], dense[k], equal_nan=True), (mode, k)
        for key, name, plan, total in (("g_params_coarse", "coarse", pc, n * nc), ("g_params_fine", "fine", pf, n * (nc + nf))):
            dense_walk = mode in ("fused", "fused_stash")  # (no list)
            kept, tot = r["bwd_kept_" + name] if not dense_walk else res[True]["bwd_kept_" + name]
            if mode == "fused_stash":
                assert np.array_equal(r[key], res["fused"][key]), ("stashed vs recomputing fused backward", key)
            if not dense_walk:
                assert tot == total and 0 < kept < total, (mode, name, kept, tot)
                assert r["bwd_kept_" + name] == res[True]["bwd_kept_" + name]
            # (mode 2 differs from mode 1 only in WHERE the kept samples' stash rows sit: same list, same rows, same tile ranges --
            # the same gradient bit for bit)
            if mode == "recompute":
                assert np.array_equal(r[key], res[True][key]), ("recomputed vs compacted", key)
            gd, gk = b.unflatten(plan, dense[key]), b.unflatten(plan, r[key])
            worst = 0.0
            for k in gd:
                assert np.isfinite(gk[k]).all(), (mode, key, k)
                d = float(np.abs(gk[k] - gd[k]).max()) / (float(np.abs(gd[k]).max()) + 1e-30)
                worst = max(worst, d)
                assert d <= ctol, ("compacted render vs dense", mode, key, k, d, ctol)
            note("render_compacted_%s_%s_%s" % (tag or n, ARITH_NAME[precision], b.name),
                 **{"%s %s" % (mode, name): worst, "zero fraction " + name: 1.0 - kept / float(tot)})
    for p in (pc, pf):
        b.lib.plan_destroy(p)


def case_render_fused_edges(b, cfg, seed=17):
    """Edges of the fused backward (nerfhip_plan_set_bwd_compaction 3 / 4, csrc/mlp64r.hip): (i) all-zero cotangents -- mode 3 multiplies
    zeros (every d(pre-activation) is an exact zero), mode 4's list is empty (no round runs; the partials are written all the same) --
    both gradients are EXACTLY zero; (ii) a batch smaller than one 64-sample round (one ray, 8 + 8 samples) against the dense backward."""
    gen = rng(seed)
    pc, _, _, packed_c = mlp_setup(b, cfg, seed=seed + 1)
    pf, _, _, packed_f = mlp_setup(b, cfg, seed=seed + 2)
    ctol = TL.bound("unit.compact_vs_dense", "fp32")
    for n, nc, nf in ((1, 8, 8), (5, 16, 8)):
        ro = torch.tensor([0.2, -0.1, 4.0]).expand(n, 3) + 0.05 * torch.randn(n, 3, generator=gen)
        rd = torch.randn(n, 3, generator=gen) * 0.3
        rd[:, 2] = -1.0
        rays = O.pack_rays(ro, rd, 2.0, 6.0, rd).numpy()
        rnp = dict(t_rand=torch.rand(n, nc, generator=gen).numpy(), noise_coarse=torch.randn(n, nc, generator=gen).numpy(),
                   u=torch.rand(n, nf, generator=gen).numpy(), noise_fine=torch.randn(n, nc + nf, generator=gen).numpy())
        opt = dict(num_coarse=nc, num_fine=nf, perturb=True, lindisp=False, white_background=False, noise_std=0.0)
        tgt = torch.rand(n, 3, generator=gen).numpy()
        res = {}
        for mode in (False, "fused", "fused_compact", "fused_stash"):
            b.set_compaction(pc, mode)
            b.set_compaction(pf, mode)
            fwd = b.render(pc, pf, packed_c, packed_f, rays, opt, rnp, training=True)
            if mode is False:
                _, gc, gf = b.mse_loss(fwd["rgb_coarse"], fwd["rgb_fine"], tgt)
            res[mode] = b.render(pc, pf, packed_c, packed_f, rays, opt, rnp, training=True, g_rgb=(gc, gf))
            zero = b.render(pc, pf, packed_c, packed_f, rays, opt, rnp, training=True, g_rgb=(np.zeros_like(gc), np.zeros_like(gf)))
            for key in ("g_params_coarse", "g_params_fine"):
                assert not zero[key].any(), ("zero cotangents", mode, key, float(np.abs(zero[key]).max()))
        for mode in ("fused", "fused_compact", "fused_stash"):
            for key, plan in (("g_params_coarse", pc), ("g_params_fine", pf)):
                gd, gk = b.unflatten(plan, res[False][key]), b.unflatten(plan, res[mode][key])
                for k in gd:
                    d = float(np.abs(gk[k] - gd[k]).max()) / (float(np.abs(gd[k]).max()) + 1e-30)
                    assert d <= ctol, ("fused vs dense, small batch", n, mode, key, k, d)
    for p in (pc, pf):
        b.lib.plan_destroy(p)


def case_f16x3_range_extremes(b, m=120):
    """The edges of the fp16-piece bookkeeping (round 5).  (i) Cotangents of 1e-30, 1e-33 and of fp32-SUBNORMAL size (1e-39):
    the per-sample exponent would be 113 / 123 / undefined -- it is clamped at 110 / the sample counts as all-zero (mlp_f16w.hip
    exp_for): every gradient stays finite; at 1e-30 it is no further from the fp64 gradient than torch's own fp32 backward (x 3), at 1e-33 within 2e-2 of
    max|g| (fewer piece bits below 2^-97).  This case found round 4's zero-sample region bound (mlp_f16w.hip ZERO_EXP): with cotangents below
    ~1e-20 the fp16-piece weight gradient lost bits, below ~1e-25 everything.  (ii) Weights
    beyond fp16's range once scaled by 2^8 (|w| up to ~440): k_pack_f16x3 saturates the pieces instead of writing Inf -- outputs finite
    (and meaningless: the limit |w| < 255.9 is in include/nerfhip.h); the fp32 kernels on the same weights agree with the oracle."""
    cfg = MLP_GEOMETRIES["default4x128"]
    dx, dd = O.model_dims(cfg)
    plan, params, flat, packed = mlp_setup(b, cfg, seed=41, precision=F16X3_TRAIN)
    gen = rng(42)
    x = torch.randn(m, dx + dd, generator=gen)
    keep = O.mlp_relu_margin(params, x, cfg) > 1e-5
    x = x[keep].contiguous()
    go1 = torch.randn(x.shape[0], 4, generator=gen)
    _, stash = b.mlp_fwd(plan, packed, x.numpy(), want_stash=True)
    for g_scale, compare in ((1e-30, True), (1e-33, True), (1e-39, False)):
        go = go1 * g_scale
        grads = b.unflatten(plan, b.mlp_bwd(plan, packed, go.numpy(), stash))
        assert all(np.isfinite(v).all() for v in grads.values()), g_scale
        if compare:
            # the yardstick: torch's OWN fp32 backward against fp64 on the same cotangents -- down here the d(pre-activation) values of the
            # deep layers reach fp32's subnormal range (2^-110 times what the transposed layers damp), whatever multiplies them
            p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
            (O.mlp_forward(p64, x.double(), cfg) * go.double()).sum().backward()
            p32 = {k: v.clone().requires_grad_(True) for k, v in params.items()}
            (O.mlp_forward(p32, x, cfg) * go).sum().backward()
            for k, v in p64.items():
                ref = v.grad.numpy()
                scale = float(np.abs(ref).max())
                e_hip = float(np.abs(grads[k] - ref).max()) / scale
                e_t32 = float(np.abs(p32[k].grad.numpy() - ref).max()) / scale
                note("f16x3_tiny_cotangents_%g_%s_%s" % (g_scale, k, b.name), hip_vs_fp64=e_hip, torch_fp32_vs_fp64=e_t32)
                # (1e-30: inside the clamp's full-precision range give or take 3 bits; 1e-33: 13 bits below it -- the pieces of the deep
                # layers' d(pre-activation) keep ~12 bits: documented in mlp_f16w.hip / DESIGN 8.8, bounded here)
                assert e_hip <= (3.0 * e_t32 + 1e-4 if g_scale >= 1e-30 else 2e-2), (k, g_scale, e_hip, e_t32)
        else:  # (cotangents below fp32's normal range: whatever survives is that small)
            assert max(float(np.abs(v).max()) for v in grads.values()) < 1e-30
    b.lib.plan_destroy(plan)
    plan, params, flat, packed = mlp_setup(b, cfg, seed=41, precision=F16X3, w_gain=5000.0)
    assert max(float(v.abs().max()) for k, v in params.items() if k.endswith("weight")) > 256.0
    got, _ = b.mlp_fwd(plan, packed, x.numpy())
    assert np.isfinite(got).all()
    b.lib.plan_destroy(plan)
    # (iii) fp32's TOP edge: input rows of 1e30 ... 1e37 -- activations up to 2^124.  A sample's exponent goes down to 13 - 127
    # (mlp_f16w.hip S_MIN); round 5 clamped it at -110 and such a sample's pieces overflowed fp16 (NaN outputs).  Wherever the oracle's
    # fp32 forward is finite the kernel's is, and agrees to 1e-4 of the row's largest output; the other rows of the batch are untouched.
    plan, params, flat, packed = mlp_setup(b, cfg, seed=41, precision=F16X3)
    xb = x.clone()
    scales = (1e30, 1e33, 1e35, 1e36, 1e37)
    for r, sc in enumerate(scales):
        xb[r] = x[r] * sc
    want = O.mlp_forward(params, xb, cfg).numpy()
    got, _ = b.mlp_fwd(plan, packed, xb.numpy())
    base, _ = b.mlp_fwd(plan, packed, x.numpy())
    assert np.array_equal(got[len(scales):], base[len(scales):])
    checked = 0
    for r in range(len(scales)):
        if np.isfinite(want[r]).all():
            assert np.isfinite(got[r]).all(), (r, scales[r], got[r], want[r])
            assert float(np.abs(got[r] - want[r]).max()) <= 1e-4 * float(np.abs(want[r]).max()), (r, scales[r], got[r], want[r])
            checked += 1
    assert checked >= 2, checked
    b.lib.plan_destroy(plan)


def case_f16x3_scale_fuzz(b, m=40, names=("default4x128", "deep8x128_skip4", "novw4x128", "llff4x64_skip3_L6"), grid=None):
    """Inputs x 1e-6 ... 1e3, weights x 0.03 ... 30, biases x 0 ... 100 (and one all-zero input row): the fp16-piece training plans
    against the oracle in fp64, with torch's own fp32 forward / backward on the same numbers as the yardstick -- forward within 10x of
    torch's distance (+ 2e-6 of the output scale), every gradient tensor within 30x (+ 1e-4 of max|g|), everything finite.
    Plus the corner weights x 1e-3 / zero biases, OUTSIDE the arithmetic's documented weight range (the packed pieces carry a fixed 2^8: a
    weight's low piece is a normal fp16 number down to |w| = 2^-10, include/nerfhip.h; torch's init x 1e-3 is |w| ~ 2^-14, whose pieces
    keep ~18 bits, and eight layers of products at 6e-6 each reach 1e-3 ... 1e-2 of max|g|): held to 5e-2 -- the gradient is THERE.  That
    corner found round 5's ReLU-bit bug: activations far below their sample's capped exponent flushed to zero PIECES and the bit was taken
    from the piece, so fc_feat's (layers_dir behind it) and layer1's (a skip layer behind it) whole gradient was gated off (error 1.0)."""
    import itertools
    corner = [(1.0, 1e-3, 0.0), (1e-6, 1e-3, 0.0)]
    grid = grid or list(itertools.product((1e-6, 1.0, 1e3), (3e-2, 1.0, 30.0), (0.0, 1.0, 100.0))) + corner
    failures = []
    for name in names:
        cfg = MLP_GEOMETRIES[name]
        dx, dd = O.model_dims(cfg)
        for x_scale, w_gain, b_gain in grid:
            plan = b.make_plan(cfg, F16X3_TRAIN)
            params = {k: (v * w_gain if k.endswith("weight") else v * b_gain) for k, v in O.init_params(cfg, seed=61).items()}
            packed = b.pack(plan, b.flatten_params(plan, {k: v.numpy() for k, v in params.items()}))
            gen = rng(62)
            x = torch.randn(m, dx + dd, generator=gen) * x_scale
            x[3] = 0.0
            go = torch.randn(m, 4, generator=gen)
            # (rows with a ReLU input within 1e-5, relative, of zero are dropped as in case_mlp_backward: with zero biases and m = 700 one
            # such unit moves a gradient tensor by 1e-2 of max|g| for the fp32 kernels and the fp16 pieces alike -- met on the emulator)
            keep = O.mlp_relu_margin(params, x, cfg, per_layer=True) > 1e-5
            x, go = x[keep].contiguous(), go[keep].contiguous()
            if x.shape[0] < m // 4:
                failures.append((name, x_scale, w_gain, b_gain, "filter left %d of %d rows" % (x.shape[0], m)))
                b.lib.plan_destroy(plan)
                continue
            p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
            y64 = O.mlp_forward(p64, x.double(), cfg)
            (y64 * go.double()).sum().backward()
            p32 = {k: v.clone().requires_grad_(True) for k, v in params.items()}
            y32 = O.mlp_forward(p32, x, cfg)
            (y32 * go).sum().backward()
            got, stash = b.mlp_fwd(plan, packed, x.numpy(), want_stash=True)
            grads = b.unflatten(plan, b.mlp_bwd(plan, packed, go.numpy(), stash))
            what = (name, x_scale, w_gain, b_gain)
            if not (np.isfinite(got).all() and all(np.isfinite(v).all() for v in grads.values())):
                failures.append(what + ("non-finite",))
            ys = float(y64.detach().abs().max()) + 1e-300
            e_f = float(np.abs(got - y64.detach().numpy()).max()) / ys
            e_f32 = float((y32.detach().double() - y64.detach()).abs().max()) / ys
            small_w = w_gain < 1e-2   # (the out-of-range corner: docstring)
            if not e_f <= (10.0 * e_f32 + 2e-6 if not small_w else 1e-3):
                failures.append(what + ("forward", e_f, e_f32))
            for k, v in p64.items():
                ref = v.grad.numpy()
                sc = float(np.abs(ref).max())
                if sc == 0.0:
                    continue
                e = float(np.abs(grads[k] - ref).max()) / sc
                e32 = float(np.abs(p32[k].grad.numpy() - ref).max()) / sc
                # a tensor whose whole gradient sits below 1e-28 comes from cotangents below the exponent clamp's full-precision range
                # (2^-97 ~ 6e-30 per sample, mlp_f16w.hip S_LIM; fp32 itself ends at 1e-38): fewer piece bits there, documented -- 2e-2
                if not e <= ((max(30.0 * e32, 1e-4) if sc >= 1e-28 else 2e-2) if not small_w else 5e-2):
                    failures.append(what + (k, e, e32, sc))
            b.lib.plan_destroy(plan)
    assert not failures, failures


def case_f16x3_dead_layers(b, m=120):
    """Samples whose hidden activations are ALL ZERO in front of a gemm that also reads encodings (the direction layer behind a dead
    fc_feat; a skip layer behind a dead layers_xyz): the reserved zero exponent must not reach the encoding rescale (2^(60 - s_x) is out
    of fp16's range: the eval test on the trained lego nets met it as wrong colours on 78 rays, round 5).  Forward and every gradient
    against the oracle, inference and training plans."""
    for name, dead in (("default4x128", "fc_feat.bias"), ("deep8x128_skip4", "layers_xyz.3.bias"), ("northstar8x256", "layers_xyz.3.bias")):
        cfg = MLP_GEOMETRIES[name]
        dx, dd = O.model_dims(cfg)
        for precision in (F16X3, F16X3_TRAIN):
            plan = b.make_plan(cfg, precision)
            params = O.init_params(cfg, seed=51)
            params[dead] = params[dead] - 30.0            # every unit of that layer dead for every sample (pre-activations are O(1))
            flat = b.flatten_params(plan, {k: v.numpy() for k, v in params.items()})
            packed = b.pack(plan, flat)
            gen = rng(52)
            x = torch.randn(m, dx + dd, generator=gen)
            go = torch.randn(m, 4, generator=gen)
            want = O.mlp_forward(params, x, cfg).numpy()
            if precision == F16X3:
                got, _ = b.mlp_fwd(plan, packed, x.numpy())
                close(got, want, *TL.bound("unit.mlp_fwd", "f16x3"), what="dead layer fwd " + name)
            else:
                keep = O.mlp_relu_margin(params, x, cfg) > 1e-6
                x, go = x[keep].contiguous(), go[keep].contiguous()
                assert x.shape[0] >= m // 4, (name, x.shape[0])
                p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
                (O.mlp_forward(p, x, cfg) * go).sum().backward()
                got, stash = b.mlp_fwd(plan, packed, x.numpy(), want_stash=True)
                close(got, O.mlp_forward(params, x, cfg).numpy(), *TL.bound("unit.mlp_fwd", "f16x3_train"), what="dead layer fwd (train) " + name)
                grads = b.unflatten(plan, b.mlp_bwd(plan, packed, go.numpy(), stash))
                tol = TL.bound("unit.mlp_bwd", "f16x3_train")["tol"]
                for k, v in p.items():
                    ref = v.grad.numpy()
                    scale = float(np.abs(ref).max()) + 1e-12
                    close(grads[k], ref, tol * scale + 1e-7, 10 * tol, what="dead layer bwd %s %s" % (name, k))
            b.lib.plan_destroy(plan)


def case_mlp_input_grad(b, names=None, m=150, precision=0, rows=None):
    """d(loss)/d(x) of FlexibleNeRFModel.forward vs the oracle's autograd (x enters layer1, the skip layers, layers_dir).
    rows: EXACTLY that many rows, margin-filtered (exact_rows), instead of m unfiltered draws."""
    for name in names or ("default4x128", "fern8x128_skip3_L6", "novw4x128", "odd5x99_skip2"):
        cfg = MLP_GEOMETRIES[name]
        plan, params, flat, packed = mlp_setup(b, cfg, seed=43, precision=precision)
        dx, dd = O.model_dims(cfg)
        gen = rng(44)
        if rows is not None:
            x = exact_rows(params, cfg, rows, gen, TL.bound("unit.mlp_bwd", ARITH_NAME[precision])["margin"])
            m = rows
        else:
            x = torch.randn(m, dx + dd, generator=gen)
        go = torch.randn(m, 4, generator=gen)
        x = x.requires_grad_(True)
        (O.mlp_forward(params, x, cfg) * go).sum().backward()
        ref = x.grad.numpy()
        _, stash = b.mlp_fwd(plan, packed, x.detach().numpy(), want_stash=True)
        _, gx = b.mlp_bwd(plan, packed, go.numpy(), stash, flat_for_input_grad=flat)
        tol = TL.bound("unit.mlp_input_grad", ARITH_NAME[precision])
        close(gx, ref, tol * float(np.abs(ref).max()) + 1e-7, 10 * tol, what="mlp input grad " + name)
        b.lib.plan_destroy(plan)


# One below, on and one above every granularity of the MLP kernels, read from their code: 16 samples per wave (one MFMA tile), the
# 32-sample stash / gradient tiles k_wgrad reads, 48, the 64-sample workgroups of the 4-wave shapes (64-, 128-, 512-wide nets: for
# m <= 64 the second workgroup of a group has no rows) and mlp64r's 64-sample rounds, the 128-sample groups, 256.
ROW_EDGES = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 256, 257)


def has_resident_image(b, plan):
    """True for the fp32 plans of 64-wide nets whose stash-free forward is the persistent k_fwd64r (csrc/mlp.hip mlp_forward_any:
    r64_off >= 0) -- exactly the plans that accept the fused backward modes."""
    try:
        b.set_compaction(plan, "fused")
    except L.NerfHipError:
        return False
    b.set_compaction(plan, False)
    return True


def case_mlp_row_edges(b, name, precision, rows_list=ROW_EDGES):
    """ONE plan at EXACT row counts (ROW_EDGES): the rows are prefixes of one margin-filtered pool (exact_rows), so every launch is
    a prefix of the next.  Per row count:
      forward    -- against the oracle's fp32 forward (`unit.mlp_fwd`) and its fp64 forward (`unit.mlp_fwd.vs_fp64_over_scale`, of the
                    launch's output scale); on training plans the stash-writing forward's outputs equal the stash-free forward's bit
                    for bit (the same kernel without its stores).  The exception is documented too: an fp32 plan
                    with an LDS-resident image (64-wide nets, has_resident_image) runs its stash-free forward on ANOTHER kernel
                    (k_fwd64r, csrc/mlp64r.hip), so there the two forwards are held to `unit.mlp_fwd` of each other instead;
      backward   -- (training plans) every parameter tensor against the oracle's fp64 autograd at `unit.mlp_bwd`'s tol of max|g| per
                    tensor, d(loss)/d(x) against it at `unit.mlp_input_grad`;
      reference  -- the oracle's OWN fp32 autograd is within tol / 4 of its fp64 autograd on these rows for every tensor, else the row
                    set is ill-conditioned and the case fails (it says nothing about the kernels then; it never skips);
      prefix     -- the first r output rows of the next larger launch equal the r-row launch's bit for bit (row i sits in the same
                    lane either way), and so do the first r rows of d(loss)/d(x) on plans whose data gradient runs in fp32; the
                    fp16-piece data gradient is scaled from the whole batch's cotangents: within 1e-6 of max|g|, the number
                    case_mlp_backward_compacted holds gx_comp to gx_dense with.  A tail that leaks into, or is fed by, rows that do
                    not exist shows here.
    The worst figures per row count go on record."""
    arith = ARITH_NAME[precision]
    cfg = MLP_GEOMETRIES[name]
    train = precision != F16X3                                   # (F16X3: inference-only, forward assertions alone)
    f16_dgrad = precision in (F16X3_FWD_DGRAD, F16X3_TRAIN)
    mb = TL.bound("unit.mlp_bwd", arith)
    margin, tol = mb["margin"], mb["tol"]
    xtol = TL.bound("unit.mlp_input_grad", arith)
    plan, params, flat, packed = mlp_setup(b, cfg, seed=71, precision=precision)
    resident = train and has_resident_image(b, plan)
    rows_list = sorted(rows_list)
    gen = rng(72)
    x_all = exact_rows(params, cfg, rows_list[-1], gen, margin)
    go_all = torch.randn(rows_list[-1], 4, generator=gen)
    p64 = {k: v.double() for k, v in params.items()}
    case = "mlp_row_edges_%s_%s_%s" % (name, arith, b.name)
    prev = None
    for r in rows_list:
        x, go = x_all[:r].contiguous(), go_all[:r].contiguous()
        what = "%s %s rows=%d" % (name, arith, r)
        rec = {}
        # -- forward
        want = O.mlp_forward(params, x, cfg).numpy()
        want64 = O.mlp_forward(p64, x.double(), cfg).numpy()
        got, _ = b.mlp_fwd(plan, packed, x.numpy())
        rec["fwd_vs_fp64_over_scale"] = float(np.abs(got - want64).max()) / float(np.abs(want64).max())
        note(case, **{"rows=%03d %s" % (r, k): v for k, v in rec.items()})
        close(got, want, *TL.bound("unit.mlp_fwd", arith), what="row edges fwd " + what)
        assert rec["fwd_vs_fp64_over_scale"] < TL.bound("unit.mlp_fwd.vs_fp64_over_scale", arith), (what, rec)
        gx = None
        if train:
            got_s, stash = b.mlp_fwd(plan, packed, x.numpy(), want_stash=True)
            if resident:
                close(got_s, got, *TL.bound("unit.mlp_fwd", arith), what="row edges stash-writing vs stash-free fwd " + what)
                close(got_s, want, *TL.bound("unit.mlp_fwd", arith), what="row edges stash-writing fwd " + what)
            else:
                assert np.array_equal(got_s, got), ("stash-writing vs stash-free forward", what, float(np.abs(got_s - got).max()))
            # -- the references: fp64 autograd, and the oracle's own fp32 autograd as the condition on the row set
            ref = {}
            for dt in (torch.float32, torch.float64):
                p = {k: v.to(dt).clone().requires_grad_(True) for k, v in params.items()}
                xr = x.to(dt).clone().requires_grad_(True)
                (O.mlp_forward(p, xr, cfg) * go.to(dt)).sum().backward()
                ref[dt] = dict({k: v.grad.double().numpy() for k, v in p.items()}, x=xr.grad.double().numpy())
            r64 = ref[torch.float64]
            scale = {k: float(np.abs(v).max()) + 1e-12 for k, v in r64.items()}
            cond = {k: float(np.abs(ref[torch.float32][k] - v).max()) / scale[k] for k, v in r64.items()}
            rec["oracle_fp32_vs_fp64"] = max(cond.values())
            assert rec["oracle_fp32_vs_fp64"] <= tol / 4, ("ill-conditioned rows: the oracle's fp32 autograd is that far from its fp64 autograd",
                                                          what, max(cond, key=cond.get), rec["oracle_fp32_vs_fp64"], tol / 4)
            # -- backward
            gflat, gx = b.mlp_bwd(plan, packed, go.numpy(), stash, flat_for_input_grad=flat)
            grads = b.unflatten(plan, gflat)
            rec["param_grad_vs_fp64"] = max(float(np.abs(grads[k] - r64[k]).max()) / scale[k] for k in grads)
            rec["input_grad_vs_fp64"] = float(np.abs(gx - r64["x"]).max()) / scale["x"]
            note(case, **{"rows=%03d %s" % (r, k): v for k, v in rec.items()})
            for k in grads:
                close(grads[k], r64[k], tol * scale[k] + 1e-7, 10 * tol, what="row edges bwd %s %s" % (what, k))
            close(gx, r64["x"], xtol * scale["x"] + 1e-7, 10 * xtol, what="row edges input grad " + what)
        # -- prefix invariance against the next smaller launch
        if prev is not None:
            pr, pgot, pgx = prev
            assert np.array_equal(got[:pr], pgot), ("forward rows 0..%d differ between the %d- and the %d-row launch" % (pr - 1, pr, r), what,
                                                    float(np.abs(got[:pr] - pgot).max()))
            if train and f16_dgrad:
                d = float(np.abs(gx[:pr] - pgx).max())
                assert d <= 1e-6 * (float(np.abs(gx).max()) + 1e-30), ("d(loss)/d(x) rows 0..%d, %d- vs %d-row launch" % (pr - 1, pr, r), what, d)
            elif train:
                assert np.array_equal(gx[:pr], pgx), ("d(loss)/d(x) rows 0..%d differ between the %d- and the %d-row launch" % (pr - 1, pr, r),
                                                      what, float(np.abs(gx[:pr] - pgx).max()))
        prev = (r, got, gx)
    b.lib.plan_destroy(plan)


def case_persistent_round_edges(b, name, precision, which=(0, 1, 2)):
    """The fp16-piece forward and data-gradient kernels are persistent: grid = min(groups of 128 rows, compute units).  With C compute
    units (b.compute_units): 128 C rows -- exactly one round --, 128 C + 1 -- one workgroup runs a second round of ONE row --,
    128 (C + 1) + 17 -- two second rounds, the last one ragged --, dense, at EXACT row counts: case_mlp_forward and (training plans)
    case_mlp_backward at their present bounds.  The fp32 plans run the same counts (their grids are not persistent)."""
    C_ = b.compute_units
    assert C_ > 0
    counts = (128 * C_, 128 * C_ + 1, 128 * (C_ + 1) + 17)
    for i in which:
        if precision == F16X3:
            case_mlp_forward_f16x3(b, names=(name,), m=counts[i], precision=F16X3)
        else:
            case_mlp_forward(b, names=(name,), m=counts[i], precision=precision)
            case_mlp_backward(b, names=(name,), precision=precision, rows=counts[i])


# ---- the whole path ----------------------------------------------------------------------------------------------------
def e2e_inputs(name):
    g = gold(name)
    meta = ast.literal_eval(str(g["meta"]))
    cfg_c = model_cfg(**{k: v for k, v in meta["cfg_c"].items()})
    cfg_f = model_cfg(**{k: v for k, v in meta["cfg_f"].items()})
    ro, rd = T(g["ro"]), T(g["rd"])
    vsrc = rd if cfg_c["use_viewdirs"] else None
    if meta["ndc"]:
        ro, rd = O.ndc_rays(int(g["H"]), int(g["W"]), float(g["focal"]), 1.0, ro, rd)
    rays = O.pack_rays(ro, rd, float(g["near"]), float(g["far"]), vsrc).numpy()
    rand = {k: g[k] for k in ("t_rand", "noise_coarse", "u", "noise_fine") if k in g.files}
    opt = dict(num_coarse=meta["nc"], num_fine=meta["nf"], perturb=meta["perturb"], lindisp=meta["lindisp"],
               white_background=meta["white"], noise_std=meta["noise"])
    return g, meta, cfg_c, cfg_f, rays, rand, opt


# Bounds on max|g_hip - g_ref| / max|g_ref| per parameter tensor of the reference-generated end-to-end goldens: (coarse
# net, fine net).  The fine net sits behind the inverse-CDF sampler; the bounds are <= 5x the worst
# value measured on MI355X (profiles/r03_parity_small_cases.json), not the 3e-2 placeholder of earlier rounds.
# Measured (coarse / fine; MI355X | CPU wave emulator):  a 4.6e-7 / 3.5e-6 | 3.8e-7 / 3.5e-6;  b 7.9e-7 / 4.9e-6 | 5.5e-7 / 4.5e-4;
# c 4.8e-7 / 1.5e-6 | 4.7e-7 / 8.6e-7;  d 6.5e-7 / 2.2e-6 | 4.8e-7 / 2.3e-6;  northstar 3.1e-7 / 1.7e-3 | 3.1e-7 / 1.7e-3.
E2E_GRAD_TOL = {"e2e_a.npz": (4e-6, 2e-5), "e2e_b.npz": (4e-6, 2.3e-3), "e2e_c.npz": (4e-6, 8e-6), "e2e_d.npz": (4e-6, 1.2e-5),
                "e2e_northstar.npz": (4e-6, 8.6e-3)}


def case_e2e_golden(b, name, with_grads=True, precision=0):
    """Fused render (+ backward) against outputs and gradients recorded from the REAL reference.
    precision: the plans' arithmetic (0 = fp32; an F16X3 training level runs the SAME assertions)."""
    g, meta, cfg_c, cfg_f, rays, rand, opt = e2e_inputs(name)
    pc, _, flat_c, packed_c = mlp_setup(b, cfg_c, seed=meta["seed"] * 2 + 1, precision=precision)
    pf, _, flat_f, packed_f = mlp_setup(b, cfg_f, seed=meta["seed"] * 2 + 2, precision=precision)
    n = rays.shape[0]
    out = b.render(pc, pf, packed_c, packed_f, rays, opt, rand, training=with_grads)
    for k in ("rgb_coarse", "acc_coarse", "rgb_fine", "acc_fine"):
        close(out[k], g[k], 1e-4, what="%s %s" % (name, k))
    for k in ("disp_coarse", "disp_fine"):
        close(out[k], g[k], 1e-4, 1e-4, what="%s %s" % (name, k))
    if with_grads:
        tgt = g["target"]
        loss, gc, gf = b.mse_loss(out["rgb_coarse"], out["rgb_fine"], tgt)
        assert abs(float(loss[2]) - float(g["loss"])) < 1e-5
        out = b.render(pc, pf, packed_c, packed_f, rays, opt, rand, training=True, g_rgb=(gc, gf))
        gc_tol, gf_tol = E2E_GRAD_TOL[name]
        for tag, plan, key, gt in (("gc_", pc, "g_params_coarse", gc_tol), ("gf_", pf, "g_params_fine", gf_tol)):
            grads = b.unflatten(plan, out[key])
            for k, v in grads.items():
                grad_close(v, g[tag + k], gt, "%s grad %s%s" % (name, tag, k), "%s_%s%s" % (name, b.name, "_p%d" % precision if precision else ""), key)
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


def case_e2e_northstar_golden(b, precision=0):
    """The headline geometry (8x256, 64 + 128) against the REAL reference (oracle/gen_golden.py e2e_sampled): outputs,
    loss, and for every parameter tensor the gradient's sum, absolute sum and 96 sampled entries."""
    name = "e2e_northstar.npz"
    g, meta, cfg_c, cfg_f, rays, rand, opt = e2e_inputs(name)
    pc, _, _, packed_c = mlp_setup(b, cfg_c, seed=meta["seed"] * 2 + 1, precision=precision)
    pf, _, _, packed_f = mlp_setup(b, cfg_f, seed=meta["seed"] * 2 + 2, precision=precision)
    out = b.render(pc, pf, packed_c, packed_f, rays, opt, rand, training=True)
    for k in ("rgb_coarse", "acc_coarse", "rgb_fine", "acc_fine"):
        close(out[k], g[k], 1e-4, what="%s %s" % (name, k))
    loss, gc, gf = b.mse_loss(out["rgb_coarse"], out["rgb_fine"], g["target"])
    assert abs(float(loss[2]) - float(g["loss"])) < 1e-5
    out = b.render(pc, pf, packed_c, packed_f, rays, opt, rand, training=True, g_rgb=(gc, gf))
    gc_tol, gf_tol = E2E_GRAD_TOL[name]
    for tag, plan, key, gt in (("gc_", pc, "g_params_coarse", gc_tol), ("gf_", pf, "g_params_fine", gf_tol)):
        for k, v in b.unflatten(plan, out[key]).items():
            sums, idx, val = g["s" + tag + k], g["i" + tag + k], g["v" + tag + k]
            scale = float(sums[2]) + 1e-12                      # max |grad| of the tensor in the reference
            flat = np.asarray(v).reshape(-1)
            worst = float(np.abs(flat[idx].astype(np.float64) - val).max()) / scale
            note("%s_%s" % (name, b.name), **{key: max(RECORD.get("%s_%s" % (name, b.name), {}).get(key, 0.0), worst)})
            close(flat[idx], val, gt * scale + 1e-9, 5e-4, what="%s sampled grad %s%s" % (name, tag, k))
            # sums over the tensor: errors average out, so a tighter relative bound on the absolute sum
            assert abs(float(np.abs(flat).sum()) - float(sums[1])) <= (gt * 0.5) * float(sums[1]) + 1e-9, (tag, k)
            assert abs(float(flat.sum()) - float(sums[0])) <= gt * float(sums[1]) + 1e-9, (tag, k)
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


def case_render_vs_oracle(b, cfg, n, nc, nf, seed=5, white=False, noise=0.3, with_grads=False, tol=1e-4,
                          grad_tol=(1e-3, 5e-3), tag="", precision=0):
    """Fused render against the oracle on random-init nets of an arbitrary geometry (e.g. the 8x256 north star).
    precision: the plans' arithmetic (0: fp32; an fp16-piece training plan: the same bounds)."""
    gen = rng(seed)
    pc, par_c, _, packed_c = mlp_setup(b, cfg, seed=seed + 1, precision=precision)
    pf, par_f, _, packed_f = mlp_setup(b, cfg, seed=seed + 2, precision=precision)
    ro = torch.tensor([0.2, -0.1, 4.0]).expand(n, 3) + 0.05 * torch.randn(n, 3, generator=gen)
    rd = torch.randn(n, 3, generator=gen) * 0.3
    rd[:, 2] = -1.0
    rays = O.pack_rays(ro, rd, 2.0, 6.0, rd if cfg["use_viewdirs"] else None)
    rand = dict(t_rand=torch.rand(n, nc, generator=gen), noise_coarse=torch.randn(n, nc, generator=gen),
                u=torch.rand(n, nf, generator=gen), noise_fine=torch.randn(n, nc + nf, generator=gen))
    opt = dict(num_coarse=nc, num_fine=nf, perturb=True, lindisp=False, white_background=white, noise_std=noise)
    tgt = torch.rand(n, 3, generator=gen)
    if with_grads:
        par_c = {k: v.requires_grad_(True) for k, v in par_c.items()}
        par_f = {k: v.requires_grad_(True) for k, v in par_f.items()}
    want = O.render_rays(rays, par_c, par_f, cfg, cfg, opt, rand)
    rnp = {k: v.numpy() for k, v in rand.items()}
    out = b.render(pc, pf, packed_c, packed_f, rays.numpy(), opt, rnp, training=with_grads)
    # Coarse pass: fp32 round-off only.  Fine pass: the inverse CDF amplifies ulp-level differences of the coarse
    # weights (measured on MI355X, 8x256 random init, 256 rays: HIP-vs-CPU rgb_fine 1.5e-5 / acc_fine 2.9e-5, while
    # PyTorch-ROCm-vs-CPU is 2.7e-5 / 5.3e-5; profiles/r01_error_floor.txt) -- rgb keeps the 1e-4 north-star bar.
    for k in ("rgb_coarse", "acc_coarse", "depth_coarse"):
        close(out[k], want[k].detach().numpy(), 1e-5, what="render %s" % k)
    close(out["rgb_fine"], want["rgb_fine"].detach().numpy(), tol, what="render rgb_fine")
    close(out["acc_fine"], want["acc_fine"].detach().numpy(), 5 * tol, what="render acc_fine")
    close(out["depth_fine"], want["depth_fine"].detach().numpy(), 20 * tol, what="render depth_fine")
    if with_grads:
        loss, _, _, _ = O.loss_and_psnr(want["rgb_coarse"], want["rgb_fine"], tgt)
        loss.backward()
        l3, gc, gf = b.mse_loss(out["rgb_coarse"], out["rgb_fine"], tgt.numpy())
        assert abs(float(l3[2]) - float(loss)) < 1e-5
        out = b.render(pc, pf, packed_c, packed_f, rays.numpy(), opt, rnp, training=True, g_rgb=(gc, gf))
        # coarse-net gradients are tight; fine-net gradients inherit the sampler's conditioning (ReLU-mask flips when
        # a fine sample moves): any two fp32 implementations differ by ~1e-3 there (see DESIGN.md "parity tolerances").
        # (1e-3 for the coarse net: with noise_std up to 1.0 and a white background the per-sample cotangents nearly
        # cancel in the early layers; the teacher-forced case_mlp_backward keeps the tight 2e-5 bound on the kernels.)
        case = "render_vs_oracle_%s_%s" % (tag or n, b.name)
        for plan, par, key, gt in ((pc, par_c, "g_params_coarse", grad_tol[0]), (pf, par_f, "g_params_fine", grad_tol[1])):
            grads = b.unflatten(plan, out[key])
            if isinstance(gt, dict):
                # coarse net (no sampler in front): held to the fp64 yardstick -- no further from an fp64 run of the oracle than the oracle's
                # own fp32 run is (x mul + add), per tensor, of max|g|
                assert key == "g_params_coarse"
                p64 = {k: v.detach().double().requires_grad_(True) for k, v in par_c.items()}
                o64 = O.render_rays(rays.double(), p64, None, cfg, cfg, dict(opt, num_fine=0), {k: v.double() for k, v in rand.items()})
                torch.nn.functional.mse_loss(o64["rgb_coarse"], tgt.double()).backward()
                for k, v in grads.items():
                    ref = p64[k].grad.numpy()
                    scale = float(np.abs(ref).max()) + 1e-30
                    e_hip = float(np.abs(np.asarray(v, np.float64) - ref).max()) / scale
                    e_t32 = float(np.abs(par[k].grad.numpy().astype(np.float64) - ref).max()) / scale
                    note(case, **{"coarse_vs_fp64 " + k: e_hip, "torch_fp32_vs_fp64 " + k: e_t32})
                    assert TL.within(e_hip, e_t32, gt), (case, k, e_hip, e_t32, gt)
                continue
            for k, v in grads.items():
                grad_close(v, par[k].grad.numpy(), gt, "grad %s %s" % (key, k), case, key)
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


def case_render_f16x3(b, cfg, n, nc, nf, seed=5, white=False, noise=0.0, tag="", precision=F16X3):
    """Inference render (training = 0) with both nets on NERFHIP_PRECISION_F16X3 plans against the oracle, beside the fp32 plans'
    result on the same inputs: the coarse pass at fp32 round-off, the fine pass inside the north-star bar like the fp32 kernels."""
    gen = rng(seed)
    ro = torch.tensor([0.2, -0.1, 4.0]).expand(n, 3) + 0.05 * torch.randn(n, 3, generator=gen)
    rd = torch.randn(n, 3, generator=gen) * 0.3
    rd[:, 2] = -1.0
    rays = O.pack_rays(ro, rd, 2.0, 6.0, rd if cfg["use_viewdirs"] else None)
    rand = dict(t_rand=torch.rand(n, nc, generator=gen), noise_coarse=torch.randn(n, nc, generator=gen),
                u=torch.rand(n, nf, generator=gen), noise_fine=torch.randn(n, nc + nf, generator=gen))
    opt = dict(num_coarse=nc, num_fine=nf, perturb=True, lindisp=False, white_background=white, noise_std=noise)
    rnp = {k: v.numpy() for k, v in rand.items()}
    outs = {}
    for prec in (0, precision):
        pc, par_c, _, packed_c = mlp_setup(b, cfg, seed=seed + 1, precision=prec)
        pf, par_f, _, packed_f = mlp_setup(b, cfg, seed=seed + 2, precision=prec)
        outs[prec] = b.render(pc, pf, packed_c, packed_f, rays.numpy(), opt, rnp, training=False)
        if prec:  # a training render is refused
            with pytest.raises(L.NerfHipError, match="inference-only"):
                b.render(pc, pf, packed_c, packed_f, rays.numpy(), opt, rnp, training=True)
        b.lib.plan_destroy(pc)
        b.lib.plan_destroy(pf)
    want = O.render_rays(rays, par_c, par_f, cfg, cfg, opt, rand)
    rec = {}
    for k in ("rgb_coarse", "acc_coarse", "rgb_fine", "acc_fine", "depth_fine"):
        w = want[k].detach().numpy()
        for prec, nm in ((0, "fp32"), (precision, "f16x3")):
            e = np.abs(outs[prec][k] - w).reshape(n, -1).max(axis=1)
            rec["%s_%s_max" % (k, nm)] = float(e.max())
            rec["%s_%s_rays_over_1e-4" % (k, nm)] = int((e > 1e-4).sum())
    note("render_f16x3_%s_%s" % (tag or n, b.name), rays=n, **rec)
    assert rec["rgb_coarse_f16x3_max"] <= 1e-5 and rec["acc_coarse_f16x3_max"] <= 1e-5, rec
    assert rec["rgb_fine_f16x3_max"] <= max(1e-4, 2 * rec["rgb_fine_fp32_max"]), rec
    assert rec["rgb_fine_f16x3_rays_over_1e-4"] <= 2 * rec["rgb_fine_fp32_rays_over_1e-4"] + 1, rec


def case_ray_grad(b, cfg, n=24, nc=16, nf=16, seed=61, white=False, noise=0.0, compact=False):
    """nerfhip_render_bwd_rays: d(loss)/d(rays) -- origin, direction and viewdirs columns -- against the oracle's autograd
    (nerf/train_utils.py:67,107: pts = ro + rd * z;  nerf/volume_rendering_utils.py:24: dists * ||rd||).
    compact (True / "recompute"): the same with both plans' backward compacted -- the d(pre-activation) images the input gradient
    is formed from are then in list order, and the samples the list dropped contribute exactly nothing."""
    gen = rng(seed)
    pc, par_c, flat_c, packed_c = mlp_setup(b, cfg, seed=seed + 1)
    pf, par_f, flat_f, packed_f = mlp_setup(b, cfg, seed=seed + 2)
    b.set_compaction(pc, compact)
    b.set_compaction(pf, compact)
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
    ref = rays.grad.numpy()
    # the yardstick: the same autograd in fp64.  Ray gradients are ill-conditioned (d/dp of sin(2^9 p), ReLU branches decided
    # by round-off): the oracle's OWN fp32 run differs from its fp64 run by 1e-2 of max|g| on a few per cent of the rays
    # (measured: 15 of 256 rays beyond 2e-3, median 1.5e-5), so the kernel is held to that distribution, not to a max
    r64 = rays.detach().double().requires_grad_(True)
    w64 = O.render_rays(r64, {k: v.double() for k, v in par_c.items()}, {k: v.double() for k, v in par_f.items()}, cfg, cfg, opt,
                        {k: v.double() for k, v in rand.items()})
    l64, _, _, _ = O.loss_and_psnr(w64["rgb_coarse"], w64["rgb_fine"], tgt.double())
    l64.backward()
    ref64 = r64.grad.numpy()
    rnp = {k: v.numpy() for k, v in rand.items()}
    rays_np = rays.detach().numpy()
    out = b.render(pc, pf, packed_c, packed_f, rays_np, opt, rnp, training=True)
    l3, gc, gf = b.mse_loss(out["rgb_coarse"], out["rgb_fine"], tgt.numpy())
    out = b.render(pc, pf, packed_c, packed_f, rays_np, opt, rnp, training=True, g_rgb=(gc, gf), ray_grad_params=(flat_c, flat_f))
    got = out["g_rays"]
    # (near / far, columns 6 and 7, are constants of the ray here; the oracle's autograd also differentiates the depths)
    rec = {}
    # (not vacuous, from the reference alone: most rays have a gradient -- with none the medians below are 0 <= 2e-6 whatever the kernel gives)
    live = float(np.any(ref64[:, 0:3] != 0.0, axis=1).mean())
    assert np.isfinite(ref64).all() and live >= 0.9, "%.2f of the rays have a gradient in the fp64 reference" % live
    for lo, hi, what in ((0, 3, "origin"), (3, 6, "direction")) + (((8, 11, "viewdirs"),) if view else ()):
        scale = float(np.abs(ref64[:, lo:hi]).max())
        assert scale > 0.0, "the fp64 reference has no %s gradient" % what
        e_hip = np.abs(got[:, lo:hi] - ref[:, lo:hi]).max(axis=1) / scale            # kernel vs the oracle's fp32 autograd
        e_yard = np.abs(ref[:, lo:hi] - ref64[:, lo:hi]).max(axis=1) / scale         # the oracle's fp32 vs its fp64 autograd
        rec[what] = dict(hip_median=float(np.median(e_hip)), yard_median=float(np.median(e_yard)), hip_over=int((e_hip > 2e-3).sum()),
                         yard_over=int((e_yard > 2e-3).sum()), hip_max=float(e_hip.max()), yard_max=float(e_yard.max()))
        assert np.median(e_hip) <= 3.0 * np.median(e_yard) + 2e-6, (what, rec[what])
        assert (e_hip > 2e-3).sum() <= 2 * (e_yard > 2e-3).sum() + 3, (what, rec[what])
    note("ray_grad_%dx%d_n%d%s_%s" % (cfg["num_layers"], cfg["hidden_size"], n, "_%s" % compact if compact else "", b.name), **{"%s_%s" % (w_, k): v for w_, d in rec.items()
                                                                                            for k, v in d.items()})
    assert np.all(got[:, 6:8] == 0.0)
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


def case_internal_rng(b):
    """Production mode (in-kernel Philox) == parity mode fed with nerfhip_rng_fill's numbers."""
    cfg = MLP_GEOMETRIES["default4x128"]
    n, nc, nf, seed, off = 6, 32, 32, 1234, 17
    pc, _, _, packed_c = mlp_setup(b, cfg, seed=7)
    pf, _, _, packed_f = mlp_setup(b, cfg, seed=8)
    gen = rng(2)
    ro = torch.tensor([0., 0., 4.0]).expand(n, 3) + 0.05 * torch.randn(n, 3, generator=gen)
    rd = torch.randn(n, 3, generator=gen) * 0.3
    rd[:, 2] = -1.0
    rays = O.pack_rays(ro, rd, 2.0, 6.0, rd).numpy()
    opt = dict(num_coarse=nc, num_fine=nf, perturb=True, lindisp=False, white_background=False, noise_std=0.5)
    a = b.render(pc, pf, packed_c, packed_f, rays, opt, None, seed=seed, ray_offset=off)
    rand = dict(t_rand=b.rng_fill(0, seed, 0, off * nc, n * nc).reshape(n, nc),
                noise_coarse=b.rng_fill(1, seed, 1, off * nc, n * nc).reshape(n, nc),
                u=b.rng_fill(0, seed, 2, off * nf, n * nf).reshape(n, nf),
                noise_fine=b.rng_fill(1, seed, 3, off * (nc + nf), n * (nc + nf)).reshape(n, nc + nf))
    c = b.render(pc, pf, packed_c, packed_f, rays, opt, rand)
    for k in ("rgb_coarse", "rgb_fine", "depth_fine", "acc_fine"):
        assert np.array_equal(a[k], c[k], equal_nan=True), k
    nrm = b.rng_fill(1, 5, 1, 0, 20000)
    assert abs(float(nrm.mean())) < 0.03 and abs(float(nrm.std()) - 1.0) < 0.03
    b.lib.plan_destroy(pc)
    b.lib.plan_destroy(pf)


def case_loss_adam(b):
    gen = rng(77)
    n = 333
    rc, rf, tg = torch.rand(n, 3, generator=gen), torch.rand(n, 3, generator=gen), torch.rand(n, 4, generator=gen)
    rc.requires_grad_(True)
    rf.requires_grad_(True)
    loss, lc, lf, _ = O.loss_and_psnr(rc, rf, tg)
    loss.backward()
    l3, gc, gf = b.mse_loss(rc.detach().numpy(), rf.detach().numpy(), tg.numpy())
    close(l3, [float(lc), float(lf), float(loss)], 1e-7, 1e-6, what="loss")
    close(gc, rc.grad.numpy(), 1e-9, 1e-6, what="g_rgb_coarse")
    close(gf, rf.grad.numpy(), 1e-9, 1e-6, what="g_rgb_fine")
    p = torch.randn(5000, generator=gen)
    m, v = torch.zeros(5000), torch.zeros(5000)
    pp, mm, vv = p.numpy().copy(), m.numpy().copy(), v.numpy().copy()
    for step in (1, 2, 3):
        gr = torch.randn(5000, generator=gen)
        O.adam_step(p, gr, m, v, step, 5e-3)
        pp, mm, vv = b.adam_step(pp, gr.numpy(), mm, vv, 5e-3, step)
        close(pp, p.numpy(), 1e-7, 1e-6, what="adam step %d" % step)


# ---- edge cases -----------------------------------------------------------------------------------------------------------
def case_edges(b):
    """Empty and ragged inputs, single samples, minimal bin counts, ties exactly at CDF values."""
    z0 = np.zeros((0, 3), np.float32)
    # empty inputs: every entry point accepts n == 0 / m == 0 and launches nothing
    assert b.cumprod_exclusive(np.zeros((0, 5), np.float32)).shape == (0, 5)
    assert b.pack_rays(z0, z0, 2.0, 6.0, z0).shape == (0, 11)
    assert b.positional_encoding(z0, O.frequency_bands(4).numpy(), True).shape == (0, 27)
    assert b.stratified_z(np.zeros((0, 11), np.float32), torch.linspace(0, 1, 8).numpy(), False, False).shape == (0, 8)
    r = b.volume_render_fwd(np.zeros((0, 4, 4), np.float32), np.zeros((0, 4), np.float32), z0)
    assert r[0].shape == (0, 3) and r[3].shape == (0, 4)
    s, i, c = b.sample_pdf(np.zeros((0, 5), np.float32), np.zeros((0, 4), np.float32), 3, det=True)
    assert s.shape == (0, 3)
    # one sample per ray: the only interval is the 1e10 tail
    raw = np.array([[[0.3, -0.2, 1.0, 0.7]], [[0.1, 0.1, 0.1, -0.5]]], np.float32)
    z = np.array([[3.0], [4.0]], np.float32)
    rd = np.array([[0, 0, -1.0], [0.5, 0, -1.0]], np.float32)
    got = b.volume_render_fwd(raw, z, rd)
    want = O.volume_render(T(raw), T(z), T(rd))
    for g_, w_ in zip(got, want):
        close(g_, w_.numpy(), 2e-6, 2e-6, what="single-sample render")
    close(b.cumprod_exclusive(np.array([[5.0], [7.0]], np.float32)), [[1.0], [1.0]], 0, what="cumprod cols=1")
    # one coarse sample (linspace(0,1,1) == [0]) with and without perturbation
    rays = np.zeros((3, 11), np.float32)
    rays[:, 6], rays[:, 7] = 2.0, 6.0
    tr = torch.rand(3, 1, generator=rng(1))
    t1 = torch.linspace(0, 1, 1).numpy()
    close(b.stratified_z(rays, t1, False, True, tr.numpy()), O.stratified_z(T(rays[:, 6:7]), T(rays[:, 7:8]), 1, False, True, tr).numpy(), 0,
          what="stratified nc=1")
    # minimal pdf: two bins / one weight; flat pdf (all-zero weights); u exactly on CDF entries (ties -> side="right")
    bins = np.array([[1.0, 2.0]], np.float32)
    s, i, c = b.sample_pdf(bins, np.array([[0.0]], np.float32), 4, u=np.array([[0.0, 0.5, 1.0, 0.999]], np.float32))
    ws, wi, wc = O.sample_pdf(T(bins), torch.zeros(1, 1), 4, u=torch.tensor([[0.0, 0.5, 1.0, 0.999]]), return_aux=True)
    assert np.array_equal(i, wi.numpy()) and np.array_equal(c, wc.numpy())
    close(s, ws.numpy(), 1e-6, what="two-bin samples")
    bins = torch.sort(torch.rand(4, 9, generator=rng(2)) * 3 + 1, -1)[0].numpy()
    w = np.zeros((4, 8), np.float32)
    s, i, c = b.sample_pdf(bins, w, 16, det=True)
    ws, wi, wc = O.sample_pdf(T(bins), T(w), 16, det=True, return_aux=True)
    close(c, wc.numpy(), 2.5e-7, what="flat cdf")
    close(s, ws.numpy(), 1e-5, what="flat pdf samples")
    w = (torch.rand(4, 8, generator=rng(3)) ** 2).numpy()
    _, _, cdf = b.sample_pdf(bins, w, 9, u=np.zeros((4, 9), np.float32))
    _, inds, _ = b.sample_pdf(bins, w, 9, u=cdf.copy())       # every u sits exactly on a CDF entry
    assert np.array_equal(inds, torch.searchsorted(T(cdf), T(cdf), right=True).numpy())
    # minimal hierarchical step: 3 coarse samples (one interior weight), 1 fine sample
    zc = np.array([[2.0, 3.0, 5.0]], np.float32)
    wf = np.array([[0.2, 0.5, 0.3]], np.float32)
    zs, zf = b.hierarchical_z(zc, wf, 1, u=np.array([[0.4]], np.float32))
    wzs, wzf = O.hierarchical_z(T(zc), T(wf), 1, u=torch.tensor([[0.4]]))
    close(zf, wzf.numpy(), 1e-6, what="minimal hierarchical")
    # ragged MLP row counts: 1 row, and one more than a workgroup tile
    cfg = MLP_GEOMETRIES["default4x128"]
    plan, params, flat, packed = mlp_setup(b, cfg, seed=5)
    for m in (1, 129):
        x = torch.randn(m, 90, generator=rng(m))
        got, _ = b.mlp_fwd(plan, packed, x.numpy())
        close(got, O.mlp_forward(params, x, cfg).numpy(), 2e-5, 2e-5, what="mlp m=%d" % m)
    b.lib.plan_destroy(plan)


# ---- rows either side of the path ----------------------------------------------------------------
def case_select(b):
    """Training-ray selection: given the reference's select indices the fused kernel must equal the reference's
    gathers (golden, recorded from its get_ray_bundle / meshgrid_xy) followed by its ray packing; with its own draw
    the indices must equal the restated permutation and be distinct."""
    import select_oracle as S
    g = gold("dataio.npz")
    for tag in "ab":
        H, W, focal, C_ = g["sel_%s_hwfc" % tag]
        H, W = int(H), int(W)
        pose, img, inds = g["sel_%s_pose" % tag], g["sel_%s_img" % tag], g["sel_%s_inds" % tag]
        ro, rd, tgt = T(g["sel_%s_ro" % tag]), T(g["sel_%s_rd" % tag]), g["sel_%s_target" % tag]
        for use_viewdirs in (True, False):
            rays, t, used = b.select_rays(H, W, focal, pose, img, len(inds), 2.0, 6.0, inds=inds, use_viewdirs=use_viewdirs)
            want = O.pack_rays(ro, rd, 2.0, 6.0, rd if use_viewdirs else None).numpy()
            close(rays, want, 1e-6, what="select rays " + tag)
            assert np.array_equal(t, tgt) and np.array_equal(used, inds)
        # NDC variant: viewdirs from the pre-NDC directions, ndc_rays(H, W, focal, 1.0, ...) (train_utils.py:143-168)
        rays, _, _ = b.select_rays(H, W, focal, pose, None, len(inds), 0.0, 1.0, inds=inds, ndc=True)
        no, nd = O.ndc_rays(H, W, focal, 1.0, ro, rd)
        close(rays, O.pack_rays(no, nd, 0.0, 1.0, rd).numpy(), 1e-5, 1e-5, what="select rays ndc " + tag)
        # same bits as the unit kernels (ray_bundle at those pixels -> pack_rays)
        pix = (inds % H) * W + inds // H
        uro, urd = b.ray_bundle(H, W, focal, pose, pix)
        rays, _, _ = b.select_rays(H, W, focal, pose, None, len(inds), 2.0, 6.0, inds=inds)
        close(rays, b.pack_rays(uro, urd, 2.0, 6.0, urd), 0, what="select == unit kernels")
        # the oracle restatement of the selection agrees with the golden as well
        oro, ord_, otg = O.select_training_rays(H, W, focal, T(pose)[:3, :4], T(img), inds)
        assert torch.equal(oro, ro) and torch.equal(ord_, rd) and np.array_equal(otg.numpy(), tgt)
        # cached branch: rows of the stored bundle
        full_o, full_d = O.get_ray_bundle(H, W, focal, T(pose)[:3, :4])
        bundle = torch.stack([full_o, full_d], 0)
        cro, crd, ctg = O.select_cached_rays(bundle, T(img), inds)
        rays, t, _ = b.select_cached_rays(H, W, focal, full_o.reshape(-1, 3).numpy(), full_d.reshape(-1, 3).numpy(),
                                          np.ascontiguousarray(img.reshape(-1, img.shape[-1])), len(inds), 2.0, 6.0, inds=inds)
        close(rays, O.pack_rays(cro, crd, 2.0, 6.0, crd).numpy(), 1e-6, what="cached rays " + tag)
        assert np.array_equal(t[:, :3], ctg.numpy())
    # own draw: bit-exact against the restated permutation; a bijection over the whole population
    for (seed, step, pop) in ((1, 0, 35), (7, 123456789012, 1000), (2 ** 63 + 5, 3, 1), (3, 9, 2), (4, 4, 4096)):
        got = b.select_indices(seed, step, pop, 0, pop)
        assert np.array_equal(got, S.select_indices(seed, step, pop, 0, pop)), (seed, step, pop)
        assert np.array_equal(np.sort(got), np.arange(pop))
    part = b.select_indices(7, 5, 160000, 4096, 512)
    assert np.array_equal(part, S.select_indices(7, 5, 160000, 4096, 512))
    rays, t, used = b.select_rays(20, 16, 14.4, g["sel_b_pose"], g["sel_b_img"], 64, 2.0, 6.0, seed=11, step=3, first=64)
    assert np.array_equal(used, S.select_indices(11, 3, 320, 64, 64))
    assert np.array_equal(t, g["sel_b_img"][used % 20, used // 20])
    # Philox stream of nerfhip_rng_fill against the restated generator (itself pinned on the Random123 vectors)
    assert np.array_equal(b.rng_fill(0, 0xDEADBEEFCAFE, 2, 2 ** 33 + 1, 64), S.uniform(0xDEADBEEFCAFE, 2, 2 ** 33 + 1, 64))


def case_select_uniformity(b):
    """Statistical sanity of the draw at the headline size: 4096 of 160000 pixels, many steps -> every pixel's hit
    count is Binomial(steps, 4096/160000); chi-square over 400 coarse cells within 5 sigma; no repeats in a batch."""
    pop, n, steps = 160000, 4096, 48
    counts = np.zeros(400)
    for s in range(steps):
        idx = b.select_indices(42, s, pop, 0, n)
        assert len(np.unique(idx)) == n and idx.min() >= 0 and idx.max() < pop
        counts += np.bincount(idx // 400, minlength=400)
    expected = steps * n / 400.0
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    assert abs(chi2 - 399) < 5 * np.sqrt(2 * 399), chi2
    # consecutive steps are unrelated: overlap of two batches ~ n*n/pop = 105 +- 5 sigma
    a, c = b.select_indices(42, 0, pop, 0, n), b.select_indices(42, 1, pop, 0, n)
    ov = len(np.intersect1d(a, c))
    assert abs(ov - n * n / pop) < 5 * np.sqrt(n * n / pop), ov


def case_image_output(b):
    g = gold("dataio.npz")
    assert np.array_equal(b.cast_to_image(g["img_in"]), g["img_out"])
    assert np.array_equal(O.cast_to_image(T(g["img_in"])), g["img_out"])
    rgba = np.concatenate([g["img_in"], np.ones_like(g["img_in"][..., :1])], -1)
    assert np.array_equal(b.cast_to_image(rgba), g["img_out"])
    for i in range(4):
        assert np.array_equal(b.cast_to_disparity_image(g["disp%d_in" % i]), g["disp%d_out" % i]), i
        assert np.array_equal(O.cast_to_disparity_image(T(g["disp%d_in" % i])), g["disp%d_out" % i]), i
    big = (torch.rand(300, 217, generator=rng(4)) * 5).numpy()      # more than one pass of the 1024-thread reduction
    assert np.array_equal(b.cast_to_disparity_image(big), O.cast_to_disparity_image(T(big)))
    x = (torch.rand(64, 50, 3, generator=rng(6)) * 1.003).numpy()        # whole defined range of the byte conversion
    assert np.array_equal(b.cast_to_image(x), O.cast_to_image(T(x)))
    # outside [0, 256) the host conversion is undefined behaviour; the library defines it as x86-64 does (truncate to
    # int32, keep the low byte; NaN -> 0)
    odd = np.array([[[-1.0, 2.0, np.nan], [1e20, -0.001, 256.5 / 255]]], np.float32)
    assert np.array_equal(b.cast_to_image(odd), np.array([[[1, 254, 0], [0, 0, 0]]], np.uint8))
