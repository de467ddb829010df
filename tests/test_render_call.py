"""nerf_pytorch_amd.render_call.RenderCall against the C ABI spelled by hand: the ONE place outside render_call.py that states the
argument lists of the fused render's entry points (include/nerfhip.h), independently of it.  Every RenderCall method must give, bit
for bit, what the same entry point gives when it is called raw through lib.* with every argument written out here -- on the wave
emulator (no GPU) and on the product library (marked gpu).  The problem is the smallest two-net render the case files use: two
4 x 64 nets with view directions, 5 rays, 8 + 5 samples, sigma noise on, all four draws given."""
import ctypes as C

import numpy as np
import pytest

import nerf_pytorch_amd._lib as L
import occupancy_cases as OC
import parity_cases as P
from nerf_pytorch_amd.render_call import RenderCall

NC, SEED, OFFSET, NOISE = 8, 11, 3, 0.3
BOTH = L.PART_COARSE | L.PART_FINE
MAPS = ("rgb_coarse", "disp_coarse", "acc_coarse", "depth_coarse", "rgb_fine", "disp_fine", "acc_fine", "depth_fine")
REGIONS = ("z_coarse", "raw_coarse", "weights_coarse", "bwd_scratch_coarse", "bwd_g_raw_coarse", "z_fine", "raw_fine", "bwd_scratch_fine",
           "bwd_g_raw_fine")


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    return request.getfixturevalue(request.param)


class Problem:
    """The inputs on the device, shared by the two sides; each side gets outputs and a workspace of its own (side())."""

    def __init__(self, b, nf=5, n=5, layout=1):
        self.b, self.n, self.nf, self.layout = b, n, nf, layout
        net = P.MLP_GEOMETRIES["llff4x64_skip3_L6"]
        self.pc, _, flat_c, self.packed_c = P.mlp_setup(b, net, seed=3)
        self.pf, _, flat_f, self.packed_f = P.mlp_setup(b, net, seed=4) if nf > 0 else (None,) * 4
        rays, rand = OC.render_inputs(net, max(n, 1), NC, nf, seed=21)
        self.stride = rays.shape[1]
        self.cfg = L.RenderCfg(NC, nf, 1, 0, 1, NOISE, self.stride)
        self.rays, self.t_vals, self.u_det = b.dev(rays.numpy()), b.dev(b._linspace01(NC)), b.dev(b._linspace01(nf)) if nf > 0 else None
        self.draws = [b.dev(rand[k].numpy()) if (nf > 0 or k.endswith("coarse") or k == "t_rand") else None
                      for k in ("t_rand", "noise_coarse", "u", "noise_fine")]
        self.flats = (b.dev(flat_c), b.devopt(flat_f))
        rng = np.random.default_rng(5)   # (six cotangents, in the struct's order)
        self.cot = [b.dev(rng.standard_normal((n, 3) if i in (0, 3) else (n,)).astype(np.float32)) for i in range(6)]
        self.wsb = b.lib.render_workspace_bytes(self.pc, self.pf, C.byref(self.cfg), n, layout)
        self.tb_rays = b.lib.render_bwd_rays_tmp_bytes(self.pc, self.pf, C.byref(self.cfg), n)
        self.tb_frozen = b.lib.render_grad_rays_tmp_bytes(self.pc, self.pf, C.byref(self.cfg), n)
        assert min(self.wsb, self.tb_rays, self.tb_frozen) >= 0

    def side(self):
        """Fresh outputs, all NaN-filled: maps, workspace, gradients, tmp, g_rays, spread losses and weight cotangents."""
        b, n = self.b, self.n
        return dict(maps=[b.empty((n, 3) if k.startswith("rgb") else (n,)) for k in MAPS], ws=b.empty((self.wsb // 4 + 1,)),
                    gpc=b.empty((b.lib.plan_num_params(self.pc),)), gpf=b.empty((b.lib.plan_num_params(self.pf),)) if self.nf > 0 else None,
                    tmp=b.empty((max(self.tb_rays, self.tb_frozen) // 4 + 4,)), g_rays=b.empty((n, self.stride)),
                    loss=[b.empty((n,)), b.empty((n,))], gw=[b.empty((n, NC)), b.empty((n, NC + self.nf))])

    def call(self, s):
        b = self.b
        return RenderCall(b.lib, self.pc, self.pf, self.cfg, b.ptr(self.rays), self.n, b.ptr(self.packed_c), b.p(self.packed_f),
                          b.ptr(self.t_vals), b.p(self.u_det), [b.p(d) for d in self.draws], SEED, OFFSET, self.layout, b.ptr(s["ws"]),
                          self.wsb)

    def destroy(self):
        for p in (self.pc, self.pf):
            if p is not None:
                self.b.lib.plan_destroy(p)


def raw_forward(q, s):
    b = q.b
    rr, out = L.RenderRand(*[b.p(d) for d in q.draws]), L.RenderOut(*[b.ptr(m) for m in s["maps"]])
    b.lib.render_fwd_parts(q.pc, q.pf, C.byref(q.cfg), b.ptr(q.rays), q.n, b.ptr(q.packed_c), b.p(q.packed_f), b.ptr(q.t_vals),
                           b.p(q.u_det), C.byref(rr), SEED, OFFSET, C.byref(out), b.ptr(s["ws"]), q.wsb, q.layout, BOTH, b.stream())


def raw_backward(q, s, form, parts):
    """The backward entry point of `form`; parts: with NERFHIP_PART_SHARED_BWD where the layout shares."""
    b = q.b
    rr, six = L.RenderRand(*[b.p(d) for d in q.draws]), [b.ptr(c) for c in q.cot]
    cot, cot_w = L.RenderCotangents(*six), L.RenderCotangentsW(*six, b.ptr(s["gw"][0]), b.ptr(s["gw"][1]))
    head = (q.pc, q.pf, C.byref(q.cfg), b.ptr(q.rays), q.n, b.ptr(q.packed_c), b.p(q.packed_f), C.byref(rr), SEED, OFFSET)
    ws, grads = (b.ptr(s["ws"]), q.wsb), (b.ptr(s["gpc"]), b.p(s["gpf"]))
    flats, tmp, g_rays = (b.ptr(q.flats[0]), b.p(q.flats[1])), b.ptr(s["tmp"]), b.ptr(s["g_rays"])
    if form == "parts":
        b.lib.render_bwd_parts(*head, C.byref(cot), *ws, *grads, parts, b.stream())
    elif form == "parts_w":
        b.lib.render_bwd_parts_w(*head, C.byref(cot_w), *ws, *grads, parts, b.stream())
    elif form == "rays":
        b.lib.render_bwd_rays(*head, C.byref(cot), *ws, *grads, parts, *flats, tmp, q.tb_rays, g_rays, b.stream())
    elif form == "rays_w":
        b.lib.render_bwd_rays_w(*head, C.byref(cot_w), *ws, *grads, parts, *flats, tmp, q.tb_rays, g_rays, b.stream())
    else:   # (frozen: no gradient slices)
        b.lib.render_grad_rays(*head, C.byref(cot), *ws, parts, *flats, tmp, q.tb_frozen, g_rays, b.stream())


def raw_region(q, name):
    off, nb = C.c_int64(), C.c_int64()
    rc = q.b.lib._dll.nerfhip_render_workspace_region(q.pc, q.pf, C.byref(q.cfg), q.n, q.layout, name.encode(), C.byref(off), C.byref(nb))
    return rc, (off.value, nb.value)


def raw_spread(q, s, fine, scale, g_loss):
    """nerfhip_spread_loss on the pass's raw rows and depths in the workspace: its noise, RNG stream 1 (coarse) / 3 (fine)."""
    b = q.b
    tag, S, noise, rng_stream = ("fine", NC + q.nf, q.draws[3], 3) if fine else ("coarse", NC, q.draws[1], 1)
    b.lib.spread_loss(b.ptr(s["ws"]) + raw_region(q, "raw_" + tag)[1][0], b.ptr(s["ws"]) + raw_region(q, "z_" + tag)[1][0], b.ptr(q.rays),
                      q.stride, q.n, S, NOISE, b.ptr(noise), SEED, rng_stream, OFFSET, scale, b.ptr(g_loss), b.ptr(s["loss"][fine]),
                      b.ptr(s["gw"][fine]), b.stream())


def same(b, got, want, what):
    g = np.array(b.host(got), copy=True)   # (the emulator's host() is the buffer itself)
    assert np.array_equal(g, np.asarray(b.host(want)), equal_nan=True), what
    return g


@pytest.mark.parametrize("layout", [1, 2])
def test_forward_spread_and_every_backward_form_equal_the_raw_calls(backend, layout):
    b = backend
    q = Problem(b, layout=layout)
    new, raw = q.side(), q.side()
    call = q.call(new)
    g_loss = b.dev(np.linspace(0.5, 1.5, q.n).astype(np.float32))

    def forwards():
        call.forward([b.ptr(m) for m in new["maps"]], BOTH, b.stream())
        raw_forward(q, raw)
        for k, m_new, m_raw in zip(MAPS, new["maps"], raw["maps"]):
            assert not np.isnan(same(b, m_new, m_raw, "forward " + k)).any(), k

    forwards()
    for fine in (0, 1):   # (fills both sides' weight cotangents: what the _w forms below take)
        call.spread(fine, 0.25, b.ptr(g_loss), b.ptr(new["loss"][fine]), b.ptr(new["gw"][fine]), b.stream())
        raw_spread(q, raw, fine, 0.25, g_loss)
        assert same(b, new["loss"][fine], raw["loss"][fine], "spread loss %d" % fine).all()
        assert same(b, new["gw"][fine], raw["gw"][fine], "spread g_weights %d" % fine).any()
    cot, grads, gw = [b.ptr(c) for c in q.cot], (b.ptr(new["gpc"]), b.ptr(new["gpf"])), (b.ptr(new["gw"][0]), b.ptr(new["gw"][1]))
    rays = (b.ptr(q.flats[0]), b.ptr(q.flats[1]), b.ptr(new["tmp"]), q.tb_rays, b.ptr(new["g_rays"]))
    frozen = rays[:3] + (q.tb_frozen,) + rays[4:]
    forms = dict(parts={}, parts_w=dict(g_weights=gw), rays=dict(rays=rays), rays_w=dict(g_weights=gw, rays=rays),
                 frozen=dict(rays=frozen, frozen=True))
    seen = {}
    for form, kw in forms.items():
        for parts in (BOTH, L.PART_FINE) if form == "parts" else (BOTH,):
            if seen:   # (a backward may use up what the forward left: every form runs over a forward of its own)
                forwards()
            for s in (new, raw):
                for k in ("gpc", "gpf", "g_rays"):
                    s[k][...] = float("nan")
            call.backward(cot, None if form == "frozen" else grads, parts, b.stream(), **kw)
            raw_backward(q, raw, form, parts | (L.PART_SHARED_BWD if layout == 2 else 0))
            gc, gf, gr = (same(b, new[k], raw[k], form + " " + k) for k in ("gpc", "gpf", "g_rays"))
            # (what each form writes, and nothing else: the comparison above is not NaN against NaN where it matters)
            assert np.isnan(gc).all() if (form == "frozen" or parts == L.PART_FINE) else np.isfinite(gc).all() and gc.any(), form
            assert np.isnan(gf).all() if form == "frozen" else np.isfinite(gf).all() and gf.any(), form
            assert np.isnan(gr).all() if form.startswith("parts") else np.isfinite(gr).all() and gr.any(), form
            seen[form, parts] = (gc, gf, gr)
    # the weight cotangent reaches the gradients: the _w forms are not the plain ones
    assert not np.array_equal(seen["parts_w", BOTH][1], seen["parts", BOTH][1])
    assert not np.array_equal(seen["rays_w", BOTH][2], seen["rays", BOTH][2])
    for bad in (dict(), dict(g_weights=gw, rays=frozen)):   # (frozen needs rays and takes no weight cotangent)
        with pytest.raises(ValueError):
            call.backward(cot, None, BOTH, b.stream(), frozen=True, **bad)
    q.destroy()


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_regions_sizes_and_stats_offset_equal_the_raw_calls(backend, layout):
    b = backend
    q = Problem(b, layout=layout)
    call = q.call(q.side())
    assert RenderCall.workspace_bytes(b.lib, q.pc, q.pf, q.cfg, q.n, layout) == q.wsb
    assert RenderCall.tmp_bytes(b.lib, q.pc, q.pf, q.cfg, q.n) == (q.tb_rays, q.tb_frozen) and min(q.tb_rays, q.tb_frozen) > 0
    assert RenderCall.occ_tmp_bytes(b.lib, q.cfg, q.n) == b.lib.render_occ_tmp_bytes(C.byref(q.cfg), q.n) > 0
    for negative in (lambda: RenderCall.workspace_bytes(b.lib, q.pc, q.pf, q.cfg, -1, layout), lambda: RenderCall.occ_tmp_bytes(b.lib, q.cfg, -1),
                     lambda: RenderCall.tmp_bytes(b.lib, q.pc, q.pf, q.cfg, -1), lambda: call.region("no_such_region")):
        with pytest.raises(L.NerfHipError):
            negative()
    for name in REGIONS:
        rc, want = raw_region(q, name)
        if layout == 0 and name.startswith("bwd_"):   # (a training layout's region)
            assert rc != 0
            with pytest.raises(L.NerfHipError):
                call.region(name)
        else:
            assert rc == 0 and call.region(name) == want == call.region(name)   # (the second answer: the cache's)
    for net, plan, samples in (("coarse", q.pc, NC), ("fine", q.pf, NC + q.nf)) if layout else ():
        assert call.stats_offset(net) == raw_region(q, "bwd_scratch_" + net)[1][0] + b.lib.plan_bwd_stats_offset(plan, q.n * samples)
    q.destroy()


def test_a_coarse_net_alone(backend):
    """num_fine = 0 with plan_f = None: the forward and the parts backward."""
    b = backend
    q = Problem(b, nf=0)
    new, raw = q.side(), q.side()
    call = q.call(new)
    call.forward([b.ptr(m) for m in new["maps"]], BOTH, b.stream())
    raw_forward(q, raw)
    for k, m_new, m_raw in zip(MAPS, new["maps"], raw["maps"]):
        assert np.isnan(same(b, m_new, m_raw, "forward " + k)).all() == k.endswith("fine"), k
    call.backward([b.ptr(c) for c in q.cot], (b.ptr(new["gpc"]), None), L.PART_COARSE, b.stream())
    raw_backward(q, raw, "parts", L.PART_COARSE)
    g = same(b, new["gpc"], raw["gpc"], "g_params_coarse")
    assert np.isfinite(g).all() and g.any()
    q.destroy()


def test_no_rays(backend):
    """n = 0: the forward returns OK and touches nothing."""
    b = backend
    q = Problem(b, n=0)
    s = q.side()
    assert q.call(s).forward([b.ptr(m) for m in s["maps"]], BOTH, b.stream()) == 0
    assert np.isnan(np.asarray(b.host(s["ws"]))).all() and all(np.asarray(b.host(m)).size == 0 for m in s["maps"])
    q.destroy()
