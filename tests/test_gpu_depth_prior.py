"""GPU suite (-m gpu) of the depth priors (DS-NeRF's expected-depth and ray-termination losses): the cases of
tests/depth_prior_cases.py on the product library -- every net, both training arithmetics, both render shapes -- and the public
routes: DepthPrior, TrainEngine(depth_loss=) with depth_prior= / depth_rays= on its steps, and the drop-in API's depth_prior=."""
import copy

import numpy as np
import pytest
import torch

import depth_prior_cases as D
import engine_scenes as ES
import spread_cases as S
from conftest import gold

pytestmark = pytest.mark.gpu


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", D.KERNEL_KINDS)
def test_kernel_against_the_definition(gpu, kind):
    D.case_kernel(gpu, kind)


def test_kernel_long_rays(gpu):
    D.check_kernel_sums(gpu, "noise_draws", 2, 2011, 8, seed=7)
    D.check_kernel_sums(gpu, "noise_stream", 3, 8192, 11, seed=8)   # (the largest S the entry point takes)


def test_kernel_refusals(gpu):
    D.case_kernel_refusals(gpu)


# ---- through the render ------------------------------------------------------------------------------------------------------------
NETS = [(net, arith) for arith in D.RENDER_ARITHS for net in D.RENDER_NETS]


@pytest.mark.parametrize("net,arith", NETS)
def test_parameter_gradients_against_the_oracle(gpu, net, arith):
    D.case_param_grads(gpu, net, arith)


@pytest.mark.parametrize("net,arith", NETS)
def test_backward_modes_with_the_depth_cotangent(gpu, net, arith):
    fused = ("fused", "fused_compact", "fused_stash") if (net, arith) == ("w64", "fp32") else ()
    for noise in (0.6, 2.0):   # (two zero fractions of the d(loss)/d(raw) rows)
        D.case_compacted(gpu, net, arith, (True, "recompute") + fused, noise=noise)


def test_culled_step_with_a_prior(gpu):
    D.case_culled_step(gpu, "w64", "fp32", 0)


def test_ray_gradient_with_a_prior(gpu):
    D.case_rays_w(gpu, "w128")


# ---- engine and drop-in ------------------------------------------------------------------------------------------------------------
CFG = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
SAMPLING = dict(num_coarse=64, num_fine=64, perturb=False, white_background=True, noise_std=0.0)
DW = ((0.05, 0.02), (0.1, 0.01))   # ((a, b) coarse, (a, b) fine)
LAM = (0.02, 0.01)


@pytest.fixture(scope="module")
def lego(gpu):
    """The lego-lowres fixture nets, 1024 rays of the fixture pose with a random target, and prior rows on about a third of them."""
    import nerf_pytorch_amd as N
    dev = torch.device("cuda", 0)
    w, r = gold("lego_lowres_weights.npz"), gold("lego_lowres_render.npz")
    mc, mf = N.FlexibleNeRFModel(**CFG), N.FlexibleNeRFModel(**CFG)
    mc.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("c_")})
    mf.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("f_")})
    mc, mf = mc.to(dev), mf.to(dev)
    H = W = 32
    focal = float(r["focal"]) * 32.0 / float(r["W"])
    pose = torch.from_numpy(r["pose"]).to(dev)
    opts = N.make_options(64, 64, perturb=False, white_background=True, radiance_field_noise_std=0.0)
    ro, rd = N.get_rays_at_pixels(H, W, focal, pose[:3, :4], torch.arange(H * W, dtype=torch.int64, device=dev))
    rays = N.pack_rays(ro, rd, opts, H, W, focal)
    target = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    rows_np = D.render_prior(rays.cpu().numpy(), seed=51)
    return dict(N=N, dev=dev, mc=mc, mf=mf, H=H, W=W, focal=focal, pose=pose, opts=opts, ro=ro, rd=rd, rays=rays, target=target,
                rows_np=rows_np, rows=torch.from_numpy(rows_np).to(dev))


def _engine(s, **kw):
    return s["N"].TrainEngine(copy.deepcopy(s["mc"]), copy.deepcopy(s["mf"]), **dict(SAMPLING, **kw))


def test_engine_without_a_prior_is_the_engine(lego):
    s = lego
    engines = [_engine(s), _engine(s, depth_loss=None), _engine(s, depth_loss=(0, 0)), _engine(s, depth_loss=((0.0, 0.0), (0.0, 0.0))),
               _engine(s, depth_loss=DW)]
    for _ in range(3):
        for e in engines:
            e.step(s["rays"], s["target"])
    a = engines[0]
    assert a.grad.abs().max() > 0
    for e in engines[1:]:
        assert e.depth_losses == (None, None)
        assert torch.equal(a.loss, e.loss) and torch.equal(a.grad, e.grad)
        assert torch.equal(a.mc.flat_params, e.mc.flat_params) and torch.equal(a.mf.flat_params, e.mf.flat_params)
    assert all(e._depth_bufs is None for e in engines[:4])


def _by_hand(s, gpu, e, spread=None):
    """One step's C calls on the engine's own plans: forward, the two losses, [spread launch,] depth launch, _w backward."""
    rays, tgt = s["rays"].cpu().numpy(), s["target"].cpu().numpy()
    r = S.RenderW(gpu, e.mc._plan, e.mf._plan, e.packed_c, e.packed_f, rays, SAMPLING, {})
    lc, gc, _ = gpu.mse_loss(r.out["rgb_coarse"], None, tgt)
    lf, gf, _ = gpu.mse_loss(r.out["rgb_fine"], None, tgt)
    gw, dl = [], []
    for fine in (0, 1):
        into = None
        if spread is not None and spread[fine] > 0:
            into = r.spread(bool(fine), spread[fine] / r.n)[1]
        lo, g = D.depth_prior_on(r, bool(fine), s["rows_np"], e.depth_loss[fine], 1.0 / r.n, into=into)
        gw.append(g)
        dl.append(lo)
    want = r.backward((gc, gf), gw, entry="parts_w")
    return want, (lc[0], lf[0]), dl


@pytest.mark.parametrize("overlap", [True, False])
def test_engine_step_is_the_c_entry_points(lego, gpu, overlap):
    """One engine step with both terms on both nets against nerfhip_render_fwd + nerfhip_mse_loss_fwd_bwd + nerfhip_depth_prior_loss +
    nerfhip_render_bwd_parts_w assembled by hand on the engine's own plans: gradient, losses and depth means bit for bit -- and not the
    plain engine's gradient."""
    s = lego
    e, plain = _engine(s, depth_loss=DW, overlap=overlap), _engine(s, overlap=overlap)
    e.forward_backward(s["rays"], s["target"], depth_prior=s["rows"])
    plain.forward_backward(s["rays"], s["target"])
    want, (lc, lf), dl = _by_hand(s, gpu, e)
    grad, loss = e.grad.cpu().numpy(), e.loss.cpu().numpy()
    assert loss[0] == lc and loss[1] == lf
    assert np.array_equal(grad[:e.nc_params], want["g_params_coarse"]) and np.array_equal(grad[e.nc_params:], want["g_params_fine"])
    n0 = e.nc_params
    assert not torch.equal(e.grad[:n0], plain.grad[:n0]) and not torch.equal(e.grad[n0:], plain.grad[n0:]) and torch.equal(e.loss, plain.loss)
    for got, lo in zip(e.depth_losses, dl):
        assert torch.equal(got.cpu(), torch.from_numpy(lo).cuda().mean(dim=0).cpu()) and (got != 0).all()


@pytest.mark.parametrize("overlap", [True, False])
def test_engine_step_with_spread_accumulates_behind_it(lego, gpu, overlap):
    """With spread= as well: the step is spread launch -> accumulating depth launch on the same cotangent -> _w backward, bit for bit; a
    spread weight on one net only leaves the other net's depth launch a plain write."""
    s = lego
    for spread in (LAM, (0.0, 0.01)):
        e = _engine(s, depth_loss=DW, spread=spread, overlap=overlap)
        only = _engine(s, spread=spread, overlap=overlap)
        e.forward_backward(s["rays"], s["target"], depth_prior=s["rows"])
        only.forward_backward(s["rays"], s["target"])
        want, _, _ = _by_hand(s, gpu, e, spread)
        grad = e.grad.cpu().numpy()
        assert np.array_equal(grad[:e.nc_params], want["g_params_coarse"]) and np.array_equal(grad[e.nc_params:], want["g_params_fine"])
        assert not torch.equal(e.grad, only.grad)


def test_engine_weights_on_one_net_and_a_ray_gradient(lego):
    """Weights on the fine net alone leave the coarse net's gradient the plain engine's bits; a ray-gradient step takes the _w form."""
    s = lego
    e, plain = _engine(s, depth_loss=((0, 0), (0.1, 0.01))), _engine(s)
    rg, rg0 = torch.empty_like(s["rays"]), torch.empty_like(s["rays"])
    e.forward_backward(s["rays"], s["target"], ray_grad=rg, depth_prior=s["rows"])
    plain.forward_backward(s["rays"], s["target"], ray_grad=rg0)
    n0 = e.nc_params
    assert torch.equal(e.grad[:n0], plain.grad[:n0]) and not torch.equal(e.grad[n0:], plain.grad[n0:])
    assert torch.equal(e.ray_grad_coarse, plain.ray_grad_coarse) and not torch.equal(rg, rg0) and torch.isfinite(rg).all()
    assert e.depth_losses[0] is None and (e.depth_losses[1] != 0).all()


def test_engine_refusals(lego):
    s = lego
    for bad in (0.1, (0.1,), (0.1, float("nan")), (0.1, 0.2, 0.3), (-0.1, 0.0), ((0.1, 0.2), (0.3,)), (0.1, float("inf"))):
        with pytest.raises(ValueError):
            _engine(s, depth_loss=bad)
    for e in (_engine(s), _engine(s, depth_loss=(0, 0))):
        with pytest.raises(ValueError, match="depth_loss"):
            e.forward_backward(s["rays"], s["target"], depth_prior=s["rows"])
    e = _engine(s, depth_loss=DW)
    with pytest.raises(ValueError, match="frozen"):
        e.forward_backward(s["rays"], s["target"], ray_grad=torch.empty_like(s["rays"]), frozen=True, depth_prior=s["rows"])
    for bad in (s["rows"][:-1], s["rows"].double(), s["rows"].cpu(), s["rows"][:, :2], torch.cat((s["rows"], s["rows"]), dim=1)[:, :3]):
        with pytest.raises(ValueError):
            e.forward_backward(s["rays"], s["target"], depth_prior=bad)


# ---- the table ------------------------------------------------------------------------------------------------------------------
def _views(s, V, H, W, seed=5):
    """V views of H x W (H != W: the shape at which the select-index order can go wrong): images, poses, focal, and [V, H, W] maps of
    depth, weight (about half the pixels) and sigma."""
    g = torch.Generator().manual_seed(seed)
    images = torch.rand(V, H, W, 3, generator=g).to(s["dev"])
    poses = s["pose"][None].repeat(V, 1, 1).clone()
    for v in range(V):
        a = 0.3 * v
        rot = torch.tensor([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=torch.float32, device=s["dev"])
        poses[v, :3, :4] = rot @ s["pose"][:3, :4]
    depth = 2.5 + 3.0 * torch.rand(V, H, W, generator=g)
    weight = torch.where(torch.rand(V, H, W, generator=g) < 0.5, 0.5 + torch.rand(V, H, W, generator=g), torch.zeros(V, H, W))
    sigma = 0.1 + 0.3 * torch.rand(V, H, W, generator=g)
    depth = torch.where(weight > 0, depth, torch.full_like(depth, float("nan")))   # (no prior: D is not interpreted)
    return images, poses.contiguous(), s["focal"] * W / s["W"], depth, weight, sigma


def _rows_at(used, H, W, depth, weight, sigma):
    """The prior rows of the selection's indices, gathered in torch from the ORIGINAL [V, H, W] maps at (v, row, col)."""
    used = used.cpu()
    v, k = used // (H * W), used % (H * W)
    row, col = k % H, k // H
    return torch.stack((depth[v, row, col], weight[v, row, col], sigma[v, row, col]), dim=1).contiguous()


def test_step_on_views_gathers_the_table_rows(lego):
    s, N = lego, lego["N"]
    V, H, W, n = 3, 6, 10, 128
    images, poses, focal, depth, weight, sigma = _views(s, V, H, W)
    P = N.DepthPrior(depth, weight, sigma, device=s["dev"])
    assert P.table.shape == (V * H * W, 3) and torch.equal(P.pixels.cpu(), torch.nonzero(P.table[:, 1].cpu() > 0).reshape(-1))
    a, b = _engine(s, depth_loss=DW, seed=9), _engine(s, depth_loss=DW, seed=9)
    a.step_on_views(images, poses, H, W, focal, s["opts"], n, depth_prior=P)
    rays, target, used = N.select_training_rays_views(H, W, focal, poses, images, n, s["opts"], seed=9, step=0, first=0)
    rows = _rows_at(used, H, W, depth, weight, sigma).to(s["dev"])
    assert 0 < int((rows[:, 1] > 0).sum()) < n
    b.forward_backward(rays, target, depth_prior=rows)
    assert torch.equal(a.grad, b.grad) and a.grad.abs().max() > 0
    for x, y in zip(a.depth_losses, b.depth_losses):
        assert torch.equal(x, y) and (x != 0).all()
    # ... and (P, inds) is the same step
    c = _engine(s, depth_loss=DW, seed=9)
    c.forward_backward(rays, target, depth_prior=(P, used))
    assert torch.equal(a.grad, c.grad)


def test_step_on_image_with_a_table_of_one_view(lego):
    s, N = lego, lego["N"]
    H, W, n = 6, 10, 48
    images, poses, focal, depth, weight, sigma = _views(s, 1, H, W, seed=6)
    P = N.DepthPrior(depth, weight, sigma, device=s["dev"])
    a, b = _engine(s, depth_loss=DW, seed=4), _engine(s, depth_loss=DW, seed=4)
    a.step_on_image(images[0], poses[0], H, W, focal, s["opts"], n, depth_prior=P)
    rays, target, used = N.select_training_rays(H, W, focal, poses[0], images[0], n, s["opts"], seed=4, step=0, first=0)
    rows = _rows_at(used, H, W, depth, weight, sigma).to(s["dev"])
    assert 0 < int((rows[:, 1] > 0).sum()) < n
    b.forward_backward(rays, target, depth_prior=rows)
    assert torch.equal(a.grad, b.grad) and a.grad.abs().max() > 0
    with pytest.raises(ValueError, match="views"):
        a.step_on_views(torch.rand(2, H, W, 3, device=s["dev"]), poses.repeat(2, 1, 1), H, W, focal, s["opts"], n, depth_prior=P)


def test_depth_rays_draws_from_the_pixels_with_a_prior(lego):
    s, N = lego, lego["N"]
    V, H, W, n, m = 3, 6, 10, 64, 24
    images, poses, focal, depth, weight, sigma = _views(s, V, H, W)
    weight = torch.where(torch.rand(V, H, W, generator=torch.Generator().manual_seed(1)) < 0.6, weight, torch.zeros_like(weight))
    P = N.DepthPrior(depth, weight, sigma, device=s["dev"])
    assert m < P.pixels.numel() < V * H * W // 2
    a, b = _engine(s, depth_loss=DW, seed=11), _engine(s, depth_loss=DW, seed=11)
    for step in range(2):
        a.step_on_views(images, poses, H, W, focal, s["opts"], n, depth_prior=P, depth_rays=m)
        b.step_on_views(images, poses, H, W, focal, s["opts"], n, depth_prior=P, depth_rays=m)
        used = a._depth_keep[2].cpu()
        plain = N.select_training_rays_views(H, W, focal, poses, images, n, s["opts"], seed=11, step=step, first=0)[2].cpu()
        assert torch.equal(used[:n - m], plain[:n - m])
        tail = used[n - m:]
        assert torch.unique(tail).numel() == m and bool(torch.isin(tail, P.pixels.cpu()).all())
        assert torch.equal(used, b._depth_keep[2].cpu()) and torch.equal(a.grad, b.grad)
    assert torch.equal(a.mf.flat_params, b.mf.flat_params)
    e = _engine(s, depth_loss=DW)
    args = (images, poses, H, W, focal, s["opts"], n)
    with pytest.raises(ValueError, match="global_rays"):
        e.step_on_views(*args, depth_prior=P, depth_rays=m, global_rays=n)
    for bad in (-1, n + 1, P.pixels.numel() + 1):
        with pytest.raises(ValueError, match="depth_rays"):
            e.step_on_views(images, poses, H, W, focal, s["opts"], 4 * n if bad > n + 1 else n, depth_prior=P, depth_rays=bad)
    with pytest.raises(ValueError, match="depth_rays"):
        e.step_on_views(*args, depth_rays=m)
    with pytest.raises(ValueError, match="depth_loss"):
        _engine(s).step_on_views(*args, depth_prior=P)


def test_depth_prior_class(lego):
    s, N = lego, lego["N"]
    V, H, W = 2, 3, 5
    d = torch.full((V, H, W), float("nan"))
    d[1, 2, 4], d[0, 1, 3] = 3.5, 2.25
    P = N.DepthPrior(d, sigma=0.07, device=s["dev"])   # (weight None: 1 where the depth is finite and > 0)
    assert P.pixels.tolist() == [0 * H * W + 3 * H + 1, 1 * H * W + 4 * H + 2]
    assert torch.equal(P.table[P.pixels].cpu(), torch.tensor([[2.25, 1.0, 0.07], [3.5, 1.0, 0.07]]))
    Q = N.DepthPrior.from_points(V, H, W, [1, 0], [2, 1], [4, 3], [3.5, 2.25], [1.0, 0.5], 0.07, device=s["dev"])
    assert torch.equal(Q.pixels, P.pixels) and torch.equal(Q.table[Q.pixels].cpu(), torch.tensor([[2.25, 0.5, 0.07], [3.5, 1.0, 0.07]]))
    ones = torch.ones(V, H, W)
    for bad in (lambda: N.DepthPrior(d, weight=ones), lambda: N.DepthPrior(ones, sigma=0.0), lambda: N.DepthPrior(ones, sigma=-ones),
                lambda: N.DepthPrior(ones, sigma=float("nan")), lambda: N.DepthPrior(ones[0]), lambda: N.DepthPrior(ones, weight=ones[0]),
                lambda: N.DepthPrior.from_points(V, H, W, [1, 1], [2, 2], [4, 4], [3.5, 2.0]),
                lambda: N.DepthPrior.from_points(V, H, W, [2], [0], [0], [3.5]),
                lambda: N.DepthPrior.from_points(V, H, W, [0], [0], [0], [float("inf")])):
        with pytest.raises(ValueError):
            bad()
    N.DepthPrior(ones, weight=torch.zeros(V, H, W), sigma=0.0)   # (no pixel with a prior: sigma is not interpreted)


# ---- drop-in ----------------------------------------------------------------------------------------------------------------------
def test_dropin_depth_prior_equals_the_engine(lego):
    """run_one_iter_of_nerf(depth_prior=rows), then (mse + a mean(E) + b mean(Tm) per net).backward(), against the engine's gradient on
    the same rays: within 1e-4 of its norm per net (the bound of test_gpu_pose.py::test_engine_pose_gradient_equals_dropin: the two
    routes differ in the backward's buffer layout); the per-ray losses bit for bit.  With spread=True as well the depth pair comes
    behind the spread pair.  Without the keyword the outputs are today's."""
    s, N = lego, lego["N"]
    mc, mf = copy.deepcopy(s["mc"]), copy.deepcopy(s["mf"])
    ex, ed = N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)
    args = (s["H"], s["W"], s["focal"], mc, mf, s["ro"], s["rd"], s["opts"])
    kw = dict(encode_position_fn=ex, encode_direction_fn=ed)
    out = N.run_one_iter_of_nerf(*args, depth_prior=s["rows"], **kw)
    plain = N.run_one_iter_of_nerf(*args, **kw)
    same = lambda a, b: torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))  # noqa: E731
    assert len(out) == 8 and len(plain) == 6 and all(same(a, b) for a, b in zip(out[:6], plain))
    dc, df = out[6], out[7]
    n = s["rays"].shape[0]
    assert dc.shape == df.shape == (n, 2) and dc.requires_grad and df.requires_grad
    mse = torch.nn.functional.mse_loss(out[0], s["target"]) + torch.nn.functional.mse_loss(out[3], s["target"])
    (mse + DW[0][0] * dc[:, 0].mean() + DW[0][1] * dc[:, 1].mean() + DW[1][0] * df[:, 0].mean() + DW[1][1] * df[:, 1].mean()).backward()
    e = _engine(s, depth_loss=DW)
    e.forward_backward(s["rays"], s["target"], depth_prior=s["rows"])
    assert torch.equal(e._depth_bufs[0][1], dc.detach()) and torch.equal(e._depth_bufs[1][1], df.detach())
    none = s["rows"][:, 1] <= 0
    assert none.any() and not dc.detach()[none].any() and (dc.detach()[~none, 0] > 0).all()
    n0 = e.nc_params
    for model, flat in ((mc, e.grad[:n0]), (mf, e.grad[n0:])):
        got = torch.cat([p.grad.reshape(-1) for p in model._ordered_params()])
        want = torch.cat([g.reshape(-1) for g in model._split_flat(flat)])
        rel = float((got - want).norm() / want.norm())
        assert rel < 1e-4, rel
    # with spread=True: (spread_coarse, spread_fine, depth_loss_coarse, depth_loss_fine), and the engine's gradient with both
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.grad = None
    out = N.run_one_iter_of_nerf(*args, spread=True, depth_prior=s["rows"], **kw)
    assert len(out) == 10 and out[6].shape == out[7].shape == (n,) and out[8].shape == out[9].shape == (n, 2)
    assert torch.equal(out[8].detach(), dc.detach()) and torch.equal(out[9].detach(), df.detach())
    mse = torch.nn.functional.mse_loss(out[0], s["target"]) + torch.nn.functional.mse_loss(out[3], s["target"])
    (mse + LAM[0] * out[6].mean() + LAM[1] * out[7].mean() + DW[0][0] * out[8][:, 0].mean() + DW[0][1] * out[8][:, 1].mean()
     + DW[1][0] * out[9][:, 0].mean() + DW[1][1] * out[9][:, 1].mean()).backward()
    e = _engine(s, depth_loss=DW, spread=LAM)
    e.forward_backward(s["rays"], s["target"], depth_prior=s["rows"])
    for model, flat in ((mc, e.grad[:n0]), (mf, e.grad[n0:])):
        got = torch.cat([p.grad.reshape(-1) for p in model._ordered_params()])
        want = torch.cat([g.reshape(-1) for g in model._split_flat(flat)])
        rel = float((got - want).norm() / want.norm())
        assert rel < 1e-4, rel
    # ... and the fine depth output alone carries a gradient to the fine net only
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.grad = None
    out = N.run_one_iter_of_nerf(*args, depth_prior=s["rows"], **kw)
    out[7].sum().backward()
    assert all(p.grad is None or not p.grad.any() for p in mc._ordered_params()) and any(p.grad.any() for p in mf._ordered_params())


def test_dropin_refusals(lego):
    s, N = lego, lego["N"]
    ex, ed = N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)
    args = (s["H"], s["W"], s["focal"], s["mc"], s["mf"], s["ro"], s["rd"], s["opts"])
    with pytest.raises(ValueError, match="train"):
        N.run_one_iter_of_nerf(*args, mode="validation", encode_position_fn=ex, encode_direction_fn=ed, depth_prior=s["rows"])
    with pytest.raises(ValueError, match="fused"):   # (a user network: the generic composition)
        wrapped = torch.nn.Sequential(s["mc"])
        N.predict_and_render_radiance(s["rays"], wrapped, wrapped, s["opts"], encode_position_fn=ex, encode_direction_fn=ed,
                                      depth_prior=s["rows"])
    with pytest.raises(ValueError):
        N.run_one_iter_of_nerf(*args, encode_position_fn=ex, encode_direction_fn=ed, depth_prior=s["rows"][:-1])


# ---- capability ------------------------------------------------------------------------------------------------------------------
# the weights (a, b) of the capability test, fixed beforehand from the CPU study with the oracle's autograd on the same setup
# (scripts/study_depth_prior_weights.py -> profiles/r19_depth_prior_study.json)
DEPTH_CAP = (1.0, 0.0)
CAP_TRAIN = (0, 2, 4)   # the 0, 40 and 80 degree views of occupancy_train_cases.CAP_ANGLES; the 60 degree view is held out


@pytest.fixture(scope="module")
def lego64(gpu):
    return ES.lego64()


def _fine_maps(N, rays, mc, mf):
    """(rgb_fine, acc_fine, depth_fine) of a dense 64 + 64 render without perturbation or noise: the slots of the render's output
    struct, through the fused node."""
    from nerf_pytorch_amd import train_utils as TU
    with torch.no_grad():
        outs = TU._FusedRender.apply(rays.contiguous(), mc, mf, (64, 64, False, False, True, 0.0, False), (None,) * 4, False, False)
    return outs[4], outs[6], outs[7]


def _few_view_scene(s):
    """The three training views as resident images and poses, the teacher's fine-pass depth as a sparse table (a keyed 5 % of their
    pixels with teacher acc_fine > 0.9, sigma = 0.05), and the held-out view's rays with the teacher's colour, acc and depth."""
    import occupancy_train_cases as OT
    if "few" in s:
        return s["few"]
    N, H, W, dev = s["N"], s["H"], s["W"], s["dev"]
    rays, rgb = OT.teacher_views(s)
    to_map = lambda t: t.reshape(H, W, *t.shape[1:]).contiguous()   # noqa: E731  (get_rays_at_pixels' linear ids: row * W + col)
    poses, images, depth, acc = [], [], [], []
    for i in CAP_TRAIN:
        a = np.deg2rad(OT.CAP_ANGLES[i])
        rot = torch.tensor([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32,
                           device=dev)
        pose = s["pose"].clone()
        pose[:3, :4] = rot[:3, :3] @ pose[:3, :4]
        poses.append(pose)
        _, a_f, d_f = _fine_maps(N, rays[i], s["mc"], s["mf"])
        images.append(to_map(rgb[i]))
        depth.append(to_map(d_f))
        acc.append(to_map(a_f))
    poses, images, depth, acc = (torch.stack(t) for t in (poses, images, depth, acc))
    # (the resident images and poses give back the teacher's rays and colours, at the select index col * H + row of every pixel)
    pix = torch.arange(H * W, dtype=torch.int64, device=dev)
    r0, t0, _ = N.select_training_rays_views(H, W, s["focal"], poses, images, H * W, s["opts"], select_inds=(pix % W) * H + pix // W + H * W)
    print("few-view scene: selection's rays against the teacher's, max difference %.3e" % float((r0 - rays[CAP_TRAIN[1]]).abs().max()))
    assert torch.equal(t0, rgb[CAP_TRAIN[1]]) and torch.allclose(r0, rays[CAP_TRAIN[1]], atol=1e-5)   # (a wrong pose or order: O(1))
    keyed = (torch.rand(depth.shape, generator=torch.Generator().manual_seed(1234)) < 0.05).to(dev)
    weight = (keyed & (acc > 0.9)).float()
    prior = N.DepthPrior(depth, weight, 0.05, device=dev)
    _, a_h, d_h = _fine_maps(N, rays[OT.CAP_HELD_OUT], s["mc"], s["mf"])
    s["few"] = dict(poses=poses.contiguous(), images=images, prior=prior, held_rays=rays[OT.CAP_HELD_OUT], held_rgb=rgb[OT.CAP_HELD_OUT],
                    held_solid=a_h > 0.9, held_depth=d_h)
    return s["few"]


def _capability_arm(s, seed, weights, steps=400, n_rays=1024, lr=5e-3, noise_std=1.0, depth_rays=256):
    N, f = s["N"], _few_view_scene(s)
    torch.manual_seed(seed)
    cfg = dict(num_layers=4, hidden_size=64, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    mc, mf = N.FlexibleNeRFModel(**cfg).to(s["dev"]), N.FlexibleNeRFModel(**cfg).to(s["dev"])
    eng = N.TrainEngine(mc, mf, 64, 64, perturb=True, white_background=True, noise_std=noise_std, lr=lr, seed=seed, depth_loss=weights)
    # (depth_rays <= len(P.pixels): on this scene the keyed 5 % with acc_fine > 0.9 are 169 pixels, fewer than the 256 asked for)
    kw = {} if weights is None else dict(depth_prior=f["prior"], depth_rays=min(depth_rays, int(f["prior"].pixels.numel())))
    losses = torch.zeros(steps, device=s["dev"])
    for i in range(steps):
        losses[i] = eng.step_on_views(f["images"], f["poses"], s["H"], s["W"], s["focal"], s["opts"], n_rays, **kw)[2]
    rgb, _, depth = _fine_maps(N, f["held_rays"], mc, mf)
    mse = float(((rgb - f["held_rgb"]).double() ** 2).mean().item())
    derr = float((depth - f["held_depth"])[f["held_solid"]].abs().double().mean().item())
    return dict(finite=bool(torch.isfinite(losses).all().item()), psnr=float(-10.0 * np.log10(max(mse, 1e-30))), depth_err=derr)


def test_capability_a_sparse_prior_improves_few_view_geometry(lego64):
    """Few views: three 64 x 64 teacher views of the fixture nets (0, 40, 80 degrees; the 60-degree view held out) train two 4 x 64
    students for 400 steps of 1024 rays (lr 5e-3, sigma noise 1.0), seeds 0, 1 and 2, without a prior against
    TrainEngine(depth_loss=DEPTH_CAP) with the teacher's fine-pass depth on a keyed 5 % of the training pixels with teacher acc_fine >
    0.9 (sigma 0.05) and depth_rays=256.  On the held-out view: for every seed the prior arm's mean |depth - teacher depth| over the
    rays with teacher acc_fine > 0.9 is below the plain arm's, and its PSNR is no lower than the plain arm's mean minus twice the plain
    arm's own spread over the seeds (the floor of test_gpu_spread.py, for its reason).
    The weights come from the CPU study (seed 0; plain 19.67 dB / depth error 0.416; (0.1, 0) 19.49 / 0.130; (1, 0) 19.64 / 0.079;
    (0, 0.01) 19.38 / 0.284; (0, 0.1) 20.09 / 0.118 -- every arm within 0.5 dB of the plain one, (1, 0) the lowest depth error).  On
    this scene the keyed 5 % with acc_fine > 0.9 are 169 pixels, so depth_rays is min(256, 169) = 169 (it cannot exceed len(P.pixels)).
    Measured on the MI355X (seeds 0 / 1 / 2): plain 19.87 / 19.14 / 19.33 dB with depth error 0.327 / 0.387 / 0.359; (1, 0)
    20.19 / 19.74 / 19.85 dB with depth error 0.088 / 0.092 / 0.094; the PSNR floor comes out at 17.98 dB."""
    plain = [_capability_arm(lego64, seed, None) for seed in (0, 1, 2)]
    prior = [_capability_arm(lego64, seed, DEPTH_CAP) for seed in (0, 1, 2)]
    print("capability:", dict(plain=plain, prior=prior, weights=DEPTH_CAP, prior_pixels=int(_few_view_scene(lego64)["prior"].pixels.numel())))
    assert all(r["finite"] for r in plain + prior)
    psnr = [r["psnr"] for r in plain]
    floor = float(np.mean(psnr)) - 2.0 * (max(psnr) - min(psnr))
    for p, r in zip(plain, prior):
        assert r["depth_err"] < p["depth_err"], (p, r)
        assert r["psnr"] >= floor, (r, floor)
