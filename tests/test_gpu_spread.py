"""GPU suite (-m gpu) of the ray-weight spread loss (mip-NeRF 360's L_dist): the cases of tests/spread_cases.py on the product library
-- every net, both training arithmetics, both render shapes, both workspace layouts -- and the two public routes: TrainEngine(spread=)
and the drop-in API's spread=True."""
import copy

import numpy as np
import pytest
import torch

import engine_scenes as ES
import spread_cases as S
from conftest import gold

pytestmark = pytest.mark.gpu


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KERNEL_KINDS)
def test_kernel_against_the_definition(gpu, kind):
    S.case_kernel(gpu, kind)


def test_kernel_many_chunks(gpu):
    S.check_kernel_sums(gpu, "noise_draws", 2, 2048 - 37, 8, seed=7)
    S.check_kernel_sums(gpu, "noise_stream", 3, 8192, 11, seed=8)   # (the largest S the entry point takes)


def test_kernel_refusals(gpu):
    S.case_kernel_refusals(gpu)


# ---- through the render ------------------------------------------------------------------------------------------------------------
NETS = [(net, arith) for arith in S.RENDER_ARITHS for net in S.RENDER_NETS]


@pytest.mark.parametrize("layout", [1, 2])
@pytest.mark.parametrize("net,arith", NETS)
def test_w_entry_points_bit_checks(gpu, net, arith, layout):
    S.case_w_bits(gpu, net, arith, layout)


@pytest.mark.parametrize("net,arith", NETS)
def test_parameter_gradients_against_the_oracle(gpu, net, arith):
    S.case_param_grads(gpu, net, arith)


@pytest.mark.parametrize("net,arith", NETS)
def test_backward_modes_with_a_weight_cotangent(gpu, net, arith):
    fused = ("fused", "fused_compact", "fused_stash") if (net, arith) == ("w64", "fp32") else ()
    for noise in (0.6, 2.0):   # (two zero fractions of the d(loss)/d(raw) rows)
        S.case_compacted(gpu, net, arith, (True, "recompute") + fused, noise=noise)


@pytest.mark.parametrize("outside", [0, 1])
@pytest.mark.parametrize("net,arith", [("w128", "fp32"), ("w64", "fp32"), ("w40of64", "f16x3_train"), ("w256", "f16x3_train")])
def test_culled_step_with_spread(gpu, net, arith, outside):
    S.case_culled_step(gpu, net, arith, outside)


def test_ray_gradient_with_spread(gpu):
    S.case_rays_w(gpu, "w128")


# ---- engine and drop-in ------------------------------------------------------------------------------------------------------------
CFG = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
SAMPLING = dict(num_coarse=64, num_fine=64, perturb=False, white_background=True, noise_std=0.0)
LAM = (0.02, 0.01)


@pytest.fixture(scope="module")
def lego(gpu):
    """The lego-lowres fixture nets and 1024 rays of the fixture pose with a random target."""
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
    return dict(N=N, dev=dev, mc=mc, mf=mf, H=H, W=W, focal=focal, opts=opts, ro=ro, rd=rd, rays=rays, target=target)


def _engine(s, **kw):
    return s["N"].TrainEngine(copy.deepcopy(s["mc"]), copy.deepcopy(s["mf"]), **dict(SAMPLING, **kw))


def test_engine_without_spread_is_the_engine(lego):
    s = lego
    engines = [_engine(s), _engine(s, spread=None), _engine(s, spread=0.0), _engine(s, spread=(0.0, 0.0))]
    for _ in range(3):
        for e in engines:
            e.step(s["rays"], s["target"])
    a = engines[0]
    assert a.grad.abs().max() > 0
    for e in engines[1:]:
        assert e.spread_losses == (None, None) and e._spread_bufs is None
        assert torch.equal(a.loss, e.loss) and torch.equal(a.grad, e.grad)
        assert torch.equal(a.mc.flat_params, e.mc.flat_params) and torch.equal(a.mf.flat_params, e.mf.flat_params)


@pytest.mark.parametrize("overlap", [True, False])
def test_engine_step_is_the_c_entry_points(lego, gpu, overlap):
    """One engine step with spread=(lambda_c, lambda_f) against nerfhip_render_fwd + nerfhip_mse_loss_fwd_bwd + nerfhip_spread_loss +
    nerfhip_render_bwd_parts_w assembled by hand on the engine's own plans: gradient, losses and spread means bit for bit -- and not the
    plain engine's gradient."""
    s = lego
    e, plain = _engine(s, spread=LAM, overlap=overlap), _engine(s, overlap=overlap)
    e.forward_backward(s["rays"], s["target"])
    plain.forward_backward(s["rays"], s["target"])
    rays, tgt = s["rays"].cpu().numpy(), s["target"].cpu().numpy()
    r = S.RenderW(gpu, e.mc._plan, e.mf._plan, e.packed_c, e.packed_f, rays, SAMPLING, {})
    lc, gc, _ = gpu.mse_loss(r.out["rgb_coarse"], None, tgt)
    lf, gf, _ = gpu.mse_loss(r.out["rgb_fine"], None, tgt)
    gw, (sc, sf) = S.spread_cotangents(r, LAM)
    want = r.backward((gc, gf), gw, entry="parts_w")
    grad, loss = e.grad.cpu().numpy(), e.loss.cpu().numpy()
    assert loss[0] == lc[0] and loss[1] == lf[0]
    assert np.array_equal(grad[:e.nc_params], want["g_params_coarse"]) and np.array_equal(grad[e.nc_params:], want["g_params_fine"])
    assert not np.array_equal(grad, plain.grad.cpu().numpy()) and torch.equal(e.loss, plain.loss)
    got_c, got_f = e.spread_losses
    assert float(got_c) == float(torch.from_numpy(sc).cuda().mean()) and float(got_f) == float(torch.from_numpy(sf).cuda().mean())
    assert float(got_c) > 0 and float(got_f) > 0


def test_engine_spread_on_one_net_and_with_a_ray_gradient(lego):
    """lambda on the fine net alone leaves the coarse net's gradient the plain engine's bits; a ray-gradient step takes the _w form too."""
    s = lego
    e, plain = _engine(s, spread=(0.0, 0.01)), _engine(s)
    rg, rg0 = torch.empty_like(s["rays"]), torch.empty_like(s["rays"])
    e.forward_backward(s["rays"], s["target"], ray_grad=rg)
    plain.forward_backward(s["rays"], s["target"], ray_grad=rg0)
    n0 = e.nc_params
    assert torch.equal(e.grad[:n0], plain.grad[:n0]) and not torch.equal(e.grad[n0:], plain.grad[n0:])
    assert torch.equal(e.ray_grad_coarse, plain.ray_grad_coarse) and not torch.equal(rg, rg0) and torch.isfinite(rg).all()
    assert e.spread_losses[0] is None and float(e.spread_losses[1]) > 0


def test_engine_refusals(lego):
    s = lego
    for bad in (-0.1, (0.1,), (0.1, float("nan")), (0.1, 0.2, 0.3)):
        with pytest.raises(ValueError):
            _engine(s, spread=bad)
    e = _engine(s, spread=0.01)
    with pytest.raises(ValueError, match="frozen"):
        e.forward_backward(s["rays"], s["target"], ray_grad=torch.empty_like(s["rays"]), frozen=True)
    image = torch.rand(s["H"], s["W"], 3, device=s["dev"])
    pose = torch.eye(4, device=s["dev"])
    with pytest.raises(ValueError, match="frozen"):
        e.localize_on_image(image, pose, s["H"], s["W"], s["focal"], s["opts"], 64, pose_grad=torch.zeros(3, 4, device=s["dev"]))


def test_dropin_spread_equals_the_engine(lego):
    """run_one_iter_of_nerf(spread=True), then (mse + lambda_f spread_fine.mean() + lambda_c spread_coarse.mean()).backward(), against
    the engine's gradient on the same rays (no draws: perturb off, no sigma noise).  Both run the same kernels; they differ in the
    backward's buffer layout, so the two gradients agree to 1e-4 of their norm per net -- the bound
    test_gpu_pose.py::test_engine_pose_gradient_equals_dropin holds the two routes to.  With spread=False the outputs are today's."""
    s, N = lego, lego["N"]
    mc, mf = copy.deepcopy(s["mc"]), copy.deepcopy(s["mf"])
    ex, ed = N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)
    args = (s["H"], s["W"], s["focal"], mc, mf, s["ro"], s["rd"], s["opts"])
    out = N.run_one_iter_of_nerf(*args, encode_position_fn=ex, encode_direction_fn=ed, spread=True)
    plain = N.run_one_iter_of_nerf(*args, encode_position_fn=ex, encode_direction_fn=ed)
    # (the disparity of a ray that hits nothing is the reference's own 0 / 0: NaN in both)
    same = lambda a, b: torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))  # noqa: E731
    assert len(out) == 8 and len(plain) == 6 and all(same(a, b) for a, b in zip(out[:6], plain))
    sc, sf = out[6], out[7]
    assert sc.shape == sf.shape == (s["rays"].shape[0],) and sc.requires_grad and sf.requires_grad
    mse = torch.nn.functional.mse_loss(out[0], s["target"]) + torch.nn.functional.mse_loss(out[3], s["target"])
    (mse + LAM[1] * sf.mean() + LAM[0] * sc.mean()).backward()
    e = _engine(s, spread=LAM)
    e.forward_backward(s["rays"], s["target"])
    assert torch.equal(e.spread_losses[0], sc.detach().mean()) and torch.equal(e.spread_losses[1], sf.detach().mean())
    n0 = e.nc_params
    for model, flat in ((mc, e.grad[:n0]), (mf, e.grad[n0:])):
        got = torch.cat([p.grad.reshape(-1) for p in model._ordered_params()])
        want = torch.cat([g.reshape(-1) for g in model._split_flat(flat)])
        rel = float((got - want).norm() / want.norm())
        assert rel < 1e-4, rel
    # ... and the spread outputs alone carry a gradient (no colour cotangent at all)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.grad = None
    out = N.run_one_iter_of_nerf(*args, encode_position_fn=ex, encode_direction_fn=ed, spread=True)
    out[7].sum().backward()
    assert all(p.grad is None or not p.grad.any() for p in mc._ordered_params()) and any(p.grad.any() for p in mf._ordered_params())


def test_dropin_refusals(lego):
    s, N = lego, lego["N"]
    ex, ed = N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)
    args = (s["H"], s["W"], s["focal"], s["mc"], s["mf"], s["ro"], s["rd"], s["opts"])
    with pytest.raises(ValueError, match="train"):
        N.run_one_iter_of_nerf(*args, mode="validation", encode_position_fn=ex, encode_direction_fn=ed, spread=True)
    with pytest.raises(ValueError, match="fused"):   # (a user network: the generic composition)
        wrapped = torch.nn.Sequential(s["mc"])
        N.predict_and_render_radiance(s["rays"], wrapped, wrapped, s["opts"], encode_position_fn=ex, encode_direction_fn=ed, spread=True)


# ---- capability ------------------------------------------------------------------------------------------------------------------
# the weight of the capability test, fixed beforehand from the CPU study with the oracle's autograd on the same setup
# (scripts/study_spread_lambda.py -> profiles/r18_spread_lambda_study.json)
LAMBDA_CAP = 0.1


@pytest.fixture(scope="module")
def lego64(gpu):
    return ES.lego64()


def _capability_arm(s, seed, lam, steps=400, n_rays=1024, lr=5e-3, noise_std=1.0):
    """occupancy_train_cases.capability's plain arm with TrainEngine(spread=lam): the held-out view's PSNR against the teacher and its
    mean fine-pass spread loss (the drop-in route's spread_fine, no perturbation, no noise)."""
    import occupancy_train_cases as OT
    N = s["N"]
    rays, rgb = OT.teacher_views(s)
    train = [i for i in range(len(OT.CAP_ANGLES)) if i != OT.CAP_HELD_OUT]
    pool_r, pool_t = rays[train].reshape(-1, rays.shape[-1]), rgb[train].reshape(-1, 3)
    torch.manual_seed(seed)
    cfg = dict(num_layers=4, hidden_size=64, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    mc, mf = N.FlexibleNeRFModel(**cfg).to(s["dev"]), N.FlexibleNeRFModel(**cfg).to(s["dev"])
    eng = N.TrainEngine(mc, mf, 64, 64, perturb=True, white_background=True, noise_std=noise_std, lr=lr, seed=seed, spread=lam)
    picks = torch.randint(0, pool_r.shape[0], (steps, n_rays), generator=torch.Generator().manual_seed(seed)).to(s["dev"])
    losses = torch.zeros(steps, device=s["dev"])
    for i in range(steps):
        idx = picks[i]
        losses[i] = eng.step(pool_r[idx].contiguous(), pool_t[idx].contiguous())[2]
    with torch.no_grad():
        out = N.predict_and_render_radiance(rays[OT.CAP_HELD_OUT], mc, mf, s["opts"], mode="train", spread=True,
                                            encode_position_fn=N.get_embedding_function(10, True, True),
                                            encode_direction_fn=N.get_embedding_function(4, True, True))
    mse = float(((out[3] - rgb[OT.CAP_HELD_OUT]).double() ** 2).mean().item())
    return dict(finite=bool(torch.isfinite(losses).all().item()), psnr=float(-10.0 * np.log10(max(mse, 1e-30))),
                spread_fine=float(out[7].double().mean().item()), spread_coarse=float(out[6].double().mean().item()))


def test_capability_the_spread_term_compacts_the_ray_weights(lego64):
    """The capability setup of test_gpu_occupancy_train.py (six 64 x 64 teacher views of the fixture nets, the 60-degree view held out,
    two 4 x 64 students, 400 steps of 1024 rays, lr 5e-3, sigma noise 1.0), seeds 0, 1 and 2, lambda = 0 against LAMBDA_CAP, measured on
    the held-out view's rays: for every seed the lambda arm's mean fine-pass L is below the plain arm's, and the lambda arm's PSNR is no
    lower than the plain arm's mean minus twice the plain arm's own spread over the three seeds (two such runs differ by that much on
    their own: DESIGN.md 3.15).
    Measured on the MI355X (seeds 0 / 1 / 2): plain 18.58 / 19.54 / 20.34 dB with fine L 0.00772 / 0.00892 / 0.00783; lambda = 0.1
    19.77 / 19.93 / 20.33 dB with fine L 0.00584 / 0.00621 / 0.00606; the PSNR floor comes out at 15.97 dB."""
    plain = [_capability_arm(lego64, seed, 0.0) for seed in (0, 1, 2)]
    reg = [_capability_arm(lego64, seed, LAMBDA_CAP) for seed in (0, 1, 2)]
    print("capability:", dict(plain=plain, spread=reg, lam=LAMBDA_CAP))
    assert all(r["finite"] for r in plain + reg)
    psnr = [r["psnr"] for r in plain]
    floor = float(np.mean(psnr)) - 2.0 * (max(psnr) - min(psnr))
    for p, r in zip(plain, reg):
        assert r["spread_fine"] < p["spread_fine"], (p, r)
        assert r["psnr"] >= floor, (r, floor)
