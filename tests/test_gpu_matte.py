"""GPU suite (-m gpu) of the alpha-matte loss: the cases of tests/matte_cases.py on the product library, and the public routes:
TrainEngine(alpha=, background=, alpha_loss=, opacity_entropy=) on its steps, and the drop-in API's matte_mse_loss."""
import copy
import json

import numpy as np
import pytest
import torch

import engine_scenes as ES
import matte_cases as M
import spread_cases as S
from conftest import gold

pytestmark = pytest.mark.gpu


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_kernel_against_the_definition(gpu, mode):
    M.case_kernel(gpu, mode)


def test_kernel_propagates_nan_to_its_ray_only(gpu):
    M.case_nan(gpu)


def test_kernel_bit_identities(gpu):
    M.case_bit_identities(gpu)


def test_kernel_refusals(gpu):
    M.case_refusals(gpu)


# ---- through the render ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,arith", M.RENDER_NETS)
def test_parameter_gradients_against_the_oracle(gpu, net, arith):
    M.case_param_grads(gpu, net, arith)


@pytest.mark.parametrize("net,arith", M.RENDER_NETS)
def test_backward_modes_with_the_opacity_cotangent(gpu, net, arith):
    fused = ("fused", "fused_compact", "fused_stash") if (net, arith) == ("w64", "fp32") else ()
    for noise in (0.6, 2.0):   # (two zero fractions of the d(loss)/d(raw) rows)
        M.case_compacted(gpu, net, arith, (True, "recompute") + fused, noise=noise)
    M.case_compacted(gpu, net, arith, (True, "recompute") + fused, noise=0.6, opaque=False)   # (mixed alphas: g_acc of both signs)


def test_culled_step_with_the_matte_loss(gpu):
    M.case_culled_step(gpu, "w64", "fp32", 0)


def test_ray_gradient_with_the_matte_loss(gpu):
    M.case_ray_grad(gpu, "w128")


# ---- engine and drop-in ------------------------------------------------------------------------------------------------------------
CFG = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
SAMPLING = dict(num_coarse=64, num_fine=64, perturb=False, white_background=False, noise_std=0.0)
LAM_A, LAM_H = (0.5, 1.0), (0.02, 0.01)   # (coarse, fine)
LAM = (0.02, 0.01)                        # (the spread weights of the stacked case)
SEED = 5


@pytest.fixture(scope="module")
def lego(gpu):
    """The lego-lowres fixture nets and 1024 rays of the fixture pose with a random RGBA target."""
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
    opts = N.make_options(64, 64, perturb=False, white_background=False, radiance_field_noise_std=0.0)
    ro, rd = N.get_rays_at_pixels(H, W, focal, pose[:3, :4], torch.arange(H * W, dtype=torch.int64, device=dev))
    rays = N.pack_rays(ro, rd, opts, H, W, focal)
    target = torch.from_numpy(M.render_targets(H * W, seed=3)[0]).to(dev)
    return dict(N=N, dev=dev, mc=mc, mf=mf, H=H, W=W, focal=focal, pose=pose, opts=opts, ro=ro, rd=rd, rays=rays, target=target)


def _engine(s, **kw):
    return s["N"].TrainEngine(copy.deepcopy(s["mc"]), copy.deepcopy(s["mf"]), **dict(SAMPLING, **kw))


def test_engine_without_alpha_is_the_engine(lego):
    s = lego
    engines = [_engine(s), _engine(s, alpha=None), _engine(s, alpha=None, alpha_loss=[0.0, 0.0], opacity_entropy=(0, 0))]
    rgb = s["target"][:, :3]   # (a strided view of the RGBA rows: what the engine always took)
    for _ in range(3):
        for e, t in zip(engines, (rgb, s["target"], s["target"])):
            e.step(s["rays"], t)
    a = engines[0]
    assert a.grad.abs().max() > 0
    for e in engines:
        assert e.matte_losses is None and "ga_c" not in e._bufs
        assert torch.equal(a.loss, e.loss) and torch.equal(a.grad, e.grad)
        assert torch.equal(a.mc.flat_params, e.mc.flat_params) and torch.equal(a.mf.flat_params, e.mf.flat_params)


def _by_hand(s, gpu, e, spread=None, bg_kw=None):
    """One step's C calls on the engine's own plans: forward, [spread launches,] the two matte losses, the backward with g_acc."""
    rays, tgt = s["rays"].cpu().numpy(), s["target"].cpu().numpy()
    r = S.RenderW(gpu, e.mc._plan, e.mf._plan, e.packed_c, e.packed_f, rays, SAMPLING, {})
    gw = None
    if spread is not None:
        gw = [r.spread(bool(fine), spread[fine] / r.n)[1] for fine in (0, 1)]
    bg_kw = dict(bg_random=True, seed=SEED, ray_offset=0) if bg_kw is None else bg_kw
    lc, grc, gac = M.matte_loss(gpu, r.out["rgb_coarse"], r.out["acc_coarse"], tgt, 0, lam=(LAM_A[0], LAM_H[0]), **bg_kw)
    lf, grf, gaf = M.matte_loss(gpu, r.out["rgb_fine"], r.out["acc_fine"], tgt, 0, lam=(LAM_A[1], LAM_H[1]), **bg_kw)
    want = r.backward((grc, grf, gac, gaf), gw, entry="parts" if gw is None else "parts_w")
    return want, (lc, lf)


@pytest.mark.parametrize("overlap", [True, False])
def test_engine_step_is_the_c_entry_points(lego, gpu, overlap):
    """One engine step with alpha="matte", alpha_loss and opacity_entropy on both nets against nerfhip_render_fwd +
    nerfhip_matte_loss_fwd_bwd + nerfhip_render_bwd_parts assembled by hand on the engine's own plans: gradient and matte_losses bit for
    bit -- and not the plain engine's gradient; then stacked behind spread= (the _w backward), and over a constant background."""
    s = lego
    kw = dict(alpha="matte", alpha_loss=LAM_A, opacity_entropy=LAM_H, overlap=overlap, seed=SEED)
    e, plain = _engine(s, **kw), _engine(s, overlap=overlap, seed=SEED)
    e.forward_backward(s["rays"], s["target"])
    plain.forward_backward(s["rays"], s["target"])
    want, (lc, lf) = _by_hand(s, gpu, e)
    n0 = e.nc_params
    grad = e.grad.cpu().numpy()
    assert np.array_equal(grad[:n0], want["g_params_coarse"]) and np.array_equal(grad[n0:], want["g_params_fine"])
    assert not torch.equal(e.grad[:n0], plain.grad[:n0]) and not torch.equal(e.grad[n0:], plain.grad[n0:])
    mc, mf = (t.cpu().numpy() for t in e.matte_losses)
    assert np.array_equal(M.bits(mc), M.bits(lc)) and np.array_equal(M.bits(mf), M.bits(lf)) and (mc > 0).all() and (mf > 0).all()
    loss = e.loss.cpu().numpy()
    assert loss[0] == lc[0] and loss[1] == lf[0] and loss[2] == np.float32(lc[0]) + np.float32(lf[0])
    # stacked behind the spread term
    e2, only = _engine(s, spread=LAM, **kw), _engine(s, spread=LAM, overlap=overlap, seed=SEED)
    e2.forward_backward(s["rays"], s["target"])
    only.forward_backward(s["rays"], s["target"])
    want2, _ = _by_hand(s, gpu, e2, LAM)
    grad = e2.grad.cpu().numpy()
    assert np.array_equal(grad[:n0], want2["g_params_coarse"]) and np.array_equal(grad[n0:], want2["g_params_fine"])
    assert not torch.equal(e2.grad, only.grad) and not torch.equal(e2.grad, e.grad)
    # a constant background
    e3 = _engine(s, background=M.BG_CONST, **kw)
    e3.forward_backward(s["rays"], s["target"])
    want3, _ = _by_hand(s, gpu, e3, bg_kw=dict(bg_const=M.BG_CONST))
    grad = e3.grad.cpu().numpy()
    assert np.array_equal(grad[:n0], want3["g_params_coarse"]) and np.array_equal(grad[n0:], want3["g_params_fine"])
    assert not torch.equal(e3.grad, e.grad)


def test_engine_random_background_follows_step_and_ray_offset(lego):
    """The draws are keyed by the step's seed and the global ray index: a second step draws other colours, ray_offset shifts them, and
    coarse_photometric=False withholds g_rgb and g_acc from the coarse pass."""
    s = lego
    kw = dict(alpha="matte", alpha_loss=LAM_A, seed=SEED)
    a, b = _engine(s, **kw), _engine(s, **kw)
    a.forward_backward(s["rays"], s["target"])
    b.forward_backward(s["rays"], s["target"], ray_offset=7)
    assert not torch.equal(a.matte_losses[1], b.matte_losses[1]) and not torch.equal(a.grad, b.grad)
    b.forward_backward(s["rays"], s["target"])
    assert torch.equal(a.grad, b.grad)
    b.forward_backward(s["rays"], s["target"], step=1)
    assert not torch.equal(a.matte_losses[1][:1], b.matte_losses[1][:1])
    w = _engine(s, alpha="weight", opacity_entropy=0.05, seed=SEED)
    w.forward_backward(s["rays"], s["target"])
    assert float(w.matte_losses[0][1]) == 0.0 and float(w.matte_losses[0][0]) > 0 and float(w.matte_losses[0][2]) > 0
    c = _engine(s, spread=LAM, coarse_photometric=False, **kw)
    d = _engine(s, spread=LAM, coarse_photometric=False, seed=SEED)
    c.forward_backward(s["rays"], s["target"])
    d.forward_backward(s["rays"], s["target"])
    n0 = c.nc_params
    assert torch.equal(c.grad[:n0], d.grad[:n0]) and not torch.equal(c.grad[n0:], d.grad[n0:])


def test_engine_without_a_fine_net(lego):
    """num_fine = 0 with alpha: loss = {photometric_c, 0, photometric_c} -- the middle word a plain zero, also when the loss is NaN --,
    matte_losses = (coarse, None), the pair weights' fine halves are not looked at."""
    s = lego
    kw = dict(SAMPLING, num_fine=0, alpha="matte", alpha_loss=(0.5, 7.0), opacity_entropy=0.02, seed=SEED)
    e = s["N"].TrainEngine(copy.deepcopy(s["mc"]), None, **kw)
    assert e.alpha_loss == (0.5, 0.0) and e.opacity_entropy == (0.02, 0.0)
    e.forward_backward(s["rays"], s["target"])
    mc, none = e.matte_losses
    assert none is None and (mc > 0).all() and torch.isfinite(e.grad).all() and e.grad.abs().max() > 0
    assert torch.equal(e.loss.cpu(), torch.stack((mc[0], torch.zeros_like(mc[0]), mc[0])).cpu())
    bad = s["target"].clone()
    bad[3, 1] = float("nan")
    e.forward_backward(s["rays"], bad)
    loss = e.loss.cpu()
    assert torch.isnan(loss[0]) and loss[1] == 0.0 and torch.isnan(loss[2])


def _views(s, V, H, W, seed=5):
    g = torch.Generator().manual_seed(seed)
    images = torch.rand(V, H, W, 4, generator=g).to(s["dev"])
    poses = s["pose"][None].repeat(V, 1, 1).clone()
    for v in range(V):
        a = 0.3 * v
        rot = torch.tensor([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=torch.float32, device=s["dev"])
        poses[v, :3, :4] = rot @ s["pose"][:3, :4]
    return images, poses.contiguous(), s["focal"] * W / s["W"]


def test_step_on_views_hands_the_rgba_rows_to_the_loss(lego):
    s, N = lego, lego["N"]
    V, H, W, n = 3, 6, 10, 128
    images, poses, focal = _views(s, V, H, W)
    kw = dict(alpha="matte", alpha_loss=LAM_A, opacity_entropy=LAM_H, seed=9)
    a, b = _engine(s, **kw), _engine(s, **kw)
    a.step_on_views(images, poses, H, W, focal, s["opts"], n)
    rays, target, used = N.select_training_rays_views(H, W, focal, poses, images, n, s["opts"], seed=9, step=0, first=0)
    assert target.shape == (n, 4)
    v, k = used.cpu() // (H * W), used.cpu() % (H * W)
    assert torch.equal(target.cpu(), images.cpu()[v, k % H, k // H])   # (the selection's index order: col * H + row)
    b.forward_backward(rays, target)
    assert torch.equal(a.grad, b.grad) and a.grad.abs().max() > 0
    assert all(torch.equal(x, y) for x, y in zip(a.matte_losses, b.matte_losses))
    with pytest.raises(ValueError, match="alpha"):
        _engine(s, **kw).step_on_views(images[..., :3].contiguous(), poses, H, W, focal, s["opts"], n)


def test_frozen_localize_step_takes_the_matte_loss(lego):
    s = lego
    V, H, W, n = 3, 6, 10, 128
    images, poses, focal = _views(s, V, H, W)
    a, p = _engine(s, alpha="matte", alpha_loss=LAM_A, seed=9), _engine(s, seed=9)
    ga, gp = (torch.zeros(V, 3, 4, device=s["dev"]) for _ in range(2))
    a.localize_on_views(images, poses, H, W, focal, s["opts"], n, pose_grads=ga)
    p.localize_on_views(images, poses, H, W, focal, s["opts"], n, pose_grads=gp)
    for x, y in ((a._ray_grad, p._ray_grad), (a.ray_grad_coarse, p.ray_grad_coarse), (ga, gp)):
        assert torch.isfinite(x).all() and x.abs().max() > 0 and not torch.equal(x, y)
    assert not a.grad.any() and float(a.matte_losses[1][1]) > 0


def test_engine_refusals(lego):
    s, N = lego, lego["N"]
    with pytest.raises(ValueError, match="white_background"):
        _engine(s, alpha="matte", white_background=True)
    _engine(s, alpha="weight", white_background=True)
    with pytest.raises(ValueError, match="alpha"):
        _engine(s, alpha="premultiplied")
    with pytest.raises(ValueError, match="alpha_loss"):
        _engine(s, alpha="weight", alpha_loss=0.1)
    for name, v in (("alpha_loss", 0.1), ("alpha_loss", (0.0, 0.1)), ("opacity_entropy", 0.1), ("background", "random"), ("background", (1, 1, 1))):
        with pytest.raises(ValueError, match=name):
            _engine(s, **{name: v})
    for name in ("alpha_loss", "opacity_entropy"):
        for bad in (-0.1, float("nan"), float("inf"), (0.1,), (0.1, 0.2, 0.3), "x", True):
            with pytest.raises(ValueError, match=name):
                _engine(s, alpha="matte", **{name: bad})
    for bad in ("white", (1, 1), (1, 1, float("nan"))):
        with pytest.raises(ValueError, match="background"):
            _engine(s, alpha="matte", background=bad)
    e = _engine(s, alpha="matte")
    with pytest.raises(ValueError, match="alpha"):
        e.forward_backward(s["rays"], s["target"][:, :3])
    X = N.Exposure(1, learn="affine", lr=1e-3, device=s["dev"])
    inds = torch.zeros(s["rays"].shape[0], dtype=torch.int64, device=s["dev"])
    with pytest.raises(ValueError, match="exposure"):
        e.forward_backward(s["rays"], s["target"], exposure=(X, inds, s["H"] * s["W"]))


# ---- drop-in ----------------------------------------------------------------------------------------------------------------------
def test_dropin_matte_mse_loss_equals_the_engine(lego, gpu):
    """run_one_iter_of_nerf, then (matte_mse_loss of each net's rgb and acc).backward(), against the engine's gradient on the same
    rays: within 1e-4 of its norm per net (the bound of test_gpu_pose.py::test_engine_pose_gradient_equals_dropin: the two routes
    differ in the backward's buffer layout); the detached parts are the engine's matte_losses on the bits."""
    s, N = lego, lego["N"]
    mc, mf = copy.deepcopy(s["mc"]), copy.deepcopy(s["mf"])
    ex, ed = N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)
    out = N.run_one_iter_of_nerf(s["H"], s["W"], s["focal"], mc, mf, s["ro"], s["rd"], s["opts"], encode_position_fn=ex, encode_direction_fn=ed)
    e = _engine(s, alpha="matte", alpha_loss=LAM_A, opacity_entropy=LAM_H, seed=SEED)
    e.forward_backward(s["rays"], s["target"])
    tc, pc = N.matte_mse_loss(out[0], out[2], s["target"], alpha_loss=LAM_A[0], opacity_entropy=LAM_H[0], seed=SEED)
    tf, pf = N.matte_mse_loss(out[3], out[5], s["target"], alpha_loss=LAM_A[1], opacity_entropy=LAM_H[1], seed=SEED)
    assert tc.requires_grad and not pc.requires_grad
    assert torch.equal(pc, e.matte_losses[0]) and torch.equal(pf, e.matte_losses[1])
    want = float(pc[0]) + LAM_A[0] * float(pc[1]) + LAM_H[0] * float(pc[2])
    assert abs(float(tc.detach()) - want) <= 1e-6 * abs(want)
    (tc + tf).backward()
    n0 = e.nc_params
    for model, flat in ((mc, e.grad[:n0]), (mf, e.grad[n0:])):
        got = torch.cat([p.grad.reshape(-1) for p in model._ordered_params()])
        ref = torch.cat([g.reshape(-1) for g in model._split_flat(flat)])
        rel = float((got - ref).norm() / ref.norm())
        print("drop-in against the engine: %.3e of the norm" % rel)
        assert rel < 1e-4, rel
    # the node hands out the kernel's cotangents times the incoming one; weight mode and a given background go through
    rgb = out[3].detach().requires_grad_(True)
    acc = out[5].detach().requires_grad_(True)
    t1, _ = N.matte_mse_loss(rgb, acc, s["target"], mode="weight", opacity_entropy=0.05)
    (3.0 * t1).backward()
    _, g_rgb, g_acc = M.matte_loss(gpu, rgb.detach().cpu().numpy(), acc.detach().cpu().numpy(), s["target"].cpu().numpy(), 1, lam=(0.0, 0.05))
    assert torch.equal(rgb.grad.cpu(), 3.0 * torch.from_numpy(g_rgb)) and torch.equal(acc.grad.cpu(), 3.0 * torch.from_numpy(g_acc))
    bg = torch.rand(rgb.shape[0], 3, device=s["dev"])
    t2, p2 = N.matte_mse_loss(rgb, acc, s["target"], background=bg)
    t3, p3 = N.matte_mse_loss(rgb, acc, s["target"], background=(1.0, 1.0, 1.0))
    assert torch.equal(t2, p2[0]) and not torch.equal(p2[0], p3[0])
    for bad in (dict(mode="x"), dict(mode="weight", alpha_loss=0.1), dict(background=(1, 1))):
        with pytest.raises(ValueError):
            N.matte_mse_loss(rgb, acc, s["target"], **bad)
    with pytest.raises(ValueError, match="target_rgba"):
        N.matte_mse_loss(rgb, acc, s["target"][:, :3].contiguous())


# ---- capability ------------------------------------------------------------------------------------------------------------------
# alpha_loss of the capability test, fixed beforehand from the CPU study with the oracle's autograd on the same setup
# (scripts/study_matte_weights.py -> profiles/r21_matte_study.json)
ALPHA_CAP = 0.1
CAP_TRAIN = (0, 2, 4)   # the 0, 40 and 80 degree views of occupancy_train_cases.CAP_ANGLES; the 60 degree view is held out


@pytest.fixture(scope="module")
def lego64(gpu):
    return ES.lego64()


def _fine_maps(N, rays, mc, mf, white):
    """(rgb_fine, acc_fine) of a dense 64 + 64 render without perturbation or noise (predict_and_render_radiance, validation mode)."""
    opts = N.make_options(64, 64, perturb=False, white_background=white, radiance_field_noise_std=0.0)
    with torch.no_grad():
        out = N.predict_and_render_radiance(rays.contiguous(), mc, mf, opts, mode="validation",
                                            encode_position_fn=N.get_embedding_function(10, True, True),
                                            encode_direction_fn=N.get_embedding_function(4, True, True))
    return out[3], out[5]


def _rgba_scene(s):
    """The teacher views as RGBA: a = clamp(teacher acc_fine, 0, 1), C = clamp((rgb_white - (1 - a)) / max(a, 1e-3), 0, 1)."""
    import occupancy_train_cases as OT
    if "rgba" in s:
        return s["rgba"]
    rays, white = OT.teacher_views(s)
    rgba = []
    for i in range(rays.shape[0]):
        a = _fine_maps(s["N"], rays[i], s["mc"], s["mf"], True)[1].clamp(0.0, 1.0)
        C = ((white[i] - (1.0 - a)[:, None]) / a.clamp(min=1e-3)[:, None]).clamp(0.0, 1.0)
        rgba.append(torch.cat((C, a[:, None]), dim=1))
    s["rgba"] = (rays, white, torch.stack(rgba))
    return s["rgba"]


def _capability_arm(s, seed, matte, steps=400, n_rays=1024, lr=5e-3, noise_std=1.0):
    import occupancy_train_cases as OT
    N = s["N"]
    rays, white, rgba = _rgba_scene(s)
    train = list(CAP_TRAIN)
    pool_r, pool_t = rays[train].reshape(-1, rays.shape[-1]), rgba[train].reshape(-1, 4)
    if not matte:   # (the parent's behaviour: the RGBA rows composited onto white, against the white-background render)
        pool_t = pool_t[:, 3:] * pool_t[:, :3] + (1.0 - pool_t[:, 3:])
    torch.manual_seed(seed)
    cfg = dict(num_layers=4, hidden_size=64, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    mc, mf = N.FlexibleNeRFModel(**cfg).to(s["dev"]), N.FlexibleNeRFModel(**cfg).to(s["dev"])
    kw = dict(white_background=False, alpha="matte", background="random", alpha_loss=ALPHA_CAP) if matte else dict(white_background=True)
    eng = N.TrainEngine(mc, mf, 64, 64, perturb=True, noise_std=noise_std, lr=lr, seed=seed, **kw)
    picks = torch.randint(0, pool_r.shape[0], (steps, n_rays), generator=torch.Generator().manual_seed(seed)).to(s["dev"])
    losses = torch.zeros(steps, device=s["dev"])
    for i in range(steps):
        losses[i] = eng.step(pool_r[picks[i]].contiguous(), pool_t[picks[i]].contiguous())[2]
    h = OT.CAP_HELD_OUT
    rgb, acc = _fine_maps(N, rays[h], mc, mf, False)
    mse = float(((rgb + (1.0 - acc)[:, None] - white[h]).double() ** 2).mean().item())
    aerr = float((acc - rgba[h][:, 3]).abs().double().mean().item())
    return dict(finite=bool(torch.isfinite(losses).all().item()), psnr=float(-10.0 * np.log10(max(mse, 1e-30))), acc_err=aerr)


def test_capability_the_matte_loss_learns_the_opacity(lego64):
    """RGBA captures: three 64 x 64 teacher views of the fixture nets (0, 40, 80 degrees; the 60-degree view held out) with a =
    clamp(teacher acc_fine) and C un-composited from the teacher's white render train two 4 x 64 students for 400 steps of 1024 rays
    (lr 5e-3, sigma noise 1.0), seeds 0, 1 and 2: white_background=True on a C + (1 - a) (the parent's behaviour) against
    white_background=False, alpha="matte", background="random", alpha_loss=ALPHA_CAP.  On the held-out view: every step's loss
    finite; for every seed the matte arm's mean |acc_fine - a| is below the plain arm's; and its PSNR over white (rgb + 1 - acc against
    the teacher) is no lower than the plain arm's mean minus twice the plain arm's own spread over the seeds (the floor of
    test_gpu_spread.py, for its reason).
    ALPHA_CAP comes from the CPU study (seed 0; plain 19.77 dB / opacity error 0.0489; alpha_loss 0: 18.77 / 0.0350; 0.01: 18.92 /
    0.0319; 0.1: 20.07 / 0.0273; 1: 18.85 / 0.0223 -- the rule fixed in the script: of the matte arms within 0.5 dB of the plain one,
    the lowest opacity error: 0.1).
    Measured on the MI355X (seeds 0 / 1 / 2): plain 19.26 / 20.11 / 18.97 dB with opacity error 0.0349 / 0.0379 / 0.0380; matte
    19.48 / 19.93 / 19.70 dB with opacity error 0.0263 / 0.0255 / 0.0246; the PSNR floor comes out at 17.17 dB."""
    assert ALPHA_CAP is not None
    plain = [_capability_arm(lego64, seed, False) for seed in (0, 1, 2)]
    matte = [_capability_arm(lego64, seed, True) for seed in (0, 1, 2)]
    print("capability: " + json.dumps(dict(plain=plain, matte=matte, alpha_loss=ALPHA_CAP)))
    assert all(r["finite"] for r in plain + matte)
    psnr = [r["psnr"] for r in plain]
    floor = float(np.mean(psnr)) - 2.0 * (max(psnr) - min(psnr))
    for p, r in zip(plain, matte):
        assert r["acc_err"] < p["acc_err"], (p, r)
        assert r["psnr"] >= floor, (r, floor)
