"""GPU suite (-m gpu) of the robust photometric loss: the cases of tests/robust_cases.py on the product library, and the public routes:
TrainEngine(photometric=, trim=) on its steps, its robust_stats, and the drop-in API's robust_mse_loss."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import engine_scenes as ES
import robust_cases as R
import spread_cases as S
from conftest import ROOT, gold

pytestmark = pytest.mark.gpu


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,param", R.KERNEL_KINDS)
def test_kernel_against_the_definition(gpu, kind, param):
    R.case_kernel(gpu, kind, param)


def test_kernel_keeps_every_tie(gpu):
    R.case_ties(gpu)


def test_kernel_bit_identities(gpu):
    R.case_bit_identities(gpu)


def test_kernel_keeps_a_nan_ray_and_reports_it(gpu):
    R.case_nan(gpu)


def test_kernel_refusals(gpu):
    R.case_refusals(gpu)


def test_kernel_selection_beyond_the_register_keys(gpu):
    """More than 4096 rays: the keys past the four a thread holds in registers are read back from tmp in every round."""
    for n in (4097, 9001):
        R.check_trimmed(gpu, n, 3, 2, 0.3, 0.8, 4000 + n)


# ---- through the render ------------------------------------------------------------------------------------------------------------
def test_parameter_gradients_against_the_oracle(gpu):
    R.case_param_grads(gpu, "w64", "fp32")


def test_backward_modes_under_a_trim(gpu):
    R.case_modes(gpu, "w64", "fp32", (True, "recompute", "fused", "fused_compact", "fused_stash"))


# ---- engine and drop-in ------------------------------------------------------------------------------------------------------------
CFG = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
SAMPLING = dict(num_coarse=64, num_fine=64, perturb=False, white_background=False, noise_std=0.0)
PHOTO = (("huber", 0.1), ("charbonnier", 1e-3))   # (coarse, fine)
TRIM = (0.8, 0.5)
LAM = (0.02, 0.01)                                # (the spread weights of the stacked case)
SEED = 5


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
    opts = N.make_options(64, 64, perturb=False, white_background=False, radiance_field_noise_std=0.0)
    ro, rd = N.get_rays_at_pixels(H, W, focal, pose[:3, :4], torch.arange(H * W, dtype=torch.int64, device=dev))
    rays = N.pack_rays(ro, rd, opts, H, W, focal)
    target = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    return dict(N=N, dev=dev, mc=mc, mf=mf, H=H, W=W, focal=focal, pose=pose, opts=opts, ro=ro, rd=rd, rays=rays, target=target)


def _engine(s, **kw):
    return s["N"].TrainEngine(copy.deepcopy(s["mc"]), copy.deepcopy(s["mf"]), **dict(SAMPLING, **kw))


def test_engine_without_the_keywords_is_the_engine(lego):
    s = lego
    engines = [_engine(s), _engine(s, photometric=None, trim=None), _engine(s, photometric="l2", trim=(1.0, 1.0))]
    for _ in range(3):
        for e in engines:
            e.step(s["rays"], s["target"])
    a = engines[0]
    assert a.grad.abs().max() > 0
    for e in engines:
        assert e.robust is None and e.robust_stats is None and "rt_c" not in e._bufs
        assert torch.equal(a.loss, e.loss) and torch.equal(a.grad, e.grad)
        assert torch.equal(a.mc.flat_params, e.mc.flat_params) and torch.equal(a.mf.flat_params, e.mf.flat_params)


def _by_hand(s, gpu, e, spread=None):
    """One step's C calls on the engine's own plans: forward, [spread launches,] the two robust losses, the backward."""
    rays, tgt = s["rays"].cpu().numpy(), s["target"].cpu().numpy()
    r = S.RenderW(gpu, e.mc._plan, e.mf._plan, e.packed_c, e.packed_f, rays, SAMPLING, {})
    gw = None
    if spread is not None:
        gw = [r.spread(bool(fine), spread[fine] / r.n)[1] for fine in (0, 1)]
    res = [R.robust_loss(gpu, r.out["rgb_" + tag], tgt, R.KINDS[PHOTO[i][0]], PHOTO[i][1], keep=TRIM[i]) for i, tag in enumerate(("coarse", "fine"))]
    want = r.backward((res[0]["g_rgb"], res[1]["g_rgb"]), gw, entry="parts" if gw is None else "parts_w")
    return want, res


@pytest.mark.parametrize("overlap", [True, False])
def test_engine_step_is_the_c_entry_points(lego, gpu, overlap):
    """One engine step with a kind and a trim per net against nerfhip_render_fwd + nerfhip_robust_loss_fwd_bwd + nerfhip_render_bwd_parts
    assembled by hand on the engine's own plans, on two streams and on one: gradient, loss and robust_stats bit for bit -- and not the
    plain engine's gradient; then stacked behind spread= (the _w backward)."""
    s = lego
    kw = dict(photometric=PHOTO, trim=TRIM, overlap=overlap, seed=SEED)
    e, plain = _engine(s, **kw), _engine(s, overlap=overlap, seed=SEED)
    e.forward_backward(s["rays"], s["target"])
    plain.forward_backward(s["rays"], s["target"])
    want, (c, f) = _by_hand(s, gpu, e)
    n0 = e.nc_params
    grad = e.grad.cpu().numpy()
    assert np.array_equal(grad[:n0], want["g_params_coarse"]) and np.array_equal(grad[n0:], want["g_params_fine"])
    assert not torch.equal(e.grad[:n0], plain.grad[:n0]) and not torch.equal(e.grad[n0:], plain.grad[n0:])
    loss = e.loss.cpu().numpy()
    assert loss[0] == c["loss"][0] and loss[1] == f["loss"][0] and loss[2] == np.float32(c["loss"][0]) + np.float32(f["loss"][0])
    # robust_stats: the kernel's words, per net
    sc, sf = (t.cpu().numpy() for t in e.robust_stats)
    assert np.array_equal(R.bits(sc), R.bits(c["loss"][1:])) and np.array_equal(R.bits(sf), R.bits(f["loss"][1:]))
    n = s["rays"].shape[0]
    assert sc[0] >= np.float32(R.keep_count(TRIM[0], n) / n) and sf[0] >= 0.5 and 0 < sc[1] < np.inf and 0 < sf[1] < np.inf
    assert sc[0] < 1.0 and sf[0] < 1.0
    # stacked behind the spread term
    e2, only = _engine(s, spread=LAM, **kw), _engine(s, spread=LAM, overlap=overlap, seed=SEED)
    e2.forward_backward(s["rays"], s["target"])
    only.forward_backward(s["rays"], s["target"])
    want2, _ = _by_hand(s, gpu, e2, LAM)
    grad = e2.grad.cpu().numpy()
    assert np.array_equal(grad[:n0], want2["g_params_coarse"]) and np.array_equal(grad[n0:], want2["g_params_fine"])
    assert not torch.equal(e2.grad, only.grad) and not torch.equal(e2.grad, e.grad)


def test_engine_trim_drops_samples_from_the_compacted_backward(lego):
    """A trimmed ray's g_rgb row is zero, so its samples' d(loss)/d(raw) rows are: the compacted backward keeps fewer samples than the
    same step untrimmed."""
    s = lego
    a, b = _engine(s, backward="compact", seed=SEED, trim=0.5), _engine(s, backward="compact", seed=SEED)
    a.forward_backward(s["rays"], s["target"])
    b.forward_backward(s["rays"], s["target"])
    ca, cb = a.backward_sample_counts(), b.backward_sample_counts()
    for name in ("coarse", "fine"):
        assert ca[name][1] == cb[name][1] and 0 < ca[name][0] < cb[name][0], (name, ca, cb)
    assert float(a.robust_stats[0][0]) >= 0.5 and float(a.robust_stats[0][0]) < 0.51
    # trim alone is kind 0: an engine whose trim keeps every ray gives the plain engine's bits
    c = _engine(s, backward="compact", seed=SEED, photometric=("huber", 1e30))
    c.forward_backward(s["rays"], s["target"])
    assert torch.equal(c.grad, b.grad) and torch.equal(c.loss, b.loss)
    assert torch.equal(c.robust_stats[1].cpu(), torch.tensor([1.0, float("inf")]))


def test_engine_without_a_fine_net(lego):
    """num_fine = 0: loss = {robust_c, 0, robust_c}, robust_stats = (coarse, None), the pairs' fine halves are not looked at."""
    s = lego
    kw = dict(SAMPLING, num_fine=0, photometric=("l1", ("huber", 0.1)), trim=(0.7, 0.2), seed=SEED)
    e = s["N"].TrainEngine(copy.deepcopy(s["mc"]), None, **kw)
    assert e.robust == ((1, 0.0, 0.7), (0, 0.0, 1.0))
    e.forward_backward(s["rays"], s["target"])
    st, none = e.robust_stats
    assert none is None and torch.isfinite(e.grad).all() and e.grad.abs().max() > 0 and 0.7 <= float(st[0]) < 0.71
    assert float(e.loss[0]) > 0 and torch.equal(e.loss.cpu(), torch.stack((e.loss[0], torch.zeros_like(e.loss[0]), e.loss[0])).cpu())


def _views(s, V, H, W, seed=5):
    g = torch.Generator().manual_seed(seed)
    images = torch.rand(V, H, W, 3, generator=g).to(s["dev"])
    poses = s["pose"][None].repeat(V, 1, 1).clone()
    for v in range(V):
        a = 0.3 * v
        rot = torch.tensor([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=torch.float32, device=s["dev"])
        poses[v, :3, :4] = rot @ s["pose"][:3, :4]
    return images, poses.contiguous(), s["focal"] * W / s["W"]


def test_frozen_localize_step_takes_the_robust_loss(lego):
    s = lego
    V, H, W, n = 3, 6, 10, 128
    images, poses, focal = _views(s, V, H, W)
    a, p = _engine(s, photometric="l1", trim=0.8, seed=9), _engine(s, seed=9)
    ga, gp = (torch.zeros(V, 3, 4, device=s["dev"]) for _ in range(2))
    a.localize_on_views(images, poses, H, W, focal, s["opts"], n, pose_grads=ga)
    p.localize_on_views(images, poses, H, W, focal, s["opts"], n, pose_grads=gp)
    for x, y in ((a._ray_grad, p._ray_grad), (a.ray_grad_coarse, p.ray_grad_coarse), (ga, gp)):
        assert torch.isfinite(x).all() and x.abs().max() > 0 and not torch.equal(x, y)
    assert not a.grad.any() and 0.8 <= float(a.robust_stats[1][0]) < 1.0 and float(a.loss[1]) > 0


def test_engine_refusals(lego):
    s, N = lego, lego["N"]
    for kw in (dict(photometric="l1"), dict(trim=0.5)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            _engine(s, alpha="weight", **kw)
    with pytest.raises(ValueError, match="photometric.*unknown kind"):
        _engine(s, photometric="tukey")
    for bad in (("huber", 0.0), ("huber", float("nan")), ("charbonnier", -1.0), ("relative",), 3):
        with pytest.raises(ValueError, match="photometric"):
            _engine(s, photometric=bad)
    for bad in (0.0, 1.5, float("nan"), (0.5,), "x"):
        with pytest.raises(ValueError, match="trim"):
            _engine(s, trim=bad)
    e = _engine(s, photometric="l1")
    X = N.Exposure(1, learn="affine", lr=1e-3, device=s["dev"])
    inds = torch.zeros(s["rays"].shape[0], dtype=torch.int64, device=s["dev"])
    with pytest.raises(ValueError, match="photometric"):
        e.forward_backward(s["rays"], s["target"], exposure=(X, inds, s["H"] * s["W"]))


def test_dropin_robust_mse_loss_equals_the_engine(lego, gpu):
    """run_one_iter_of_nerf, then (robust_mse_loss of each net's rgb).backward(), against the engine's gradient on the same rays: within
    1e-4 of its norm per net (the bound of test_gpu_matte.py's drop-in test, for its reason); the detached words are the engine's."""
    s, N = lego, lego["N"]
    mc, mf = copy.deepcopy(s["mc"]), copy.deepcopy(s["mf"])
    ex, ed = N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)
    out = N.run_one_iter_of_nerf(s["H"], s["W"], s["focal"], mc, mf, s["ro"], s["rd"], s["opts"], encode_position_fn=ex, encode_direction_fn=ed)
    e = _engine(s, photometric=PHOTO, trim=TRIM, seed=SEED)
    e.forward_backward(s["rays"], s["target"])
    lc, (kc, tc) = N.robust_mse_loss(out[0], s["target"], *PHOTO[0], trim=TRIM[0])
    lf, (kf, tf) = N.robust_mse_loss(out[3], s["target"], *PHOTO[1], trim=TRIM[1])
    assert lc.requires_grad and not kc.requires_grad and not tc.requires_grad
    assert torch.equal(torch.stack((lc.detach(), lf.detach())), e.loss[:2])
    assert torch.equal(torch.stack((kc, tc)), e.robust_stats[0]) and torch.equal(torch.stack((kf, tf)), e.robust_stats[1])
    (lc + lf).backward()
    n0 = e.nc_params
    for model, flat in ((mc, e.grad[:n0]), (mf, e.grad[n0:])):
        got = torch.cat([p.grad.reshape(-1) for p in model._ordered_params()])
        ref = torch.cat([g.reshape(-1) for g in model._split_flat(flat)])
        rel = float((got - ref).norm() / ref.norm())
        print("drop-in against the engine: %.3e of the norm" % rel)
        assert rel < 1e-4, rel
    # the node hands out the kernel's cotangent times the incoming one
    rgb = out[3].detach().requires_grad_(True)
    l1, _ = N.robust_mse_loss(rgb, s["target"], "l1")
    (3.0 * l1).backward()
    want = R.robust_loss(gpu, rgb.detach().cpu().numpy(), s["target"].cpu().numpy(), 1)["g_rgb"]
    assert torch.equal(rgb.grad.cpu(), 3.0 * torch.from_numpy(want))
    for bad in (dict(kind="x"), dict(kind="huber", param=0.0), dict(trim=0.0), dict(trim=2.0)):
        with pytest.raises(ValueError):
            N.robust_mse_loss(rgb, s["target"], **bad)


# ---- capability ------------------------------------------------------------------------------------------------------------------
# The robust arm of the capability test, fixed beforehand from the CPU study with the oracle's autograd on the same setup
# (scripts/study_robust.py -> profiles/r22_robust_study.json)
STUDY = os.path.join(ROOT, "profiles", "r22_robust_study.json")
CAP_TRAIN = (0, 2, 4)   # the 0, 40 and 80 degree views of occupancy_train_cases.CAP_ANGLES; the 60 degree view is held out


@pytest.fixture(scope="module")
def lego64(gpu):
    return ES.lego64()


def _capability_arm(s, seed, spec, steps=400, n_rays=1024, lr=5e-3, noise_std=1.0):
    import occupancy_train_cases as OT
    N = s["N"]
    rays, white = OT.teacher_views(s)
    train = list(CAP_TRAIN)
    dirty, _ = R.corrupt(white[train].cpu(), spec["corruption_rate"])
    pool_r, pool_t = rays[train].reshape(-1, rays.shape[-1]), dirty.reshape(-1, 3).to(s["dev"])
    torch.manual_seed(seed)
    cfg = dict(num_layers=4, hidden_size=64, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    mc, mf = N.FlexibleNeRFModel(**cfg).to(s["dev"]), N.FlexibleNeRFModel(**cfg).to(s["dev"])
    kw = {} if spec["kind"] is None else dict(photometric=spec["kind"] if spec["kind"] in ("l1", "l2") else (spec["kind"], spec["param"]),
                                              trim=spec["trim"] if spec["trim"] < 1.0 else None)
    eng = N.TrainEngine(mc, mf, 64, 64, perturb=True, white_background=True, noise_std=noise_std, lr=lr, seed=seed, **kw)
    picks = torch.randint(0, pool_r.shape[0], (steps, n_rays), generator=torch.Generator().manual_seed(seed)).to(s["dev"])
    losses = torch.zeros(steps, device=s["dev"])
    for i in range(steps):
        losses[i] = eng.step(pool_r[picks[i]].contiguous(), pool_t[picks[i]].contiguous())[2]
    h = OT.CAP_HELD_OUT
    with torch.no_grad():
        out = N.predict_and_render_radiance(rays[h], mc, mf, s["opts"], mode="validation", encode_position_fn=N.get_embedding_function(10, True, True),
                                            encode_direction_fn=N.get_embedding_function(4, True, True))
    mse = float(((out[3] - white[h]).double() ** 2).mean().item())
    return dict(finite=bool(torch.isfinite(losses).all().item()), psnr_clean=float(-10.0 * np.log10(max(mse, 1e-30))))


def test_capability_the_robust_loss_ignores_the_outliers(lego64):
    """Three 64 x 64 teacher views of the fixture nets over white (0, 40, 80 degrees; the 60-degree view held out), a fixed random 30 %
    of every training view's pixels replaced by saturated random colours (robust_cases.corrupt), train two 4 x 64 students for 400 steps
    of 1024 rays (lr 5e-3, sigma noise 1.0), seeds 0, 1 and 2: the plain squared error against the arm the CPU study chose
    (profiles/r22_robust_study.json, the rule fixed in scripts/study_robust.py: the highest held-out PSNR against the clean view).  The
    MSE optimum at a pixel is 0.7 C + 0.3 E[o], so the plain arm's PSNR against the CLEAN held-out view is capped; the L1 / Huber
    optimum is the median, C.  Every step's loss is finite, and for every seed the robust arm's held-out clean PSNR exceeds the plain
    arm's.
    The study (seed 0; plain at seeds 0 / 1 / 2: 8.80 / 9.23 / 12.40 dB, so the margin is 3.60 dB; a model at the MSE optimum scores
    17.60 dB): l1 8.22, Huber 0.05 8.22, Huber 0.1 19.00, Huber 0.2 17.90, Charbonnier 1e-3 8.22, Huber 0.1 with trim 0.6 8.22 dB
    (8.22 dB is the all-white image) -- Huber 0.1 without a trim.
    Measured on the MI355X (seeds 0 / 1 / 2): plain 9.70 / 14.20 / 13.08 dB; Huber 0.1 19.66 / 19.19 / 19.22 dB."""
    with open(STUDY) as f:
        study = json.load(f)
    assert study["wins"], "the CPU study found no robust arm that beats the plain one by the plain arm's own spread"
    chosen = dict(study["chosen"], corruption_rate=study["corruption_rate"])
    none = dict(kind=None, corruption_rate=study["corruption_rate"])
    plain = [_capability_arm(lego64, seed, none) for seed in (0, 1, 2)]
    robust = [_capability_arm(lego64, seed, chosen) for seed in (0, 1, 2)]
    print("capability: " + json.dumps(dict(plain=plain, robust=robust, chosen=chosen, margin_db=study["margin_db"])))
    assert all(r["finite"] for r in plain + robust)
    for p, r in zip(plain, robust):
        assert r["psnr_clean"] > p["psnr_clean"], (p, r)
