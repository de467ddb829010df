"""GPU suite (-m gpu): the device-resident intrinsics -- the kernels of tests/intrinsics_cases.py on the product library, the drop-in
autograd node (select_training_rays_views(intrinsics=...)), cameras.Intrinsics and TrainEngine.step_on_views / localize_on_views
(intrinsics=...), and a focal length that starts 5 % off recovered against frozen nets."""
import json

import numpy as np
import pytest
import torch

import engine_scenes as ES
import intrinsics_cases as IC
import pose_vjp as P

pytestmark = pytest.mark.gpu


# ---- the kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("layout", ["4x4", "embedded"])
def test_selection_with_the_scalar_camera_as_intrinsics_has_the_scalar_bits(gpu, ndc, view, layout):
    IC.case_selection_bits(gpu, ndc, view, layout)


def test_ray_bundle_from_intrinsics(gpu):
    IC.case_bundle_bits(gpu)


@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
def test_selection_rows_against_fp64(gpu, ndc, view):
    IC.case_selection_fp64(gpu, ndc, view)


@pytest.mark.parametrize("n", [1, 63, 256, 257, 700])
@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("two,stride", [(False, 11), (True, 16), (True, 11), (False, 16)])
def test_vjp_against_fp64(gpu, n, ndc, view, two, stride):
    IC.case_vjp(gpu, n, ndc, view, two, stride)


@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
def test_vjp_against_fp64_4096_rays_over_100_views(gpu, ndc, view):
    IC.case_vjp(gpu, 4096, ndc, view, True, 11, big=True)


@pytest.mark.parametrize("n", [1, 63, 256, 257, 700])
@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
def test_vjp_pose_gradient_has_the_scalar_bits(gpu, n, ndc, view):
    IC.case_vjp_poses_equal_the_scalar_form(gpu, n, ndc, view)


def test_vjp_of_no_rays_an_empty_view_and_dropped_indices(gpu):
    IC.case_vjp_edges(gpu)


@pytest.mark.parametrize("tie", [False, True])
def test_parametrisation_forward(gpu, tie):
    IC.case_param_fwd(gpu, tie)


@pytest.mark.parametrize("tie", [False, True])
@pytest.mark.parametrize("mask", IC.MASKS, ids=["".join(map(str, m)) for m in IC.MASKS])
def test_parametrisation_pull_back_and_masks(gpu, tie, mask):
    IC.case_param_bwd(gpu, tie, mask)


def test_entry_points_reject_bad_arguments(gpu):
    IC.case_refusals(gpu)


# ---- drop-in autograd ---------------------------------------------------------------------------------------------------------------
def test_dropin_intrinsics_gradient_is_the_kernel_and_none_is_the_existing_path():
    """select_training_rays_views(intrinsics=t): with t (and with the poses) requiring grad, backward() leaves the bits of the _bwd
    call; the forward is the plain launch; intrinsics=None is today's node and function; the bundle forms take the intrinsics
    forward only."""
    import nerf_pytorch_amd as N
    dev = ES.dev()
    _, _, H, W, focal, pose0 = ES.lego(dev)
    V, n = 3, 700
    g = torch.Generator().manual_seed(8)
    imgs = torch.rand(V, H, W, 3, generator=g).to(dev)
    gr = torch.randn(n, 11, generator=g).to(dev)
    opts = N.make_options(64, 64)
    poses = ES.views(pose0, dev, V)
    intr = torch.tensor([focal * 1.03, focal * 0.98, W * 0.5 + 1.25, H * 0.5 - 0.75], dtype=torch.float32, device=dev)
    plain = N.select_training_rays_views(H, W, focal, poses, imgs, n, opts, seed=4, step=1, intrinsics=intr)
    assert plain[0].grad_fn is None
    want_p, want_i = N.select_training_rays_views_bwd(H, W, focal, poses, plain[2], gr, opts, intrinsics=intr)
    assert tuple(want_p.shape) == (V, 3, 4) and tuple(want_i.shape) == (4,)
    assert torch.all(torch.isfinite(want_i)) and torch.all(want_i != 0)
    for with_poses in (False, True):
        t = intr.clone().requires_grad_(True)
        p = poses.clone().requires_grad_(with_poses)
        rays, tgt, used = N.select_training_rays_views(H, W, focal, p, imgs, n, opts, seed=4, step=1, intrinsics=t)
        assert rays.grad_fn is not None and not tgt.requires_grad and not used.requires_grad
        for a, b in zip((rays, tgt, used), plain):
            assert torch.equal(a, b)
        (rays * gr).sum().backward()
        assert torch.equal(t.grad, want_i)
        if with_poses:
            assert torch.equal(p.grad[:, :3, :4], want_p) and torch.all(p.grad[:, 3] == 0)
        else:
            assert p.grad is None
    # the poses alone require grad: the intrinsics get none
    p = poses.clone().requires_grad_(True)
    rays, _, _ = N.select_training_rays_views(H, W, focal, p, imgs, n, opts, seed=4, step=1, intrinsics=intr)
    (rays * gr).sum().backward()
    assert torch.equal(p.grad[:, :3, :4], want_p) and intr.grad is None
    # out= / out_intrinsics= are written in place
    op, oi = torch.full((V, 3, 4), float("nan"), device=dev), torch.full((4,), float("nan"), device=dev)
    N.select_training_rays_views_bwd(H, W, focal, poses, plain[2], gr, opts, out=op, intrinsics=intr, out_intrinsics=oi)
    assert torch.equal(op, want_p) and torch.equal(oi, want_i)
    # the intrinsics' gradient alone: the same bits, no pose gradient
    no_p, only_i = N.select_training_rays_views_bwd(H, W, focal, poses, plain[2], gr, opts, intrinsics=intr, want_poses=False)
    assert no_p is None and torch.equal(only_i, want_i)
    with pytest.raises(RuntimeError, match="want_poses"):
        N.select_training_rays_views_bwd(H, W, focal, poses, plain[2], gr, opts, want_poses=False)
    # intrinsics=None: the existing node and function, unchanged
    p = poses.clone().requires_grad_(True)
    r0 = N.select_training_rays_views(H, W, focal, p, imgs, n, opts, seed=4, step=1, intrinsics=None)
    r1 = N.select_training_rays_views(H, W, focal, p, imgs, n, opts, seed=4, step=1)
    r2 = N.select_training_rays_views(H, W, focal, poses, imgs, n, opts, seed=4, step=1)
    for a, b, c in zip(r0, r1, r2):
        assert torch.equal(a, b) and torch.equal(a, c)
    (r0[0] * gr).sum().backward()
    assert torch.equal(p.grad[:, :3, :4], N.select_training_rays_views_bwd(H, W, focal, poses, r2[2], gr, opts))
    # the scalar camera as intrinsics: the bits of the scalar call; one view through select_training_rays
    cen = torch.tensor([focal, focal, W * 0.5, H * 0.5], dtype=torch.float32, device=dev)
    rc = N.select_training_rays_views(H, W, focal, poses, imgs, n, opts, seed=4, step=1, intrinsics=cen)
    assert torch.equal(rc[0], r2[0]) and torch.equal(rc[2], r2[2])
    s0 = N.select_training_rays(H, W, focal, poses[1], imgs[1], 256, opts, seed=2, step=0)
    s1 = N.select_training_rays(H, W, focal, poses[1], imgs[1], 256, opts, seed=2, step=0, intrinsics=cen)
    assert torch.equal(s0[0], s1[0]) and torch.equal(s0[1], s1[1]) and torch.equal(s0[2], s1[2])
    # the bundle forms: forward only
    ro0, rd0 = N.get_ray_bundle(H, W, focal, poses[0])
    ro1, rd1 = N.get_ray_bundle(H, W, focal, poses[0], intrinsics=cen)
    assert torch.equal(ro0, ro1) and torch.equal(rd0, rd1)
    pix = torch.tensor([0, 5, H * W - 1], device=dev)
    a, b = N.get_rays_at_pixels(H, W, focal, poses[0], pix, intrinsics=intr)
    full = N.get_ray_bundle(H, W, focal, poses[0], intrinsics=intr)
    assert torch.equal(b, full[1].reshape(-1, 3)[pix]) and not torch.equal(full[1], rd0)
    with pytest.raises(RuntimeError, match="forward only"):
        N.get_ray_bundle(H, W, focal, poses[0].clone().requires_grad_(True), intrinsics=intr)


# ---- cameras.Intrinsics and the engine ------------------------------------------------------------------------------------------------
def test_intrinsics_object_values_masks_and_state():
    import nerf_pytorch_amd as N
    dev = ES.dev()
    I = N.Intrinsics(378, 504, 407.5, learn="focal", lr=1e-2, device=dev)
    assert torch.equal(I.values(), torch.tensor([407.5, 407.5, 252.0, 189.0], device=dev))
    g = torch.tensor([0.5, -0.25, 3.0, -2.0], device=dev)
    for _ in range(3):
        I.backward(g)
        I.step()
    v = I.values().clone()
    assert I.step_count == 3 and float(I.q[0]) != 0 and torch.all(I.q[1:] == 0)
    assert float(v[0]) == float(v[1]) != 407.5 and float(v[2]) == 252.0 and float(v[3]) == 189.0   # tied focals, a fixed principal point
    J = N.Intrinsics(378, 504, (400.0, 410.0, 250.0, 190.0), learn="all", lr=1e-2, device=dev)
    assert torch.equal(J.values(), torch.tensor([400.0, 410.0, 250.0, 190.0], device=dev))
    J.backward(g)
    J.step()
    assert torch.all(J.q != 0)
    state = J.state_dict()
    K = N.Intrinsics(378, 504, 1.0, learn="all", lr=1e-2, device=dev)
    K.load_state_dict(state)
    for o in (J, K):
        o.backward(g)
        o.step()
    assert K.step_count == J.step_count == 2
    for name in ("q", "exp_avg", "exp_avg_sq", "g_q", "base"):
        assert torch.equal(getattr(J, name), getattr(K, name)), name
    assert torch.equal(J.values(), K.values())
    with pytest.raises(RuntimeError, match="learn"):
        N.Intrinsics(378, 504, 407.5, learn="everything", device=dev)
    with pytest.raises(RuntimeError, match="learn"):
        N.Intrinsics(378, 504, 407.5, learn="focal", device=dev).load_state_dict(state)


def _by_hand(eng, N, T, I, imgs, H, W, focal, opts, n):
    """One step of step_on_views(cameras=T, intrinsics=I) from its parts, in its order."""
    k, poses = I.values(), T.poses()
    with torch.no_grad():
        rays, tgt, used = N.select_training_rays_views(H, W, focal, poses, imgs, n, opts, seed=eng.seed, step=eng.step_count, first=0,
                                                       intrinsics=k)
    rg = torch.empty_like(rays)
    eng.forward_backward(rays, tgt, 0, None, None, rg)
    N.select_training_rays_views_bwd(H, W, focal, poses, used, rg, opts, eng.ray_grad_coarse, out=T.g_poses, intrinsics=k,
                                     out_intrinsics=I.g_intr)
    T.backward()
    I.backward()
    eng.optimizer_step()
    T.step()
    I.step()
    return eng.loss


def test_step_on_views_with_intrinsics_equals_its_parts():
    """Five steps of step_on_views(cameras=T, intrinsics=I) against the same calls made by hand: loss, nets, twists and q on the bits."""
    import nerf_pytorch_amd as N
    dev = ES.dev()
    V, n = 3, 256
    opts = N.make_options(32, 32)
    res = {}
    for arm in ("engine", "parts"):
        mc, mf, H, W, focal, pose0 = ES.lego(dev)
        eng = N.TrainEngine(mc, mf, 32, 32, perturb=True, white_background=True, noise_std=0.2, seed=3, lr=5e-4, world_size=1, rank=0)
        imgs = torch.rand(V, H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
        T = N.CameraTable(ES.views(pose0, dev, V), lr=2e-3)
        I = N.Intrinsics(H, W, focal * 1.02, learn="all", lr=1e-3, device=dev)
        seen = []
        for _ in range(5):
            if arm == "engine":
                loss = eng.step_on_views(imgs, None, H, W, focal, opts, n, cameras=T, intrinsics=I)
            else:
                loss = _by_hand(eng, N, T, I, imgs, H, W, focal, opts, n)
            seen.append([t.clone() for t in (loss, mc.flat_params, mf.flat_params, T.xi, I.q, I.exp_avg, I.exp_avg_sq, I.g_intr)])
        torch.cuda.synchronize()
        res[arm] = seen
        assert eng.step_count == T.step_count == I.step_count == 5
        assert torch.all(torch.isfinite(I.q)) and torch.all(I.q != 0) and float(T.xi.abs().sum()) > 0
    for step, (a, b) in enumerate(zip(res["engine"], res["parts"])):
        for name, x, y in zip(("loss", "coarse", "fine", "xi", "q", "exp_avg", "exp_avg_sq", "g_intr"), a, b):
            assert torch.equal(x, y), (step, name)


def test_intrinsics_that_learn_nothing_leave_the_step_what_it_was():
    """learn=() at the scalar camera's values: after five steps nets, twists and loss are those of step_on_views(cameras=T) without
    intrinsics, on the bits (the same rays, the same pose gradients)."""
    import nerf_pytorch_amd as N
    dev = ES.dev()
    V, n = 3, 256
    opts = N.make_options(32, 32)
    res = {}
    for arm in ("with", "without"):
        mc, mf, H, W, focal, pose0 = ES.lego(dev)
        eng = N.TrainEngine(mc, mf, 32, 32, perturb=True, white_background=True, noise_std=0.2, seed=3, lr=5e-4, world_size=1, rank=0)
        imgs = torch.rand(V, H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
        T = N.CameraTable(ES.views(pose0, dev, V), lr=2e-3)
        I = N.Intrinsics(H, W, focal, learn=(), device=dev) if arm == "with" else None
        for _ in range(5):
            loss = eng.step_on_views(imgs, None, H, W, focal, opts, n, cameras=T, intrinsics=I)
        torch.cuda.synchronize()
        res[arm] = [t.clone() for t in (loss, mc.flat_params, mf.flat_params, T.xi)]
        if I is not None:
            assert I.step_count == 5 and torch.all(I.q == 0) and torch.all(I.g_q == 0) and float(I.g_intr.abs().sum()) > 0
    for name, x, y in zip(("loss", "coarse", "fine", "xi"), res["with"], res["without"]):
        assert torch.equal(x, y), name


def test_localize_with_intrinsics_leaves_the_nets_alone_and_refusals():
    import nerf_pytorch_amd as N
    dev = ES.dev()
    mc, mf, H, W, focal, pose0 = ES.small(dev)
    V, n = 3, 256
    opts = N.make_options(8, 8)
    imgs = torch.rand(V, H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    base = ES.views(pose0, dev, V)
    eng = N.TrainEngine(mc, mf, 8, 8, perturb=True, white_background=True, noise_std=0.2, seed=3, lr=5e-4, world_size=1, rank=0)
    eng.grad.normal_(), eng.exp_avg.normal_(), eng.exp_avg_sq.uniform_()
    before = ES.state(eng)
    I = N.Intrinsics(H, W, focal * 1.05, learn="focal", lr=1e-3, device=dev)
    for _ in range(3):
        eng.localize_on_views(imgs, base, H, W, focal, opts, n, intrinsics=I)     # the intrinsics alone
    pg = torch.full((3, 4), float("nan"), device=dev)
    eng.localize_on_image(imgs[0], base[0], H, W, focal, opts, n, pose_grad=pg, intrinsics=I)
    torch.cuda.synchronize()
    for name, a, b in zip(("coarse", "fine", "exp_avg", "exp_avg_sq", "grad", "packed_c", "packed_f"), before, ES.state(eng)):
        assert torch.equal(a, b), name
    assert eng.step_count == 0 and eng.localize_count == 4 and I.step_count == 4
    assert float(I.q[0]) != 0 and torch.all(I.q[1:] == 0) and torch.all(torch.isfinite(pg)) and float(pg.abs().sum()) > 0
    with pytest.raises(RuntimeError, match="Intrinsics"):
        eng.step_on_views(imgs, base, H, W, focal, opts, n, intrinsics=I.values())
    eng2 = N.TrainEngine(mc, mf, 8, 8, world_size=2, rank=0)
    with pytest.raises(NotImplementedError, match="world size 2"):
        eng2.step_on_views(imgs, base, H, W, focal, opts, n, intrinsics=I)
    with pytest.raises(RuntimeError, match="needs"):
        eng.localize_on_views(imgs, base, H, W, focal, opts, n)


# ---- the capability: a focal length 5 % off, recovered against frozen nets ----------------------------------------------------------------
STEPS, LR, RAYS = 300, 3e-3, 1024


def test_a_focal_five_per_cent_off_is_recovered_on_frozen_nets():
    """Frozen lego-lowres nets; two views at their exact poses with targets rendered at the true focal (64 + 64 samples, no perturb,
    white background); the focal starts at 1.05 x the true one.  Engine arm: STEPS localize_on_views(intrinsics=I) steps of RAYS rays,
    learn="focal".  Reference arm: the same run (the same select indices and targets every step) with the rays made by a torch
    restatement of pin-hole + packing from a torch log-focal leaf, the nets under set_frozen(True), torch.optim.Adam at the same lr.
    The bar: the engine arm's final |f / f_true - 1| is at most 3 x the reference arm's (the margin tests/test_gpu_views.py and
    tests/test_gpu_cameras.py give two chaotic 300-step runs); the reference arm alone must end below one fifth of its start.
    Measured (MI355X, STEPS = 300, LR = 3e-3): see profiles/r13_intrinsics.json, "capability"."""
    import nerf_pytorch_amd as N
    dev = ES.dev()
    mc, mf, H, W, f_true, pose0 = ES.lego(dev)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)
    ex, ed = ES.ex_ed()
    opts = N.make_options(64, 64, perturb=False, white_background=True, radiance_field_noise_std=0.0)
    gt0 = torch.from_numpy(pose0).to(dev)
    turn = torch.eye(4, device=dev)
    turn[:3, :3] = P.rodrigues(torch.tensor([0.0, 0.0, np.deg2rad(20.0)], dtype=torch.float64)).float().to(dev)
    gts = torch.stack([gt0, turn @ gt0]).contiguous()
    with torch.no_grad():
        targets = []
        for v in range(2):
            ro, rd = N.get_ray_bundle(H, W, f_true, gts[v])
            targets.append(N.run_one_iter_of_nerf(H, W, f_true, mc, mf, ro, rd, opts, mode="validation", encode_position_fn=ex,
                                                  encode_direction_fn=ed)[3])
        targets = torch.stack(targets).contiguous()
    f0 = float(np.float32(1.05 * f_true))
    err = lambda f: abs(float(f) / f_true - 1.0)  # noqa: E731
    marks = lambda it: it % 50 == 0 or it == STEPS - 1  # noqa: E731

    # engine arm
    eng = N.TrainEngine(mc, mf, 64, 64, perturb=False, white_background=True, noise_std=0.0, lr=0.0, world_size=1, rank=0)
    I = N.Intrinsics(H, W, f0, learn="focal", lr=LR, device=dev)
    curve_e = [(-1, err(f0))]
    for it in range(STEPS):
        eng.localize_on_views(targets, gts, H, W, f0, opts, RAYS, intrinsics=I)
        if marks(it):
            curve_e.append((it, err(I.values()[0])))
    v = I.values()
    assert float(v[0]) == float(v[1]) and float(v[2]) == float(np.float32(W * 0.5)) and float(v[3]) == float(np.float32(H * 0.5))

    # reference arm: torch arithmetic from a log-focal leaf
    q = torch.zeros((), device=dev, requires_grad=True)
    opt = torch.optim.Adam([q], lr=LR)
    mc.set_frozen(True), mf.set_frozen(True)
    curve_r = [(-1, err(f0))]
    hw, near, far = H * W, float(opts.dataset.near), float(opts.dataset.far)
    try:
        for it in range(STEPS):
            with torch.no_grad():
                _, tgt, used = N.select_training_rays_views(H, W, f0, gts, targets, RAYS, opts, seed=eng.seed, step=it, first=0)
            opt.zero_grad()
            f = f0 * torch.exp(q)
            vid, k = used // hw, used % hw
            row, col = (k % H).float(), (k // H).float()
            dc = torch.stack([(col - W * 0.5) / f, -(row - H * 0.5) / f, -torch.ones_like(col)], -1)
            d = (gts[vid][:, :3, :3] * dc[:, None, :]).sum(-1)
            o = gts[vid][:, :3, 3]
            rays = torch.cat([o, d, torch.full_like(d[:, :1], near), torch.full_like(d[:, :1], far), d / d.norm(dim=-1, keepdim=True)], -1)
            out = N.predict_and_render_radiance(rays, mc, mf, opts, encode_position_fn=ex, encode_direction_fn=ed)
            loss = torch.nn.functional.mse_loss(out[0], tgt) + torch.nn.functional.mse_loss(out[3], tgt)
            loss.backward()
            opt.step()
            if marks(it):
                curve_r.append((it, err(f0 * float(torch.exp(q.detach())))))
    finally:
        mc.set_frozen(False), mf.set_frozen(False)
    print("focal recovery, engine arm (step, |f / f_true - 1|): %s" % curve_e)
    print("focal recovery, reference arm: %s" % curve_r)
    print("INTRINSICS_CAPABILITY " + json.dumps(dict(steps=STEPS, lr=LR, rays=RAYS, start=1.05, engine=curve_e, reference=curve_r)))
    assert curve_r[-1][1] < curve_r[0][1] / 5, curve_r        # the reference arm alone
    assert curve_e[-1][1] <= 3 * curve_r[-1][1], (curve_e, curve_r)
