"""GPU suite (-m gpu): pose refinement -- d(loss)/d(pose) through the drop-in API (get_ray_bundle, get_rays_at_pixels,
select_training_rays under autograd) and through TrainEngine.step_on_image(pose_grad=...), against fp64 oracle autograd
under the bound of tests/pose_vjp.py, and a pose recovered from a perturbed start on the lego-lowres fixture nets."""
import numpy as np
import pytest
import torch

import engine_scenes as ES
import pose_vjp as P

pytestmark = pytest.mark.gpu

CFG = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)


def _close(got, want, mag, n, what):
    b = P.bound(n, mag)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    assert np.all(err <= b), (what, float((err / np.maximum(b, 1e-300)).max()))


def test_dropin_pose_gradient_exists_matches_oracle_and_keeps_the_forward():
    import nerf_pytorch_amd as N
    dev = ES.dev()
    H, W, focal = 21, 34, float(np.float32(30.5))
    g = torch.Generator().manual_seed(0)
    base = torch.eye(4)
    base[:3, :3] = P.rodrigues(torch.tensor([0.1, -0.2, 0.05], dtype=torch.float64)).float()
    base[:3, 3] = torch.tensor([0.3, -0.1, 3.0])
    for shape in ("4x4", "3x4", "view"):
        if shape == "view":
            stack = torch.stack([base, base]).to(dev).requires_grad_(True)
            pose, leaf = stack[1, :3, :4], stack
        else:
            leaf = (base if shape == "4x4" else base[:3, :4].contiguous()).to(dev).requires_grad_(True)
            pose = leaf
        ro, rd = N.get_ray_bundle(H, W, focal, pose)
        assert ro.grad_fn is not None and rd.grad_fn is not None
        with torch.no_grad():
            ro0, rd0 = N.get_ray_bundle(H, W, focal, pose)
        assert torch.equal(ro, ro0) and torch.equal(rd, rd0)
        go, gd = torch.randn(H, W, 3, generator=g), torch.randn(H, W, 3, generator=g)
        ((ro * go.to(dev)).sum() + (rd * gd.to(dev)).sum()).backward()
        gp = leaf.grad if shape != "view" else leaf.grad[1]
        assert tuple(leaf.grad.shape) == tuple(leaf.shape) and leaf.grad.dtype == leaf.dtype
        if shape == "4x4":
            assert torch.all(leaf.grad[3] == 0)
        if shape == "view":
            assert torch.all(leaf.grad[0] == 0)
        want = P.oracle_bundle_vjp(H, W, focal, base.numpy(), None, go.reshape(-1, 3).numpy(), gd.reshape(-1, 3).numpy())
        mag = P.magnitude(H, W, focal, base.numpy(), None, False, g_o=go.reshape(-1, 3).numpy(), g_d=gd.reshape(-1, 3).numpy())
        _close(gp[:3, :4].cpu().numpy(), want, mag, H * W, "get_ray_bundle " + shape)

    # get_rays_at_pixels: only the direction used (the origin's cotangent never arrives)
    pix = torch.randperm(H * W, generator=g)[:257]
    leaf = base.clone().to(dev).requires_grad_(True)
    ro, rd = N.get_rays_at_pixels(H, W, focal, leaf, pix.to(dev))
    assert rd.grad_fn is not None
    gd = torch.randn(257, 3, generator=g)
    (rd * gd.to(dev)).sum().backward()
    want = P.oracle_bundle_vjp(H, W, focal, base.numpy(), pix.numpy(), None, gd.numpy())
    _close(leaf.grad[:3, :4].cpu().numpy(), want, P.magnitude(H, W, focal, base.numpy(), pix.numpy(), False, g_d=gd.numpy()), 257,
           "get_rays_at_pixels")

    # select_training_rays, blender and NDC options, with and without viewdirs
    img = torch.rand(H, W, 4, generator=g).to(dev)
    for no_ndc, view in ((True, True), (False, True), (False, False)):
        opts = N.make_options(8, 8, no_ndc=no_ndc, use_viewdirs=view)
        pose_np = base.numpy().copy()
        if not no_ndc:
            pose_np[:3, 3] = [0.1, -0.05, 0.2]
        leaf = torch.from_numpy(pose_np).to(dev).requires_grad_(True)
        rays, tgt, used = N.select_training_rays(H, W, focal, leaf, img, 300, opts, seed=5, step=2)
        assert rays.grad_fn is not None and not tgt.requires_grad
        with torch.no_grad():
            rays0, tgt0, used0 = N.select_training_rays(H, W, focal, leaf, img, 300, opts, seed=5, step=2)
        assert torch.equal(rays, rays0) and torch.equal(tgt, tgt0) and torch.equal(used, used0)
        gr = torch.randn(rays.shape, generator=g)
        (rays * gr.to(dev)).sum().backward()
        gr64 = gr.double().numpy()
        want = P.oracle_select_vjp(H, W, focal, pose_np, used.cpu().numpy(), gr64, not no_ndc, view)
        mag = P.magnitude(H, W, focal, pose_np, used.cpu().numpy(), True, g_rays=np.abs(gr64), ndc=not no_ndc, view=view)
        _close(leaf.grad[:3, :4].cpu().numpy(), want, mag, 300, "select_training_rays ndc=%s view=%s" % (not no_ndc, view))
        assert torch.all(leaf.grad[3] == 0)


@pytest.mark.parametrize("no_ndc", [True, False])
def test_reference_loop_backpropagates_to_the_pose(no_ndc):
    """get_ray_bundle -> index with select_inds -> run_one_iter_of_nerf -> loss.backward() (train_nerf.py:210-259) with
    pose = pose0 @ exp(xi): xi.grad is filled, and pose.grad is fp64 oracle autograd of get_ray_bundle applied to the ray
    cotangents captured with retain_grad() (isolating the new layer from the sampler's conditioning)."""
    import nerf_pytorch_amd as N
    dev = ES.dev()
    mc, mf, H, W, focal, pose0 = ES.lego(dev)
    near_far = dict(near=2.0, far=6.0)
    if not no_ndc:  # (LLFF options; NDC space misses the lego scene, so untrained nets give the render something to differentiate)
        torch.manual_seed(5)
        mc, mf = N.FlexibleNeRFModel(**CFG).to(dev), N.FlexibleNeRFModel(**CFG).to(dev)
        near_far = dict(near=0.0, far=1.0)
    ex, ed = ES.ex_ed()
    opts = N.make_options(64, 64, perturb=True, white_background=True, radiance_field_noise_std=0.0, no_ndc=no_ndc, **near_far)
    torch.manual_seed(3)
    xi = (torch.randn(6) * 0.01).to(dev).requires_grad_(True)
    pose = torch.from_numpy(pose0).to(dev) @ ES.se3(xi)
    pose.retain_grad()
    ro, rd = N.get_ray_bundle(H, W, focal, pose[:3, :4])
    ro.retain_grad(), rd.retain_grad()
    sel = torch.randperm(H * W)[:512].to(dev)
    ro_s, rd_s = ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]
    target = torch.rand(512, 3, device=dev)
    out = N.run_one_iter_of_nerf(H, W, focal, mc, mf, ro_s, rd_s, opts, encode_position_fn=ex, encode_direction_fn=ed)
    loss = torch.nn.functional.mse_loss(out[0], target) + torch.nn.functional.mse_loss(out[3], target)
    loss.backward()
    assert xi.grad is not None and torch.all(torch.isfinite(xi.grad)) and float(xi.grad.abs().sum()) > 0
    go, gd = ro.grad.reshape(-1, 3).cpu().numpy(), rd.grad.reshape(-1, 3).cpu().numpy()
    p64 = pose.detach().cpu().numpy()
    want = P.oracle_bundle_vjp(H, W, focal, p64, None, go, gd)
    _close(pose.grad[:3, :4].cpu().numpy(), want, P.magnitude(H, W, focal, p64, None, False, g_o=go, g_d=gd), H * W,
           "reference loop no_ndc=%s" % no_ndc)


@pytest.mark.parametrize("precision", ["fp32", "f16x3_train"])
@pytest.mark.parametrize("backward", [None, "auto"])
def test_engine_pose_gradient_equals_dropin(precision, backward):
    """The same rays and draws through TrainEngine.forward_backward(ray_grad=...) + select_training_rays_bwd and through the
    drop-in chain (select_training_rays -> predict_and_render_radiance -> backward).  Both run the same kernels on the same
    draws; they differ in the backward's buffer layout and, with "auto", in the compacted list (the same sum with its zero terms
    dropped), so the two pose gradients agree to 1e-4 of their norm (fp32 rounding of a sum of ~10^5 terms, with margin)."""
    import nerf_pytorch_amd as N
    from nerf_pytorch_amd.train_utils import select_training_rays_bwd
    dev = ES.dev()
    mc, mf, H, W, focal, pose0 = ES.lego(dev)
    if precision != "fp32":
        mc.set_training_precision(precision), mf.set_training_precision(precision)
    if backward == "auto":
        mc.set_backward_compaction("auto"), mf.set_backward_compaction("auto")
    ex, ed = ES.ex_ed()
    opts = N.make_options(64, 64, perturb=True, white_background=True, radiance_field_noise_std=0.0)
    n = 1024
    g = torch.Generator().manual_seed(4)
    img = torch.rand(H, W, 3, generator=g).to(dev)
    draws = (torch.rand(n, 64, generator=g).to(dev), None, torch.rand(n, 64, generator=g).to(dev), None)
    leaf = torch.from_numpy(pose0).to(dev).requires_grad_(True)
    rays, tgt, used = N.select_training_rays(H, W, focal, leaf, img, n, opts, seed=9, step=0)
    real = ES.queue_draws([draws[0], draws[2]])
    try:
        out = N.predict_and_render_radiance(rays, mc, mf, opts, encode_position_fn=ex, encode_direction_fn=ed)
    finally:
        torch.rand, torch.randn = real
    loss = torch.nn.functional.mse_loss(out[0], tgt) + torch.nn.functional.mse_loss(out[3], tgt)
    loss.backward()
    want = leaf.grad[:3, :4].clone()
    eng = N.TrainEngine(mc, mf, 64, 64, perturb=True, white_background=True, noise_std=0.0, lr=0.0, world_size=1, rank=0,
                        backward=backward)
    rg = torch.empty_like(rays)
    eng.forward_backward(rays.detach(), tgt, draws=draws, ray_grad=rg)
    got = select_training_rays_bwd(H, W, focal, leaf, used, rg, opts, eng.ray_grad_coarse)
    torch.cuda.synchronize()
    rel = float((got - want).norm() / want.norm())
    assert rel < 1e-4, rel
    assert torch.allclose(eng.loss[2], loss.detach(), rtol=1e-4)


def test_engine_pose_gradient_two_stream_equals_one_stream():
    """Extends test_two_stream_step_equals_single_stream_step's invariant to pose_grad: the coarse part of the ray gradient lands
    in its own buffer on the side stream and the pose kernel adds the two parts row by row -- the same bits in both orders."""
    import nerf_pytorch_amd as N
    dev = ES.dev()
    outs = []
    for overlap in (True, False):
        mc, mf, H, W, focal, pose0 = ES.lego(dev)
        eng = N.TrainEngine(mc, mf, 32, 32, perturb=True, white_background=True, noise_std=0.2, seed=3, world_size=1, rank=0,
                            overlap=overlap)
        img = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
        pose = torch.from_numpy(pose0).to(dev)
        grads = []
        for _ in range(3):
            pg = torch.empty(3, 4, device=dev)
            eng.step_on_image(img, pose, H, W, focal, N.make_options(32, 32), 640, pose_grad=pg)
            grads.append(pg)
        torch.cuda.synchronize()
        outs.append((torch.stack(grads), mc.flat_params.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.all(torch.isfinite(outs[0][0])) and float(outs[0][0].abs().sum()) > 0


def test_engine_pose_gradient_refuses_data_parallel_steps():
    import nerf_pytorch_amd as N
    dev = ES.dev()
    mc, mf, H, W, focal, pose0 = ES.lego(dev)
    eng = N.TrainEngine(mc, mf, 32, 32, world_size=2, rank=0)
    img = torch.rand(H, W, 3, device=dev)
    with pytest.raises(NotImplementedError, match="world size 2"):
        eng.step_on_image(img, torch.from_numpy(pose0).to(dev), H, W, focal, N.make_options(32, 32), 256,
                          pose_grad=torch.empty(3, 4, device=dev))
    rays = torch.zeros(256, 11, device=dev)
    with pytest.raises(NotImplementedError):
        eng.forward_backward(rays, torch.zeros(256, 3, device=dev), ray_grad=torch.empty_like(rays))


# ---- the capability: a perturbed pose recovered on frozen nets -------------------------------------------------------------
STEPS, LR, RAYS = 300, 3e-3, 1024


def _recover(dev, through_engine):
    import nerf_pytorch_amd as N
    mc, mf, H, W, focal, pose0 = ES.lego(dev)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)
    ex, ed = ES.ex_ed()
    opts_val = N.make_options(64, 64, perturb=False, white_background=True, radiance_field_noise_std=0.0)
    gt = torch.from_numpy(pose0).to(dev)
    with torch.no_grad():
        ro, rd = N.get_ray_bundle(H, W, focal, gt)
        target = N.run_one_iter_of_nerf(H, W, focal, mc, mf, ro, rd, opts_val, mode="validation", encode_position_fn=ex,
                                        encode_direction_fn=ed)[3].contiguous()
    # the start: ~2 degrees about a fixed axis and 0.05 units
    axis = torch.tensor([0.3, -0.8, 0.5], dtype=torch.float32)
    delta = torch.cat([axis / axis.norm() * np.deg2rad(2.0), torch.tensor([0.03, -0.03, 0.0277])]).to(dev)
    start = (gt @ ES.se3(delta)).detach()
    xi = torch.zeros(6, device=dev, requires_grad=True)
    opt = torch.optim.Adam([xi], lr=LR)
    eng = N.TrainEngine(mc, mf, 64, 64, perturb=False, white_background=True, noise_std=0.0, lr=0.0, world_size=1,
                        rank=0) if through_engine else None
    pg = torch.empty(3, 4, device=dev)

    def errors():
        est = (start @ ES.se3(xi)).detach().cpu().numpy().astype(np.float64)
        g = pose0.astype(np.float64)
        return P.rot_angle_deg(est[:3, :3].T @ g[:3, :3]), float(np.linalg.norm(est[:3, 3] - g[:3, 3]))

    curve = [(-1,) + errors()]

    for it in range(STEPS):
        opt.zero_grad()
        pose = start @ ES.se3(xi)
        if through_engine:
            eng.step_on_image(target, pose.detach(), H, W, focal, opts_val, RAYS, lr=0.0, pose_grad=pg)
            torch.autograd.backward(pose[:3, :4], pg)
        else:
            rays, tgt, _ = N.select_training_rays(H, W, focal, pose, target, RAYS, opts_val, seed=1, step=it)
            out = N.predict_and_render_radiance(rays, mc, mf, opts_val, encode_position_fn=ex, encode_direction_fn=ed)
            loss = torch.nn.functional.mse_loss(out[0], tgt) + torch.nn.functional.mse_loss(out[3], tgt)
            loss.backward()
        opt.step()
        if it % 50 == 0 or it == STEPS - 1:
            curve.append((it,) + errors())
    return curve


@pytest.mark.parametrize("through_engine", [False, True])
def test_perturbed_pose_is_recovered_on_frozen_nets(through_engine):
    """Frozen lego-lowres nets, target rendered at the fixture pose; start 2 degrees and 0.05 units off; Adam on a 6-vector
    (rotation, translation) for STEPS steps of RAYS rays, through the drop-in loop and through TrainEngine.step_on_image(pose_grad=...)
    with lr=0 for the nets.  Rotation and translation errors each fall at least 4x below their starting values.
    Measured on MI355X (profiles/r07_pose_grad.json): 2.00 deg / 0.0507 -> 0.079 deg / 0.0058 (drop-in) and 0.068 deg / 0.0027
    (engine) after 300 steps, i.e. 25-29x in rotation and 8.7-19x in translation: the 4x asserted leaves a factor >= 2 of margin."""
    dev = ES.dev()
    curve = _recover(dev, through_engine)
    print("pose recovery (%s): %s" % ("engine" if through_engine else "drop-in", curve))
    (_, r0, t0), (_, r1, t1) = curve[0], curve[-1]
    assert r1 * 4 <= r0 and t1 * 4 <= t0, curve
