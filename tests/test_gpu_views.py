"""GPU suite (-m gpu): one ray batch over a stack of views -- the kernels of tests/views_cases.py on the product library, the
drop-in autograd node (select_training_rays_views), TrainEngine.step_on_views, and two cameras refined jointly from one batch."""
import json

import numpy as np
import pytest
import torch

import engine_scenes as ES
import pose_vjp as P
import views_cases as VC

pytestmark = pytest.mark.gpu


# ---- the kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("channels", [3, 4, None])
def test_selection_rows_equal_the_single_view_rows(gpu, ndc, view, channels):
    VC.case_selection(gpu, ndc, view, channels, "4x4")


def test_selection_reads_a_strided_pose_table(gpu):
    VC.case_selection(gpu, True, True, 3, "embedded")


@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("channels", [3, 4, None])
def test_selection_of_one_view_is_select_rays(gpu, ndc, view, channels):
    VC.case_single_view_is_select_rays(gpu, ndc, view, channels)


def test_single_view_entry_points_read_a_row_stride_other_than_4(gpu):
    VC.case_single_view_row_stride(gpu)


@pytest.mark.parametrize("view", [False, True])
def test_cached_selection_rows_equal_the_select_rays_rows(gpu, view):
    VC.case_cached_rows_are_select_rays_rows(gpu, view)


def test_selection_honours_explicit_indices_and_rank_slices_are_disjoint(gpu):
    VC.case_explicit_indices_and_rank_slices(gpu)


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("two", [False, True])
def test_views_vjp_equals_the_single_view_vjp_per_view(gpu, which, ndc, view, two):
    VC.case_vjp(gpu, which, ndc, view, two)


@pytest.mark.parametrize("n", [1, 257, 256 * 64 + 1])
def test_single_view_vjp_sum_at_its_edges(gpu, n):
    VC.case_single_view_vjp_sum_edges(gpu, n)


def test_views_vjp_of_no_rays_is_zero(gpu):
    VC.case_vjp_no_rays(gpu)


def test_views_entry_points_reject_bad_arguments(gpu):
    VC.case_refusals(gpu)


# ---- drop-in autograd ---------------------------------------------------------------------------------------------------------------
def test_dropin_views_pose_gradients_equal_the_single_view_path():
    """select_training_rays_views -> predict_and_render_radiance -> MSE -> backward(): poses.grad[v] is, bit for bit, the gradient
    the same rays of view v give through select_training_rays(select_inds=...) with the same draws.  (The render is per ray, and
    the loss is written as sum / (3 n) with the full batch's n in both routes, so each ray's cotangent is the same.)"""
    import nerf_pytorch_amd as N
    dev = ES.dev()
    mc, mf, H, W, focal, pose0 = ES.lego(dev)
    ex, ed = ES.ex_ed()
    opts = N.make_options(64, 64, perturb=True, white_background=True, radiance_field_noise_std=0.0)
    V, n = 3, 768
    g = torch.Generator().manual_seed(6)
    imgs = torch.rand(V, H, W, 3, generator=g).to(dev)
    t_rand, u = torch.rand(n, 64, generator=g).to(dev), torch.rand(n, 64, generator=g).to(dev)
    poses = ES.views(pose0, dev, V).requires_grad_(True)

    def loss_of(rays, tgt, tr, uu):
        real = ES.queue_draws([tr, uu])
        try:
            out = N.predict_and_render_radiance(rays, mc, mf, opts, encode_position_fn=ex, encode_direction_fn=ed)
        finally:
            torch.rand, torch.randn = real
        return (((out[0] - tgt) ** 2).sum() + ((out[3] - tgt) ** 2).sum()) * (1.0 / (3 * n))

    rays, tgt, used = N.select_training_rays_views(H, W, focal, poses, imgs, n, opts, seed=4, step=1)
    assert rays.grad_fn is not None and not tgt.requires_grad and not used.requires_grad
    with torch.no_grad():
        r0, t0, u0 = N.select_training_rays_views(H, W, focal, poses, imgs, n, opts, seed=4, step=1)
    r1, t1, u1 = N.select_training_rays_views(H, W, focal, poses.detach(), imgs, n, opts, seed=4, step=1)
    assert r1.grad_fn is None and not r1.requires_grad
    for rr, tt, uu in ((r0, t0, u0), (r1, t1, u1)):
        assert torch.equal(rays, rr) and torch.equal(tgt, tt) and torch.equal(used, uu)
    loss_of(rays, tgt, t_rand, u).backward()
    assert tuple(poses.grad.shape) == (V, 4, 4) and torch.all(poses.grad[:, 3] == 0)
    view = used // (H * W)
    for v in range(V):
        rows = torch.nonzero(view == v).flatten()
        assert rows.numel() > 0
        leaf = poses[v].detach().clone().requires_grad_(True)
        rv, tv, _ = N.select_training_rays(H, W, focal, leaf, imgs[v], rows.numel(), opts, select_inds=used[rows] - v * H * W)
        assert torch.equal(rv, rays[rows]) and torch.equal(tv, tgt[rows])
        loss_of(rv, tv, t_rand[rows].contiguous(), u[rows].contiguous()).backward()
        assert float(leaf.grad[:3, :4].abs().sum()) > 0
        assert torch.equal(poses.grad[v, :3, :4], leaf.grad[:3, :4]), (v, poses.grad[v, :3, :4], leaf.grad[:3, :4])
    # a (V, 3, 4) table: the gradient has its shape
    p34 = poses.detach()[:, :3, :4].contiguous().requires_grad_(True)
    r34, _, _ = N.select_training_rays_views(H, W, focal, p34, imgs, n, opts, seed=4, step=1)
    assert torch.equal(r34, rays)
    gr = torch.randn(rays.shape, generator=g).to(dev)
    (r34 * gr).sum().backward()
    assert tuple(p34.grad.shape) == (V, 3, 4) and torch.all(torch.isfinite(p34.grad))


# ---- the engine -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x3_train"])
@pytest.mark.parametrize("backward", [None, "auto"])
def test_step_on_views_of_one_view_equals_step_on_image(precision, backward):
    import nerf_pytorch_amd as N
    dev = ES.dev()
    outs = []
    for views in (False, True):
        mc, mf, H, W, focal, pose0 = ES.lego(dev, precision)
        eng = N.TrainEngine(mc, mf, 32, 32, perturb=True, white_background=True, noise_std=0.2, seed=3, world_size=1, rank=0,
                            backward=backward)
        img = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
        pose = torch.from_numpy(pose0).to(dev)
        opts = N.make_options(32, 32)
        grads, losses = [], []
        for _ in range(2):
            if views:
                pg = torch.full((1, 3, 4), float("nan"), device=dev)
                loss = eng.step_on_views(img[None], pose[None], H, W, focal, opts, 640, pose_grads=pg)
                pg = pg[0]
            else:
                pg = torch.full((3, 4), float("nan"), device=dev)
                loss = eng.step_on_image(img, pose, H, W, focal, opts, 640, pose_grad=pg)
            grads.append(pg), losses.append(loss.clone())
        torch.cuda.synchronize()
        outs.append((torch.stack(losses), mc.flat_params.clone(), mf.flat_params.clone(), torch.stack(grads)))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.all(torch.isfinite(outs[0][3])) and float(outs[0][3].abs().sum()) > 0


def test_step_on_views_equals_its_parts_and_two_streams_equal_one():
    """step_on_views(V = 3, pose_grads) against select_training_rays_views -> step(ray_grad=...) -> select_training_rays_views_bwd
    on ray_grad and ray_grad_coarse; and the two-stream step against the one-stream step."""
    import nerf_pytorch_amd as N
    dev = ES.dev()
    V, n = 3, 640
    opts = N.make_options(32, 32)
    res = {}
    for arm in ("views", "parts", "views_one_stream"):
        mc, mf, H, W, focal, pose0 = ES.lego(dev)
        eng = N.TrainEngine(mc, mf, 32, 32, perturb=True, white_background=True, noise_std=0.2, seed=3, world_size=1, rank=0,
                            overlap=(arm != "views_one_stream"))
        imgs = torch.rand(V, H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
        poses = ES.views(pose0, dev, V)
        grads, losses = [], []
        for it in range(2):
            pg = torch.full((V, 3, 4), float("nan"), device=dev)
            if arm == "parts":
                rays, tgt, used = N.select_training_rays_views(H, W, focal, poses, imgs, n, opts, seed=eng.seed, step=eng.step_count,
                                                               first=0)
                rg = torch.empty_like(rays)
                loss = eng.step(rays, tgt, ray_offset=0, ray_grad=rg)
                N.select_training_rays_views_bwd(H, W, focal, poses, used, rg, opts, eng.ray_grad_coarse, out=pg)
            else:
                loss = eng.step_on_views(imgs, poses, H, W, focal, opts, n, pose_grads=pg)
            grads.append(pg), losses.append(loss.clone())
        torch.cuda.synchronize()
        res[arm] = (torch.stack(losses), mc.flat_params.clone(), mf.flat_params.clone(), torch.stack(grads))
    for other in ("parts", "views_one_stream"):
        for a, b in zip(res["views"], res[other]):
            assert torch.equal(a, b), other
    g = res["views"][3]
    assert torch.all(torch.isfinite(g)) and all(float(g[:, v].abs().sum()) > 0 for v in range(V))


def test_step_on_views_data_parallel_slices_and_refusal():
    import nerf_pytorch_amd as N
    dev = ES.dev()
    V, n = 3, 256
    mc, mf, H, W, focal, pose0 = ES.lego(dev)
    poses = ES.views(pose0, dev, V)
    # every pixel of every view carries its own (view, row, col)
    vv, rr, cc = torch.meshgrid(torch.arange(V), torch.arange(H), torch.arange(W), indexing="ij")
    imgs = torch.stack([vv, rr, cc], -1).float().to(dev)
    opts = N.make_options(32, 32)
    seen = []
    for rank in range(2):
        eng = N.TrainEngine(mc, mf, 32, 32, world_size=2, rank=rank)
        with pytest.raises(NotImplementedError, match="world size 2"):
            eng.step_on_views(imgs, poses, H, W, focal, opts, n, pose_grads=torch.empty(V, 3, 4, device=dev))
        got = {}
        eng.step = lambda rays, target, **kw: got.update(rays=rays, target=target, **kw)  # (no process group here: the step itself is not run)
        eng.step_on_views(imgs, poses, H, W, focal, opts, n)
        assert got["ray_offset"] == rank * n and tuple(got["rays"].shape) == (n, 11)
        seen.append({tuple(int(x) for x in row) for row in got["target"].cpu().tolist()})
        assert len(seen[-1]) == n
    assert not (seen[0] & seen[1])
    assert {t[0] for t in seen[0] | seen[1]} == set(range(V))


# ---- the capability: two cameras refined from one batch -----------------------------------------------------------------------------------
STEPS, LR = 300, 3e-3


def test_two_perturbed_poses_are_recovered_jointly_on_frozen_nets():
    """Frozen lego-lowres nets; two ground-truth poses with their rendered targets (64 + 64 samples, no perturb, white background);
    each pose starts 2 degrees / 0.05 units off.  Joint arm: STEPS Adam steps on two 6-vectors, 1024 rays per step across both views,
    through step_on_views(pose_grads=...) with lr = 0 for the nets.  Comparison arm (what step_on_image(pose_grad=...) could already
    do): each pose alone at 512 rays per step.  Each of the four joint final errors (rotation, translation; per view) is at most 3x
    the single-view one: the arms see different ray draws, and two equivalent single-view routes already differ by up to 2.2x in final
    translation error (profiles/r07_pose_grad.json: 0.0058 against 0.0027)."""
    import nerf_pytorch_amd as N
    dev = ES.dev()
    mc, mf, H, W, focal, pose0 = ES.lego(dev)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)
    ex, ed = ES.ex_ed()
    opts = N.make_options(64, 64, perturb=False, white_background=True, radiance_field_noise_std=0.0)
    gt0 = torch.from_numpy(pose0).to(dev)
    # the second view: the first one turned by 20 degrees about the world's z axis (the lego turntable)
    turn = torch.eye(4, device=dev)
    turn[:3, :3] = P.rodrigues(torch.tensor([0.0, 0.0, np.deg2rad(20.0)], dtype=torch.float64)).float().to(dev)
    gts = torch.stack([gt0, turn @ gt0])
    with torch.no_grad():
        targets = []
        for v in range(2):
            ro, rd = N.get_ray_bundle(H, W, focal, gts[v])
            targets.append(N.run_one_iter_of_nerf(H, W, focal, mc, mf, ro, rd, opts, mode="validation", encode_position_fn=ex,
                                                  encode_direction_fn=ed)[3])
        targets = torch.stack(targets).contiguous()
    deltas = []
    for axis, shift in (([0.3, -0.8, 0.5], [0.03, -0.03, 0.0277]), ([-0.6, 0.2, 0.7], [-0.0277, 0.03, 0.03])):
        axis = torch.tensor(axis)
        deltas.append(torch.cat([axis / axis.norm() * np.deg2rad(2.0), torch.tensor(shift)]).float().to(dev))
    starts = torch.stack([(gts[v] @ ES.se3(deltas[v])).detach() for v in range(2)])
    gts64 = gts.cpu().numpy().astype(np.float64)

    def errors(est, v):
        e = est.detach().cpu().numpy().astype(np.float64)
        return P.rot_angle_deg(e[:3, :3].T @ gts64[v][:3, :3]), float(np.linalg.norm(e[:3, 3] - gts64[v][:3, 3]))

    def engine():
        return N.TrainEngine(mc, mf, 64, 64, perturb=False, white_background=True, noise_std=0.0, lr=0.0, world_size=1, rank=0)

    def run(views):
        """Adam on one 6-vector per view of `views`; returns {view: [(step, rot_deg, trans), ...]}."""
        xi = torch.zeros(len(views), 6, device=dev, requires_grad=True)
        opt = torch.optim.Adam([xi], lr=LR)
        eng = engine()
        pg = torch.empty(len(views), 3, 4, device=dev)
        poses_of = lambda: torch.stack([starts[v] @ ES.se3(xi[j]) for j, v in enumerate(views)])  # noqa: E731
        curve = {v: [(-1,) + errors(starts[v], v)] for v in views}
        for it in range(STEPS):
            opt.zero_grad()
            poses = poses_of()
            if len(views) == 2:
                eng.step_on_views(targets, poses.detach(), H, W, focal, opts, 1024, lr=0.0, pose_grads=pg)
            else:
                eng.step_on_image(targets[views[0]], poses[0].detach(), H, W, focal, opts, 512, lr=0.0, pose_grad=pg[0])
            torch.autograd.backward(poses[:, :3, :4], pg)
            opt.step()
            if it % 50 == 0 or it == STEPS - 1:
                with torch.no_grad():
                    now = poses_of()
                for j, v in enumerate(views):
                    curve[v].append((it,) + errors(now[j], v))
        return curve

    joint = run([0, 1])
    single = {0: run([0])[0], 1: run([1])[1]}
    print("joint refinement of two poses (step, rotation deg, translation): %s" % joint)
    print("each pose alone (step_on_image): %s" % single)
    # (one parseable line: scripts/bench_views.py --capability-log carries it into profiles/r08_views.json)
    print("VIEWS_CAPABILITY " + json.dumps(dict(steps=STEPS, lr=LR, joint_rays=1024, single_rays=512,
                                                 joint={str(k): v for k, v in joint.items()},
                                                 single={str(k): v for k, v in single.items()})))
    for v in range(2):
        (_, r0, t0), (_, rj, tj), (_, rs, ts) = joint[v][0], joint[v][-1], single[v][-1]
        assert rj < r0 and tj < t0, (v, joint[v])
        assert rj <= 3 * rs and tj <= 3 * ts, (v, joint[v], single[v])
