"""GPU suite (-m gpu): camera localisation on frozen nets -- nerfhip_render_grad_rays (csrc/nh_raygrad.h) through the cases of
tests/localize_cases.py, TrainEngine.forward_backward(frozen=True) / localize_on_image / localize_on_views, the drop-in loop with
FlexibleNeRFModel.set_frozen, and the two-camera recovery of tests/test_gpu_views.py driven by localize_on_views(cameras=...)."""
import json

import numpy as np
import pytest
import torch

import engine_scenes as ES
import localize_cases as LC
import parity_cases as PC
import pose_vjp as P

pytestmark = pytest.mark.gpu

# (geometry, rays, coarse, fine, backward mode, precision, problem options)
CASES = [
    ("default4x128", 300, 64, 64, False, 0, {}),
    ("northstar8x256", 64, 32, 32, False, 0, dict(noise=0.2)),                   # two xyz terms (layer1 and the skip layer)
    ("novw3x64_skip1", 100, 16, 16, False, 0, dict(white=True, noise=0.5)),      # 8-column rays, every layer a skip layer
    ("wide2x320", 40, 16, 16, False, 0, {}),                                     # two 256-row regions, the second one padded
    ("odd5x99_skip2", 40, 16, 16, False, 0, {}),                                 # 99 of 128 units: a masked last chunk
    ("L12_4x128", 100, 32, 32, False, 0, {}),                                    # extended encoding registers (112 / 64 slots), resident
    ("L16_Ld6_8x256", 64, 32, 32, False, 0, dict(noise=0.2)),                    # 261 KB of weight slices: streamed term by term, dense
    ("L16_Ld6_8x256", 50, 24, 16, True, 0, dict(noise=0.2)),                     # ... and over a list; ragged last tile
    ("llff4x64_skip3_L6", 12, 8, 8, "fused_stash", 0, {}),                       # runs as mode 2; S = 8 and 16: several rays per wave tile
    ("llff4x64_skip3_L6", 333, 24, 16, "fused_stash", 0, {}),                    # S = 24 and 40: no multiples of 16, a ragged last tile
    ("default4x128", 300, 64, 64, False, PC.F16X3_TRAIN, {}),
    ("default4x128", 1, 16, 16, True, 0, {}),
]
IDS = ["%s-n%d-%d+%d-%s-p%d" % c[:6] for c in CASES]
# teacher-forced on the kernels' own depths: (..., all six cotangents?).  The smallest shapes that still cross every tile edge; the sigma
# noise is what gives the nets whose initial densities are not positive something to render (every ray a gradient); the 256- and 512-wide
# nets at 8 + 8 samples so that the ReLU filter (every sample of a ray decided) leaves more than half of the rays
TF_CASES = [
    ("default4x128", 200, 16, 16, False, 0, {}, True),                           # 3200 / 6400 rows: 25 / 50 tiles; g_acc_*, g_depth_* drive g_norm
    ("default4x128", 200, 16, 16, False, PC.F16X3_TRAIN, {}, False),
    ("northstar8x256", 96, 8, 8, False, 0, dict(noise=0.2), True),               # two xyz terms, resident
    ("novw3x64_skip1", 100, 16, 16, False, 0, dict(white=True, noise=0.5), False),   # 8-column rays, every layer a skip layer
    ("noinput_linear", 100, 16, 16, False, 0, dict(noise=1.0), False),           # qin = -1 twice; 3 L = 15 / 9: half-filled last quads; linear bands
    ("narrow3x40", 100, 24, 16, True, 0, {}, False),                             # nu = 40 / 20: masked chunks in both kinds of term; S = 24 / 40 over a list
    ("Ld5_4x128_skip2", 100, 16, 16, False, 0, {}, False),                       # 3 Ld = 15 alone asks for the extended registers
    ("L11_novw3x64_skip1", 100, 16, 16, False, 0, dict(noise=0.5), False),       # 3 L = 33: odd, extended, no direction term
    ("L12_Ld10_2x512", 48, 8, 8, False, 0, dict(noise=0.5), False),              # two 256-unit terms per tensor, Ld at its limit
    ("wide3x512_skip2", 48, 8, 8, True, 0, dict(noise=0.5), False),              # ... with a skip layer, over a list
    ("L16_Ld6_8x256", 96, 8, 8, False, 0, dict(noise=0.2), False),               # streamed weight slices, dense
    ("L16_Ld6_8x256", 96, 8, 8, "recompute", 0, dict(noise=0.2), False),         # ... and over a list
    ("odd5x99_skip2", 64, 16, 16, False, 0, {}, False),                          # 99 of 128 units
    ("wide2x320", 64, 8, 8, False, 0, {}, False),                                # two regions, the second one padded
    ("one_layer", 64, 16, 16, False, 0, dict(noise=0.5), False),                 # layer1 and the direction layer alone
    ("llff4x64_skip3_L6", 333, 24, 16, "fused_stash", 0, {}, False),             # runs as mode 2; ragged last tile
    ("default4x128", 1, 16, 16, True, 0, {}, False),
]
TF_IDS = ["%s-n%d-%d+%d-%s-p%d" % c[:6] + ("-allcot" if c[7] else "") for c in TF_CASES]


@pytest.mark.parametrize("name,n,nc,nf,mode,precision,kw,allcot", TF_CASES, ids=TF_IDS)
def test_both_ray_gradient_chains_match_fp64_on_their_own_depths_ray_for_ray(gpu, name, n, nc, nf, mode, precision, kw, allcot):
    LC.case_teacher_forced(gpu, name, n, nc, nf, mode, precision, allcot, floor=LC.DECIDED_GPU, **kw)


@pytest.mark.parametrize("name,n,nc,nf,mode,precision,kw", CASES, ids=IDS)
def test_frozen_ray_gradient_matches_the_oracle(gpu, name, n, nc, nf, mode, precision, kw):
    LC.case_vs_oracle(gpu, name, n, nc, nf, mode, precision, **kw)


@pytest.mark.parametrize("name,n,nc,nf,mode,precision,kw", CASES, ids=IDS)
def test_frozen_ray_gradient_matches_the_trainable_path(gpu, name, n, nc, nf, mode, precision, kw):
    LC.case_vs_trainable_path(gpu, name, n, nc, nf, mode, precision, **kw)


def test_backward_modes_give_the_same_bits(gpu):
    LC.case_modes_give_the_same_bits(gpu, n=150, nc=24, nf=16)       # (6000 fine samples: 47 workgroup tiles, the last one ragged)
    LC.case_modes_give_the_same_bits(gpu, "northstar8x256", n=40, nc=16, nf=16)


def test_fused_modes_run_as_mode_2_and_give_the_same_bits(gpu):
    LC.case_modes_give_the_same_bits(gpu, "llff4x64_skip3_L6", n=90, nc=8, nf=8, modes=(False, "recompute", "fused", "fused_compact", "fused_stash"))


def test_streamed_weight_slices_give_the_same_bits_in_every_mode(gpu):
    """L16_Ld6_8x256: two 112-slot xyz images of 114 KB and a 64-slot direction image -- 261 KB, beyond the 160 KB of LDS: every term is
    staged behind its barriers for every 128-row tile (here 2000 fine rows: 16 tiles over persistent workgroups, the last one ragged)."""
    LC.case_modes_give_the_same_bits(gpu, "L16_Ld6_8x256", n=50, nc=24, nf=16)


def test_parts_layouts_and_open_window_on_the_bits(gpu):
    LC.case_parts_layouts_window(gpu, n=70, nc=16, nf=16)


def test_entry_point_rejects_bad_arguments(gpu):
    LC.case_refusals(gpu)


# ---- the engine -------------------------------------------------------------------------------------------------------------------------
def test_localize_leaves_the_nets_and_their_optimizer_alone():
    """Three localize_on_views steps with pose_grads, then three with a camera table: parameters, Adam moments, the gradient buffer
    and both packed images are what they were on the bits, step_count has not moved, localize_count counts, the table's twists move."""
    import nerf_pytorch_amd as N
    dev = ES.dev()
    mc, mf, H, W, focal, pose0 = ES.small(dev)
    V, n = 3, 256
    opts = N.make_options(8, 8)
    imgs = torch.rand(V, H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    base = ES.views(pose0, dev, V)
    for use_table in (False, True):
        eng = N.TrainEngine(mc, mf, 8, 8, perturb=True, white_background=True, noise_std=0.2, seed=3, lr=5e-4, world_size=1, rank=0)
        eng.grad.normal_()     # (what a training step left there stays there)
        eng.exp_avg.normal_()
        eng.exp_avg_sq.uniform_()
        before = ES.state(eng)
        T = N.CameraTable(base, lr=2e-3) if use_table else None
        grads = []
        for _ in range(3):
            if use_table:
                eng.localize_on_views(imgs, None, H, W, focal, opts, n, cameras=T)
            else:
                pg = torch.full((V, 3, 4), float("nan"), device=dev)
                eng.localize_on_views(imgs, base, H, W, focal, opts, n, pose_grads=pg)
                grads.append(pg)
        torch.cuda.synchronize()
        for name, a, b in zip(("coarse", "fine", "exp_avg", "exp_avg_sq", "grad", "packed_c", "packed_f"), before, ES.state(eng)):
            assert torch.equal(a, b), (use_table, name)
        assert eng.step_count == 0 and eng.localize_count == 3
        if use_table:
            assert T.step_count == 3 and torch.all(torch.isfinite(T.xi)) and all(float(T.xi[v].abs().sum()) > 0 for v in range(V))
        else:
            g = torch.stack(grads)
            assert torch.all(torch.isfinite(g)) and float(g.abs().sum()) > 0
            assert not torch.equal(g[0], g[1])     # (localize_count keys the selection and the draws: another batch every step)


def test_localize_on_views_equals_its_parts_and_two_streams_equal_one():
    import nerf_pytorch_amd as N
    from nerf_pytorch_amd.train_utils import select_training_rays_views, select_training_rays_views_bwd
    dev = ES.dev()
    V, n = 3, 256
    opts = N.make_options(8, 8)
    res = {}
    for arm in ("whole", "parts", "one_stream"):
        mc, mf, H, W, focal, pose0 = ES.small(dev)
        eng = N.TrainEngine(mc, mf, 8, 8, perturb=True, white_background=True, noise_std=0.2, seed=3, world_size=1, rank=0,
                            overlap=arm != "one_stream")
        imgs = torch.rand(V, H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
        poses = ES.views(pose0, dev, V)
        seen = []
        for it in range(3):
            pg = torch.full((V, 3, 4), float("nan"), device=dev)
            if arm == "parts":
                rays, tgt, used = select_training_rays_views(H, W, focal, poses, imgs, n, opts, seed=eng.seed, step=eng.localize_count, first=0)
                rg = torch.empty_like(rays)
                eng.forward_backward(rays, tgt, 0, None, None, rg, frozen=True, step=eng.localize_count)
                select_training_rays_views_bwd(H, W, focal, poses, used, rg, opts, eng.ray_grad_coarse, out=pg)
                eng.localize_count += 1
                loss = eng.loss
            else:
                loss = eng.localize_on_views(imgs, poses, H, W, focal, opts, n, pose_grads=pg)
            seen.append((loss.clone(), pg))
        torch.cuda.synchronize()
        res[arm] = seen
    for arm in ("parts", "one_stream"):
        for it, ((la, ga), (lb, gb)) in enumerate(zip(res["whole"], res[arm])):
            assert torch.equal(la, lb) and torch.equal(ga, gb), (arm, it)
    assert all(torch.all(torch.isfinite(g)) and float(g.abs().sum()) > 0 for _, g in res["whole"])


def test_dropin_frozen_pose_gradient_equals_the_engine_and_leaves_no_parameter_gradient():
    """select_training_rays (pose requiring grad) -> predict_and_render_radiance -> loss.backward() on two set_frozen nets: the pose
    gradient of TrainEngine.forward_backward(frozen=True) + select_training_rays_bwd on the same rays and draws, on the bits (the
    same kernels on the same numbers: the node's one buffer takes the fine part and accumulates the coarse one, the engine's pose
    kernel adds its two buffers row by row); no parameter has a gradient; the node keeps the flag of its forward."""
    import nerf_pytorch_amd as N
    from nerf_pytorch_amd.train_utils import select_training_rays_bwd
    dev = ES.dev()
    mc, mf, H, W, focal, pose0 = ES.lego(dev)
    ex, ed = ES.ex_ed()
    opts = N.make_options(64, 64, perturb=True, white_background=True, radiance_field_noise_std=0.0)
    n = 512
    g = torch.Generator().manual_seed(4)
    img = torch.rand(H, W, 3, generator=g).to(dev)
    draws = (torch.rand(n, 64, generator=g).to(dev), None, torch.rand(n, 64, generator=g).to(dev), None)
    mc.set_frozen(True), mf.set_frozen(True)
    leaf = torch.from_numpy(pose0).to(dev).requires_grad_(True)
    with pytest.raises(RuntimeError, match="frozen"):     # (the fixture's parameters still require grad)
        rays, tgt, used = N.select_training_rays(H, W, focal, leaf, img, n, opts, seed=9, step=0)
        N.predict_and_render_radiance(rays, mc, mf, opts, encode_position_fn=ex, encode_direction_fn=ed)
    params = list(mc.parameters()) + list(mf.parameters())
    for p in params:
        p.requires_grad_(False)
    got = []
    for switch in (False, True):
        leaf = torch.from_numpy(pose0).to(dev).requires_grad_(True)
        rays, tgt, used = N.select_training_rays(H, W, focal, leaf, img, n, opts, seed=9, step=0)
        real = ES.queue_draws([draws[0], draws[2]])
        try:
            out = N.predict_and_render_radiance(rays, mc, mf, opts, encode_position_fn=ex, encode_direction_fn=ed)
        finally:
            torch.rand, torch.randn = real
        loss = torch.nn.functional.mse_loss(out[0], tgt) + torch.nn.functional.mse_loss(out[3], tgt)
        if switch:     # (between forward and backward: the node runs the backward of its forward)
            mc.set_frozen(False), mf.set_frozen(False)
        loss.backward()
        mc.set_frozen(True), mf.set_frozen(True)
        got.append(leaf.grad[:3, :4].clone())
        assert all(p.grad is None for p in params)
    eng = N.TrainEngine(mc, mf, 64, 64, perturb=True, white_background=True, noise_std=0.0, lr=0.0, world_size=1, rank=0)
    rg = torch.empty_like(rays)
    eng.forward_backward(rays.detach(), tgt, draws=draws, ray_grad=rg, frozen=True)
    want = select_training_rays_bwd(H, W, focal, leaf, used, rg, opts, eng.ray_grad_coarse)
    torch.cuda.synchronize()
    print("LOCALIZE dropin vs engine: relative difference %.3e" % float((got[0] - want).norm() / want.norm()))
    assert torch.all(torch.isfinite(want)) and float(want.abs().sum()) > 0
    assert torch.equal(got[0], got[1])
    assert torch.equal(got[0], want)


def test_localize_refuses_what_it_cannot_do():
    import nerf_pytorch_amd as N
    dev = ES.dev()
    mc, mf, H, W, focal, pose0 = ES.small(dev)
    V = 2
    T = N.CameraTable(ES.views(pose0, dev, V))
    imgs = torch.zeros(V, H, W, 3, device=dev)
    opts = N.make_options(8, 8)
    eng = N.TrainEngine(mc, mf, 8, 8, world_size=1, rank=0)
    with pytest.raises(RuntimeError, match="poses=None"):
        eng.localize_on_views(imgs, T.poses(), H, W, focal, opts, 64, cameras=T)
    with pytest.raises(RuntimeError, match="pose_grads"):
        eng.localize_on_views(imgs, None, H, W, focal, opts, 64, pose_grads=torch.empty(V, 3, 4, device=dev), cameras=T)
    rays = torch.zeros(64, 11, device=dev)
    with pytest.raises(RuntimeError, match="ray_grad"):
        eng.forward_backward(rays, torch.zeros(64, 3, device=dev), frozen=True)
    eng2 = N.TrainEngine(mc, mf, 8, 8, world_size=2, rank=0)
    with pytest.raises(NotImplementedError, match="world size 2"):
        eng2.localize_on_views(imgs, None, H, W, focal, opts, 64, cameras=T)
    with pytest.raises(NotImplementedError, match="world size 2"):
        eng2.localize_on_views(imgs, T.poses(), H, W, focal, opts, 64, pose_grads=torch.empty(V, 3, 4, device=dev))
    with pytest.raises(NotImplementedError, match="world size 2"):
        eng2.localize_on_image(imgs[0], T.poses()[0], H, W, focal, opts, 64, torch.empty(3, 4, device=dev))
    assert T.step_count == 0 and eng.step_count == 0 and eng.localize_count == 0 and eng2.localize_count == 0


# ---- the capability -----------------------------------------------------------------------------------------------------------------------
STEPS, LR = 300, 3e-3


def test_two_perturbed_poses_are_recovered_by_localize_on_views():
    """The two-camera recovery of tests/test_gpu_views.py (frozen lego-lowres nets, each pose 2 degrees / 0.05 units off, STEPS steps
    of 1024 rays across both views) driven by localize_on_views(cameras=T).  The yardstick is the same run through the existing path,
    step_on_views(lr=0.0, cameras=T): every final error is below its start and at most 3x the yardstick's (the two runs share
    kernels up to the ray gradient's summation order; x3 is what the sibling tests give two such runs over 300 chaotic steps)."""
    import nerf_pytorch_amd as N
    dev = ES.dev()
    mc, mf, H, W, focal, pose0 = ES.lego(dev)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)
    ex, ed = ES.ex_ed()
    opts = N.make_options(64, 64, perturb=False, white_background=True, radiance_field_noise_std=0.0)
    gt0 = torch.from_numpy(pose0).to(dev)
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

    def run(localize):
        eng = N.TrainEngine(mc, mf, 64, 64, perturb=False, white_background=True, noise_std=0.0, lr=0.0, world_size=1, rank=0)
        T = N.CameraTable(starts, lr=LR)
        curve = {v: [(-1,) + errors(starts[v], v)] for v in range(2)}
        for it in range(STEPS):
            if localize:
                eng.localize_on_views(targets, None, H, W, focal, opts, 1024, cameras=T)
            else:
                eng.step_on_views(targets, None, H, W, focal, opts, 1024, lr=0.0, cameras=T)
            if it % 50 == 0 or it == STEPS - 1:
                est = T.pose_matrices()
                for v in range(2):
                    curve[v].append((it,) + errors(est[v], v))
        return curve

    new, old = run(True), run(False)
    # (one parseable line: scripts/bench_localize.py --capability-log carries it into profiles/r11_localize.json)
    print("LOCALIZE_CAPABILITY " + json.dumps(dict(steps=STEPS, lr=LR, rays=1024, localize_on_views={str(k): v for k, v in new.items()},
                                                    step_on_views_lr0={str(k): v for k, v in old.items()})))
    for v in range(2):
        (_, r0, t0), (_, rn, tn), (_, ro_, to_) = new[v][0], new[v][-1], old[v][-1]
        assert rn < r0 and tn < t0, (v, new[v])
        assert rn <= 3 * ro_ and tn <= 3 * to_, (v, new[v], old[v])
