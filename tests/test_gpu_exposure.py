"""GPU suite (-m gpu): the per-view exposure -- the kernels of tests/exposure_cases.py on the product library, the drop-in autograd
node (train_utils.exposure_mse_loss), cameras.Exposure and TrainEngine.step_on_views / localize_on_views (exposure=...), the kernels
one step of each new form launches (tests/step_launches_exposure.json, recorded by this module:

    python tests/test_gpu_exposure.py --record tests/step_launches_exposure.json

) and the exposure rows of two re-exposed views recovered against frozen nets (the test-time fit)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import conftest  # noqa: F401 (first: run as a script, --record, this is what puts the package and the oracle on sys.path)
import engine_scenes as ES
import exposure_cases as EC
import pose_vjp as P

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(conftest.ROOT, "tests", "step_launches_exposure.json")


# ---- the kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", [1.0, 0.75])
@pytest.mark.parametrize("n,V,stride,fine", EC.GRID, ids=EC.GRID_IDS)
def test_loss_and_cotangents_against_fp64(gpu, n, V, stride, fine, gs):
    EC.case_loss_fp64(gpu, n, V, stride, fine, gs)


@pytest.mark.parametrize("gs", [1.0, 0.75])
@pytest.mark.parametrize("n,V,stride,fine", EC.GRID, ids=EC.GRID_IDS)
def test_table_gradient_against_fp64(gpu, n, V, stride, fine, gs):
    EC.case_grad_fp64(gpu, n, V, stride, fine, gs)


@pytest.mark.parametrize("n,V,stride,fine,kind", EC.BIG, ids=EC.BIG_IDS)
def test_table_gradient_against_fp64_over_many_views_and_in_one(gpu, n, V, stride, fine, kind):
    EC.case_grad_fp64(gpu, n, V, stride, fine, 1.0, kind)


@pytest.mark.parametrize("gs", [1.0, 0.75])
@pytest.mark.parametrize("n,V,stride,fine", EC.GRID, ids=EC.GRID_IDS)
def test_zero_table_gives_the_plain_loss_bits(gpu, n, V, stride, fine, gs):
    EC.case_zero_table_bits(gpu, n, V, stride, fine, gs)


def test_table_gradient_bits_do_not_depend_on_how_the_views_interleave(gpu):
    EC.case_view_order_bits(gpu)


@pytest.mark.parametrize("mask", EC.MASKS)
def test_masked_entries_get_exact_zeros_and_never_move(gpu, mask):
    EC.case_mask(gpu, mask)


def test_no_rays_and_indices_of_no_view(gpu):
    EC.case_edges(gpu)


def test_hundreds_of_indices_of_no_view_on_either_side(gpu):
    EC.case_many_indices_of_no_view(gpu)


def test_entry_points_reject_bad_arguments(gpu):
    EC.case_refusals(gpu)


# ---- drop-in autograd ---------------------------------------------------------------------------------------------------------------
def _case_on(dev, n=700, V=3, stride=4):
    c = EC.batch(n, V, True, stride)
    t = lambda k, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev).to(dt)  # noqa: E731
    return c, t("rc"), t("rf"), t("tgt"), t("inds", torch.int64), t("table")


def test_dropin_exposure_loss_is_the_kernels_from_one_node(gpu):
    """exposure_mse_loss: the forward is the plain launch (its loss words); (coarse + fine).backward() leaves the entry points' bits
    in rgb.grad and table.grad from ONE node; a table that does not require grad gets none; rgb_fine=None is the coarse-only net;
    other cotangents scale."""
    import nerf_pytorch_amd as N
    dev = ES.dev()
    c, rc, rf, tgt, inds, table = _case_on(dev)
    lo, gc, gf = EC.loss_views(gpu, c["rc"], c["rf"], c["tgt"], c["inds"], EC.HW, c["table"])
    ge = EC.expo_bwd(gpu, c["rc"], c["rf"], c["tgt"], c["inds"], EC.HW, c["table"])
    a, b, x = rc.clone().requires_grad_(True), rf.clone().requires_grad_(True), table.clone().requires_grad_(True)
    lc, lf = N.exposure_mse_loss(a, b, tgt, inds, EC.HW, x)
    assert lc.grad_fn is lf.grad_fn and type(lc.grad_fn).__name__.startswith("_ExposureLoss")
    assert float(lc.detach()) == float(lo[0]) and float(lf.detach()) == float(lo[1])
    (lc + lf).backward()
    assert np.array_equal(a.grad.cpu().numpy(), gc) and np.array_equal(b.grad.cpu().numpy(), gf)
    assert np.array_equal(EC.bits(x.grad.cpu().numpy()), EC.bits(ge))
    # ... and that backward was ONE nerfhip_exposure_bwd call; two cotangent tensors make it three
    for make, calls in ((lambda lc, lf: lc + lf, 1), (lambda lc, lf: 1.0 * lc + 1.0 * lf, 3)):
        x1 = table.clone().requires_grad_(True)
        lc, lf = N.exposure_mse_loss(rc, rf, tgt, inds, EC.HW, x1)
        assert _launches_of(lambda: make(lc, lf).backward()).get("k_expo_part") == calls
        assert torch.equal(x1.grad, x.grad)
    # the table does not require grad: none; the rgb gradients are the same
    a2, b2 = rc.clone().requires_grad_(True), rf.clone().requires_grad_(True)
    lc, lf = N.exposure_mse_loss(a2, b2, tgt, inds, EC.HW, table)
    (lc + lf).backward()
    assert table.grad is None and torch.equal(a2.grad, a.grad) and torch.equal(b2.grad, b.grad)
    # the table alone requires grad
    x2 = table.clone().requires_grad_(True)
    lc, lf = N.exposure_mse_loss(rc, rf, tgt, inds, EC.HW, x2)
    (lc + lf).backward()
    assert torch.equal(x2.grad, x.grad)
    # other cotangents: one multiply per element on the rgb; the table's gradient is the two nets' calls, each scaled
    a3, b3, x3 = rc.clone().requires_grad_(True), rf.clone().requires_grad_(True), table.clone().requires_grad_(True)
    lc, lf = N.exposure_mse_loss(a3, b3, tgt, inds, EC.HW, x3)
    (2.0 * lc + 0.5 * lf).backward()
    assert torch.equal(a3.grad, a.grad * 2.0) and torch.equal(b3.grad, b.grad * 0.5)
    g_c = EC.expo_bwd(gpu, c["rc"], None, c["tgt"], c["inds"], EC.HW, c["table"])
    g_f = EC.expo_bwd(gpu, c["rf"], None, c["tgt"], c["inds"], EC.HW, c["table"])
    assert np.array_equal(x3.grad.cpu().numpy(), g_c * np.float32(2.0) + g_f * np.float32(0.5))
    # coarse only
    a4, x4 = rc.clone().requires_grad_(True), table.clone().requires_grad_(True)
    lc, lf = N.exposure_mse_loss(a4, None, tgt, inds, EC.HW, x4)
    assert float(lf.detach()) == 0.0
    (lc + lf).backward()
    lo1, gc1, _ = EC.loss_views(gpu, c["rc"], None, c["tgt"], c["inds"], EC.HW, c["table"])
    assert float(lc.detach()) == float(lo1[0]) and np.array_equal(a4.grad.cpu().numpy(), gc1)
    assert np.array_equal(EC.bits(x4.grad.cpu().numpy()), EC.bits(g_c))
    with pytest.raises(RuntimeError, match=r"\(V, 6\)"):
        N.exposure_mse_loss(rc, rf, tgt, inds, EC.HW, table[:, :4])


def _launches_of(fn):
    """{kernel name: launches} of the library's kernels while fn() runs."""
    import nerf_pytorch_amd as N
    with N.LaunchProfile() as prof:
        fn()
    return prof.counts()


# ---- cameras.Exposure ------------------------------------------------------------------------------------------------------------------
def test_exposure_object_masks_backward_steps_and_state(gpu):
    import nerf_pytorch_amd as N
    dev = ES.dev()
    c, rc, rf, tgt, inds, table = _case_on(dev)
    X = N.Exposure(3, learn="affine", lr=1e-2, device=dev)
    assert torch.equal(X.values(), torch.zeros(3, 6, device=dev)) and X.values().data_ptr() == X.expo.data_ptr()
    assert X.mask.tolist() == [[0] * 6, [1] * 6, [1] * 6] and X.anchor == (0,)
    assert N.Exposure(3, learn="gain", anchor=(), device=dev).mask.tolist() == [[1, 1, 1, 0, 0, 0]] * 3
    assert N.Exposure(2, learn=(), device=dev).mask.tolist() == [[0] * 6] * 2
    assert N.Exposure(3, learn="gain", anchor=(2, 0), device=dev).mask.tolist() == [[0] * 6, [1, 1, 1, 0, 0, 0], [0] * 6]
    # backward() is the entry point under the object's mask, into its own buffer; the scratch is grown once
    X.expo.copy_(table)
    g = X.backward(rc, rf, tgt, inds, EC.HW, 0.75)
    want = EC.expo_bwd(gpu, c["rc"], c["rf"], c["tgt"], c["inds"], EC.HW, c["table"], 0.75, mask=X.mask.cpu().numpy())
    assert g.data_ptr() == X.g_expo.data_ptr() and np.array_equal(EC.bits(g.cpu().numpy()), EC.bits(want))
    tmp = X._tmp.data_ptr()
    X.backward(rc[:100], rf[:100], tgt[:100], inds[:100], EC.HW)
    assert X._tmp.data_ptr() == tmp
    # backward() refuses what the kernels could not read safely
    left = X.g_expo.clone()
    for bad in ((rc.double(), rf, tgt, inds), (rc[:, :2], rf, tgt, inds), (rc.t().contiguous().t(), rf, tgt, inds), (rc, rf[:-1], tgt, inds),
                (rc, rf, tgt.t().contiguous().t(), inds), (rc, rf, tgt[:, :2], inds), (rc, rf, tgt[:-1], inds), (rc, rf, tgt, inds.int()),
                (rc, rf, tgt, inds[:-1]), (rc, rf, tgt, torch.stack([inds, inds], 1)[:, 0]),
                (rc.cpu(), rf, tgt, inds), (rc, rf, tgt, inds.cpu())):
        with pytest.raises(RuntimeError, match="exposure_grad|CPU|devices"):
            X.backward(*bad, EC.HW)
    assert torch.equal(X.g_expo, left)   # (refused before anything was launched)
    # 20 steps never move a masked entry
    G = N.Exposure(3, learn="gain", anchor=(1,), lr=1e-2, device=dev)
    G.expo.copy_(table)
    for _ in range(20):
        G.backward(rc, rf, tgt, inds, EC.HW)
        G.step()
    still = G.mask == 0
    assert G.step_count == 20 and torch.equal(G.expo[still], table[still]) and torch.all(G.expo[~still] != table[~still])
    # apply: the row's correction in plain torch
    img = torch.rand(5, 7, 3, device=dev)
    assert torch.equal(G.apply(img, 2), img * torch.exp(G.expo[2, :3]) + G.expo[2, 3:])
    # state
    state = G.state_dict()
    assert sorted(state) == ["anchor", "exp_avg", "exp_avg_sq", "expo", "learn", "step"]
    K = N.Exposure(3, learn="gain", anchor=(1,), lr=1e-2, device=dev)
    K.load_state_dict(state)
    for o in (G, K):
        o.backward(rc, rf, tgt, inds, EC.HW)
        o.step()
    for name in ("expo", "exp_avg", "exp_avg_sq", "g_expo"):
        assert torch.equal(getattr(G, name), getattr(K, name)), name
    assert K.step_count == G.step_count == 21
    with pytest.raises(RuntimeError, match="learn"):
        N.Exposure(3, learn="offset", device=dev)
    with pytest.raises(RuntimeError, match="learn"):
        N.Exposure(3, learn="affine", anchor=(1,), device=dev).load_state_dict(state)
    with pytest.raises(RuntimeError, match="anchor"):
        N.Exposure(3, learn="gain", anchor=(0,), device=dev).load_state_dict(state)
    with pytest.raises(RuntimeError, match="anchor"):
        N.Exposure(3, anchor=(3,), device=dev)
    with pytest.raises(RuntimeError, match="shape"):
        N.Exposure(4, learn="gain", anchor=(1,), device=dev).load_state_dict(state)


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
def _lego_engine(N, dev, overlap=None, **kw):
    mc, mf, H, W, focal, pose0 = ES.lego(dev)
    eng = N.TrainEngine(mc, mf, 32, 32, perturb=True, white_background=True, noise_std=0.2, seed=3, lr=5e-4, world_size=1, rank=0,
                        overlap=overlap, **kw)
    imgs = torch.rand(3, H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    return eng, mc, mf, H, W, focal, imgs, ES.views(pose0, dev, 3)


def test_a_zero_table_that_learns_nothing_leaves_the_step_what_it_was():
    """Exposure(learn=()) at zero: three steps of step_on_views(exposure=X) give the loss, grad, flat_params and Adam moments of
    step_on_views without it, by torch.equal (fp32 plans, the lego-lowres geometry, 256 rays)."""
    import nerf_pytorch_amd as N
    dev = ES.dev()
    opts = N.make_options(32, 32)
    res = {}
    for arm in ("with", "without"):
        eng, mc, mf, H, W, focal, imgs, base = _lego_engine(N, dev)
        X = N.Exposure(3, learn=(), device=dev) if arm == "with" else None
        losses = []
        for _ in range(3):
            losses.append(eng.step_on_views(imgs, base, H, W, focal, opts, 256, exposure=X).clone())
        torch.cuda.synchronize()
        res[arm] = [torch.stack(losses)] + [t.clone() for t in (eng.grad, mc.flat_params, mf.flat_params, eng.exp_avg, eng.exp_avg_sq)]
        assert eng.step_count == 3
        if X is not None:
            assert X.step_count == 3 and torch.all(X.expo == 0) and torch.all(X.g_expo == 0) and torch.all(X.exp_avg == 0)
    for name, a, b in zip(("losses", "grad", "coarse", "fine", "exp_avg", "exp_avg_sq"), res["with"], res["without"]):
        assert torch.equal(a, b), name
    assert float(res["with"][1].abs().sum()) > 0


def test_two_streams_and_one_stream_give_the_same_bits_under_a_table():
    """A non-zero table: the two-stream step and the one-stream step leave the same bits in grad and X.g_expo, and X.g_expo is
    nerfhip_exposure_bwd on the engine's own rgb buffers under X.mask."""
    import nerf_pytorch_amd as N
    from nerf_pytorch_amd.cameras import exposure_grad
    dev = ES.dev()
    opts = N.make_options(32, 32)
    table = torch.from_numpy(EC.batch(700, 3, True, 4)["table"]).to(dev)
    res = {}
    for overlap in (True, False):
        eng, mc, mf, H, W, focal, imgs, base = _lego_engine(N, dev, overlap=overlap)
        X = N.Exposure(3, learn="affine", lr=1e-3, device=dev)
        X.expo.copy_(table)
        with torch.no_grad():
            rays, tgt, used = N.select_training_rays_views(H, W, focal, base, imgs, 256, opts, seed=3, step=0, first=0)
        eng.forward_backward(rays, tgt, exposure=(X, used, H * W))
        by_hand = exposure_grad(eng._bufs["rgb_c"], eng._bufs["rgb_f"], tgt, used, H * W, X.expo, 1.0, X.mask)
        torch.cuda.synchronize()
        assert torch.equal(by_hand, X.g_expo) and torch.all(X.g_expo[0] == 0) and torch.all(X.g_expo[1:] != 0)
        res[overlap] = [t.clone() for t in (eng.grad, X.g_expo, eng.loss)]
        for bad in ((X, used[:-1], H * W), (X, used.int(), H * W), (X.expo, used, H * W)):
            with pytest.raises(RuntimeError, match="exposure|inds"):
                eng.forward_backward(rays, tgt, exposure=bad)
    for name, a, b in zip(("grad", "g_expo", "loss"), res[True], res[False]):
        assert torch.equal(a, b), name
    assert float(res[True][0].abs().sum()) > 0


def test_the_test_time_fit_alone_leaves_the_nets_alone_and_the_refusals():
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
    X = N.Exposure(V, learn="affine", lr=1e-2, device=dev)
    T = N.CameraTable(base, lr=2e-3)
    for _ in range(3):
        eng.localize_on_views(imgs, base, H, W, focal, opts, n, exposure=X)      # the test-time fit alone
    eng.localize_on_views(imgs, None, H, W, focal, opts, n, cameras=T, exposure=X)
    torch.cuda.synchronize()
    for name, a, b in zip(("coarse", "fine", "exp_avg", "exp_avg_sq", "grad", "packed_c", "packed_f"), before, ES.state(eng)):
        assert torch.equal(a, b), name
    assert eng.step_count == 0 and eng.localize_count == 4 and X.step_count == 4 and T.step_count == 1
    assert torch.all(X.expo[0] == 0) and torch.all(X.expo[1:] != 0) and torch.all(torch.isfinite(X.expo))
    # refusals
    R = RuntimeError
    for call, exc, msg in (
            (lambda: eng.step_on_image(imgs[0], base[0], H, W, focal, opts, n, exposure=X), R, "no view axis"),
            (lambda: eng.localize_on_image(imgs[0], base[0], H, W, focal, opts, n, exposure=X), R, "no view axis"),
            (lambda: eng.step_on_views(imgs, base, H, W, focal, opts, n, exposure=X.values()), R, "cameras.Exposure"),
            (lambda: eng.localize_on_views(imgs, base, H, W, focal, opts, n, exposure=(X, None, 1)), R, "cameras.Exposure"),
            (lambda: eng.step_on_views(imgs, base, H, W, focal, opts, n, exposure=N.Exposure(V + 1, device=dev)), R, "holds 4 views"),
            (lambda: eng.localize_on_views(imgs, base, H, W, focal, opts, n, exposure=N.Exposure(V - 1, device=dev)), R, "holds 2 views"),
            (lambda: eng.localize_on_views(imgs, base, H, W, focal, opts, n), R, "needs")):
        with pytest.raises(exc, match=msg):
            call()
    X.dev = torch.device("cpu")   # (a table of another device: one GPU is all a test may count on)
    with pytest.raises(R, match="lives on cpu"):
        eng.step_on_views(imgs, base, H, W, focal, opts, n, exposure=X)
    X.dev = dev
    eng2 = N.TrainEngine(mc, mf, 8, 8, world_size=2, rank=0)
    rays, tgt = torch.zeros(64, 11, device=dev), torch.zeros(64, 3, device=dev)
    for call in (lambda: eng2.step_on_views(imgs, base, H, W, focal, opts, n, exposure=X),
                 lambda: eng2.forward_backward(rays, tgt, exposure=(X, torch.zeros(64, dtype=torch.int64, device=dev), H * W))):
        with pytest.raises(NotImplementedError, match="exposure with world size 2"):
            call()
    with pytest.raises(NotImplementedError, match="world size 2"):
        eng2.localize_on_views(imgs, base, H, W, focal, opts, n, exposure=X)
    assert X.step_count == 4 and eng.localize_count == 4


# ---- the kernels one step of each new form launches ---------------------------------------------------------------------------------------
def _forms(s):
    """{form: (engine, cameras, intrinsics, distortion, exposure) -> one step of that form}."""
    vw, no_poses = s.views_args(), s.views_args(poses=False)
    gv34 = lambda: torch.empty(ES.V, 3, 4, device=s.dev)  # noqa: E731
    return {
        "step_on_views exposure": lambda e, T, I, D, X: e.step_on_views(*vw, exposure=X),
        "step_on_views pose_grads exposure": lambda e, T, I, D, X: e.step_on_views(*vw, pose_grads=gv34(), exposure=X),
        "step_on_views cameras intrinsics distortion exposure": lambda e, T, I, D, X: e.step_on_views(*no_poses, cameras=T, intrinsics=I,
                                                                                                    distortion=D, exposure=X),
        "localize_on_views exposure": lambda e, T, I, D, X: e.localize_on_views(*vw, exposure=X),
        "localize_on_views cameras exposure": lambda e, T, I, D, X: e.localize_on_views(*no_poses, cameras=T, exposure=X),
    }


def _launches():
    """{form: {kernel name: launches}} of the second step of every form (the first one warms up), fresh objects for each."""
    s = ES.Scene()
    return ES.form_launches(s, _forms(s), lambda: (s.engine(world_size=1), s.table(), s.intrinsics(), s.distortion(), s.exposure()))


BACKWARD = ("bwd", "dgrad", "wgrad")                                          # what a render backward launches
RAY_GRAD = ("k_point_grad", "k_ray_grad", "k_mlp_input_grad", "k_pose_views_part", "k_pose_vjp_sum")   # the ray gradient and its consumers


def test_every_exposure_step_form_launches_what_the_fixture_recorded():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = _launches()
    assert sorted(got) == sorted(want) and len(got) == 5
    with open(ES.STEP_LAUNCHES) as f:
        plain = json.load(f)["step_on_views"]
    for form in want:
        assert got[form] and got[form] == want[form], (form, got[form], want[form])
        assert got[form]["k_mse_loss_views"] == 2 and "k_mse_loss" not in got[form]
        assert got[form]["k_expo_part"] == 1 and got[form]["k_expo_sum"] == 1
        assert got[form]["k_pose_views_group"] == (2 if "pose_grads" in form or "cameras" in form else 1)
    alone = dict(got["step_on_views exposure"])
    assert not any(k.startswith(RAY_GRAD) for k in alone)                        # the exposure does not turn the ray gradient on
    for k, c in (("k_mse_loss_views", 2), ("k_pose_views_group", 1), ("k_expo_part", 1), ("k_expo_sum", 1)):
        assert alone.pop(k) == c
    alone["k_mse_loss"], alone["k_adam"] = 2, alone["k_adam"] - 1               # (X.step(): one more Adam launch)
    assert alone == plain                                                        # everything else is the plain step
    fit = got["localize_on_views exposure"]
    assert not any(b in k for k in fit for b in BACKWARD) and not any(k.startswith(RAY_GRAD) for k in fit)
    assert fit["k_adam"] == 1 and fit["k_volume_render_fwd"] == 2


# ---- the capability: the exposure of two re-exposed views recovered against frozen nets (the test-time fit) ---------------------------------
# The search space of the issue, in its order; CHOSEN is the first combination whose REFERENCE arm alone ends below one fifth of its
# starting max |row - true| (found by `python tests/test_gpu_exposure.py --search`, which runs the reference arm only).
SEARCH = [(lr, steps) for lr in (1e-2, 3e-2) for steps in (300, 600)]
CHOSEN = SEARCH[0]
RAYS = 1024
TRUE_ROWS = ((0.0, 0.0, 0.0, 0.0, 0.0, 0.0),            # view 0: untouched, the anchor
             (0.25, -0.2, 0.35, 0.03, -0.05, 0.02),     # gains exp(+-0.2 ... 0.35), offsets +-0.02 ... 0.06, per channel
             (-0.3, 0.22, -0.25, -0.04, 0.06, -0.02))


def _capability_scene(dev):
    import nerf_pytorch_amd as N
    mc, mf, H, W, focal, pose0 = ES.lego(dev)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)
    ex, ed = ES.ex_ed()
    opts = N.make_options(64, 64, perturb=False, white_background=True, radiance_field_noise_std=0.0)
    gt0 = torch.from_numpy(pose0).to(dev)
    gts = [gt0]
    for deg in (20.0, -20.0):
        turn = torch.eye(4, device=dev)
        turn[:3, :3] = P.rodrigues(torch.tensor([0.0, 0.0, np.deg2rad(deg)], dtype=torch.float64)).float().to(dev)
        gts.append(turn @ gt0)
    gts = torch.stack(gts).contiguous()
    true = torch.tensor(TRUE_ROWS, dtype=torch.float32, device=dev)
    with torch.no_grad():
        targets = []
        for v in range(3):
            ro, rd = N.get_ray_bundle(H, W, focal, gts[v])
            img = N.run_one_iter_of_nerf(H, W, focal, mc, mf, ro, rd, opts, mode="validation", encode_position_fn=ex,
                                         encode_direction_fn=ed)[3]
            targets.append(img[..., :3] * torch.exp(true[v, :3]) + true[v, 3:])   # the view as its camera exposed it
        targets = torch.stack(targets).contiguous()
    return N, mc, mf, H, W, focal, ex, ed, opts, gts, targets, true


def _error(table, true):
    return float((table.detach() - true).abs().max())


def _reference_arm(scene, lr, steps, seed):
    """The reference arm: the engine arm's batches and the library's forwards; the loss and the table gradient by torch autograd on a
    (3, 6) leaf (row 0, the anchor, gets no gradient), torch.optim.Adam."""
    N, mc, mf, H, W, focal, ex, ed, opts, gts, targets, true = scene
    dev = gts.device
    table = torch.zeros(3, 6, device=dev, requires_grad=True)
    opt = torch.optim.Adam([table], lr=lr)
    learned = torch.ones(3, 6, device=dev)
    learned[0] = 0
    curve = [(-1, _error(table, true))]
    for it in range(steps):
        with torch.no_grad():
            rays, tgt, used = N.select_training_rays_views(H, W, focal, gts, targets, RAYS, opts, seed=seed, step=it, first=0)
            out = N.predict_and_render_radiance(rays, mc, mf, opts, encode_position_fn=ex, encode_direction_fn=ed)
        opt.zero_grad()
        row = table[used // (H * W)]
        loss = sum(torch.nn.functional.mse_loss(torch.exp(row[:, :3]) * rgb + row[:, 3:], tgt) for rgb in (out[0], out[3]))
        loss.backward()
        table.grad.mul_(learned)
        opt.step()
        if it % 50 == 0 or it == steps - 1:
            curve.append((it, _error(table, true)))
    return curve


def test_the_exposure_of_re_exposed_views_is_recovered_on_frozen_nets():
    """Frozen lego-lowres nets; three views at their exact poses with targets rendered through the library (64 + 64 samples, no
    perturb, white background); views 1 and 2 re-exposed with TRUE_ROWS, view 0 untouched and the anchor.  Engine arm: STEPS
    localize_on_views(exposure=X) steps of RAYS rays, X = Exposure(3, learn="affine") from zero.  Reference arm: _reference_arm.  The
    bar: the engine arm's final max |row - true| is at most 3 x the reference arm's (the project's margin for an optimiser trajectory
    compared across two arithmetic paths); the reference arm alone must end below one fifth of its start, which is what fixed CHOSEN."""
    dev = ES.dev()
    lr, steps = CHOSEN
    scene = _capability_scene(dev)
    N, mc, mf, H, W, focal, ex, ed, opts, gts, targets, true = scene
    eng = N.TrainEngine(mc, mf, 64, 64, perturb=False, white_background=True, noise_std=0.0, lr=0.0, world_size=1, rank=0)
    before = ES.state(eng)
    X = N.Exposure(3, learn="affine", lr=lr, device=dev)
    curve_e = [(-1, _error(X.expo, true))]
    for it in range(steps):
        eng.localize_on_views(targets, gts, H, W, focal, opts, RAYS, exposure=X)
        if it % 50 == 0 or it == steps - 1:
            curve_e.append((it, _error(X.expo, true)))
    assert torch.all(X.expo[0] == 0) and torch.all(torch.isfinite(X.expo)) and eng.localize_count == steps and eng.step_count == 0
    for a, b in zip(before, ES.state(eng)):
        assert torch.equal(a, b)
    curve_r = _reference_arm(scene, lr, steps, eng.seed)
    print("exposure recovery, engine arm (step, max |row - true|): %s" % curve_e)
    print("exposure recovery, reference arm: %s" % curve_r)
    print("EXPOSURE_CAPABILITY " + json.dumps(dict(steps=steps, lr=lr, rays=RAYS, engine=curve_e, reference=curve_r)))
    assert curve_r[-1][1] < curve_r[0][1] / 5, curve_r        # the reference arm alone
    assert curve_e[-1][1] <= 3 * curve_r[-1][1], (curve_e, curve_r)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        with open(sys.argv[2], "w") as f:
            json.dump(_launches(), f, indent=1, sort_keys=True)
            f.write("\n")
    elif len(sys.argv) == 2 and sys.argv[1] == "--search":
        for lr, steps in SEARCH:   # the reference arm alone, in the issue's order; the first that passes is CHOSEN
            curve = _reference_arm(_capability_scene(torch.device("cuda", 0)), lr, steps, 0)
            ok = curve[-1][1] < curve[0][1] / 5
            print("EXPOSURE_SEARCH " + json.dumps(dict(lr=lr, steps=steps, passes=ok, reference=curve)), flush=True)
            if ok:
                break
    else:
        sys.exit("usage: python tests/test_gpu_exposure.py --record PATH | --search")
