"""GPU suite (-m gpu): the occupancy grid in training -- the cases of tests/occupancy_train_cases.py on the product library, TrainEngine
with a grid (warm-up, the culled step against the C entry points assembled by hand, grid updates, refusals), the density state of
OccupancyGrid, and the capability claim on a student of the lego-lowres fixture nets."""
import copy

import numpy as np
import pytest
import torch

import engine_scenes as ES
import occupancy_cases as OC
import occupancy_train_cases as OT
import parity_cases as P

pytestmark = pytest.mark.gpu

NETS = [("w64", "fp32"), ("w128", "fp32"), ("w256", "fp32"), ("w40of64", "fp32"), ("novw128", "fp32"), ("w64", "f16x3_train"),
        ("w128", "f16x3_train"), ("w256", "f16x3_train"), ("w40of64", "f16x3_train")]


@pytest.mark.parametrize("net,arith", NETS)
def test_all_ones_grid_is_the_recomputing_step(gpu, net, arith):
    OT.case_all_ones(gpu, net, arith)


@pytest.mark.parametrize("outside", [0, 1])
@pytest.mark.parametrize("net,arith", [("w128", "fp32"), ("w256", "fp32"), ("w64", "fp32"), ("w40of64", "f16x3_train"), ("w256", "f16x3_train")])
def test_half_empty_grid_is_the_substituted_dense_arm(gpu, net, arith, outside):
    OT.case_half_empty(gpu, net, arith, outside)


def test_half_empty_grid_over_several_list_blocks(gpu):
    """150 rays: 2250 fine samples, more than one 2048-sample block of the list kernels and several workgroups of every MLP kernel."""
    OT.case_half_empty(gpu, "w128", "fp32", 0, n=150)
    OT.case_half_empty(gpu, "w64", "fp32", 1, n=150)


@pytest.mark.parametrize("net,arith", [("w128", "fp32"), ("w64", "fp32"), ("w256", "f16x3_train")])
def test_all_zero_grid(gpu, net, arith):
    OT.case_all_zero(gpu, net, arith)


@pytest.mark.parametrize("net,arith", [("w128", "fp32"), ("w256", "f16x3_train")])
@pytest.mark.parametrize("res,ranges", [((1, 1, 32), ((0, 32),)), ((4, 6, 8), ((32, 96),)), ((8, 8, 8), ((0, 256), (256, 256)))])
def test_density_update_against_numpy(gpu, net, arith, res, ranges):
    OT.case_density_update(gpu, net, arith, res, ranges)


def test_density_update_nan_raw_keeps_the_decayed_value(gpu):
    OT.case_density_update(gpu, "w64", "fp32", (1, 1, 32), ((0, 32),), nan_weights=True)


@pytest.mark.parametrize("res", [(1, 1, 32), (4, 6, 8), (64, 64, 64)])
def test_density_bits_against_numpy(gpu, res):
    OT.case_density_bits(gpu, res)


def test_refusals(gpu):
    OT.case_refusals(gpu)


# ---- the engine ----------------------------------------------------------------------------------------------------------------
AABB = ES.AABB
SAMPLING = dict(num_coarse=64, num_fine=64, perturb=False, white_background=True, noise_std=0.0)


@pytest.fixture(scope="module")
def lego(gpu):
    return ES.lego64()


def _engine(s, **kw):
    return s["N"].TrainEngine(copy.deepcopy(s["mc"]), copy.deepcopy(s["mf"]), **dict(SAMPLING, **kw))


def test_engine_without_a_grid_is_the_engine(lego):
    s = lego
    a, b = _engine(s), _engine(s, occupancy=None)
    for e in (a, b):
        e.step(s["rays"], s["target"])
    assert b.occupancy_counts is None
    assert torch.equal(a.loss, b.loss) and torch.equal(a.grad, b.grad) and a.grad.abs().max() > 0
    assert torch.equal(a.mc.flat_params, b.mc.flat_params) and torch.equal(a.mf.flat_params, b.mf.flat_params)


@pytest.mark.parametrize("backward", [None, "recompute", "auto"])
def test_engine_warm_up_then_culled_steps(lego, backward):
    """occupancy_warmup = 3, a live 32^3 grid updated after every step: steps 0 - 2 are the plain engine's in the same `backward`, bit
    for bit (the updates run next to them); from step 3 on the forwards are culled: kept < total in both passes."""
    s, N = lego, lego["N"]
    grid = N.OccupancyGrid.for_training(AABB, resolution=32, device=s["dev"])
    plain, live = _engine(s, backward=backward), _engine(s, backward=backward, occupancy=grid, occupancy_warmup=3, occupancy_every=1)
    for step in range(5):
        for e in (plain, live):
            e.step(s["rays"], s["target"])
        kc, tc, kf, tf = live.occupancy_counts.tolist()
        if step < 3:
            assert torch.equal(plain.loss, live.loss) and torch.equal(plain.grad, live.grad), step
            assert torch.equal(plain.mf.flat_params, live.mf.flat_params) and (kc, tc, kf, tf) == (0, 0, 0, 0)
        else:
            assert (tc, tf) == (4096 * 64, 4096 * 128) and 0 < kc < tc and 0 < kf < tf, (step, kc, tc, kf, tf)
            assert torch.isfinite(live.loss).all() and torch.isfinite(live.grad).all()
            assert [m.backward_compaction for m in (live.mc, live.mf)] == [2, 2]
            counts = live.backward_sample_counts()
            assert counts["coarse"][0] <= kc and counts["fine"][0] <= kf and counts["fine"][1] == tf
    assert grid.update_count == 5 and 0.0 < grid.occupied_fraction() < 1.0
    if backward == "auto":
        assert live.backward_modes_used["fine"][2] == 2 and sum(live.backward_modes_used["fine"]) == 5


def test_engine_step_is_the_c_entry_points(lego, gpu):
    """One culled engine step (the from_models grid at its defaults, warm-up 0, no update) against nerfhip_render_fwd_occ_train +
    nerfhip_mse_loss_fwd_bwd + nerfhip_render_bwd_parts assembled by hand on the engine's own plans: loss and gradient bit for bit;
    the kept fractions are within the grid's capability bounds for this view (tests/test_gpu_occupancy.py)."""
    s = lego
    g = s["grid"]
    e = _engine(s, occupancy=g, occupancy_warmup=0, occupancy_every=1 << 30)
    e.forward_backward(s["rays"], s["target"])
    kc, tc, kf, tf = e.occupancy_counts.tolist()
    assert kc / tc <= 0.25 and kf / tf <= 0.5, (kc, tc, kf, tf)
    rays, tgt = s["rays"].cpu().numpy(), s["target"].cpu().numpy()
    cg = OC.Grid(gpu, g.bits.cpu().numpy().view(np.uint32), g.aabb[0], g.aabb[1], g.resolution, g.outside)
    assert gpu.lib.plan_bwd_compaction(e.mc._plan) == 2 and gpu.lib.plan_bwd_compaction(e.mf._plan) == 2   # (the engine set them)
    st = OT.Step(gpu, e.mc._plan, e.mf._plan, e.packed_c, e.packed_f, rays, SAMPLING)
    st.fwd_occ(cg)
    assert list(st.counts()) == [kc, tc, kf, tf]
    m = st.maps()
    lc, gc, _ = gpu.mse_loss(m["rgb_coarse"], None, tgt)
    lf, gf, _ = gpu.mse_loss(m["rgb_fine"], None, tgt)
    r = st.bwd(gc, gf)
    loss, grad = e.loss.cpu().numpy(), e.grad.cpu().numpy()
    assert loss[0] == lc[0] and loss[1] == lf[0] and loss[2] == np.float32(lc[0]) + np.float32(lf[0])
    assert np.array_equal(grad[:e.nc_params], r["g_coarse"]) and np.array_equal(grad[e.nc_params:], r["g_fine"]) and grad.any()
    counts = e.backward_sample_counts()
    assert counts["coarse"] == r["kept_coarse"] and counts["fine"] == r["kept_fine"]


def test_grid_update_changes_bits_through_density_and_covers_the_grid(lego, gpu):
    s, N = lego, lego["N"]
    g = N.OccupancyGrid.for_training(AABB, resolution=32, device=s["dev"])
    assert g.occupied_fraction() == 1.0 and not g.density.any() and g.density.shape == (32 ** 3,)
    nets = ((s["mc"]._inference_plan(), s["mc"]._inference_packed()), (s["mf"]._inference_plan(), s["mf"]._inference_packed()))
    g.density.fill_(5.0)   # (a sentinel no probe returns; decay 0: a probed cell becomes relu(sigma))
    slab = 32 ** 3 // 4
    for k in range(4):
        g.update_density(nets, step=k, decay=0.0)
        d = g.density.cpu().numpy()
        touched = d != 5.0
        assert touched[:slab * (k + 1)].mean() > 0.999 and not touched[slab * (k + 1):].any(), k
        thr = float(g.last_threshold.item())
        ref = min(np.float32(0.01), np.float32(d.astype(np.float64).mean()))
        assert abs(thr - float(ref)) <= float(np.spacing(ref)), (thr, ref)
        want = OC.np_dilate((d > thr).reshape(32, 32, 32))
        assert np.array_equal(OC.unpack_bits(g.bits.cpu().numpy(), (32, 32, 32)), want), k
    assert g.update_count == 4 and 0.0 < g.occupied_fraction() < 0.6
    # the max over the nets: each net alone gives no more than both
    both = g.density.clone()
    for net in nets:
        g.density.fill_(0.0)
        g.update_count = 3
        g.update_density((net,), step=3, decay=0.0)
        assert (g.density <= both).all()
    g2 = N.OccupancyGrid.from_models(s["mc"], s["mf"], AABB, resolution=32)
    with pytest.raises(RuntimeError, match="for_training"):
        g2.update_density(nets, step=0)


def test_state_dict_round_trips_with_density(lego):
    s, N = lego, lego["N"]
    g = N.OccupancyGrid.for_training(AABB, resolution=(32, 16, 8), outside=True, device=s["dev"])
    g.update_density(((s["mf"]._inference_plan(), s["mf"]._inference_packed()),), step=0, fraction=1.0)
    sd = g.state_dict()
    assert all(isinstance(v, torch.Tensor) and not v.is_cuda for v in sd.values()) and "density" in sd
    g2 = N.OccupancyGrid.from_state_dict(sd, s["dev"])
    assert torch.equal(g2.bits, g.bits) and torch.equal(g2.density, g.density) and g2.density.any() and g2.update_count == 1
    assert g2.resolution == (32, 16, 8) and g2.outside is True
    # state without a density loads as it always did, and leaves no density behind
    old = s["grid"].state_dict()
    assert "density" not in old
    g2.load_state_dict(old)
    assert g2.density is None and torch.equal(g2.bits, s["grid"].bits)


def test_engine_refusals(lego):
    s, N = lego, lego["N"]
    g = s["grid"]
    for mode in ("dense", "compact", "fused", "fused_stash", True, 0):
        with pytest.raises(ValueError, match="occupancy"):
            _engine(s, occupancy=g, backward=mode)
    with pytest.raises(NotImplementedError, match="world size 2"):
        _engine(s, occupancy=g, world_size=2, rank=0)
    e = _engine(s, occupancy=g, occupancy_warmup=100)
    with pytest.raises(NotImplementedError, match="ray gradient"):
        e.forward_backward(s["rays"], s["target"], ray_grad=torch.zeros_like(s["rays"]))
    with pytest.raises(NotImplementedError, match="ray gradient"):
        e.forward_backward(s["rays"], s["target"], ray_grad=torch.zeros_like(s["rays"]), frozen=True)
    image = torch.rand(64, 64, 3, device=s["dev"])
    with pytest.raises(NotImplementedError, match="ray gradient"):
        e.step_on_image(image, s["pose"], 64, 64, s["focal"], s["opts"], 256, pose_grad=torch.zeros(3, 4, device=s["dev"]))
    with pytest.raises(NotImplementedError, match="ray gradient"):
        e.localize_on_image(image, s["pose"], 64, 64, s["focal"], s["opts"], 256, pose_grad=torch.zeros(3, 4, device=s["dev"]))
    assert e.step_count == 0 and not e.grad.any()


# ---- capability ----------------------------------------------------------------------------------------------------------------
# the plain arm's held-out PSNR spread (max - min) over seeds 0, 1, 2, measured on the MI355X: 18.58 / 19.54 / 20.34 dB
# (profiles/r17_occupancy_train.json `capability`)
PLAIN_SPREAD_DB = 1.757


def test_capability_a_student_trains_as_well_with_a_live_grid(lego):
    """Six teacher views at 64 x 64 (the fixture nets' dense render, on poses rotated by 0, 20, .. 100 degrees about the scene's up
    axis from the fixture pose; the 60-degree view is held out), two 4 x 64 students from seed 0 trained for 400 steps of 1024 rays
    (lr 5e-3, sigma noise 1.0 as in the reference's LLFF configs: without it two of the three seeds start with sigma = relu(raw[3]) = 0
    everywhere and never move, in both arms): one plain, one with OccupancyGrid.for_training (64^3, warm-up 100, update every 16).
    Both losses finite throughout; the grid arm ends with an occupied fraction < 1 and a kept fine fraction < 1, and its held-out PSNR
    against the teacher is no worse than the plain arm's minus twice the plain arm's own spread over three seeds.
    Measured on the MI355X (seeds 0 / 1 / 2): plain 18.58 / 19.54 / 20.34 dB -> spread 1.757 dB, margin 3.51 dB; grid arm 18.75 /
    19.22 / 19.31 dB, kept 0.22 - 0.45 coarse and 0.32 - 0.62 fine, occupied fraction 0.27 - 0.70."""
    rec = OT.capability(lego, seed=0, with_grid=True)
    plain = OT.capability(lego, seed=0, with_grid=False)
    print("capability:", dict(plain=plain, grid=rec, plain_spread_db=PLAIN_SPREAD_DB))
    P.note("occupancy_train_capability_gpu", psnr_plain=plain["psnr"], psnr_grid=rec["psnr"], kept_fine=rec["kept_fine"],
           kept_coarse=rec["kept_coarse"], occupied_fraction=rec["occupied_fraction"])
    assert plain["finite"] and rec["finite"]
    assert rec["occupied_fraction"] < 1.0 and rec["kept_fine"] < 1.0, rec
    assert rec["psnr"] >= plain["psnr"] - 2.0 * PLAIN_SPREAD_DB, (rec, plain)
