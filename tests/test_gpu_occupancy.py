"""GPU suite (-m gpu): the occupancy grid of the inference render -- the cases of tests/occupancy_cases.py on the product library, the
capability claim on the lego-lowres fixture nets, and the Python surface (OccupancyGrid, the occupancy= keyword)."""
import numpy as np
import pytest
import torch

import occupancy_cases as OC
import parity_cases as P
from conftest import gold

pytestmark = pytest.mark.gpu

ALL = [(net, arith) for arith in ("fp32", "f16x3") for net in ("w64", "w128", "w256", "w40of64")] + [("novw128", "fp32")]


@pytest.mark.parametrize("res,outside", OC.MARK_GRIDS)
def test_mark_against_numpy(gpu, res, outside):
    OC.case_mark(gpu, res, outside)


@pytest.mark.parametrize("net,arith", ALL)
def test_listed_forward_exact(gpu, net, arith):
    # (... and 300 rays: the list runs over several workgroups of every kernel)
    OC.case_listed_forward(gpu, net, arith, shapes=((5, 8, 0), (20, 8, 16), (9, 13, 5), (1, 3, 1), (300, 13, 131)))


@pytest.mark.parametrize("net,arith", ALL)
def test_render_all_ones_is_the_dense_render(gpu, net, arith):
    OC.case_render_all_ones(gpu, net, arith)


@pytest.mark.parametrize("net,arith", [("w128", "fp32"), ("w256", "fp32"), ("w64", "fp32"), ("w40of64", "f16x3"), ("w256", "f16x3")])
def test_render_half_empty(gpu, net, arith):
    OC.case_render_half_empty(gpu, net, arith, n=150)


@pytest.mark.parametrize("net,arith", [("w128", "fp32"), ("w256", "f16x3")])
def test_render_all_zero(gpu, net, arith):
    OC.case_render_all_zero(gpu, net, arith)


@pytest.mark.parametrize("net,arith", [("w128", "fp32"), ("novw128", "fp32"), ("w64", "fp32"), ("w256", "fp32"), ("w128", "f16x3")])
def test_update(gpu, net, arith):
    OC.case_update(gpu, net, arith)


def test_dilate(gpu):
    OC.case_dilate(gpu)


def test_refusals(gpu):
    OC.case_refusals(gpu)


# ---- the Python surface and the capability claim -----------------------------------------------------------------------------
CFG = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
AABB = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))


@pytest.fixture(scope="module")
def lego(gpu):
    """The lego-lowres fixture nets, the fixture pose cut to 64 x 64 rays, and ONE grid from from_models at its defaults."""
    import nerf_pytorch_amd as N
    dev = torch.device("cuda", 0)
    w, r = gold("lego_lowres_weights.npz"), gold("lego_lowres_render.npz")
    mc, mf = N.FlexibleNeRFModel(**CFG), N.FlexibleNeRFModel(**CFG)
    mc.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("c_")})
    mf.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("f_")})
    mc, mf = mc.to(dev), mf.to(dev)
    # 64 x 64 rays over the fixture view's field: the same camera at 64 x 64 pixels
    H = W = 64
    focal = float(r["focal"]) * 64.0 / float(r["W"])
    pose = torch.from_numpy(r["pose"]).to(dev)
    grid = N.OccupancyGrid.from_models(mc, mf, AABB)
    ex, ed = N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)
    opts = N.make_options(64, 64, perturb=False, white_background=True, radiance_field_noise_std=0.0)
    return dict(N=N, dev=dev, mc=mc, mf=mf, H=H, W=W, focal=focal, pose=pose, grid=grid, ex=ex, ed=ed, opts=opts)


def _rows(s, **kw):
    with torch.no_grad():
        out, _ = s["N"].render_pose_rows(s["H"], s["W"], s["focal"], s["pose"], s["mc"], s["mf"], s["opts"], s["ex"], s["ed"], **kw)
    return out


def test_capability_on_the_fixture_nets(lego):
    """64 x 64 rays, 64 + 64 samples, white background, from_models at its defaults over [-1.5, 1.5]^3: MSE of rgb_fine against the
    dense render of the same library <= 1 / (12 * 255^2) (PSNR >= 58.9 dB: below the 8-bit output stage's own quantisation noise);
    kept fractions <= 0.25 (coarse) and <= 0.5 (fine).  The CPU oracle gives 65-69 dB and 0.11 / 0.32 (tests/test_occupancy.py)."""
    s = lego
    dense = _rows(s)
    got = _rows(s, occupancy=s["grid"])
    kc, tc, kf, tf = (int(v) for v in s["grid"].view_counts.tolist())
    assert s["grid"].last_counts.tolist() == [kc, tc, kf, tf]  # (one chunk: the view's counts are the chunk's)
    mse = float(((got[3] - dense[3]).double() ** 2).mean())
    rec = dict(mse_rgb_fine=mse, psnr_rgb_fine=float(-10 * np.log10(max(mse, 1e-30))), max_abs_rgb_fine=float((got[3] - dense[3]).abs().max()),
               kept_coarse=kc / tc, kept_fine=kf / tf, occupied_fraction=s["grid"].occupied_fraction())
    print("capability:", rec)
    P.note("occupancy_capability_gpu", **rec)
    assert tc == 64 * 64 * 64 and tf == 64 * 64 * 128
    assert mse <= 1.0 / (12 * 255 ** 2), rec
    assert kc / tc <= 0.25 and kf / tf <= 0.5, rec


def test_render_pose_rows_with_a_grid_is_the_c_entry_point(lego, gpu):
    """render_pose_rows(occupancy=g) against the same call assembled by hand: get_rays_at_pixels -> pack_rays -> nerfhip_render_fwd_occ on
    the models' inference plans and packed images, bit for bit; occupancy=None is today's render, bit for bit."""
    s, N = lego, lego["N"]
    got = _rows(s, occupancy=s["grid"])
    pix = torch.arange(s["H"] * s["W"], dtype=torch.int64, device=s["dev"])
    ro, rd = N.get_rays_at_pixels(s["H"], s["W"], s["focal"], s["pose"][:3, :4], pix)
    rays = N.pack_rays(ro, rd, s["opts"], s["H"], s["W"], s["focal"]).cpu().numpy()
    g = s["grid"]
    cg = OC.Grid(gpu, g.bits.cpu().numpy().view(np.uint32), g.aabb[0], g.aabb[1], g.resolution, g.outside)
    opt = dict(num_coarse=64, num_fine=64, perturb=False, white_background=True, noise_std=0.0)
    with torch.no_grad():
        hand = OC.render_occ(gpu, s["mc"]._inference_plan(), s["mf"]._inference_plan(), s["mc"]._inference_packed(),
                             s["mf"]._inference_packed(), rays, opt, cg)
    for i, k in enumerate(("rgb_coarse", "disp_coarse", "acc_coarse", "rgb_fine", "disp_fine", "acc_fine")):
        assert np.array_equal(got[i].cpu().numpy(), hand[k].reshape(tuple(got[i].shape)), equal_nan=True), k
    assert tuple(int(v) for v in g.last_counts.tolist()) == hand["counts"] == tuple(int(v) for v in g.view_counts.tolist())
    # rendered in ray chunks (the last one partial): the same bits, and view_counts are the sums over the chunks -- the view's counts --
    # while last_counts are the last chunk's alone
    small = N.make_options(64, 64, perturb=False, white_background=True, radiance_field_noise_std=0.0, chunksize=1000)
    with torch.no_grad():
        chunked, _ = N.render_pose_rows(s["H"], s["W"], s["focal"], s["pose"], s["mc"], s["mf"], small, s["ex"], s["ed"], occupancy=g)
    for x, y in zip(got, chunked):
        assert torch.equal(x.isnan(), y.isnan()) and torch.equal(x.nan_to_num(), y.nan_to_num())
    assert tuple(int(v) for v in g.view_counts.tolist()) == hand["counts"]
    assert g.last_counts.tolist()[1::2] == [96 * 64, 96 * 128]  # 4096 rays = 4 x 1000 + 96
    # occupancy=None: the keyword changes nothing
    a, b_ = _rows(s), _rows(s, occupancy=None)
    with torch.no_grad():
        ro_i, rd_i = ro.view(s["H"], s["W"], 3), rd.view(s["H"], s["W"], 3)
        c = N.run_one_iter_of_nerf(s["H"], s["W"], s["focal"], s["mc"], s["mf"], ro_i, rd_i, s["opts"], mode="validation",
                                   encode_position_fn=s["ex"], encode_direction_fn=s["ed"])
    for x, y, z in zip(a, b_, c):  # (bits, the NaN disparity of empty rays included)
        for other in (y, z):
            assert torch.equal(x.isnan(), other.isnan()) and torch.equal(x.nan_to_num(), other.nan_to_num())


def test_train_mode_with_a_grid_raises(lego):
    s, N = lego, lego["N"]
    pix = torch.arange(64, dtype=torch.int64, device=s["dev"])
    ro, rd = N.get_rays_at_pixels(s["H"], s["W"], s["focal"], s["pose"][:3, :4], pix)
    with pytest.raises(NotImplementedError, match="inference render only"):
        N.run_one_iter_of_nerf(s["H"], s["W"], s["focal"], s["mc"], s["mf"], ro, rd, s["opts"], mode="train", encode_position_fn=s["ex"],
                               encode_direction_fn=s["ed"], occupancy=s["grid"])
    rays = N.pack_rays(ro, rd, s["opts"], s["H"], s["W"], s["focal"])
    with pytest.raises(NotImplementedError, match="inference render only"):
        N.predict_and_render_radiance(rays, s["mc"], s["mf"], s["opts"], mode="train", encode_position_fn=s["ex"],
                                      encode_direction_fn=s["ed"], occupancy=s["grid"])
    # mode="validation" with a gradient wanted (no torch.no_grad()): the training forward would run -- refused as well
    with pytest.raises(NotImplementedError, match="inference render only"):
        N.predict_and_render_radiance(rays, s["mc"], s["mf"], s["opts"], mode="validation", encode_position_fn=s["ex"],
                                      encode_direction_fn=s["ed"], occupancy=s["grid"])


def test_state_dict_round_trips(lego):
    s, N = lego, lego["N"]
    g = s["grid"]
    sd = g.state_dict()
    assert all(isinstance(v, torch.Tensor) and not v.is_cuda for v in sd.values())
    g2 = N.OccupancyGrid.from_state_dict(sd, s["dev"])
    assert torch.equal(g2.bits, g.bits) and g2.aabb == g.aabb and g2.resolution == g.resolution and g2.outside == g.outside
    g3 = N.OccupancyGrid(torch.zeros(1, dtype=torch.int32, device=s["dev"]), ((0, 0, 0), (1, 1, 1)), (1, 1, 32), True).load_state_dict(sd)
    assert torch.equal(g3.bits, g.bits) and g3.resolution == g.resolution and g3.outside is False
    assert 0.0 < g.occupied_fraction() < 0.5 and g2.occupied_fraction() == g.occupied_fraction()
    out_a, out_b = _rows(s, occupancy=g), _rows(s, occupancy=g2)
    assert torch.equal(out_a[3], out_b[3])
