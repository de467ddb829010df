"""CPU suite of the occupancy grid: the cases of tests/occupancy_cases.py on the wave emulator (kernel index algebra, list walk,
scatter of the raw rows, refusals), the case generators' own promises, and the capability claim on the CPU oracle."""
import numpy as np
import pytest
import torch

import nerf_oracle as O
import occupancy_cases as OC
from conftest import gold


@pytest.mark.parametrize("res,outside", OC.MARK_GRIDS)
def test_mark_against_numpy(emu, res, outside):
    OC.case_mark(emu, res, outside)


@pytest.mark.parametrize("res,outside", OC.MARK_GRIDS)
def test_mark_reference_excludes_under_one_percent(res, outside):
    c = OC.mark_case(res, outside, seed=11)  # (asserts the generator's promises itself)
    assert c["near"].mean() < 0.01


@pytest.mark.parametrize("net,arith", [("w64", "fp32"), ("w128", "fp32"), ("w256", "fp32"), ("w40of64", "fp32"), ("novw128", "fp32"),
                                       ("w64", "f16x3"), ("w128", "f16x3"), ("w256", "f16x3"), ("w40of64", "f16x3")])
def test_listed_forward_exact(emu, net, arith):
    OC.case_listed_forward(emu, net, arith)


@pytest.mark.parametrize("net,arith", [("w128", "fp32"), ("w64", "fp32"), ("w128", "f16x3")])
def test_render_all_ones_is_the_dense_render(emu, net, arith):
    OC.case_render_all_ones(emu, net, arith, n=9)


@pytest.mark.parametrize("net,arith", [("w128", "fp32"), ("w40of64", "f16x3")])
def test_render_half_empty(emu, net, arith):
    OC.case_render_half_empty(emu, net, arith)


def test_render_all_zero(emu):
    OC.case_render_all_zero(emu, "w128", "fp32")


@pytest.mark.parametrize("net,arith", [("w128", "fp32"), ("novw128", "fp32"), ("w64", "fp32")])
def test_update(emu, net, arith):
    OC.case_update(emu, net, arith)


def test_dilate(emu):
    OC.case_dilate(emu)


def test_refusals(emu):
    OC.case_refusals(emu)


# ---- capability, on the CPU oracle ----------------------------------------------------------------------------------------
def oracle_grid(par_c, par_f, cfg, aabb, res, passes, threshold, seed):
    """OccupancyGrid.from_models restated on the oracle: centre probe + passes - 1 jittered probes per cell and net, then one dilation."""
    lo, hi = np.asarray(aabb[0], np.float32), np.asarray(aabb[1], np.float32)
    ncells = res ** 3
    ids = np.arange(ncells)
    ijk = np.stack((ids % res, (ids // res) % res, ids // (res * res)), axis=1).astype(np.float32)
    cell = (hi - lo) / np.float32(res)
    g = np.random.default_rng(seed)
    occ = np.zeros(ncells, bool)
    view = torch.tensor([[0.0, 0.0, 1.0]]).expand(ncells, 3)
    with torch.no_grad():
        for k in range(passes):
            u = np.full((ncells, 3), 0.5, np.float32) if k == 0 else g.random((ncells, 3), dtype=np.float32)
            pts = torch.from_numpy(lo + (ijk + u) * cell)
            rays = torch.cat((pts, torch.zeros(ncells, 5), view), dim=1)
            for par in (par_c, par_f):
                raw = O.run_network(par, pts[:, None, :], rays, cfg, chunksize=1 << 16)
                occ |= raw[:, 0, 3].numpy() > threshold
    return OC.pack_bits(OC.np_dilate(occ.reshape(res, res, res)))


def test_capability_on_the_oracle():
    """The lego-lowres fixture nets at the fixture pose, 32 x 32 rays, 64 + 64 samples, white background; a 64^3 grid over
    [-1.5, 1.5]^3 (sigma > 0.01 at the centre or at three jittered probes of either net, dilated once): the culled render is within
    MSE 1 / (12 * 255^2) (PSNR 58.9 dB: the 8-bit output stage's own quantisation noise) of the dense one and keeps at most a quarter
    of the coarse and half of the fine samples."""
    w, r = gold("lego_lowres_weights.npz"), gold("lego_lowres_render.npz")
    cfg = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4, use_viewdirs=True)
    par_c = {k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("c_")}
    par_f = {k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("f_")}
    H, W, focal = int(r["H"]), int(r["W"]), float(r["focal"])
    ro, rd = O.get_ray_bundle(H, W, focal, torch.from_numpy(r["pose"])[:3, :4])
    ys, xs = np.linspace(0, H - 1, 32).round().astype(int), np.linspace(0, W - 1, 32).round().astype(int)
    ro, rd = ro[ys][:, xs].reshape(-1, 3), rd[ys][:, xs].reshape(-1, 3)
    rays = O.pack_rays(ro, rd, 2.0, 6.0, rd)
    opt = dict(num_coarse=64, num_fine=64, perturb=False, lindisp=False, white_background=True, noise_std=0.0)
    aabb = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
    bits = oracle_grid(par_c, par_f, cfg, aabb, 64, 4, 0.01, seed=0)
    empty = torch.from_numpy(OC.EMPTY)
    with torch.no_grad():
        dense = O.render_rays(rays, par_c, par_f, cfg, cfg, opt)
        z = dense["z_coarse"]
        fc = OC.np_mark(rays.numpy(), z.numpy(), bits, aabb[0], aabb[1], (64, 64, 64), 0).astype(bool)
        raw_c = torch.where(torch.from_numpy(fc)[..., None], dense["raw_coarse"], empty)
        _, _, _, w_c, _ = O.volume_render(raw_c, z, rays[:, 3:6], 0.0, None, True)
        _, z_f = O.hierarchical_z(z, w_c, 64, det=True)
        ff = OC.np_mark(rays.numpy(), z_f.numpy(), bits, aabb[0], aabb[1], (64, 64, 64), 0).astype(bool)
        pts = rays[:, None, :3] + rays[:, None, 3:6] * z_f[..., None]
        raw_f = torch.where(torch.from_numpy(ff)[..., None], O.run_network(par_f, pts, rays, cfg), empty)
        rgb_f = O.volume_render(raw_f, z_f, rays[:, 3:6], 0.0, None, True)[0]
    mse = float(((rgb_f - dense["rgb_fine"]).double() ** 2).mean())
    print("oracle capability: mse %.3e (psnr %.1f dB), kept coarse %.3f fine %.3f, occupied %.3f" % (
        mse, -10 * np.log10(max(mse, 1e-30)), fc.mean(), ff.mean(), OC.unpack_bits(bits, (64, 64, 64)).mean()))
    assert mse <= 1.0 / (12 * 255 ** 2), mse
    assert fc.mean() <= 0.25 and ff.mean() <= 0.5, (fc.mean(), ff.mean())
