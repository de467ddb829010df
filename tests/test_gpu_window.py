"""GPU suite (-m gpu): the coarse-to-fine encoding window -- the cases of tests/window_cases.py on the product library, the drop-in
loop under FlexibleNeRFModel.set_encoding_window against the engine's step, and TrainEngine(window=...)."""
import numpy as np
import pytest
import torch

import engine_scenes as ES
import nerf_oracle as O
import parity_cases as PC
import window_cases as WC

pytestmark = pytest.mark.gpu

CFG = WC.GEOMETRIES["fern4x64"]


# ---- the kernels and the library path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WC.GEOMETRIES))
def test_code_table_is_the_tensor_table_restated(gpu, name):
    WC.case_code_table(gpu, name)


def test_kernels_are_numpy_fp32_multiplies_on_the_bits(gpu):
    WC.case_kernels_bit_exact(gpu)


def test_entry_points_reject_bad_arguments(gpu):
    WC.case_refusals(gpu)


def test_open_window_is_no_window_on_the_bits(gpu):
    WC.case_open_window_is_no_window(gpu)


def test_integer_alpha_is_zeroed_columns_on_the_bits(gpu):
    WC.case_integer_alpha_is_zeroed_columns(gpu)


@pytest.mark.parametrize("name,precision", [("fern4x64", 0), ("skip8x128", 0), ("fern4x64", PC.F16X3)])
def test_windowed_forward_matches_the_fp64_wrapper(gpu, name, precision):
    WC.case_forward_fractional(gpu, name, precision)


@pytest.mark.parametrize("name", ["fern4x64", "skip8x128"])
def test_windowed_backward_matches_fp64_autograd_of_the_wrapper(gpu, name):
    WC.case_backward_fractional(gpu, name)


@pytest.mark.parametrize("mode", [None, "fused_stash"])
def test_windowed_fused_render_matches_the_fp64_oracle_render(gpu, mode):
    """Dense, and in the mode 4 x 64 nets run by default (the fused backward over the register-image stash)."""
    WC.case_render(gpu, mode)


# ---- the drop-in loop -------------------------------------------------------------------------------------------------------------
def _nets(dev, seeds=(2, 4)):
    # (seeds whose random-init nets have sigma > 0 on these scenes: seed 1's fc_alpha is negative on every sample, and a net whose
    # relu(sigma) is off everywhere has an all-zero gradient -- nothing to compare, nothing that trains)
    import nerf_pytorch_amd as N
    mc, mf = N.FlexibleNeRFModel(**CFG), N.FlexibleNeRFModel(**CFG)
    mc.load_state_dict(O.init_params(CFG, seed=seeds[0]))
    mf.load_state_dict(O.init_params(CFG, seed=seeds[1]))
    return mc.to(dev), mf.to(dev)


def _scene():
    r = ES.gold("lego_lowres_render.npz")
    return int(r["H"]), int(r["W"]), float(np.float32(r["focal"])), r["pose"].astype(np.float32)


def test_dropin_loop_returns_the_windowed_gradients_of_the_engine_step():
    """set_encoding_window on both models, get_ray_bundle -> run_one_iter_of_nerf -> loss.backward(): every tensor's .grad against the
    engine's flat gradient of the same rays and draws, and the pose's gradient against the engine's ray gradient pulled back through the
    same torch graph -- both to the 1e-4 of the norm tests/test_gpu_pose.py::test_engine_pose_gradient_equals_dropin holds the two
    paths to (same kernels, another buffer layout).  The node pins its forward's window; closed bands get exact zeros."""
    import nerf_pytorch_amd as N
    dev = ES.dev()
    H, W, focal, pose0 = _scene()
    mc, mf = _nets(dev)
    ax, ad = WC.FRACTIONAL["fern4x64"]
    mc.set_encoding_window(ax, ad), mf.set_encoding_window(ax, ad)
    ex, ed = N.get_embedding_function(6, True, True), N.get_embedding_function(4, True, True)
    opts = N.make_options(16, 16, perturb=True, white_background=True, radiance_field_noise_std=0.0)
    n = 512
    g = torch.Generator().manual_seed(4)
    sel = torch.randperm(H * W, generator=g)[:n].to(dev)
    tgt = torch.rand(n, 3, generator=g).to(dev)
    draws = (torch.rand(n, 16, generator=g).to(dev), None, torch.rand(n, 16, generator=g).to(dev), None)

    def bundle(leaf):
        ro, rd = N.get_ray_bundle(H, W, focal, leaf[:3, :4])
        return ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]

    def dropin(leaf):
        ro, rd = bundle(leaf)
        real = ES.queue_draws([draws[0], draws[2]])
        try:
            out = N.run_one_iter_of_nerf(H, W, focal, mc, mf, ro, rd, opts, encode_position_fn=ex, encode_direction_fn=ed)
        finally:
            torch.rand, torch.randn = real
        return torch.nn.functional.mse_loss(out[0], tgt) + torch.nn.functional.mse_loss(out[3], tgt)

    leaf = torch.from_numpy(pose0).to(dev).requires_grad_(True)
    loss = dropin(leaf)
    mc.set_encoding_window(0.0, 0.0)          # (changed between forward and backward: the node runs under its forward's window)
    loss.backward()
    mc.set_encoding_window(ax, ad)
    assert leaf.grad is not None and torch.all(torch.isfinite(leaf.grad)) and float(leaf.grad.abs().sum()) > 0

    eng = N.TrainEngine(mc, mf, 16, 16, perturb=True, white_background=True, noise_std=0.0, lr=0.0, world_size=1, rank=0)
    leaf2 = torch.from_numpy(pose0).to(dev).requires_grad_(True)
    rays = N.pack_rays(*bundle(leaf2), opts)
    rg = torch.empty_like(rays)
    eng.forward_backward(rays.detach().contiguous(), tgt, draws=draws, ray_grad=rg)
    rays.backward(rg + eng.ray_grad_coarse)
    torch.cuda.synchronize()
    assert torch.allclose(eng.loss[2], loss.detach(), rtol=1e-4)
    for model, flat in ((mc, eng.grad[:eng.nc_params]), (mf, eng.grad[eng.nc_params:])):
        codes = model._codes()
        t = torch.from_numpy(WC.lut(CFG, ax, ad)).to(dev)[codes.long()]
        got = torch.cat([p.grad.reshape(-1) for p in model._ordered_params()])
        for name, off, rows, cols in model._layout:
            sl = slice(off, off + rows * max(cols, 1))
            assert float(flat[sl].norm()) > 0, name
            rel = float((got[sl] - flat[sl]).norm() / flat[sl].norm())
            assert rel < 1e-4, (name, rel)
        assert bool((t == 0).any()) and not bool(got[t == 0].any()) and not bool(flat[t == 0].any())
        assert bool(got[(t > 0) & (t < 1)].any())
    rel = float((leaf.grad - leaf2.grad).norm() / leaf2.grad.norm())
    assert rel < 1e-4, rel
    # ... and it is the WINDOWED pose gradient: the unwindowed nets give another one
    mc.set_encoding_window(), mf.set_encoding_window()
    leaf3 = torch.from_numpy(pose0).to(dev).requires_grad_(True)
    dropin(leaf3).backward()
    assert float((leaf3.grad - leaf.grad).norm() / leaf3.grad.norm()) > 1e-2


# ---- the engine -------------------------------------------------------------------------------------------------------------------
STEPS, RAYS = 40, 256


def _run(dev, steps, overlap=None, record=False, **kw):
    import nerf_pytorch_amd as N
    mc, mf = _nets(dev)
    eng = N.TrainEngine(mc, mf, 16, 16, noise_std=0.2, seed=11, lr=5e-3, world_size=1, rank=0, overlap=overlap, **kw)
    rays, rgba = TV_rays(RAYS, dev)
    init = (mc.flat_params.clone(), mf.flat_params.clone())
    seen, losses = [], []
    for _ in range(steps):
        losses.append(eng.step(rays, rgba[:, :3]).clone())
        if record:
            seen.append((mc.flat_params.clone(), mf.flat_params.clone()))
    torch.cuda.synchronize()
    return eng, mc, mf, init, seen, torch.stack(losses)


def TV_rays(n, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    ro = torch.tensor([0.0, 0.0, 4.0]).expand(n, 3)
    rd = torch.randn(n, 3, generator=g) * 0.3
    rd[:, 2] = -1.0
    return O.pack_rays(ro, rd, 2.0, 6.0, rd).to(dev), torch.rand(n, 4, generator=g).to(dev)


def test_engine_with_an_open_window_equals_the_engine_without():
    dev = ES.dev()
    _, mc0, mf0, _, _, l0 = _run(dev, 20)
    eng, mc1, mf1, _, _, l1 = _run(dev, 20, window=(-2.0, -1.0), total_steps=STEPS)
    assert eng.window_alphas(0)[0] >= CFG["num_encoding_fn_xyz"] and mc1.encoding_window is not None
    assert torch.equal(mc0.flat_params, mc1.flat_params) and torch.equal(mf0.flat_params, mf1.flat_params) and torch.equal(l0, l1)
    _, mc2, mf2, _, _, _ = _run(dev, 20, window=lambda step: (6.0, 4.0))
    assert torch.equal(mc0.flat_params, mc2.flat_params) and torch.equal(mf0.flat_params, mf2.flat_params)


def test_engine_schedule_keeps_closed_bands_at_their_initial_values():
    """window=(0.1, 0.6) over 40 steps: a band's weight columns are torch.equal to their initial values after every step up to the
    last one it was closed in, and have moved by the end of the run once it has opened; the two-stream step gives the one-stream bits."""
    dev = ES.dev()
    runs = {ov: _run(dev, STEPS, overlap=ov, record=True, window=(0.1, 0.6), total_steps=STEPS) for ov in (True, False)}
    eng, mc, mf, init, seen, losses = runs[True]
    assert torch.all(torch.isfinite(losses)) and all(bool(torch.all(torch.isfinite(m.flat_params))) for m in (mc, mf))
    opened_some = closed_some = 0
    for net, model in enumerate((mc, mf)):
        codes = model._codes()
        for first, bands, which in ((1, CFG["num_encoding_fn_xyz"], 0), (17, CFG["num_encoding_fn_dir"], 1)):
            for k in range(bands):
                cols = codes == first + k
                assert int(cols.sum()) > 0
                closed = [eng.window_alphas(t)[which] <= k for t in range(STEPS)]     # (step t ran under window_alphas(t))
                last_closed = max([t for t in range(STEPS) if closed[t]], default=-1)
                assert all(closed[:last_closed + 1])                                   # (the schedule only opens)
                for t in range(last_closed + 1):
                    assert torch.equal(seen[t][net][cols], init[net][cols]), (net, first + k, t)
                    closed_some += 1
                if last_closed < STEPS - 1:
                    assert not torch.equal(seen[-1][net][cols], init[net][cols]), (net, first + k)
                    opened_some += 1
    assert opened_some > 4 and closed_some > 40
    assert eng.window_alphas(0)[0] < 0 and eng.window_alphas(STEPS - 1)[0] >= CFG["num_encoding_fn_xyz"]
    other = runs[False]
    assert torch.equal(mc.flat_params, other[1].flat_params) and torch.equal(mf.flat_params, other[2].flat_params)
    assert torch.equal(losses, other[5])
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(seen, other[4]))


def test_step_on_views_with_cameras_runs_under_a_schedule():
    import nerf_pytorch_amd as N
    dev = ES.dev()
    H, W, focal, pose0 = _scene()
    mc, mf = _nets(dev)
    V = 3
    imgs = torch.rand(V, H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    T = N.CameraTable(ES.views(pose0, dev, V), lr=2e-3)
    eng = N.TrainEngine(mc, mf, 16, 16, seed=3, lr=5e-4, world_size=1, rank=0, window=(0.0, 0.5), total_steps=8)
    opts = N.make_options(16, 16)
    init = mc.flat_params.clone()
    seen = []
    for _ in range(8):
        under = mc.encoding_window                     # (the window the step about to run was packed under)
        loss = eng.step_on_views(imgs, None, H, W, focal, opts, RAYS, cameras=T)
        seen.append((under, loss.clone()))
    torch.cuda.synchronize()
    assert [w for w, _ in seen] == [eng.window_alphas(t) for t in range(8)] and seen[0][0] == (0.0, 0.0) and mf.encoding_window == mc.encoding_window
    assert mc.encoding_window == eng.window_alphas(8) and T.step_count == 8 and eng.step_count == 8
    assert torch.all(torch.isfinite(T.xi)) and float(T.xi.abs().sum()) > 0 and all(bool(torch.isfinite(l).all()) for _, l in seen)
    assert not torch.equal(mc.flat_params, init)
    with pytest.raises(ValueError, match="total_steps"):
        N.TrainEngine(mc, mf, 16, 16, world_size=1, rank=0, window=(0.1, 0.6))
