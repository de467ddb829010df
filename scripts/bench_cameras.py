"""Cost of the camera parametrisation of pose refinement.  (1) The pose update alone -- compose V poses from V twists, pull a (V, 3, 4)
gradient back, one Adam step -- at V = 2, 100, 1000, three ways: (a) the per-view torch loop of tests/test_gpu_cameras.py's comparison arm (one
4 x 4 exponential per view, torch autograd, torch Adam), (b) the same restated batched over the views in torch, (c) CameraTable (three
launches).  Wall ms per step (median, smallest and largest of 5 timed windows) and device kernels per step (torch profiler; None
where it is not available or not taken).  (2) ms/step of
TrainEngine.step_on_views(cameras=...) against step_on_views(pose_grads=...) alone, for lego 8x256 and fern 4x64 at 4096 rays,
the two arms alternating over two rounds (`same_arm_spread_pct`: what one arm differs by between its rounds).
Every measurement runs in a child process of its own under its own time limit; the first one that fails ends the run.  Nothing
here asserts a speed.  Writes profiles/r09_cameras.json (and prints it as one JSON line); with --capability-log, the error curves
tests/test_gpu_cameras.py prints (its CAMERAS_CAPABILITY line, pytest -s) are carried along.

    python scripts/bench_cameras.py [--steps 30] [--warmup 5] [--timeout 240] [--out profiles/r09_cameras.json] [--capability-log LOG]
"""
import argparse
import os
import sys

from bench_common import LINES, ROOT, child_spec, emit, pair_cost, pose_stack, run_specs, scrape_log, timed, write_out

sys.path.insert(0, os.path.join(ROOT, "tests"))   # (the per-view torch exponential is the one the GPU test compares against)

TAG = "BENCH_CAMERAS_RESULT "


def _exp_batched(xi):
    """(V, 4, 4) exponentials of (V, 6) twists, batched over the views."""
    import torch
    w, v = xi[:, :3], xi[:, 3:]
    x = (w * w).sum(-1)
    small = x < 1e-2
    xs = torch.where(small, torch.ones_like(x), x)
    th = torch.sqrt(xs)
    a = torch.where(small, 1 - x / 6 + x * x / 120, torch.sin(th) / th)[:, None, None]
    b = torch.where(small, 0.5 - x / 24 + x * x / 720, (1 - torch.cos(th)) / xs)[:, None, None]
    c = torch.where(small, 1 / 6 - x / 120 + x * x / 5040, (th - torch.sin(th)) / (xs * th))[:, None, None]
    z = torch.zeros_like(x)
    K = torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], -1), torch.stack([w[:, 2], z, -w[:, 0]], -1),
                     torch.stack([-w[:, 1], w[:, 0], z], -1)], -2)
    eye = torch.eye(3, dtype=xi.dtype, device=xi.device)
    K2 = K @ K
    top = torch.cat([eye + a * K + b * K2, (eye + b * K + c * K2) @ v[:, :, None]], 2)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=xi.dtype, device=xi.device).expand(xi.shape[0], 1, 4)
    return torch.cat([top, bottom], 1)


def one_update(arm, V, steps, warmup):
    import torch

    import nerf_pytorch_amd as N
    from engine_scenes import se3_exp as exp_one
    dev = torch.device("cuda", 0)
    base = pose_stack(V, dev, 4.0)
    pg = torch.randn(V, 3, 4, generator=torch.Generator().manual_seed(3)).to(dev)
    if arm == "table":
        T = N.CameraTable(base, lr=1e-3)

        def step():
            T.poses()
            T.backward(pg)
            T.step()
    else:
        xi = torch.zeros(V, 6, device=dev, requires_grad=True)
        opt = torch.optim.Adam([xi], lr=1e-3)

        def step():
            opt.zero_grad()
            if arm == "torch_loop":
                poses = torch.stack([base[v] @ exp_one(xi[v]) for v in range(V)])
            else:
                poses = base @ _exp_batched(xi)
            torch.autograd.backward(poses[:, :3, :4], pg)
            opt.step()
    # (the profiler's record of the per-view loop at V = 1000, some 1.8e5 kernels, comes back cut short: not counted)
    return timed(step, steps, warmup, count_kernels=not (arm == "torch_loop" and V >= 1000))


def one_line(name, arm, steps, warmup, rays):
    import torch

    import nerf_pytorch_amd as N
    w = LINES[name]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    mc, mf = N.FlexibleNeRFModel(**w["model"]).to(dev), N.FlexibleNeRFModel(**w["model"]).to(dev)
    H, W, V = w["H"], w["W"], w["views"]
    opts = N.make_options(w["nc"], w["nf"], no_ndc=w["no_ndc"], near=w["near"], far=w["far"], radiance_field_noise_std=w["noise"])
    imgs = torch.rand(V, H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    poses = pose_stack(V, dev, 4.0 if w["no_ndc"] else 0.0)
    eng = N.TrainEngine(mc, mf, w["nc"], w["nf"], noise_std=w["noise"], lr=1e-6, world_size=1, rank=0)
    if arm == "cameras":
        T = N.CameraTable(poses, lr=1e-4)
        step = lambda: eng.step_on_views(imgs, None, H, W, w["focal"], opts, rays, cameras=T)  # noqa: E731
    else:
        pg = torch.empty(V, 3, 4, device=dev)
        step = lambda: eng.step_on_views(imgs, poses, H, W, w["focal"], opts, rays, pose_grads=pg)  # noqa: E731
    res = timed(step, steps, warmup)
    res["views"] = V
    return res


def child(spec):
    if spec["kind"] == "update":
        res = one_update(spec["arm"], spec["V"], spec["steps"], spec["warmup"])
    else:
        res = one_line(spec["line"], spec["arm"], spec["steps"], spec["warmup"], spec["rays"])
    emit(TAG, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_cameras.json"))
    ap.add_argument("--capability-log", default=None, help="output of pytest -s tests/test_gpu_cameras.py")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(child_spec(a.child))
    out = dict(metric="camera_table_cost", rays=a.rays, steps=a.steps, pose_update={}, lines={})
    specs = []
    for V in (2, 100, 1000):
        for arm in ("torch_loop", "torch_batched", "table"):
            # (the per-view loop at V = 1000 issues some 10^5 launches per step: fewer steps; the table's step is some 30 us: more)
            steps = max(2, a.steps // 15) if (arm == "torch_loop" and V >= 1000) else (a.steps * 20 if arm == "table" else a.steps)
            specs.append((("pose_update", "V%d" % V, arm), dict(kind="update", arm=arm, V=V, steps=steps, warmup=min(a.warmup, steps))))
    for name in LINES:   # (the two arms alternate, two rounds each)
        for arm in ("pose_grads", "cameras", "pose_grads_again", "cameras_again"):
            specs.append((("lines", name, arm), dict(kind="line", line=name, arm=arm.split("_again")[0], steps=a.steps, warmup=a.warmup,
                                                     rays=a.rays)))
    run_specs(__file__, TAG, specs, out, a.timeout)
    for name, r in out["lines"].items():
        if all(k in r for k in ("cameras", "pose_grads", "cameras_again", "pose_grads_again")):
            cost = pair_cost([r[k]["ms"] for k in ("cameras", "cameras_again")], [r[k]["ms"] for k in ("pose_grads", "pose_grads_again")])
            r["cameras_cost_pct"], r["same_arm_spread_pct"] = cost["cost_pct"], cost["same_arm_spread_pct"]
    if a.capability_log:
        scrape_log(out, a.capability_log, "CAMERAS_CAPABILITY ")
    write_out(out, a.out)


if __name__ == "__main__":
    main()
