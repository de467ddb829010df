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
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # (the per-view torch exponential is the one the GPU test compares against)

LINES = {
    "lego_8x256": dict(H=400, W=400, focal=555.5555, nc=64, nf=128, no_ndc=True, noise=0.2, near=2.0, far=6.0, views=100,
                       model=dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)),
    "fern_4x64": dict(H=378, W=504, focal=407.5, nc=64, nf=64, no_ndc=False, noise=1.0, near=0.0, far=1.0, views=20,
                      model=dict(num_layers=4, hidden_size=64, skip_connect_every=3, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)),
}
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


WINDOWS = 5


def _timed(step, steps, warmup, count_kernels=True):
    """ms per step over WINDOWS timed windows of `steps` steps each (median, smallest, largest), and the device kernels of one step."""
    import torch
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    ms.sort()
    kernels = None
    if count_kernels:
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                step()
                torch.cuda.synchronize()
            kernels = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        except Exception:
            pass
    return dict(ms=round(ms[len(ms) // 2], 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4), windows=WINDOWS, steps=steps,
                kernels=kernels)


def pose_stack(V, dev, z):
    import torch
    g = torch.Generator().manual_seed(2)
    p = torch.eye(4).repeat(V, 1, 1)
    p[:, :3, 3] = torch.randn(V, 3, generator=g) * 0.05
    p[:, 2, 3] += z
    return p.to(dev)


def one_update(arm, V, steps, warmup):
    import torch

    import nerf_pytorch_amd as N
    from test_gpu_cameras import _se3_exp as exp_one
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
    return _timed(step, steps, warmup, count_kernels=not (arm == "torch_loop" and V >= 1000))


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
    res = _timed(step, steps, warmup)
    res["views"] = V
    return res


def child(spec):
    if spec["kind"] == "update":
        res = one_update(spec["arm"], spec["V"], spec["steps"], spec["warmup"])
    else:
        res = one_line(spec["line"], spec["arm"], spec["steps"], spec["warmup"], spec["rays"])
    print(TAG + json.dumps(res))


def measure(spec, limit):
    """Runs one measurement in a fresh process under `limit` seconds; returns its result, or None (and the reason) on failure."""
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(spec)], timeout=limit, capture_output=True,
                           text=True)
    except subprocess.TimeoutExpired:
        return None, "time limit of %d s" % limit
    for ln in p.stdout.splitlines():
        if ln.startswith(TAG):
            return json.loads(ln[len(TAG):]), None
    return None, "exit status %d: %s" % (p.returncode, p.stderr.strip().splitlines()[-1:] or "")


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
        return child(json.loads(a.child))
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
    for (top, mid, arm), spec in specs:
        res, why = measure(spec, a.timeout)
        if res is None:
            out["stopped_at"] = dict(measurement=[top, mid, arm], reason=why)
            break
        out[top].setdefault(mid, {})[arm] = res
    for name, r in out["lines"].items():
        if all(k in r for k in ("cameras", "pose_grads", "cameras_again", "pose_grads_again")):
            cam, pg = [r[k]["ms"] for k in ("cameras", "cameras_again")], [r[k]["ms"] for k in ("pose_grads", "pose_grads_again")]
            r["cameras_cost_pct"] = round(100.0 * (sum(cam) / sum(pg) - 1.0), 2)
            # what the same arm differs by between its two rounds: a difference between the arms below this is not resolved
            r["same_arm_spread_pct"] = round(100.0 * max(abs(cam[0] - cam[1]) / min(cam), abs(pg[0] - pg[1]) / min(pg)), 2)
    if a.capability_log:
        with open(a.capability_log) as f:
            for ln in f:
                if "CAMERAS_CAPABILITY " in ln:
                    out["capability"] = json.loads(ln[ln.index("CAMERAS_CAPABILITY ") + len("CAMERAS_CAPABILITY "):])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
