"""Cost of the pose gradient in TrainEngine.step_on_image: ms/step with and without pose_grad, and the pose VJP kernels' own
time (nerfhip_profile_*), for lego 8x256 (4096 rays, 64 + 128), 4x128 and fern 4x64 (NDC, the fused backward mode 5 by
default; a step with pose_grad runs it as mode 2).  Prints one JSON line.

    python scripts/bench_pose.py [--steps 30] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import nerf_pytorch_amd as N  # noqa: E402

LINES = {
    "lego_8x256": dict(H=400, W=400, focal=555.5555, nc=64, nf=128, no_ndc=True, noise=0.2, near=2.0, far=6.0,
                       model=dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)),
    "lego_4x128": dict(H=400, W=400, focal=555.5555, nc=64, nf=64, no_ndc=True, noise=0.2, near=2.0, far=6.0,
                       model=dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)),
    "fern_4x64": dict(H=378, W=504, focal=407.5, nc=64, nf=64, no_ndc=False, noise=1.0, near=0.0, far=1.0,
                      model=dict(num_layers=4, hidden_size=64, skip_connect_every=3, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)),
}


def run_line(name, w, steps, warmup, rays):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    mc, mf = N.FlexibleNeRFModel(**w["model"]).to(dev), N.FlexibleNeRFModel(**w["model"]).to(dev)
    H, W = w["H"], w["W"]
    opts = N.make_options(w["nc"], w["nf"], no_ndc=w["no_ndc"], near=w["near"], far=w["far"], radiance_field_noise_std=w["noise"])
    img = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    pose = torch.eye(4, device=dev)
    pose[2, 3] = 4.0 if w["no_ndc"] else 0.0
    res = dict(modes=(mc.backward_compaction, mf.backward_compaction))
    for arm in ("plain", "pose_grad"):
        eng = N.TrainEngine(mc, mf, w["nc"], w["nf"], noise_std=w["noise"], lr=1e-6, world_size=1, rank=0)
        pg = torch.empty(3, 4, device=dev) if arm == "pose_grad" else None
        for _ in range(warmup):
            eng.step_on_image(img, pose, H, W, w["focal"], opts, rays, pose_grad=pg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.step_on_image(img, pose, H, W, w["focal"], opts, rays, pose_grad=pg)
        torch.cuda.synchronize()
        res[arm + "_ms"] = round((time.perf_counter() - t0) * 1e3 / steps, 4)
        if pg is not None:  # the two new launches by themselves, timed per launch
            with N.LaunchProfile(200 * steps) as prof:
                for _ in range(steps):
                    eng.step_on_image(img, pose, H, W, w["focal"], opts, rays, pose_grad=pg)
            res["kernels_us_per_step"] = {k: round(ms * 1e3 / steps, 2) for k, (_, ms) in prof.rows.items()
                                          if k in ("k_pose_vjp_part", "k_pose_vjp_sum", "k_ray_grad")}
            res["pose_grad_finite"] = bool(torch.isfinite(pg).all())
    res["pose_grad_cost_pct"] = round(100.0 * (res["pose_grad_ms"] / res["plain_ms"] - 1.0), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=4096)
    a = ap.parse_args()
    out = dict(metric="pose_grad_step_cost", rays=a.rays, steps=a.steps, lines={})
    for name, w in LINES.items():
        out["lines"][name] = run_line(name, w, a.steps, a.warmup, a.rays)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
