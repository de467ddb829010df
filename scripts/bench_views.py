"""Cost of a ray batch over a stack of views: per-launch times (nerfhip_profile_*) of the views selection and the views pose VJP
at (n, V) = (4096, 1), (4096, 100), (65536, 1000) on 400 x 400 views, next to the single-view launches at the same n in the same
process; and ms/step of TrainEngine.step_on_views against step_on_image, with and without pose gradients, for lego 8x256
(4096 rays, 64 + 128, 100 views) and fern 4x64 (NDC, 20 views).  Writes profiles/r08_views.json (and prints it as one JSON line);
with --capability-log, the error curves that tests/test_gpu_views.py prints (its VIEWS_CAPABILITY line, pytest -s) are carried along.

    python scripts/bench_views.py [--steps 30] [--warmup 5] [--reps 50] [--out profiles/r08_views.json] [--capability-log LOG]
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
from nerf_pytorch_amd import train_utils as T  # noqa: E402

LINES = {
    "lego_8x256": dict(H=400, W=400, focal=555.5555, nc=64, nf=128, no_ndc=True, noise=0.2, near=2.0, far=6.0, views=100,
                       model=dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)),
    "fern_4x64": dict(H=378, W=504, focal=407.5, nc=64, nf=64, no_ndc=False, noise=1.0, near=0.0, far=1.0, views=20,
                      model=dict(num_layers=4, hidden_size=64, skip_connect_every=3, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)),
}
SEL = ("k_select_rays",)                                                       # (one kernel: a single image is a stack of one view)
VJP1 = ("k_pose_vjp_part", "k_pose_vjp_sum")                                    # the single-view VJP's two launches
VJPV = ("k_pose_views_group", "k_pose_views_part", "k_pose_vjp_sum")             # the views VJP's three (the sum kernel is shared)


def kernel_us(prof, names):
    return {k: round(ms * 1e3 / launches, 2) for k, (launches, ms) in prof.rows.items() if k in names}   # us per launch


def pose_stack(V, dev, z):
    g = torch.Generator().manual_seed(2)
    p = torch.eye(4).repeat(V, 1, 1)
    p[:, :3, 3] = torch.randn(V, 3, generator=g) * 0.05
    p[:, 2, 3] += z
    return p.to(dev)


def profiled(reps, fn):
    for _ in range(3):
        fn()
    with N.LaunchProfile(8 * reps) as prof:
        for _ in range(reps):
            fn()
    return prof


def launches(n, V, reps):
    dev = torch.device("cuda", 0)
    H = W = 400
    opts = N.make_options(64, 128)
    imgs = torch.rand(V, H, W, 3, device=dev)
    poses = pose_stack(V, dev, 4.0)
    g = torch.randn(n, 11, device=dev)
    g2 = torch.randn(n, 11, device=dev)
    res = {}
    _, _, used = T.select_training_rays_views(H, W, 555.5555, poses, imgs, n, opts, seed=1, step=0)
    _, _, used1 = T.select_training_rays(H, W, 555.5555, poses[0], imgs[0], n, opts, seed=1, step=0)
    out, out1 = torch.empty(V, 3, 4, device=dev), torch.empty(3, 4, device=dev)
    prof = profiled(reps, lambda: T.select_training_rays_views(H, W, 555.5555, poses, imgs, n, opts, seed=1, step=0))
    res["select_views_us"] = kernel_us(prof, SEL)[SEL[0]]
    prof = profiled(reps, lambda: T.select_training_rays(H, W, 555.5555, poses[0], imgs[0], n, opts, seed=1, step=0))
    res["select_single_us"] = kernel_us(prof, SEL)[SEL[0]]
    prof = profiled(reps, lambda: T.select_training_rays_views_bwd(H, W, 555.5555, poses, used, g, opts, g2, out=out))
    res["views_vjp_kernels_us"] = kernel_us(prof, VJPV)
    prof = profiled(reps, lambda: T.select_training_rays_bwd(H, W, 555.5555, poses[0], used1, g, opts, g2, out=out1))
    res["single_vjp_kernels_us"] = kernel_us(prof, VJP1)
    res["views_vjp_us"] = round(sum(res["views_vjp_kernels_us"].values()), 2)
    res["single_vjp_us"] = round(sum(res["single_vjp_kernels_us"].values()), 2)
    res["views_without_a_ray"] = int((torch.bincount(used // (H * W), minlength=V) == 0).sum())
    res["finite"] = bool(torch.isfinite(out).all())
    return res


def run_line(w, steps, warmup, rays):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    mc, mf = N.FlexibleNeRFModel(**w["model"]).to(dev), N.FlexibleNeRFModel(**w["model"]).to(dev)
    H, W, V = w["H"], w["W"], w["views"]
    opts = N.make_options(w["nc"], w["nf"], no_ndc=w["no_ndc"], near=w["near"], far=w["far"], radiance_field_noise_std=w["noise"])
    imgs = torch.rand(V, H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    poses = pose_stack(V, dev, 4.0 if w["no_ndc"] else 0.0)
    res = dict(views=V)
    for arm in ("image", "views", "image_pose_grad", "views_pose_grads"):
        eng = N.TrainEngine(mc, mf, w["nc"], w["nf"], noise_std=w["noise"], lr=1e-6, world_size=1, rank=0)
        if arm.startswith("image"):
            pg = torch.empty(3, 4, device=dev) if arm.endswith("grad") else None
            step = lambda: eng.step_on_image(imgs[0], poses[0], H, W, w["focal"], opts, rays, pose_grad=pg)  # noqa: E731
        else:
            pg = torch.empty(V, 3, 4, device=dev) if arm.endswith("grads") else None
            step = lambda: eng.step_on_views(imgs, poses, H, W, w["focal"], opts, rays, pose_grads=pg)  # noqa: E731
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        res[arm + "_ms"] = round((time.perf_counter() - t0) * 1e3 / steps, 4)
        if pg is not None:
            res[arm + "_finite"] = bool(torch.isfinite(pg).all())
    res["views_cost_pct"] = round(100.0 * (res["views_ms"] / res["image_ms"] - 1.0), 2)
    res["views_pose_grads_cost_pct"] = round(100.0 * (res["views_pose_grads_ms"] / res["image_pose_grad_ms"] - 1.0), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_views.json"))
    ap.add_argument("--capability-log", default=None, help="output of pytest -s tests/test_gpu_views.py")
    a = ap.parse_args()
    out = dict(metric="views_batch_cost", rays=a.rays, steps=a.steps, reps=a.reps, launches_us={}, lines={})
    for n, V in ((4096, 1), (4096, 100), (65536, 1000)):
        out["launches_us"]["n%d_V%d" % (n, V)] = launches(n, V, a.reps)
        torch.cuda.empty_cache()
    for name, w in LINES.items():
        out["lines"][name] = run_line(w, a.steps, a.warmup, a.rays)
        torch.cuda.empty_cache()
    vjp = out["launches_us"]["n4096_V100"]["views_vjp_us"]
    out["views_vjp_pct_of_8x256_pose_grad_step"] = round(100.0 * vjp * 1e-3 / out["lines"]["lego_8x256"]["image_pose_grad_ms"], 3)
    if a.capability_log:
        with open(a.capability_log) as f:
            for ln in f:
                if "VIEWS_CAPABILITY " in ln:
                    out["capability"] = json.loads(ln[ln.index("VIEWS_CAPABILITY ") + len("VIEWS_CAPABILITY "):])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
