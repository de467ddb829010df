"""Cost of lens distortion.  (1) ms/step of TrainEngine.step_on_views(cameras=T, intrinsics=I, distortion=D) against
step_on_views(cameras=T, intrinsics=I) alone, for lego 8x256 and fern 4x64 at 4096 rays, the two arms alternating over two rounds
(`same_arm_spread_pct`: what one arm differs by between its rounds).  (2) The device time per launch (HIP events on the launch stream,
nerfhip_profile_enable) of k_select_rays with and without `dist` and of the VJP's launches (k_dist_vjp_part, k_dist_vjp_sum, and the
pose and intrinsics launches that run the solve when `dist` is given), in the lego step.  (3) With --parent-root DIR (a checkout of
the parent commit with its library built), `parent_build`: the `intrinsics` arm with the package imported from there, one figure
after each round of this tree's two arms, and `bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs` of this tree and of the parent
checkout, alternating over two rounds, the first round's dumped arrays compared on the bits (the feature unused: bench.py's step must
compute the parent build's bytes).  Every measurement runs in a child process of its own under its own time limit; the first one
that fails ends the run.  Nothing here asserts a speed.  Writes profiles/r14_distortion.json (and prints it as one JSON line); with
--test-log, what tests/test_gpu_distortion.py prints under pytest -s is carried along: its DISTORTION_CAPABILITY line (both error
curves) and the worst measured error over the bound of the forward rows.

    python scripts/bench_distortion.py [--steps 30] [--warmup 5] [--timeout 240] [--parent-root DIR] [--test-log LOG]
                                       [--out profiles/r14_distortion.json]
"""
import argparse
import os

from bench_common import (LINES, ROOT, child_spec, emit, launch_costs, pair_cost, parent_bench, pose_stack, run_specs, scrape_log, timed,
                          write_out)

TAG = "BENCH_DISTORTION_RESULT "
KERNELS = ("k_select_rays", "k_dist_vjp_part", "k_dist_vjp_sum", "k_intr_vjp_part", "k_intr_vjp_sum", "k_pose_views_part", "k_pose_vjp_sum")
ARMS = ("intrinsics", "distortion", "intrinsics_again", "distortion_again")


def _setup(name, arm, rays):
    import torch

    import nerf_pytorch_amd as N
    w = LINES[name]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    mc, mf = N.FlexibleNeRFModel(**w["model"]).to(dev), N.FlexibleNeRFModel(**w["model"]).to(dev)
    H, W, V = w["H"], w["W"], w["views"]
    opts = N.make_options(w["nc"], w["nf"], no_ndc=w["no_ndc"], near=w["near"], far=w["far"], radiance_field_noise_std=w["noise"])
    imgs = torch.rand(V, H, W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    eng = N.TrainEngine(mc, mf, w["nc"], w["nf"], noise_std=w["noise"], lr=1e-6, world_size=1, rank=0)
    T = N.CameraTable(pose_stack(V, dev, 4.0 if w["no_ndc"] else 0.0), lr=1e-4)
    I = N.Intrinsics(H, W, w["focal"], learn="all", lr=1e-5, device=dev)
    kw = {}   # (the `intrinsics` arm also runs on the parent commit's package)
    if arm == "distortion":
        kw = dict(distortion=N.Distortion((-0.05, 0.01, 1e-3, -1e-3), learn="all", lr=1e-6, device=dev))
    return (lambda: eng.step_on_views(imgs, None, H, W, w["focal"], opts, rays, cameras=T, intrinsics=I, **kw)), V


def one_line(name, arm, steps, warmup, rays):
    step, V = _setup(name, arm, rays)
    res = timed(step, steps, warmup)
    res["views"] = V
    return res


def launches(name, arm, steps, warmup, rays):
    """Device us per launch of the selection and of the VJP's kernels over `steps` steps of the arm."""
    step, _ = _setup(name, arm, rays)
    return launch_costs(step, steps, warmup, KERNELS)


def child(spec):
    if spec["kind"] == "launches":
        res = launches(spec["line"], spec["arm"], spec["steps"], spec["warmup"], spec["rays"])
    else:
        res = one_line(spec["line"], spec["arm"], spec["steps"], spec["warmup"], spec["rays"])
    emit(TAG, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_distortion.json"))
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit (library built): its `intrinsics` arm and bench.py")
    ap.add_argument("--test-log", default=None, help="output of pytest -s tests/test_gpu_distortion.py")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(child_spec(a.child))
    out = dict(metric="lens_distortion_cost", rays=a.rays, steps=a.steps, lines={}, launches={})
    parent_root = os.path.abspath(a.parent_root) if a.parent_root else None
    if parent_root:
        out["parent_build"] = dict(intrinsics_arm={})
    specs = []
    for name in LINES:   # (the two arms alternate, two rounds each; the parent build's `intrinsics` arm closes each round)
        for arm in ARMS:
            specs.append((("lines", name, arm), dict(kind="line", line=name, arm=arm.split("_again")[0], steps=a.steps, warmup=a.warmup,
                                                     rays=a.rays)))
            if parent_root and arm.startswith("distortion"):
                specs.append((("parent_build", "intrinsics_arm", name, "intrinsics" + arm[len("distortion"):]),
                              dict(kind="line", line=name, arm="intrinsics", steps=a.steps, warmup=a.warmup, rays=a.rays, root=parent_root)))
    for arm in ("intrinsics", "distortion"):
        specs.append((("launches", "lego_8x256", arm), dict(kind="launches", line="lego_8x256", arm=arm, steps=a.steps, warmup=a.warmup,
                                                            rays=a.rays)))
    run_specs(__file__, TAG, specs, out, a.timeout)
    for name, r in out["lines"].items():
        if all(k in r for k in ARMS):
            cost = pair_cost([r[k]["ms"] for k in ("distortion", "distortion_again")], [r[k]["ms"] for k in ("intrinsics", "intrinsics_again")])
            r["distortion_cost_pct"], r["distortion_cost_us"], r["same_arm_spread_pct"] = cost["cost_pct"], cost["cost_us"], cost["same_arm_spread_pct"]
    if parent_root and "stopped_at" not in out:
        parent_bench(out, parent_root, a.timeout)
    if a.test_log:
        rows = scrape_log(out, a.test_log, "DISTORTION_CAPABILITY ",
                          dict(rows=r"distortion rows vs fp64 \((.*)\): worst error / bound = ([0-9.]+)"))["rows"]
        ratios = [dict(case=case, error_over_bound=float(ratio)) for case, ratio in rows]
        if ratios:
            out["forward_rows_vs_fp64"] = dict(cases=ratios, worst_error_over_bound=max(r["error_over_bound"] for r in ratios))
    write_out(out, a.out)


if __name__ == "__main__":
    main()
