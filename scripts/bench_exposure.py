"""Cost of the per-view exposure.  (1) ms/step at 4096 rays, for lego 8x256 (100 views) and fern 4x64 NDC (20 views), of
TrainEngine.step_on_views with and without exposure=X (`plain` / `exposure`, X = Exposure(V, learn="affine")), of the same pair with
cameras=T, intrinsics=I, distortion=D on both sides (`cameras` / `cameras_exposure`: the exposure's grouping launch runs next to the
pose VJP's), and of localize_on_views(exposure=X) alone (`fit`: the test-time fit, no render backward); the arms of a pair alternate
over two rounds (`same_arm_spread_pct`: what one arm differs by between its rounds).  (2) The device time per launch (HIP events on
the launch stream, nerfhip_profile_enable) of the loss (k_mse_loss in the `plain` step, k_mse_loss_views under the table),
k_pose_views_group, k_expo_part, k_expo_sum and k_adam in the `plain`, `exposure` and `cameras_exposure` steps of both lines.
(3) With --parent-root DIR (a checkout of the parent commit with its library built), `parent_build`: `bench.py --gpus 1 --steps 20
--warmup 3 --dump-outputs` of this tree and of the parent checkout, alternating over two rounds, the first round's dumped arrays
compared on the bits (the feature unused: bench.py's step must compute the parent build's bytes).  Every measurement runs in a
child process of its own under its own time limit; the first one that fails ends the run.  Nothing here asserts a speed.  Writes
profiles/r15_exposure.json (and prints it as one JSON line); with --test-log, what tests/test_gpu_exposure.py prints under
pytest -s is carried along: its EXPOSURE_CAPABILITY line (both error curves) and the worst measured error over the bound of g_rgb
and g_expo in the kernel cases.

    python scripts/bench_exposure.py [--steps 30] [--warmup 5] [--timeout 240] [--parent-root DIR] [--test-log LOG]
                                     [--out profiles/r15_exposure.json]
"""
import argparse
import os

from bench_common import (LINES, ROOT, child_spec, emit, launch_costs, pair_cost, parent_bench, pose_stack, run_specs, scrape_log, timed,
                          write_out)

TAG = "BENCH_EXPOSURE_RESULT "
KERNELS = ("k_mse_loss", "k_mse_loss_views", "k_pose_views_group", "k_expo_part", "k_expo_sum", "k_adam")
PAIRS = (("plain", "exposure"), ("cameras", "cameras_exposure"))


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
    poses = pose_stack(V, dev, 4.0 if w["no_ndc"] else 0.0)
    kw = {}
    if arm in ("exposure", "cameras_exposure", "fit"):
        kw["exposure"] = N.Exposure(V, learn="affine", lr=1e-6, device=dev)
    if arm.startswith("cameras"):
        kw.update(cameras=N.CameraTable(poses, lr=1e-4), intrinsics=N.Intrinsics(H, W, w["focal"], learn="all", lr=1e-5, device=dev),
                  distortion=N.Distortion((-0.05, 0.01, 1e-3, -1e-3), learn="all", lr=1e-6, device=dev))
        poses = None
    if arm == "fit":
        return (lambda: eng.localize_on_views(imgs, poses, H, W, w["focal"], opts, rays, **kw)), V
    return (lambda: eng.step_on_views(imgs, poses, H, W, w["focal"], opts, rays, **kw)), V


def one_line(name, arm, steps, warmup, rays):
    step, V = _setup(name, arm, rays)
    res = timed(step, steps, warmup)
    res["views"] = V
    return res


def launches(name, arm, steps, warmup, rays):
    """Device us per launch of the loss and of the table gradient's kernels over `steps` steps of the arm."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_exposure.json"))
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit (library built): its bench.py")
    ap.add_argument("--test-log", default=None, help="output of pytest -s tests/test_gpu_exposure.py")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(child_spec(a.child))
    out = dict(metric="per_view_exposure_cost", rays=a.rays, steps=a.steps, lines={}, launches={})
    parent_root = os.path.abspath(a.parent_root) if a.parent_root else None
    if parent_root:
        out["parent_build"] = {}
    specs = []
    for name in LINES:   # (the two arms of a pair alternate, two rounds each; then the fit alone, twice)
        order = [arm + rnd for base, with_x in PAIRS for rnd in ("", "_again") for arm in (base, with_x)] + ["fit", "fit_again"]
        for arm in order:
            specs.append((("lines", name, arm), dict(kind="line", line=name, arm=arm.split("_again")[0], steps=a.steps, warmup=a.warmup,
                                                     rays=a.rays)))
    for name in LINES:
        for arm in ("plain", "exposure", "cameras_exposure"):
            specs.append((("launches", name, arm), dict(kind="launches", line=name, arm=arm, steps=a.steps, warmup=a.warmup, rays=a.rays)))
    run_specs(__file__, TAG, specs, out, a.timeout)
    for name, r in out["lines"].items():
        for base, with_x in PAIRS:
            if all(k + rnd in r for k in (base, with_x) for rnd in ("", "_again")):
                cost = pair_cost([r[with_x + rnd]["ms"] for rnd in ("", "_again")], [r[base + rnd]["ms"] for rnd in ("", "_again")])
                r.update({with_x + "_" + k: v for k, v in cost.items()})
    if parent_root and "stopped_at" not in out:
        parent_bench(out, parent_root, a.timeout)
        b = out["parent_build"].get("bench", {})
        if all(k in b for k in ("this", "parent", "this_again", "parent_again")):
            t, p = [b[k]["ms_per_step"] for k in ("this", "this_again")], [b[k]["ms_per_step"] for k in ("parent", "parent_again")]
            if all(v is not None for v in t + p):
                cost = pair_cost(t, p)
                out["parent_build"]["bench_this_over_parent_pct"] = cost["cost_pct"]
                out["parent_build"]["bench_same_arm_spread_pct"] = cost["same_arm_spread_pct"]
    if a.test_log:
        worst = {}
        for what, ratio in scrape_log(out, a.test_log, "EXPOSURE_CAPABILITY ",
                                      dict(worst=r"(g_rgb|g_expo) worst error / bound ([0-9.eE+-]+)"))["worst"]:
            worst[what] = max(worst.get(what, 0.0), float(ratio))
        if worst:
            out["kernel_cases_worst_error_over_bound"] = worst
    write_out(out, a.out)


if __name__ == "__main__":
    main()
