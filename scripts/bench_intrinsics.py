"""Cost of learned intrinsics.  (1) ms/step of TrainEngine.step_on_views(cameras=T, intrinsics=I) against step_on_views(cameras=T)
alone, for lego 8x256 and fern 4x64 at 4096 rays, the two arms alternating over two rounds (`same_arm_spread_pct`: what one arm
differs by between its rounds).  (2) The device time per launch (HIP events on the launch stream, nerfhip_profile_enable) of the two
launches the intrinsics gradient adds to the selection's VJP (k_intr_vjp_part, k_intr_vjp_sum: the <4> form of k_pose_vjp_sum) and of the three launches of
cameras.Intrinsics (values, backward, step), in the lego step.  (3) With --parent-root DIR (a checkout of the parent commit with its
library built), `parent_build`: the `cameras` arm with the package imported from there, one figure after each round of this tree's
two arms, and `bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs` of this tree and of the parent checkout, alternating over two
rounds: ms/step of each run, and the first round's dumped arrays compared on the bits (the feature unused: bench.py's step must
compute the parent build's bytes).  Every measurement runs in a child process of its own under its own time limit; the first one
that fails ends the run.  Nothing here asserts a speed.  Writes profiles/r13_intrinsics.json (and prints it as one JSON line); with
--capability-log, the error curves tests/test_gpu_intrinsics.py prints (its INTRINSICS_CAPABILITY line, pytest -s) are carried along.

    python scripts/bench_intrinsics.py [--steps 30] [--warmup 5] [--timeout 240] [--parent-root DIR] [--capability-log LOG]
                                       [--out profiles/r13_intrinsics.json]
"""
import argparse
import os

from bench_common import (LINES, ROOT, child_spec, emit, launch_costs, pair_cost, parent_bench, pose_stack, run_specs, scrape_log, timed,
                          write_out)

TAG = "BENCH_INTRINSICS_RESULT "
NEW_KERNELS = ("k_intr_vjp_part", "k_intr_vjp_sum", "k_intrinsics_fwd", "k_intrinsics_bwd")


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
    I = N.Intrinsics(H, W, w["focal"], learn="all", lr=1e-5, device=dev) if arm == "intrinsics" else None
    kw = dict(intrinsics=I) if I is not None else {}   # (the `cameras` arm also runs on the parent commit's package)
    return (lambda: eng.step_on_views(imgs, None, H, W, w["focal"], opts, rays, cameras=T, **kw)), V


def one_line(name, arm, steps, warmup, rays):
    step, V = _setup(name, arm, rays)
    res = timed(step, steps, warmup)
    res["views"] = V
    return res


def launches(name, steps, warmup, rays):
    """Device us per launch of the kernels the feature adds, over `steps` steps of the intrinsics arm (name: a line), or over
    `steps` rounds of values() / backward() / step() of a cameras.Intrinsics alone (name "object": its k_adam is the 4-float one)."""
    import torch

    import nerf_pytorch_amd as N
    if name == "object":
        I = N.Intrinsics(400, 400, 555.5555, learn="all", lr=1e-5, device=torch.device("cuda", 0))
        I.g_intr.fill_(1e-3)

        def step():
            I.values()
            I.backward()
            I.step()
    else:
        step, _ = _setup(name, "intrinsics", rays)
    return launch_costs(step, steps, warmup, NEW_KERNELS + (("k_adam",) if name == "object" else ()))


def child(spec):
    if spec["kind"] == "launches":
        res = launches(spec["line"], spec["steps"], spec["warmup"], spec["rays"])
    else:
        res = one_line(spec["line"], spec["arm"], spec["steps"], spec["warmup"], spec["rays"])
    emit(TAG, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_intrinsics.json"))
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit (library built): its `cameras` arm and bench.py")
    ap.add_argument("--capability-log", default=None, help="output of pytest -s tests/test_gpu_intrinsics.py")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(child_spec(a.child))
    out = dict(metric="learned_intrinsics_cost", rays=a.rays, steps=a.steps, lines={}, launches={})
    parent_root = os.path.abspath(a.parent_root) if a.parent_root else None
    if parent_root:
        out["parent_build"] = dict(cameras_arm={})
    specs = []
    for name in LINES:   # (the two arms alternate, two rounds each; the parent build's `cameras` arm closes each round)
        for arm in ("cameras", "intrinsics", "cameras_again", "intrinsics_again"):
            specs.append((("lines", name, arm), dict(kind="line", line=name, arm=arm.split("_again")[0], steps=a.steps, warmup=a.warmup,
                                                     rays=a.rays)))
            if parent_root and arm.startswith("intrinsics"):
                specs.append((("parent_build", "cameras_arm", name, "cameras" + arm[len("intrinsics"):]),
                              dict(kind="line", line=name, arm="cameras", steps=a.steps, warmup=a.warmup, rays=a.rays, root=parent_root)))
    specs.append((("launches", "lego_8x256"), dict(kind="launches", line="lego_8x256", steps=a.steps, warmup=a.warmup, rays=a.rays)))
    specs.append((("launches", "object"), dict(kind="launches", line="object", steps=a.steps * 10, warmup=a.warmup, rays=a.rays)))
    run_specs(__file__, TAG, specs, out, a.timeout)
    for name, r in out["lines"].items():
        if all(k in r for k in ("cameras", "intrinsics", "cameras_again", "intrinsics_again")):
            cost = pair_cost([r[k]["ms"] for k in ("intrinsics", "intrinsics_again")], [r[k]["ms"] for k in ("cameras", "cameras_again")])
            r["intrinsics_cost_pct"], r["intrinsics_cost_us"], r["same_arm_spread_pct"] = cost["cost_pct"], cost["cost_us"], cost["same_arm_spread_pct"]
    if parent_root and "stopped_at" not in out:
        parent_bench(out, parent_root, a.timeout)
    if a.capability_log:
        scrape_log(out, a.capability_log, "INTRINSICS_CAPABILITY ")
    write_out(out, a.out)


if __name__ == "__main__":
    main()
