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
import ctypes
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_cameras import LINES, _timed, pose_stack  # noqa: E402
from bench_intrinsics import parent_bench  # noqa: E402

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
    res = _timed(step, steps, warmup)
    res["views"] = V
    return res


def launches(name, arm, steps, warmup, rays):
    """Device us per launch of the selection and of the VJP's kernels over `steps` steps of the arm."""
    import torch

    import nerf_pytorch_amd as N
    lib = N._lib.get_lib()
    step, _ = _setup(name, arm, rays)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    lib.profile_reserve(128 * steps)
    lib.profile_enable(1)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    lib.profile_enable(0)
    buf = ctypes.create_string_buffer(1 << 16)
    lib.profile_report(buf, len(buf))
    out = {}
    for ln in buf.value.decode().splitlines():
        parts = ln.rsplit(None, 2)
        if len(parts) == 3 and parts[0] in KERNELS:
            out[parts[0]] = dict(launches_per_step=round(int(parts[1]) / steps, 2), us_per_launch=round(1e3 * float(parts[2]) / int(parts[1]), 2))
    return out


def child(spec):
    if spec.get("root"):   # (the package of another checkout: the parent commit's build)
        sys.path.insert(0, spec["root"])
    if spec["kind"] == "launches":
        res = launches(spec["line"], spec["arm"], spec["steps"], spec["warmup"], spec["rays"])
    else:
        res = one_line(spec["line"], spec["arm"], spec["steps"], spec["warmup"], spec["rays"])
    print(TAG + json.dumps(res))


def measure(spec, limit):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_distortion.json"))
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit (library built): its `intrinsics` arm and bench.py")
    ap.add_argument("--test-log", default=None, help="output of pytest -s tests/test_gpu_distortion.py")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(json.loads(a.child))
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
                specs.append((("parent_build", name, "intrinsics" + arm[len("distortion"):]),
                              dict(kind="line", line=name, arm="intrinsics", steps=a.steps, warmup=a.warmup, rays=a.rays, root=parent_root)))
    for arm in ("intrinsics", "distortion"):
        specs.append((("launches", "lego_8x256", arm), dict(kind="launches", line="lego_8x256", arm=arm, steps=a.steps, warmup=a.warmup,
                                                            rays=a.rays)))
    for (top, mid, arm), spec in specs:
        res, why = measure(spec, a.timeout)
        if res is None:
            out["stopped_at"] = dict(measurement=[top, mid, arm], reason=why)
            break
        if top == "parent_build":
            out[top]["intrinsics_arm"].setdefault(mid, {})[arm] = res
        else:
            out[top].setdefault(mid, {})[arm] = res
    for name, r in out["lines"].items():
        if all(k in r for k in ARMS):
            dist, intr = [r[k]["ms"] for k in ("distortion", "distortion_again")], [r[k]["ms"] for k in ("intrinsics", "intrinsics_again")]
            r["distortion_cost_pct"] = round(100.0 * (sum(dist) / sum(intr) - 1.0), 2)
            r["distortion_cost_us"] = round(1e3 * (sum(dist) - sum(intr)) / 2, 1)
            # what the same arm differs by between its two rounds: a difference between the arms below this is not resolved
            r["same_arm_spread_pct"] = round(100.0 * max(abs(dist[0] - dist[1]) / min(dist), abs(intr[0] - intr[1]) / min(intr)), 2)
    if parent_root and "stopped_at" not in out:
        parent_bench(out, parent_root, a.timeout)
    if a.test_log:
        ratios = []
        with open(a.test_log) as f:
            for ln in f:
                if "DISTORTION_CAPABILITY " in ln:
                    out["capability"] = json.loads(ln[ln.index("DISTORTION_CAPABILITY ") + len("DISTORTION_CAPABILITY "):])
                m = re.search(r"distortion rows vs fp64 \((.*)\): worst error / bound = ([0-9.]+)", ln)
                if m:
                    ratios.append(dict(case=m.group(1), error_over_bound=float(m.group(2))))
        if ratios:
            out["forward_rows_vs_fp64"] = dict(cases=ratios, worst_error_over_bound=max(r["error_over_bound"] for r in ratios))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
