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
import ctypes
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_cameras import LINES, _timed, pose_stack  # noqa: E402

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
    res = _timed(step, steps, warmup)
    res["views"] = V
    return res


def launches(name, steps, warmup, rays):
    """Device us per launch of the kernels the feature adds, over `steps` steps of the intrinsics arm (name: a line), or over
    `steps` rounds of values() / backward() / step() of a cameras.Intrinsics alone (name "object": its k_adam is the 4-float one)."""
    import torch

    import nerf_pytorch_amd as N
    lib = N._lib.get_lib()
    if name == "object":
        I = N.Intrinsics(400, 400, 555.5555, learn="all", lr=1e-5, device=torch.device("cuda", 0))
        I.g_intr.fill_(1e-3)

        def step():
            I.values()
            I.backward()
            I.step()
    else:
        step, _ = _setup(name, "intrinsics", rays)
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
        if len(parts) == 3 and parts[0] in NEW_KERNELS + (("k_adam",) if name == "object" else ()):
            out[parts[0]] = dict(launches_per_step=round(int(parts[1]) / steps, 2), us_per_launch=round(1e3 * float(parts[2]) / int(parts[1]), 2))
    return out


def child(spec):
    if spec.get("root"):   # (the package of another checkout: the parent commit's build)
        sys.path.insert(0, spec["root"])
    if spec["kind"] == "launches":
        res = launches(spec["line"], spec["steps"], spec["warmup"], spec["rays"])
    else:
        res = one_line(spec["line"], spec["arm"], spec["steps"], spec["warmup"], spec["rays"])
    print(TAG + json.dumps(res))


def bench_run(root, dump_dir, limit):
    """`bench.py --dump-outputs dump_dir` of the checkout `root` in a process of its own: (its result line, None) or (None, reason)."""
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3", "--no-labelled-lines",
           "--no-cpu-baseline", "--dump-outputs", dump_dir]
    try:
        p = subprocess.run(cmd, cwd=root, timeout=limit, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        return None, "time limit of %d s" % limit
    for ln in p.stdout.splitlines():
        if ln.startswith("{"):
            r = json.loads(ln)
            return {k: r.get(k) for k in ("metric", "value", "unit", "ms_per_step", "final_loss")}, None
    return None, "exit status %d: %s" % (p.returncode, p.stderr.strip().splitlines()[-1:] or "")


def parent_bench(out, parent_root, limit):
    """bench.py of this tree and of the parent checkout, alternating over two rounds; the first round's dumps compared on the bits."""
    import numpy as np
    pb = out["parent_build"]
    pb["bench"] = {}
    tmp = tempfile.mkdtemp(prefix="bench_intrinsics_")
    try:
        for rnd in ("", "_again"):
            for arm, root in (("this", ROOT), ("parent", parent_root)):
                d = os.path.join(tmp, arm + rnd)
                res, why = bench_run(root, d, limit)
                if res is None:
                    out["stopped_at"] = dict(measurement=["parent_build", "bench", arm + rnd], reason=why)
                    return
                pb["bench"][arm + rnd] = res
        this, parent = os.path.join(tmp, "this"), os.path.join(tmp, "parent")
        names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(this, "*.npy")))
        same = {n: bool(os.path.exists(os.path.join(parent, n)) and np.array_equal(np.load(os.path.join(this, n)).view(np.uint32),
                                                                                  np.load(os.path.join(parent, n)).view(np.uint32))) for n in names}
        pb["bench_dump_outputs_vs_parent"] = dict(arrays=len(names), identical_bytes=same, all_identical=bool(names) and all(same.values()))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_intrinsics.json"))
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit (library built): its `cameras` arm and bench.py")
    ap.add_argument("--capability-log", default=None, help="output of pytest -s tests/test_gpu_intrinsics.py")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(json.loads(a.child))
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
                specs.append((("parent_build", name, "cameras" + arm[len("intrinsics"):]),
                              dict(kind="line", line=name, arm="cameras", steps=a.steps, warmup=a.warmup, rays=a.rays, root=parent_root)))
    specs.append((("launches", "lego_8x256", None), dict(kind="launches", line="lego_8x256", steps=a.steps, warmup=a.warmup, rays=a.rays)))
    specs.append((("launches", "object", None), dict(kind="launches", line="object", steps=a.steps * 10, warmup=a.warmup, rays=a.rays)))
    for (top, mid, arm), spec in specs:
        res, why = measure(spec, a.timeout)
        if res is None:
            out["stopped_at"] = dict(measurement=[top, mid, arm], reason=why)
            break
        if arm is None:
            out[top][mid] = res
        elif top == "parent_build":
            out[top]["cameras_arm"].setdefault(mid, {})[arm] = res
        else:
            out[top].setdefault(mid, {})[arm] = res
    for name, r in out["lines"].items():
        if all(k in r for k in ("cameras", "intrinsics", "cameras_again", "intrinsics_again")):
            intr, cam = [r[k]["ms"] for k in ("intrinsics", "intrinsics_again")], [r[k]["ms"] for k in ("cameras", "cameras_again")]
            r["intrinsics_cost_pct"] = round(100.0 * (sum(intr) / sum(cam) - 1.0), 2)
            r["intrinsics_cost_us"] = round(1e3 * (sum(intr) - sum(cam)) / 2, 1)
            # what the same arm differs by between its two rounds: a difference between the arms below this is not resolved
            r["same_arm_spread_pct"] = round(100.0 * max(abs(intr[0] - intr[1]) / min(intr), abs(cam[0] - cam[1]) / min(cam)), 2)
    if parent_root and "stopped_at" not in out:
        parent_bench(out, parent_root, a.timeout)
    if a.capability_log:
        with open(a.capability_log) as f:
            for ln in f:
                if "INTRINSICS_CAPABILITY " in ln:
                    out["capability"] = json.loads(ln[ln.index("INTRINSICS_CAPABILITY ") + len("INTRINSICS_CAPABILITY "):])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
