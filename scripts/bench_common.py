"""What the scripts/bench_*.py family shares: the workloads of the camera scripts, the timed windows, the launch costs (on
nerf_pytorch_amd.LaunchProfile), the child protocol -- every measurement in a fresh process under its own time limit, no retry, the
first failure ends the run --, the two-arms-over-two-rounds cost figures, the scraper of a test log, and the comparison every
host-side change runs against its parent commit: bench.py of this tree and of a parent checkout, alternating, the dumped arrays
compared on the bits.  That comparison alone:

    python scripts/bench_common.py --parent-root DIR [--rounds 5] [--timeout 240] --out FILE

(DIR: a checkout of the parent commit with its library built.)  Writes per arm every run's ms_per_step with its median, smallest and
largest, bench.py's lib_sources_sha16 of both, and the first round's dumped arrays compared byte by byte.  Nothing here asserts a speed.
"""
import argparse
import glob
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINES = {
    "lego_8x256": dict(H=400, W=400, focal=555.5555, nc=64, nf=128, no_ndc=True, noise=0.2, near=2.0, far=6.0, views=100,
                       model=dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)),
    "fern_4x64": dict(H=378, W=504, focal=407.5, nc=64, nf=64, no_ndc=False, noise=1.0, near=0.0, far=1.0, views=20,
                      model=dict(num_layers=4, hidden_size=64, skip_connect_every=3, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)),
}
WINDOWS = 5


def pose_stack(V, dev, z):
    import torch
    g = torch.Generator().manual_seed(2)
    p = torch.eye(4).repeat(V, 1, 1)
    p[:, :3, 3] = torch.randn(V, 3, generator=g) * 0.05
    p[:, 2, 3] += z
    return p.to(dev)


# ---- measuring in this process ------------------------------------------------------------------------------------------------------
def timed(step, steps, warmup, count_kernels=True):
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


def launch_profile(reserve):
    """A LaunchProfile on the library of the package this process imported.  A parent checkout's package may predate the class: then
    this tree's module is loaded into that package, and reads that package's library."""
    import nerf_pytorch_amd as N
    if not hasattr(N, "LaunchProfile"):
        spec = importlib.util.spec_from_file_location(N.__name__ + ".launch_profile", os.path.join(ROOT, "nerf-pytorch_amd", "launch_profile.py"))
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        N.LaunchProfile = module.LaunchProfile
    return N.LaunchProfile(reserve)


def profiled(step, steps, warmup, reserve_per_step=128):
    """The LaunchProfile of `steps` calls of step() after `warmup` unprofiled ones."""
    for _ in range(warmup):
        step()
    with launch_profile(reserve_per_step * steps) as prof:
        for _ in range(steps):
            step()
    return prof


def launch_costs(step, steps, warmup, names):
    """{name: dict(launches_per_step, us_per_launch)} of the kernels of `names`: device time between two HIP events per launch."""
    return profiled(step, steps, warmup).per_launch(names, steps)


# ---- the child protocol: one measurement, one fresh process ---------------------------------------------------------------------------
def child_spec(text):
    """The spec a child was started with; spec["root"] (set by measure(root=...)) is the checkout its package is imported from."""
    spec = json.loads(text)
    if spec.get("root"):
        sys.path.insert(0, spec["root"])
    return spec


def emit(tag, res):
    print(tag + json.dumps(res))


def measure(script, tag, spec, limit, root=None):
    """Runs `script --child spec` in a fresh process under `limit` seconds, once; (what it emitted, None) or (None, reason)."""
    if root:
        spec = dict(spec, root=root)
    try:
        p = subprocess.run([sys.executable, os.path.abspath(script), "--child", json.dumps(spec)], timeout=limit, capture_output=True,
                           text=True)
    except subprocess.TimeoutExpired:
        return None, "time limit of %d s" % limit
    for ln in p.stdout.splitlines():
        if ln.startswith(tag):
            return json.loads(ln[len(tag):]), None
    return None, "exit status %d: %s" % (p.returncode, p.stderr.strip().splitlines()[-1:] or "")


def run_specs(script, tag, specs, out, limit):
    """specs: [(key path, spec)], measured in order, each result stored at its key path in `out` (out[k0][k1]...[kn]); the first one
    that fails is recorded as out["stopped_at"] and nothing more is started."""
    for key, spec in specs:
        res, why = measure(script, tag, spec, limit)
        if res is None:
            out["stopped_at"] = dict(measurement=list(key), reason=why)
            return
        at = out
        for k in key[:-1]:
            at = at.setdefault(k, {})
        at[key[-1]] = res


def pair_cost(with_ms, base_ms):
    """Two arms that alternated over rounds, as their ms per round: what the first costs over the second, in per cent and in us per
    step, and what one arm differs by between its rounds -- a difference between the arms below that is not resolved."""
    return dict(cost_pct=round(100.0 * (sum(with_ms) / sum(base_ms) - 1.0), 2),
                cost_us=round(1e3 * (sum(with_ms) - sum(base_ms)) / len(with_ms), 1),
                same_arm_spread_pct=round(100.0 * max((max(v) - min(v)) / min(v) for v in (with_ms, base_ms)), 2))


def scrape_log(out, path, tag, patterns=None):
    """A test log (pytest -s): the JSON behind its `tag` line becomes out["capability"]; returns {name: [the groups of every match
    of patterns[name]]}."""
    found = {name: [] for name in patterns or {}}
    with open(path) as f:
        for ln in f:
            if tag in ln:
                out["capability"] = json.loads(ln[ln.index(tag) + len(tag):])
            for name, pattern in (patterns or {}).items():
                m = re.search(pattern, ln)
                if m:
                    found[name].append(m.groups())
    return found


def write_out(out, path):
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


# ---- bench.py against a parent checkout ------------------------------------------------------------------------------------------------
BENCH_KEYS = ("metric", "value", "unit", "ms_per_step", "final_loss")


def bench_run(root, dump_dir, limit, keys=BENCH_KEYS):
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
            return {k: r.get(k) for k in keys}, None
    return None, "exit status %d: %s" % (p.returncode, p.stderr.strip().splitlines()[-1:] or "")


def round_name(arm, rnd):
    return arm + ("", "_again")[rnd] if rnd < 2 else "%s_%d" % (arm, rnd)


def parent_bench(out, parent_root, limit, rounds=2, keys=BENCH_KEYS):
    """bench.py of this tree and of the parent checkout, alternating over `rounds` rounds, into out["parent_build"]["bench"]; the
    first round's dumps compared on the bits."""
    import numpy as np
    pb = out["parent_build"]
    pb["bench"] = {}
    tmp = tempfile.mkdtemp(prefix="bench_parent_")
    try:
        for rnd in range(rounds):
            for arm, root in (("this", ROOT), ("parent", parent_root)):
                d = os.path.join(tmp, round_name(arm, rnd))
                res, why = bench_run(root, d, limit, keys)
                if res is None:
                    out["stopped_at"] = dict(measurement=["parent_build", "bench", round_name(arm, rnd)], reason=why)
                    return
                pb["bench"][round_name(arm, rnd)] = res
        this, parent = os.path.join(tmp, "this"), os.path.join(tmp, "parent")
        names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(this, "*.npy")))
        same = {n: bool(os.path.exists(os.path.join(parent, n)) and np.array_equal(np.load(os.path.join(this, n)).view(np.uint32),
                                                                                  np.load(os.path.join(parent, n)).view(np.uint32))) for n in names}
        pb["bench_dump_outputs_vs_parent"] = dict(arrays=len(names), identical_bytes=same, all_identical=bool(names) and all(same.values()))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True, help="checkout of the parent commit (library built)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per bench.py run")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    out = dict(metric="bench_vs_parent", rounds=a.rounds, parent_build={},
               command="python bench.py --gpus 1 --steps 20 --warmup 3 --no-labelled-lines --no-cpu-baseline --dump-outputs DIR")
    parent_bench(out, os.path.abspath(a.parent_root), a.timeout, a.rounds, BENCH_KEYS + ("lib_sources_sha16",))
    runs = out["parent_build"]["bench"]
    out["arms"], out["lib_sources_sha16"] = {}, {}
    for arm in ("this", "parent"):
        mine = [runs[k] for k in (round_name(arm, rnd) for rnd in range(a.rounds)) if k in runs]
        ms = [r["ms_per_step"] for r in mine]
        sha = sorted({str(r["lib_sources_sha16"]) for r in mine})
        out["lib_sources_sha16"][arm] = sha[0] if len(sha) == 1 else sha     # (one string: every run of the arm saw the same sources)
        out["arms"][arm] = dict(ms_per_step=ms, median=sorted(ms)[len(ms) // 2] if ms else None, min=min(ms, default=None),
                                max=max(ms, default=None))
    if "stopped_at" not in out:
        p, t = out["arms"]["parent"], out["arms"]["this"]
        spread = p["max"] - p["min"]
        # the parent's own runs of this session set the allowance: its [min, max], widened on each side by (max - min)
        out["this_median_within_parent_min_max_widened_by_its_spread"] = bool(p["min"] - spread <= t["median"] <= p["max"] + spread)
        out["parent_allowance_ms_per_step"] = [round(p["min"] - spread, 3), round(p["max"] + spread, 3)]
    write_out(out, a.out)


if __name__ == "__main__":
    main()
