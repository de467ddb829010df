"""What the occupancy grid buys the inference render: rays/s of the validation render of the lego-lowres fixture
nets (4 x 128, 64 + 64 samples, white background, the fixture pose at 400 x 400 and 800 x 800) without and with the grid of
OccupancyGrid.from_models at its defaults over [-1.5, 1.5]^3, fp32 and fp16 pieces; the kept fractions, the grid's build time, PSNR
and max abs of rgb_fine against the dense render, and the per-launch times of the new small kernels next to the two forwards.

The two arms alternate over ROUNDS rounds in one process; a timed window is at least REPEATS renders and at least MIN_WINDOW_S of
work (sized from one timed render after WARMUP renders of the same shape) and ends in a device synchronise; the kept fractions are
the view's (OccupancyGrid.view_counts: summed over its ray chunks); `same_arm_spread_pct` is what one arm differs by between its rounds -- a difference between
the arms below it is not resolved.  The kernel times come from a pass of their own under the library's launch profile
(nerfhip_profile_enable), never from the timed windows.

--bench-eval: also the plain `bench.py --mode eval` line of this tree, and with --parent-root DIR (a checkout of the parent commit
with its library built) the parent's, alternating, each in a child process under its own time limit: the dense path must be
unchanged.  Reported, not asserted: nothing here fails on a number.  Writes profiles/r16_occupancy.json (and prints it as one line).

    python scripts/bench_occupancy.py [--sizes 400 800] [--rounds 3] [--repeats 3] [--bench-eval [--no-render]] [--parent-root DIR] [--out FILE]
    python scripts/bench_occupancy.py --merge-only --parity-record PATH/parity_small_cases.json   # + the GPU suite's capability entry
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CFG = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
AABB = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
WARMUP = 2
MIN_WINDOW_S = 0.5


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def render_arms(sizes, rounds, repeats):
    import numpy as np
    import torch

    import nerf_pytorch_amd as N
    if not torch.cuda.is_available():
        raise SystemExit("bench_occupancy needs the GPU: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    gold = os.path.join(ROOT, "tests", "golden")
    w, r = np.load(os.path.join(gold, "lego_lowres_weights.npz")), np.load(os.path.join(gold, "lego_lowres_render.npz"))
    mc, mf = N.FlexibleNeRFModel(**CFG), N.FlexibleNeRFModel(**CFG)
    mc.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("c_")})
    mf.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("f_")})
    mc, mf = mc.to(dev), mf.to(dev)
    pose = torch.from_numpy(r["pose"]).to(dev)
    ex, ed = N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)
    opts = N.make_options(64, 64, perturb=False, white_background=True, radiance_field_noise_std=0.0)
    rec = {}
    for arith in ("fp32", "f16x3"):
        mc.set_inference_precision(arith), mf.set_inference_precision(arith)
        # the grid: built twice, the second build timed (the first loads the code objects)
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            grid = N.OccupancyGrid.from_models(mc, mf, AABB)
            torch.cuda.synchronize()
            build_ms = (time.perf_counter() - t0) * 1e3
        a = rec[arith] = dict(grid_build_ms=round(build_ms, 2), occupied_fraction=grid.occupied_fraction(), resolution=list(grid.resolution))
        for side in sizes:
            focal = float(r["focal"]) * side / float(r["W"])

            def render(occ):
                with torch.no_grad():
                    return N.render_pose_rows(side, side, focal, pose, mc, mf, opts, ex, ed, occupancy=occ)[0]

            def window(occ, reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    render(occ)
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            reps = {}
            for name, occ in (("dense", None), ("grid", grid)):
                for _ in range(WARMUP):
                    render(occ)
                # enough renders per timed window for MIN_WINDOW_S of work (a shorter one measures the clock and the scheduler)
                reps[name] = max(repeats, int(MIN_WINDOW_S / window(occ, 1)) + 1)
            dense, got = render(None), render(grid)
            kc, tc, kf, tf = (int(v) for v in grid.view_counts.tolist())  # summed over every ray chunk of the view
            assert tc == side * side * 64 and tf == side * side * 128
            mse = float(((got[3] - dense[3]).double() ** 2).mean())
            rates, secs = {"dense": [], "grid": []}, {"dense": [], "grid": []}
            for _ in range(rounds):  # (the arms alternate)
                for name, occ in (("dense", None), ("grid", grid)):
                    secs[name].append(window(occ, reps[name]))
                    rates[name].append(side * side * reps[name] / secs[name][-1])
            # per-launch kernel times: a pass of its own under the launch profile
            kernels = {}
            for name, occ in (("dense", None), ("grid", grid)):
                with N.LaunchProfile() as prof:
                    render(occ)
                kernels[name] = {k: dict(launches=launches, ms_per_launch=round(ms / launches, 4)) for k, (launches, ms) in prof.rows.items()}
            spread = max((max(v) - min(v)) / median(v) for v in rates.values()) * 100.0
            a["%dx%d" % (side, side)] = dict(
                rays_per_s_dense=round(median(rates["dense"])), rays_per_s_grid=round(median(rates["grid"])),
                rays_per_s_dense_all=[round(v) for v in rates["dense"]], rays_per_s_grid_all=[round(v) for v in rates["grid"]],
                ratio=round(median(rates["grid"]) / median(rates["dense"]), 3), same_arm_spread_pct=round(spread, 2),
                kept_coarse=kc / tc, kept_fine=kf / tf, psnr_rgb_fine_db=round(-10 * np.log10(max(mse, 1e-30)), 2),
                max_abs_rgb_fine=float((got[3] - dense[3]).abs().max()), kernels=kernels, rounds=rounds, warmup=WARMUP,
                renders_per_window=reps, window_s={k: [round(v, 3) for v in secs[k]] for k in secs},
                ray_chunks=[min(opts.nerf.validation.chunksize, side * side - c) for c in range(0, side * side, opts.nerf.validation.chunksize)],
                kernels_note="ms_per_launch: mean over the launches of ONE render of the view, i.e. over its ray chunks (ray_chunks: the last "
                             "one is partial) and both passes")
    return rec


def bench_eval(root, timeout):
    """One `bench.py --mode eval` line of the tree at `root`, in a child process under its own time limit."""
    try:
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--mode", "eval", "--steps", "3", "--warmup", "1",
                            "--no-labelled-lines", "--no-cpu-baseline"], cwd=root, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return dict(error="time limit of %d s" % timeout)
    if p.returncode != 0:
        return dict(error="exit status %d" % p.returncode, stderr=p.stderr[-400:])
    for line in reversed(p.stdout.splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    return dict(error="no JSON line")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[400, 800])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bench-eval", action="store_true")
    ap.add_argument("--no-render", action="store_true", help="skip the render arms (with --bench-eval: the eval lines alone)")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--parity-record", default=None, help="the suite's parity record (parity_small_cases.json, which tests/conftest.py writes at the end of a GPU session): its "
                                                          "occupancy_capability_gpu entry is copied in")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_occupancy.json"))
    ap.add_argument("--merge-only", action="store_true", help="no measurement: copy --parity-record's entry into the existing --out")
    args = ap.parse_args()
    if args.merge_only:
        with open(args.out) as f:
            rec = json.load(f)
        with open(args.parity_record) as f:
            rec["capability_test"] = json.load(f)["occupancy_capability_gpu"]
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
        return
    rec = {}
    if args.no_render and os.path.exists(args.out):  # (the eval lines alone, into an existing record)
        with open(args.out) as f:
            rec = json.load(f)
    if not args.no_render:
        rec = dict(what="validation render of the lego-lowres fixture nets (4x128, 64 + 64, white background, fixture pose), dense vs "
                        "OccupancyGrid.from_models defaults over [-1.5, 1.5]^3", render=render_arms(args.sizes, args.rounds, args.repeats))
    if args.bench_eval:
        lines = {"this_tree": [], "parent": []}
        for _ in range(2):  # (alternating)
            lines["this_tree"].append(bench_eval(ROOT, args.timeout))
            if args.parent_root:
                lines["parent"].append(bench_eval(os.path.abspath(args.parent_root), args.timeout))
        rec["bench_eval"] = lines
    if args.parity_record and os.path.exists(args.parity_record):
        with open(args.parity_record) as f:
            rec["capability_test"] = json.load(f).get("occupancy_capability_gpu")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
