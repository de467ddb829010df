"""Cost record of localisation on frozen nets: TrainEngine.localize_on_views(pose_grads=...) (the ray gradient alone,
nerfhip_render_grad_rays) against what stood in for it, step_on_views(lr=0.0, pose_grads=...) (the whole training backward and an
Adam step at lr 0).

Workloads: 4096 rays on lego 8x256 (64+128), lego 4x128 (64+64) and fern 4x64 in NDC (64+64).  The two arms alternate over ROUNDS
rounds, every figure in a child process of its own under its own time limit, WINDOWS timed windows of --steps steps per figure
(median, smallest, largest); `same_arm_spread_pct` is what one arm differs by between its rounds -- a difference between the arms
below it is not resolved.  With --parent-root DIR (a checkout of the parent commit with its library built) the step_on_views arm
imports the package from there: the parent commit's build; without it, it is this build's unchanged trainable path, and the record
says which.  Each child also records per-launch event times of its ray-gradient stage -- k_point_grad_pack + k_point_grad +
k_ray_grad_sum (+ k_point_grad_zero over a list) here, k_mlp_input_grad + k_ray_grad + k_zero_floats there -- and, for the new stage,
its algorithmic HBM bytes (each term's d(pre-activation) rows once, the rays' and depths' reads, the [M][8] store and its read-back)
as a fraction of the 6.3 TB/s DESIGN.md calls achievable.  --capability-log FILE carries the LOCALIZE_CAPABILITY line of
tests/test_gpu_localize.py (both recovery curves) into the record; --dump-outputs-dirs THIS PARENT compares two `bench.py
--dump-outputs` directories (this tree's and the parent build's, the feature unused) array by array on the bits.  Reported, not asserted: nothing here fails on a number.

Writes profiles/rNN_localize.json under the next free round number (and prints it as one JSON line).

    python scripts/bench_localize.py [--steps 30] [--warmup 5] [--timeout 240] [--parent-root DIR] [--capability-log FILE]
                                       [--dump-outputs-dirs THIS PARENT] [--out FILE]
"""
import argparse
import glob
import json
import os
import re
import time

from bench_common import ROOT, child_spec, emit, measure, profiled

LINES = {
    "lego_8x256": dict(H=400, W=400, focal=555.5555, nc=64, nf=128, no_ndc=True, noise=0.2, near=2.0, far=6.0,
                       model=dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)),
    "lego_4x128": dict(H=400, W=400, focal=555.5555, nc=64, nf=64, no_ndc=True, noise=0.2, near=2.0, far=6.0,
                       model=dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)),
    "fern_4x64": dict(H=378, W=504, focal=407.5, nc=64, nf=64, no_ndc=False, noise=1.0, near=0.0, far=1.0,
                      model=dict(num_layers=4, hidden_size=64, skip_connect_every=3, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)),
}
STAGE = {"localize": ("k_point_grad_pack", "k_point_grad", "k_ray_grad_sum", "k_point_grad_zero"),
         "step_lr0": ("k_mlp_input_grad", "k_ray_grad", "k_zero_floats")}
TAG = "BENCH_LOCALIZE_RESULT "
WINDOWS, ROUNDS, VIEWS = 5, 2, 2
HBM_TBPS = 6.3


def stage_bytes(model, rays, nc, nf):
    """Algorithmic HBM bytes of k_point_grad + k_ray_grad_sum over both passes: the real units of every term's image rows once, z and
    the ray row per sample, the 32-byte store and its read-back."""
    H, L, skip = model["hidden_size"], model["num_layers"], model["skip_connect_every"]
    units = H + sum(H for i in range(L - 1) if i % skip == 0 and i > 0) + H // 2
    per_sample = 4 * units + 4 + 4 * 11 + 32 + 32 + 4
    return per_sample * rays * (nc + (nc + nf))


def one_line(name, arm, steps, warmup, rays):
    import torch

    import nerf_pytorch_amd as N
    w = LINES[name]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    mc, mf = N.FlexibleNeRFModel(**w["model"]).to(dev), N.FlexibleNeRFModel(**w["model"]).to(dev)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)
    Hh, Ww = w["H"], w["W"]
    opts = N.make_options(w["nc"], w["nf"], no_ndc=w["no_ndc"], near=w["near"], far=w["far"], radiance_field_noise_std=w["noise"])
    imgs = torch.rand(VIEWS, Hh, Ww, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    poses = torch.eye(4, device=dev).repeat(VIEWS, 1, 1).contiguous()
    poses[:, 2, 3] = 4.0 if w["no_ndc"] else 0.0
    poses[1, 0, 3] = 0.1
    pg = torch.empty(VIEWS, 3, 4, device=dev)
    eng = N.TrainEngine(mc, mf, w["nc"], w["nf"], noise_std=w["noise"], lr=0.0, world_size=1, rank=0)
    if arm == "localize":
        step = lambda: eng.localize_on_views(imgs, poses, Hh, Ww, w["focal"], opts, rays, pose_grads=pg)  # noqa: E731
    else:
        step = lambda: eng.step_on_views(imgs, poses, Hh, Ww, w["focal"], opts, rays, lr=0.0, pose_grads=pg)  # noqa: E731
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
    rows = profiled(step, steps, 0, reserve_per_step=400).rows
    stage_us = {kk: round(rows[kk][1] * 1e3 / steps, 2) for kk in rows if kk in STAGE[arm]}
    res = dict(ms=round(ms[len(ms) // 2], 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4), windows=WINDOWS, steps=steps,
               stage_us_per_step=stage_us, stage_total_us=round(sum(stage_us.values()), 2), pose_grads_finite=bool(torch.isfinite(pg).all()),
               modes=(mc.backward_compaction, mf.backward_compaction),
               build="this" if os.path.dirname(os.path.dirname(os.path.abspath(N.__file__))) == ROOT else "parent")
    if arm == "localize":
        b = stage_bytes(w["model"], rays, w["nc"], w["nf"])
        mfma_us = sum(stage_us.get(kk, 0.0) for kk in ("k_point_grad", "k_ray_grad_sum"))
        res["stage_hbm_bytes"] = b
        if mfma_us > 0:
            res["stage_hbm_fraction_of_%.1f_TBps" % HBM_TBPS] = round(b / (mfma_us * 1e-6) / (HBM_TBPS * 1e12), 4)
    return res


def next_round_file():
    rounds = [int(m.group(1)) for f in glob.glob(os.path.join(ROOT, "profiles", "r*")) for m in [re.match(r"r(\d+)_", os.path.basename(f))] if m]
    return os.path.join(ROOT, "profiles", "r%02d_localize.json" % (max(rounds, default=0) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per figure")
    ap.add_argument("--lines", default=",".join(LINES))
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit (library built): the step_on_views arm runs there")
    ap.add_argument("--capability-log", default=None, help="a test log holding the LOCALIZE_CAPABILITY line of tests/test_gpu_localize.py")
    ap.add_argument("--dump-outputs-dirs", nargs=2, metavar=("THIS", "PARENT"), default=None,
                    help="two `bench.py --dump-outputs` directories, of this tree and of the parent build: compared array by array on the bits")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        spec = child_spec(a.child)
        return emit(TAG, one_line(spec["line"], spec["arm"], spec["steps"], spec["warmup"], spec["rays"]))
    base_root = os.path.abspath(a.parent_root) if a.parent_root else ROOT
    out = dict(metric="localize_step_cost", rays=a.rays, steps=a.steps, views=VIEWS, lines={},
               step_lr0_arm="parent build" if a.parent_root else "this build (its unchanged trainable path)")
    if a.dump_outputs_dirs:   # (the feature unused: bench.py's step must compute the parent build's bytes)
        import numpy as np
        this, parent = a.dump_outputs_dirs
        names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(this, "*.npy")))
        same = {n: bool(os.path.exists(os.path.join(parent, n)) and np.array_equal(np.load(os.path.join(this, n)).view(np.uint32),
                                                                                  np.load(os.path.join(parent, n)).view(np.uint32))) for n in names}
        out["bench_dump_outputs_vs_parent"] = dict(arrays=len(names), identical_bytes=same, all_identical=bool(names) and all(same.values()))
    if a.capability_log:
        for ln in open(a.capability_log):
            if "LOCALIZE_CAPABILITY " in ln:
                out["capability"] = json.loads(ln[ln.index("LOCALIZE_CAPABILITY ") + len("LOCALIZE_CAPABILITY "):])
    for name in a.lines.split(","):
        for rnd in range(ROUNDS):
            for arm in ("step_lr0", "localize"):
                res, why = measure(__file__, TAG, dict(line=name, arm=arm, steps=a.steps, warmup=a.warmup, rays=a.rays), a.timeout,
                                   root=base_root if arm == "step_lr0" else ROOT)
                if res is None:   # (nothing more is started on the device after a failure)
                    out["stopped_at"] = dict(measurement=[name, arm, rnd], reason=why)
                    break
                out["lines"].setdefault(name, {})["%s_%d" % (arm, rnd)] = res
            if "stopped_at" in out:
                break
        if "stopped_at" in out:
            break
    for name, r in out["lines"].items():
        if all("%s_%d" % (arm, rnd) in r for arm in ("step_lr0", "localize") for rnd in range(ROUNDS)):
            new, old = [r["localize_%d" % i]["ms"] for i in range(ROUNDS)], [r["step_lr0_%d" % i]["ms"] for i in range(ROUNDS)]
            r["step_speedup"] = round(sum(old) / sum(new), 3)
            r["stage_speedup"] = round(sum(r["step_lr0_%d" % i]["stage_total_us"] for i in range(ROUNDS))
                                       / max(1e-9, sum(r["localize_%d" % i]["stage_total_us"] for i in range(ROUNDS))), 2)
            r["same_arm_spread_pct"] = round(100.0 * max((max(new) - min(new)) / min(new), (max(old) - min(old)) / min(old)), 2)
    path = a.out or next_round_file()
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
