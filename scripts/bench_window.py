"""Cost and capability record of the coarse-to-fine encoding window (FlexibleNeRFModel.set_encoding_window, TrainEngine(window=...)).

(1) Cost: ms/step of TrainEngine.step at 4096 rays for fern 4x64 and lego 8x256, with a window schedule against no window.  The two
arms alternate over ROUNDS rounds, every measurement in a child process of its own under its own time limit, WINDOWS timed windows
per measurement (median, smallest, largest); `same_arm_spread_pct` is what one arm differs by between its rounds -- a difference
between the arms below it is not resolved.  With --parent-root DIR (a checkout of the parent commit with its library built) the
no-window arm imports the package from there: the parent commit's build; without it, it is this build with no window set (the hot
kernels are the same source either way), and the record says which.

(2) Capability: 4 x 64 students trained from scratch together with a CameraTable on images the lego-lowres fixture nets (the
teacher) render from V views, the cameras started well off (--deg / --shift; view 0 is the anchor: exact and frozen), once with
the schedule and once without.  Final rotation (degrees) and translation errors per view of both arms are recorded.  Reported, not
asserted: nothing here fails on a number.

Writes profiles/rNN_window.json under the next free round number (and prints it as one JSON line).

    python scripts/bench_window.py [--steps 30] [--warmup 5] [--timeout 240] [--parent-root DIR] [--capability-steps 1500] [--out FILE]
"""
import argparse
import glob
import json
import os
import re
import sys
import time

from bench_common import ROOT, child_spec, emit, measure

LINES = {
    "fern_4x64": dict(nc=64, nf=64, noise=1.0,
                      model=dict(num_layers=4, hidden_size=64, skip_connect_every=3, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)),
    "lego_8x256": dict(nc=64, nf=128, noise=0.2,
                       model=dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)),
}
TAG = "BENCH_WINDOW_RESULT "
WINDOWS, ROUNDS = 5, 2


def one_line(name, arm, steps, warmup, rays):
    import torch

    import nerf_pytorch_amd as N
    w = LINES[name]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    mc, mf = N.FlexibleNeRFModel(**w["model"]).to(dev), N.FlexibleNeRFModel(**w["model"]).to(dev)
    # (the schedule is half open over the timed steps: fractional weights, closed bands and open ones -- the cost does not depend on them)
    kw = dict(window=lambda step: (w["model"]["num_encoding_fn_xyz"] / 2.0, w["model"]["num_encoding_fn_dir"] / 2.0)) if arm == "window" else {}
    eng = N.TrainEngine(mc, mf, w["nc"], w["nf"], noise_std=w["noise"], lr=1e-6, world_size=1, rank=0, **kw)
    g = torch.Generator().manual_seed(3)
    rd = torch.randn(rays, 3, generator=g) * 0.3
    rd[:, 2] = -1.0
    batch = torch.cat([torch.tensor([0.0, 0.0, 4.0]).expand(rays, 3), rd, torch.full((rays, 1), 2.0), torch.full((rays, 1), 6.0),
                       rd / rd.norm(dim=-1, keepdim=True)], 1).contiguous().to(dev)
    target = torch.rand(rays, 3, generator=g).to(dev)
    for _ in range(warmup):
        eng.step(batch, target)
    torch.cuda.synchronize()
    ms = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.step(batch, target)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    ms.sort()
    return dict(ms=round(ms[len(ms) // 2], 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4), windows=WINDOWS, steps=steps,
                build="this" if os.path.dirname(os.path.dirname(os.path.abspath(N.__file__))) == ROOT else "parent")


def capability(schedule, steps, rays, deg, shift, views):
    import numpy as np
    import torch

    for d in ("tests", "oracle"):   # (tests/pose_vjp.py: Rodrigues' formula and the rotation angle; it imports the oracle)
        sys.path.insert(0, os.path.join(ROOT, d))
    import nerf_pytorch_amd as N
    import pose_vjp as P
    dev = torch.device("cuda", 0)
    gold = lambda f: np.load(os.path.join(ROOT, "tests", "golden", f), allow_pickle=False)  # noqa: E731
    wts, r = gold("lego_lowres_weights.npz"), gold("lego_lowres_render.npz")
    teacher_cfg = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    tc, tf = N.FlexibleNeRFModel(**teacher_cfg), N.FlexibleNeRFModel(**teacher_cfg)
    tc.load_state_dict({k[2:]: torch.from_numpy(wts[k]) for k in wts.files if k.startswith("c_")})
    tf.load_state_dict({k[2:]: torch.from_numpy(wts[k]) for k in wts.files if k.startswith("f_")})
    tc, tf = tc.to(dev), tf.to(dev)
    H, W, focal = int(r["H"]), int(r["W"]), float(np.float32(r["focal"]))
    gt0 = torch.from_numpy(r["pose"].astype(np.float32)).to(dev)
    ex, ed = N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)
    opts = N.make_options(64, 64, perturb=False, white_background=True, radiance_field_noise_std=0.0)

    def se3(rot, t):
        T = torch.eye(4, device=dev)
        T[:3, :3] = P.rodrigues(torch.as_tensor(rot, dtype=torch.float64)).float().to(dev)
        T[:3, 3] = torch.as_tensor(t, dtype=torch.float32).to(dev)
        return T

    gts = torch.stack([se3([0.0, 0.0, np.deg2rad(360.0 * v / views)], [0.0, 0.0, 0.0]) @ gt0 for v in range(views)])
    with torch.no_grad():
        targets = []
        for v in range(views):
            ro, rd = N.get_ray_bundle(H, W, focal, gts[v])
            targets.append(N.run_one_iter_of_nerf(H, W, focal, tc, tf, ro, rd, opts, mode="validation", encode_position_fn=ex,
                                                  encode_direction_fn=ed)[3])
        targets = torch.stack(targets).contiguous()
    rng = np.random.default_rng(11)
    starts = [gts[0]]
    for v in range(1, views):
        axis = rng.normal(size=3)
        off = rng.normal(size=3)
        starts.append(gts[v] @ se3(axis / np.linalg.norm(axis) * np.deg2rad(deg), off / np.linalg.norm(off) * shift))
    starts = torch.stack(starts).contiguous()
    gts64 = gts.cpu().numpy().astype(np.float64)

    def errors(est):
        e = est.detach().cpu().numpy().astype(np.float64)
        return [(round(P.rot_angle_deg(e[v][:3, :3].T @ gts64[v][:3, :3]), 4), round(float(np.linalg.norm(e[v][:3, 3] - gts64[v][:3, 3])), 5))
                for v in range(views)]

    student = dict(num_layers=4, hidden_size=64, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
    torch.manual_seed(0)
    mc, mf = N.FlexibleNeRFModel(**student).to(dev), N.FlexibleNeRFModel(**student).to(dev)
    T = N.CameraTable(starts, lr=1e-3, active=[False] + [True] * (views - 1))
    kw = dict(window=(0.1, 0.5), total_steps=steps) if schedule else {}
    eng = N.TrainEngine(mc, mf, 64, 64, perturb=True, white_background=True, noise_std=0.2, lr=1e-3, seed=5, world_size=1, rank=0, **kw)
    sopts = N.make_options(64, 64, white_background=True)
    curve = [dict(step=0, errors=errors(starts))]
    loss = None
    for it in range(steps):
        loss = eng.step_on_views(targets, None, H, W, focal, sopts, rays, cameras=T)
        if (it + 1) % max(1, steps // 6) == 0 or it == steps - 1:
            curve.append(dict(step=it + 1, errors=errors(T.pose_matrices()), loss=round(float(loss[2]), 6)))
    final = curve[-1]["errors"][1:]
    return dict(schedule=[0.1, 0.5] if schedule else None, steps=steps, rays=rays, views=views, start_deg=deg, start_shift=shift,
                student=student, curve=curve, final_rot_deg_mean=round(float(np.mean([e[0] for e in final])), 4),
                final_trans_mean=round(float(np.mean([e[1] for e in final])), 5))


def child(spec):
    if spec["kind"] == "line":
        res = one_line(spec["line"], spec["arm"], spec["steps"], spec["warmup"], spec["rays"])
    else:
        res = capability(spec["schedule"], spec["steps"], spec["rays"], spec["deg"], spec["shift"], spec["views"])
    emit(TAG, res)


def next_round_file():
    rounds = [int(m.group(1)) for f in glob.glob(os.path.join(ROOT, "profiles", "r*")) for m in [re.match(r"r(\d+)_", os.path.basename(f))] if m]
    return os.path.join(ROOT, "profiles", "r%02d_window.json" % (max(rounds, default=0) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per measurement")
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit (library built): the no-window arm runs there")
    ap.add_argument("--capability-steps", type=int, default=1500)
    ap.add_argument("--capability-rays", type=int, default=1024)
    ap.add_argument("--deg", type=float, default=8.0)
    ap.add_argument("--shift", type=float, default=0.2)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-capability", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(child_spec(a.child))
    base_root = os.path.abspath(a.parent_root) if a.parent_root else ROOT
    out = dict(metric="encoding_window", rays=a.rays, steps=a.steps, no_window_arm="parent build" if a.parent_root else "this build", lines={},
               capability={})
    specs = []
    if not a.skip_cost:
        for name in LINES:
            for rnd in range(ROUNDS):
                for arm in ("none", "window"):
                    specs.append((("lines", name, "%s_%d" % (arm, rnd)), base_root if arm == "none" else ROOT,
                                  dict(kind="line", line=name, arm=arm, steps=a.steps, warmup=a.warmup, rays=a.rays), a.timeout))
    if not a.skip_capability:
        for schedule in (True, False):
            specs.append((("capability", "joint", "window" if schedule else "none"), ROOT,
                          dict(kind="capability", schedule=schedule, steps=a.capability_steps, rays=a.capability_rays, deg=a.deg,
                               shift=a.shift, views=a.views), 2 * a.timeout))
    for (top, mid, arm), root, spec, limit in specs:
        res, why = measure(__file__, TAG, spec, limit, root=root)
        if res is None:
            out["stopped_at"] = dict(measurement=[top, mid, arm], reason=why)
            break
        out[top].setdefault(mid, {})[arm] = res
    for name, r in out["lines"].items():
        if all("%s_%d" % (arm, rnd) in r for arm in ("none", "window") for rnd in range(ROUNDS)):
            win, non = [r["window_%d" % i]["ms"] for i in range(ROUNDS)], [r["none_%d" % i]["ms"] for i in range(ROUNDS)]
            r["window_cost_pct"] = round(100.0 * (sum(win) / sum(non) - 1.0), 2)
            r["same_arm_spread_pct"] = round(100.0 * max((max(win) - min(win)) / min(win), (max(non) - min(non)) / min(non)), 2)
    path = a.out or next_round_file()
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
