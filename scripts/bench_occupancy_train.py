"""What the occupancy grid does to a TRAINING step: ms per TrainEngine step on the lego-lowres fixture nets (4 x 128,
64 + 64 samples, white background, 4096 rays per step drawn from six 100 x 100 teacher views rendered from the same nets) in three
arms that start from the same weights and see the same data stream:

    plain   TrainEngine(backward="auto")
    static  the same with the grid of OccupancyGrid.from_models at its defaults (never updated), warm-up 0
    live    the same with OccupancyGrid.for_training (resolution 128) kept alive by the engine (update every 16 steps), timed after
            LIVE_PRE_STEPS steps of its own

Protocol of scripts/bench_occupancy.py: the arms alternate over ROUNDS rounds in one process; a timed window is at least
MIN_WINDOW_S of steps (sized from one timed window after WARMUP steps) and ends in a device synchronise; `same_arm_spread_pct` is
what one arm differs by between its rounds -- a difference between arms below it is not resolved.  The steps run with lr = 0: Adam,
the re-pack and the grid updates all run, the weights (and with them the kept fractions) stay where they were, so that the rounds of
an arm measure the same work.  Also recorded: the kept fractions of the forwards and of the backwards, the cost of one
OccupancyGrid.update_density call (timed in a window of its own) and that cost amortised over `occupancy_every` steps, and the
distance of a culled step's gradient from the plain step's on the same rays.  Reported, not asserted: nothing here fails on a number.

    python scripts/bench_occupancy_train.py [--precisions fp32 f16x3_train] [--rounds 3] [--capability-record FILE] [--out FILE]
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CFG = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
AABB = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
ANGLES = (0.0, 20.0, 40.0, 60.0, 80.0, 100.0)
SIDE, RAYS, EVERY = 100, 4096, 16
WARMUP, MIN_WINDOW_S, LIVE_PRE_STEPS = 5, 0.5, 160


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def teacher(N, torch, np, dev, mc, mf):
    """Packed rays and teacher colours of the six views (the fixture pose rotated about the scene's up axis), as two pools."""
    r = np.load(os.path.join(ROOT, "tests", "golden", "lego_lowres_render.npz"))
    focal = float(r["focal"]) * SIDE / float(r["W"])
    base = torch.from_numpy(r["pose"]).to(dev)
    opts = N.make_options(64, 64, perturb=False, white_background=True, radiance_field_noise_std=0.0)
    ex, ed = N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)
    rays, rgb = [], []
    for deg in ANGLES:
        a = np.deg2rad(deg)
        rot = torch.tensor([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32, device=dev)
        pose = base.clone()
        pose[:3, :4] = rot @ pose[:3, :4]
        pix = torch.arange(SIDE * SIDE, dtype=torch.int64, device=dev)
        ro, rd = N.get_rays_at_pixels(SIDE, SIDE, focal, pose[:3, :4].contiguous(), pix)
        rays.append(N.pack_rays(ro, rd, opts, SIDE, SIDE, focal))
        with torch.no_grad():
            out, _ = N.render_pose_rows(SIDE, SIDE, focal, pose, mc, mf, opts, ex, ed)
        rgb.append(out[3].reshape(-1, 3).contiguous())
    return torch.cat(rays), torch.cat(rgb)


def run(precisions, rounds):
    import numpy as np
    import torch

    import nerf_pytorch_amd as N
    if not torch.cuda.is_available():
        raise SystemExit("bench_occupancy_train needs the GPU: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    w = np.load(os.path.join(ROOT, "tests", "golden", "lego_lowres_weights.npz"))
    mc, mf = N.FlexibleNeRFModel(**CFG), N.FlexibleNeRFModel(**CFG)
    mc.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("c_")})
    mf.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("f_")})
    mc, mf = mc.to(dev), mf.to(dev)
    pool_r, pool_t = teacher(N, torch, np, dev, mc, mf)
    picks = torch.randint(0, pool_r.shape[0], (64, RAYS), generator=torch.Generator().manual_seed(0)).to(dev)
    batches = [(pool_r[i].contiguous(), pool_t[i].contiguous()) for i in picks]   # (the data stream: 64 batches, cycled)
    rec = dict(net="lego-lowres fixture nets, 4 x 128", rays_per_step=RAYS, samples="64 + 64", views="%d at %d x %d" % (len(ANGLES), SIDE, SIDE),
               occupancy_every=EVERY, lr=0.0, rounds=rounds, min_window_s=MIN_WINDOW_S, live_pre_steps=LIVE_PRE_STEPS)
    static = N.OccupancyGrid.from_models(mc, mf, AABB)
    rec["static_grid_occupied_fraction"] = static.occupied_fraction()
    for prec in precisions:
        def engine(**kw):
            a, b = copy.deepcopy(mc), copy.deepcopy(mf)
            if prec != "fp32":
                a.set_training_precision(prec), b.set_training_precision(prec)
            return N.TrainEngine(a, b, 64, 64, perturb=True, white_background=True, noise_std=0.0, backward="auto", **kw)
        live_grid = N.OccupancyGrid.for_training(AABB, device=dev)
        arms = dict(plain=engine(), static=engine(occupancy=static, occupancy_warmup=0, occupancy_every=EVERY),
                    live=engine(occupancy=live_grid, occupancy_warmup=32, occupancy_every=EVERY))
        state = dict.fromkeys(arms, 0)

        def steps(name, k):
            e = arms[name]
            for _ in range(k):
                rays, tgt = batches[state[name] % len(batches)]
                e.step(rays, tgt, lr=0.0)
                state[name] += 1

        def window(name, k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(name, k)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        steps("live", LIVE_PRE_STEPS)
        size = {}
        for name in arms:
            steps(name, WARMUP)
            t = window(name, 16) / 16
            size[name] = max(16, int(MIN_WINDOW_S / t) // EVERY * EVERY + EVERY)   # (a multiple of occupancy_every: every window holds as many updates)
        ms = {name: [] for name in arms}
        for _ in range(rounds):
            for name in arms:
                ms[name].append(1e3 * window(name, size[name]) / size[name])
        out = {}
        for name, e in arms.items():
            m = median(ms[name])
            out[name] = dict(ms_per_step=round(m, 4), rounds_ms=[round(v, 4) for v in ms[name]], steps_per_window=size[name],
                             same_arm_spread_pct=round(100.0 * (max(ms[name]) - min(ms[name])) / m, 2),
                             backward_modes_used=e.backward_modes_used)
            bc = e.backward_sample_counts()
            out[name]["backward_kept"] = {k: (None if v is None else round(v[0] / float(v[1]), 4)) for k, v in bc.items()}
            if e.occupancy is not None:
                kc, tc, kf, tf = e.occupancy_counts.tolist()
                out[name].update(kept_coarse=round(kc / tc, 4), kept_fine=round(kf / tf, 4), occupied_fraction=round(e.occupancy.occupied_fraction(), 4))
        for name in ("static", "live"):
            out[name]["speedup_vs_plain"] = round(out["plain"]["ms_per_step"] / out[name]["ms_per_step"], 3)
        # one update_density call (a quarter of the 128^3 grid probed through both nets, bits, one dilation), in a window of its own
        e = arms["live"]
        nets = ((e.mc._plan, e.packed_c), (e.mf._plan, e.packed_f))
        for k in range(3):
            live_grid.update_density(nets, k)
        torch.cuda.synchronize()
        t0, k = time.perf_counter(), 0
        while time.perf_counter() - t0 < MIN_WINDOW_S or k < 8:
            live_grid.update_density(nets, k)
            k += 1
            if k % 8 == 0:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        upd = 1e3 * (time.perf_counter() - t0) / k
        out["update"] = dict(ms_per_call=round(upd, 4), calls=k, amortised_ms_per_step=round(upd / EVERY, 4), grid="128^3, fraction 0.25")
        # the culled step's gradient against the plain step's, same weights, same rays, same in-kernel draws (step 0 of fresh engines)
        p, c = engine(), engine(occupancy=static, occupancy_warmup=0, occupancy_every=1 << 30)
        for x in (p, c):
            x.forward_backward(*batches[0])
        torch.cuda.synchronize()
        d = (c.grad - p.grad).double()
        out["culled_vs_plain_gradient"] = dict(rel_l2=float(d.norm() / p.grad.double().norm()), max_abs_over_max_abs=float(d.abs().max() / p.grad.abs().max()),
                                               loss_plain=[float(v) for v in p.loss.tolist()], loss_culled=[float(v) for v in c.loss.tolist()])
        rec[prec] = out
        print(prec, json.dumps(out), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", nargs="+", default=["fp32", "f16x3_train"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--capability-record", default=None, help="the capability arms' record (three seeds, both arms) to merge in")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_occupancy_train.json"))
    args = ap.parse_args()
    rec = run(args.precisions, args.rounds)
    if args.capability_record:
        rec["capability"] = json.load(open(args.capability_record))
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
