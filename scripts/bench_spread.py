"""What the ray-weight spread loss (mip-NeRF 360's L_dist) adds to a TRAINING step: ms per TrainEngine step with
spread=None against spread=LAMBDA in this build, on the lego-lowres fixture nets (4 x 128) and on two 8 x 256 nets, 4096 rays of
64 + 64 samples, white background; and the time of one nerfhip_spread_loss launch per pass, in windows of its own.

Protocol of scripts/bench_occupancy_train.py: the arms alternate over ROUNDS rounds in one process; a timed window is at least
MIN_WINDOW_S of steps (sized from one timed window after WARMUP steps) and ends in a device synchronise; `same_arm_spread_pct` is what
one arm differs by between its rounds -- a difference between arms below it is not resolved.  The steps run with lr = 0, so that the
rounds of an arm measure the same work.  Reported, not asserted: nothing here fails on a number.

    python scripts/bench_spread.py [--precisions fp32 f16x3_train] [--rounds 3] [--out FILE]
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NETS = {"lego4x128": dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4),
        "8x256": dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)}
SIDE, RAYS, LAMBDA = 100, 4096, 0.01
WARMUP, MIN_WINDOW_S = 5, 0.5


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def run(precisions, rounds):
    import numpy as np
    import torch

    import nerf_pytorch_amd as N
    if not torch.cuda.is_available():
        raise SystemExit("bench_spread needs the GPU: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    w = np.load(os.path.join(ROOT, "tests", "golden", "lego_lowres_weights.npz"))
    r = np.load(os.path.join(ROOT, "tests", "golden", "lego_lowres_render.npz"))
    focal = float(r["focal"]) * SIDE / float(r["W"])
    pose = torch.from_numpy(r["pose"]).to(dev)
    opts = N.make_options(64, 64, perturb=False, white_background=True, radiance_field_noise_std=0.0)
    ro, rd = N.get_rays_at_pixels(SIDE, SIDE, focal, pose[:3, :4].contiguous(), torch.arange(SIDE * SIDE, dtype=torch.int64, device=dev))
    pool = N.pack_rays(ro, rd, opts, SIDE, SIDE, focal)
    gen = torch.Generator().manual_seed(0)
    picks = torch.randint(0, pool.shape[0], (16, RAYS), generator=gen).to(dev)
    batches = [(pool[i].contiguous(), torch.rand(RAYS, 3, generator=gen).to(dev)) for i in picks]
    rec = dict(rays_per_step=RAYS, samples="64 + 64", lr=0.0, rounds=rounds, min_window_s=MIN_WINDOW_S, spread=LAMBDA)
    for net, cfg in NETS.items():
        torch.manual_seed(1)
        mc, mf = N.FlexibleNeRFModel(**cfg), N.FlexibleNeRFModel(**cfg)
        if net == "lego4x128":
            mc.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("c_")})
            mf.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("f_")})
        mc, mf = mc.to(dev), mf.to(dev)
        for prec in precisions:
            def engine(**kw):
                a, b = copy.deepcopy(mc), copy.deepcopy(mf)
                if prec != "fp32":
                    a.set_training_precision(prec), b.set_training_precision(prec)
                return N.TrainEngine(a, b, 64, 64, perturb=True, white_background=True, noise_std=0.0, **kw)
            arms = dict(plain=engine(), spread=engine(spread=LAMBDA))
            state = dict.fromkeys(arms, 0)

            def window(name, k):
                e = arms[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(k):
                    e.step(*batches[state[name] % len(batches)], lr=0.0)
                    state[name] += 1
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            size = {}
            for name in arms:
                window(name, WARMUP)
                size[name] = max(16, int(MIN_WINDOW_S / (window(name, 16) / 16)) + 1)
            ms = {name: [] for name in arms}
            for _ in range(rounds):
                for name in arms:
                    ms[name].append(1e3 * window(name, size[name]) / size[name])
            out = {}
            for name in arms:
                m = median(ms[name])
                out[name] = dict(ms_per_step=round(m, 4), rounds_ms=[round(v, 4) for v in ms[name]], steps_per_window=size[name],
                                 same_arm_spread_pct=round(100.0 * (max(ms[name]) - min(ms[name])) / m, 2))
            out["spread_over_plain_pct"] = round(100.0 * (out["spread"]["ms_per_step"] / out["plain"]["ms_per_step"] - 1.0), 2)
            # one nerfhip_spread_loss launch per pass, over the workspace the last step left (the engine's last RenderCall), into
            # buffers of its own, in windows of its own
            render, st = arms["spread"].render_call, torch.cuda.current_stream(dev).cuda_stream
            for fine, tag in ((0, "coarse"), (1, "fine")):
                gw, sl = torch.empty(RAYS, 64 + 64 * fine, device=dev), torch.empty(RAYS, device=dev)
                call = lambda: render.spread(fine, LAMBDA / RAYS, None, sl.data_ptr(), gw.data_ptr(), st)  # noqa: E731
                for _ in range(10):
                    call()
                torch.cuda.synchronize()
                t0, k = time.perf_counter(), 0
                while time.perf_counter() - t0 < MIN_WINDOW_S:
                    for _ in range(64):
                        call()
                    k += 64
                    torch.cuda.synchronize()
                out["kernel_us_per_launch_" + tag] = round(1e6 * (time.perf_counter() - t0) / k, 3)
            rec["%s %s" % (net, prec)] = out
            print(net, prec, json.dumps(out), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", nargs="+", default=["fp32", "f16x3_train"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_spread.json"))
    args = ap.parse_args()
    rec = run(args.precisions, args.rounds)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
