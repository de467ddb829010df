"""What the alpha-matte loss costs: the time of one nerfhip_matte_loss_fwd_bwd launch against one
nerfhip_mse_loss_fwd_bwd launch (k_mse_loss: unchanged by the feature, so this tree's is the parent commit's) -- the device time
between two HIP events per launch (LaunchProfile) and, next to it, launches back to back from the host --, and ms per TrainEngine
step with alpha="matte" (random background, alpha_loss and opacity_entropy on both nets) against the plain step -- without alpha= the
parent commit's launches --, for two 4 x 64 nets (64 + 64 samples) and two 8 x 256 nets (64 + 128 samples), 4096 rays, on one stream
and on two.

Protocol of scripts/bench_spread.py: the arms alternate over ROUNDS rounds in one process; a timed window is at least MIN_WINDOW_S of
steps (sized from one timed window after WARMUP steps) and ends in a device synchronise; bench_common.pair_cost gives what the matte
arm costs over the plain one and what one arm differs by between its rounds -- a difference between arms below that is not resolved.
The steps run with lr = 0, so that the rounds of an arm measure the same work.  Reported, not asserted: nothing here fails on a number.
--test-log FILE: a `pytest -s` log of tests/test_gpu_matte.py, whose capability line is recorded as well.

    python scripts/bench_matte.py [--rounds 3] [--test-log FILE] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_common as BC  # noqa: E402

NETS = {"4x64 64+64": (dict(num_layers=4, hidden_size=64, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4), 64),
        "8x256 64+128": (dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4), 128)}
SIDE, RAYS, ALPHA_LOSS, ENTROPY = 100, 4096, 0.1, 0.01
WARMUP, MIN_WINDOW_S = 5, 0.5


def launch_us(call):
    import torch
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    t0, k = time.perf_counter(), 0
    while time.perf_counter() - t0 < MIN_WINDOW_S:
        for _ in range(64):
            call()
        k += 64
        torch.cuda.synchronize()
    return round(1e6 * (time.perf_counter() - t0) / k, 3)


def run(rounds):
    import numpy as np
    import torch

    import nerf_pytorch_amd as N
    from nerf_pytorch_amd import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("bench_matte needs the GPU: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    r = np.load(os.path.join(ROOT, "tests", "golden", "lego_lowres_render.npz"))
    focal = float(r["focal"]) * SIDE / float(r["W"])
    pose = torch.from_numpy(r["pose"]).to(dev)
    opts = N.make_options(64, 64, perturb=False, white_background=False, radiance_field_noise_std=0.0)
    ro, rd = N.get_rays_at_pixels(SIDE, SIDE, focal, pose[:3, :4].contiguous(), torch.arange(SIDE * SIDE, dtype=torch.int64, device=dev))
    pool = N.pack_rays(ro, rd, opts, SIDE, SIDE, focal)
    gen = torch.Generator().manual_seed(0)
    picks = torch.randint(0, pool.shape[0], (16, RAYS), generator=gen).to(dev)
    batches = [(pool[i].contiguous(), torch.rand(RAYS, 4, generator=gen).to(dev)) for i in picks]
    rec = dict(rays_per_step=RAYS, lr=0.0, rounds=rounds, min_window_s=MIN_WINDOW_S, alpha_loss=ALPHA_LOSS, opacity_entropy=ENTROPY)

    # one launch of each loss kernel on 4096 rays, back to back on one stream, in windows of its own
    lib, st = L.get_lib(), torch.cuda.current_stream(dev).cuda_stream
    rgb, acc, tgt = torch.rand(RAYS, 3, device=dev), torch.rand(RAYS, device=dev), batches[0][1]
    g_rgb, g_acc, loss, bg = torch.empty(RAYS, 3, device=dev), torch.empty(RAYS, device=dev), torch.empty(3, device=dev), torch.rand(RAYS, 3, device=dev)
    ptr = lambda t: t.data_ptr()  # noqa: E731
    matte = lambda mode, bgp, rnd, la: lib.matte_loss_fwd_bwd(ptr(rgb), ptr(acc), ptr(tgt), 4, RAYS, mode, bgp, rnd, 1.0, 1.0, 1.0, 7, 0, la,  # noqa: E731
                                                              ENTROPY, 1.0, ptr(g_rgb), ptr(g_acc), ptr(loss), st)
    calls = {"k_mse_loss (one net)": lambda: lib.mse_loss_fwd_bwd(ptr(rgb), None, ptr(tgt), 4, RAYS, 1.0, ptr(g_rgb), None, ptr(loss), st),
             "k_matte_loss matte random": lambda: matte(0, None, 1, ALPHA_LOSS),
             "k_matte_loss matte constant": lambda: matte(0, None, 0, ALPHA_LOSS),
             "k_matte_loss matte given": lambda: matte(0, ptr(bg), 0, ALPHA_LOSS),
             "k_matte_loss weight": lambda: matte(1, None, 0, 0.0)}
    # back to back from the host (launch throughput bounds it from below) ...
    rec["kernel_us_per_launch_back_to_back"] = {name: launch_us(call) for name, call in calls.items()}
    # ... and the device time of each launch between two HIP events on its stream (nerfhip_profile_enable: LaunchProfile)
    rec["kernel_us_per_launch_device_events"] = {}
    for name, call in calls.items():
        cost = BC.launch_costs(call, 200, 10, ("k_mse_loss", "k_matte_loss"))
        rec["kernel_us_per_launch_device_events"][name] = next(iter(cost.values()))["us_per_launch"]
    print(json.dumps({k: rec[k] for k in ("kernel_us_per_launch_back_to_back", "kernel_us_per_launch_device_events")}), flush=True)

    for net, (cfg, nf) in NETS.items():
        for streams, overlap in (("one stream", False), ("two streams", True)):
            def engine(**kw):
                torch.manual_seed(1)
                return N.TrainEngine(N.FlexibleNeRFModel(**cfg).to(dev), N.FlexibleNeRFModel(**cfg).to(dev), 64, nf, perturb=True,
                                     white_background=False, noise_std=0.0, overlap=overlap, **kw)
            arms = dict(plain=engine(), matte=engine(alpha="matte", background="random", alpha_loss=ALPHA_LOSS, opacity_entropy=ENTROPY))
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
            out = {name: dict(rounds_ms=[round(v, 4) for v in ms[name]], steps_per_window=size[name]) for name in arms}
            out["matte_over_plain"] = BC.pair_cost(ms["matte"], ms["plain"])
            rec["%s, %s" % (net, streams)] = out
            print(net, streams, json.dumps(out), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--test-log", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_matte.json"))
    args = ap.parse_args()
    out = run(args.rounds)
    if args.test_log:
        BC.scrape_log(out, args.test_log, "capability: ")
    BC.write_out(out, args.out)


if __name__ == "__main__":
    main()
