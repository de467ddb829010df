"""What the robust photometric losses cost, in three parts:

  1. one nerfhip_robust_loss_fwd_bwd launch over 4096 rays for each kind, and for Huber with trim = 0.8 (the per-ray walk and the
     31-round selection), against one nerfhip_mse_loss_fwd_bwd launch (k_mse_loss: unchanged by the feature, so this tree's is the
     parent commit's) -- the device time between two HIP events per launch (LaunchProfile) and, next to it, launches back to back
     from the host;
  2. ms per TrainEngine step with photometric=("huber", 0.1), and with trim=0.8 on top, against the plain step -- without the keywords
     the parent commit's launches --, for two 4 x 64 nets (64 + 64 samples) and two 8 x 256 nets (64 + 128 samples), 4096 rays, on one
     stream and on two;
  3. the trained regime: the lego-lowres fixture nets (4 x 128, 64 + 64 samples) on 4096 rays of a 100 x 100 view against their own
     render plus noise, backward="compact": trim=0.8 against untrimmed, with the kept-sample fractions each arm's backward ran on.

Protocol of scripts/bench_matte.py: the arms alternate over ROUNDS rounds in one process; a timed window is at least MIN_WINDOW_S of
steps (sized from one timed window after WARMUP steps) and ends in a device synchronise; bench_common.pair_cost gives what an arm costs
over the plain one and what one arm differs by between its rounds -- a difference between arms below that is not resolved.  The steps
run with lr = 0, so that the rounds of an arm measure the same work.  Reported, not asserted: nothing here fails on a number.
--test-log FILE: a `pytest -s` log of tests/test_gpu_robust.py, whose capability line is recorded as well.

    python scripts/bench_robust.py [--rounds 3] [--test-log FILE] [--out FILE]
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
LEGO = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
SIDE, RAYS, HUBER, TRIM = 100, 4096, 0.1, 0.8
KINDS = (("l2", 0, 0.0), ("l1", 1, 0.0), ("huber", 2, HUBER), ("charbonnier", 3, 1e-3), ("relative", 4, 1e-3))
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


def alternate(arms, batches, rounds, base="plain"):
    """{arm: rounds_ms, steps_per_window; arm_over_<base>: pair_cost} of engines that alternate over `rounds` rounds."""
    import torch
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
    for name in arms:
        if name != base:
            out["%s_over_%s" % (name, base)] = BC.pair_cost(ms[name], ms[base])
    return out


def run(rounds):
    import numpy as np
    import torch

    import nerf_pytorch_amd as N
    from nerf_pytorch_amd import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("bench_robust needs the GPU: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    r = np.load(os.path.join(ROOT, "tests", "golden", "lego_lowres_render.npz"))
    focal = float(r["focal"]) * SIDE / float(r["W"])
    pose = torch.from_numpy(r["pose"]).to(dev)
    opts = N.make_options(64, 64, perturb=False, white_background=False, radiance_field_noise_std=0.0)
    ro, rd = N.get_rays_at_pixels(SIDE, SIDE, focal, pose[:3, :4].contiguous(), torch.arange(SIDE * SIDE, dtype=torch.int64, device=dev))
    pool = N.pack_rays(ro, rd, opts, SIDE, SIDE, focal)
    gen = torch.Generator().manual_seed(0)
    picks = torch.randint(0, pool.shape[0], (16, RAYS), generator=gen).to(dev)
    batches = [(pool[i].contiguous(), torch.rand(RAYS, 3, generator=gen).to(dev)) for i in picks]
    rec = dict(rays_per_step=RAYS, lr=0.0, rounds=rounds, min_window_s=MIN_WINDOW_S, huber_delta=HUBER, trim=TRIM)

    # 1. one launch of each loss kernel on 4096 rays, back to back on one stream, in windows of its own
    lib, st = L.get_lib(), torch.cuda.current_stream(dev).cuda_stream
    rgb, tgt = torch.rand(RAYS, 3, device=dev), batches[0][1]
    g_rgb, loss = torch.empty(RAYS, 3, device=dev), torch.empty(3, device=dev)
    tmp = torch.empty(lib.robust_loss_tmp_bytes(RAYS) // 4, device=dev)
    ptr = lambda t: t.data_ptr()  # noqa: E731
    robust = lambda kind, param, keep: lib.robust_loss_fwd_bwd(ptr(rgb), ptr(tgt), 3, RAYS, kind, param, keep, 1.0, ptr(g_rgb), None, None,  # noqa: E731
                                                               ptr(loss), ptr(tmp), 4 * tmp.numel(), st)
    calls = {"k_mse_loss (one net)": lambda: lib.mse_loss_fwd_bwd(ptr(rgb), None, ptr(tgt), 3, RAYS, 1.0, ptr(g_rgb), None, ptr(loss), st)}
    for name, kind, param in KINDS:
        calls["k_robust_loss " + name] = lambda kind=kind, param=param: robust(kind, param, 1.0)
    calls["k_robust_loss huber trim %.1f" % TRIM] = lambda: robust(2, HUBER, TRIM)
    calls["k_robust_loss l2 trim %.1f" % TRIM] = lambda: robust(0, 0.0, TRIM)
    # back to back from the host (launch throughput bounds it from below) ...
    rec["kernel_us_per_launch_back_to_back"] = {name: launch_us(call) for name, call in calls.items()}
    # ... and the device time of each launch between two HIP events on its stream (nerfhip_profile_enable: LaunchProfile)
    rec["kernel_us_per_launch_device_events"] = {}
    for name, call in calls.items():
        cost = BC.launch_costs(call, 200, 10, ("k_mse_loss", "k_robust_loss"))
        rec["kernel_us_per_launch_device_events"][name] = next(iter(cost.values()))["us_per_launch"]
    print(json.dumps({k: rec[k] for k in ("kernel_us_per_launch_back_to_back", "kernel_us_per_launch_device_events")}), flush=True)

    # 2. the steps
    for net, (cfg, nf) in NETS.items():
        for streams, overlap in (("one stream", False), ("two streams", True)):
            def engine(**kw):
                torch.manual_seed(1)
                return N.TrainEngine(N.FlexibleNeRFModel(**cfg).to(dev), N.FlexibleNeRFModel(**cfg).to(dev), 64, nf, perturb=True,
                                     white_background=False, noise_std=0.0, overlap=overlap, **kw)
            arms = dict(plain=engine(), huber=engine(photometric=("huber", HUBER)), huber_trim=engine(photometric=("huber", HUBER), trim=TRIM))
            out = alternate(arms, batches, rounds)
            rec["%s, %s" % (net, streams)] = out
            print(net, streams, json.dumps(out), flush=True)

    # 3. the trained regime, compacted backward: trim against untrimmed, with the kept-sample fractions
    w = np.load(os.path.join(ROOT, "tests", "golden", "lego_lowres_weights.npz"))

    def lego_engine(**kw):
        mc, mf = N.FlexibleNeRFModel(**LEGO), N.FlexibleNeRFModel(**LEGO)
        mc.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("c_")})
        mf.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("f_")})
        return N.TrainEngine(mc.to(dev), mf.to(dev), 64, 64, perturb=True, white_background=True, noise_std=0.0, backward="compact", **kw)

    arms = dict(plain=lego_engine(), trim=lego_engine(trim=TRIM), huber_trim=lego_engine(photometric=("huber", HUBER), trim=TRIM))
    with torch.no_grad():   # (targets: the nets' own render of each batch plus noise -- the residuals of a trained model)
        ex, ed = N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)
        wopts = N.make_options(64, 64, perturb=False, white_background=True, radiance_field_noise_std=0.0)
        own = [N.predict_and_render_radiance(b[0], arms["plain"].mc, arms["plain"].mf, wopts, mode="validation", encode_position_fn=ex,
                                             encode_direction_fn=ed)[3] for b in batches]
    trained = [(b[0], (o + 0.05 * torch.randn(o.shape, generator=gen).to(dev)).contiguous()) for b, o in zip(batches, own)]
    out = alternate(arms, trained, rounds)
    for name, e in arms.items():
        c = e.backward_sample_counts()
        out[name]["kept_sample_fraction"] = {net: round(k / t, 4) for net, (k, t) in c.items()}
        if e.robust_stats is not None:
            out[name]["kept_ray_fraction"] = [round(float(s[0]), 4) for s in e.robust_stats]
    rec["trained 4x128 64+64, compacted backward"] = out
    print("trained", json.dumps(out), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--test-log", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_robust.json"))
    args = ap.parse_args()
    out = run(args.rounds)
    if args.test_log:
        BC.scrape_log(out, args.test_log, "capability: ")
    BC.write_out(out, args.out)


if __name__ == "__main__":
    main()
