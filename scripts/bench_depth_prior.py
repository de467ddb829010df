"""What the depth priors (DS-NeRF's expected-depth and termination terms) add to a TRAINING step: ms per TrainEngine
step without a prior against the same engine stepped with prior rows on 5 % and on 100 % of its rays (both terms on both nets), on the
lego-lowres fixture nets (4 x 128, 64 + 64 samples) and on two 8 x 256 nets (64 + 128 samples), 4096 rays, white background; and the
time of one nerfhip_depth_prior_loss launch per pass, in windows of its own.

Protocol of scripts/bench_spread.py: the arms alternate over ROUNDS rounds in one process; a timed window is at least MIN_WINDOW_S of
steps (sized from one timed window after WARMUP steps) and ends in a device synchronise; bench_common.pair_cost gives what an arm costs
over the plain one and what one arm differs by between its rounds -- a difference between arms below that is not resolved.  The steps
run with lr = 0, so that the rounds of an arm measure the same work.  Reported, not asserted: nothing here fails on a number.

    python scripts/bench_depth_prior.py [--precisions fp32 f16x3_train] [--rounds 3] [--out FILE]
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_common as BC  # noqa: E402

NETS = {"lego4x128 64+64": (dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4), 64),
        "8x256 64+128": (dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4), 128)}
SIDE, RAYS, WEIGHTS = 100, 4096, (0.1, 0.01)
FRACTIONS = {"prior_5pct": 0.05, "prior_100pct": 1.0}
WARMUP, MIN_WINDOW_S = 5, 0.5


def run(precisions, rounds):
    import numpy as np
    import torch

    import nerf_pytorch_amd as N
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_prior needs the GPU: a CPU run measures nothing")
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

    def rows(frac):   # (depth in the middle of [near, far] = [2, 6], weight 1 on `frac` of the rays, sigma 0.05)
        has = (torch.rand(RAYS, generator=gen) < frac).float()
        return torch.stack((3.0 + 2.0 * torch.rand(RAYS, generator=gen), has, torch.full((RAYS,), 0.05)), dim=1).contiguous().to(dev)
    priors = {name: [rows(frac) for _ in batches] for name, frac in FRACTIONS.items()}
    rec = dict(rays_per_step=RAYS, lr=0.0, rounds=rounds, min_window_s=MIN_WINDOW_S, depth_loss=list(WEIGHTS))
    for net, (cfg, nf) in NETS.items():
        torch.manual_seed(1)
        mc, mf = N.FlexibleNeRFModel(**cfg), N.FlexibleNeRFModel(**cfg)
        if net.startswith("lego"):
            mc.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("c_")})
            mf.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("f_")})
        mc, mf = mc.to(dev), mf.to(dev)
        for prec in precisions:
            def engine(**kw):
                a, b = copy.deepcopy(mc), copy.deepcopy(mf)
                if prec != "fp32":
                    a.set_training_precision(prec), b.set_training_precision(prec)
                return N.TrainEngine(a, b, 64, nf, perturb=True, white_background=True, noise_std=0.0, **kw)
            arms = dict(plain=engine(), **{name: engine(depth_loss=WEIGHTS) for name in FRACTIONS})
            state = dict.fromkeys(arms, 0)

            def window(name, k):
                e = arms[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(k):
                    i = state[name] % len(batches)
                    kw = {} if name == "plain" else dict(depth_prior=priors[name][i])
                    e.step(*batches[i], lr=0.0, **kw)
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
            for name in FRACTIONS:
                out[name + "_over_plain"] = BC.pair_cost(ms[name], ms["plain"])
            # one nerfhip_depth_prior_loss launch per pass, over the workspace the last step left (the engine's last RenderCall), into
            # buffers of its own, in windows of its own
            e = arms["prior_100pct"]
            render, st = e.render_call, torch.cuda.current_stream(dev).cuda_stream
            for name in FRACTIONS:
                table = priors[name][0]
                for fine, tag in ((0, "coarse"), (1, "fine")):
                    gw, dl = torch.empty(RAYS, 64 + nf * fine, device=dev), torch.empty(RAYS, 2, device=dev)
                    call = lambda: render.depth_prior(fine, table.data_ptr(), 3, None, RAYS, WEIGHTS[0], WEIGHTS[1], 1.0 / RAYS, None,  # noqa: E731
                                                      dl.data_ptr(), gw.data_ptr(), False, st)
                    for _ in range(10):
                        call()
                    torch.cuda.synchronize()
                    t0, k = time.perf_counter(), 0
                    while time.perf_counter() - t0 < MIN_WINDOW_S:
                        for _ in range(64):
                            call()
                        k += 64
                        torch.cuda.synchronize()
                    out["kernel_us_per_launch_%s_%s" % (name, tag)] = round(1e6 * (time.perf_counter() - t0) / k, 3)
            rec["%s %s" % (net, prec)] = out
            print(net, prec, json.dumps(out), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", nargs="+", default=["fp32", "f16x3_train"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_depth_prior.json"))
    args = ap.parse_args()
    BC.write_out(run(args.precisions, args.rounds), args.out)


if __name__ == "__main__":
    main()
