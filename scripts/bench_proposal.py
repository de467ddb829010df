"""What the interlevel proposal loss (mip-NeRF 360's L_prop) costs: one nerfhip_proposal_loss launch over 4096 rays
at 64 + 192 samples; ms per TrainEngine step of two 8 x 256 nets (64 + 128 samples) and of two 4 x 64 nets (64 + 64) with and without
proposal=1, on one stream and on two -- with the term the coarse net's pass starts behind the fine forward, so on two streams it
overlaps the fine backward only: the lost overlap is the difference between the two-stream costs and the one-stream costs --; and the
mixed setup the term exists for, a 4 x 64 coarse net on coarse_photometric=False feeding an 8 x 256 fine net, against the 8 x 256 +
8 x 256 step.  4096 random rays, white background, lr = 0 (every step of an arm is the same work).

Protocol of scripts/bench_common.py: every measurement in a fresh process under its own time limit, no retry, the first failure ends
the run.  --test-log: a `pytest -s` log of tests/test_gpu_proposal.py, whose capability line is copied in.  Reported, not asserted.

    python scripts/bench_proposal.py [--test-log FILE] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_common as BC  # noqa: E402

TAG = "BENCH_PROPOSAL "
RAYS = 4096
NETS = {"8x256": (dict(num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4), 128),
        "4x64": (dict(num_layers=4, hidden_size=64, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4), 64)}


def random_rays(torch, dev, n):
    g = torch.Generator().manual_seed(0)
    rays = torch.zeros(n, 11)
    rays[:, 2] = 4.0
    rays[:, 3:6] = torch.randn(n, 3, generator=g) * 0.3
    rays[:, 5] = -1.0
    rays[:, 6], rays[:, 7] = 2.0, 6.0
    rays[:, 8:11] = rays[:, 3:6] / rays[:, 3:6].norm(dim=1, keepdim=True)
    return rays.to(dev).contiguous(), torch.rand(n, 3, generator=g).to(dev)


def child_kernel(spec):
    """us per nerfhip_proposal_loss launch (both outputs) over random rows: windows of 64 launches, each ended by a synchronise."""
    import time

    import torch

    import nerf_pytorch_amd._lib as L
    lib, dev = L.get_lib(), torch.device("cuda", 0)
    n, sc, sf = spec["rays"], spec["sc"], spec["sf"]
    g = torch.Generator().manual_seed(1)
    rays, _ = random_rays(torch, dev, n)
    zc = (2.0 + 4.0 * torch.rand(n, sc, generator=g)).sort(dim=1).values
    zf = torch.cat((zc, 2.0 + 4.0 * torch.rand(n, sf - sc, generator=g)), dim=1).sort(dim=1).values
    raw_c, raw_f = torch.randn(n, sc, 4, generator=g) * 1.5, torch.randn(n, sf, 4, generator=g) * 1.5
    zc, zf, raw_c, raw_f = (t.to(dev).contiguous() for t in (zc, zf, raw_c, raw_f))
    loss, gw = torch.empty(n, device=dev), torch.empty(n, sc, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    call = lambda: lib.proposal_loss(raw_c.data_ptr(), zc.data_ptr(), sc, raw_f.data_ptr(), zf.data_ptr(), sf, rays.data_ptr(), 11, n, 0.0,  # noqa: E731
                                     None, None, 0, 0, 1.0 / n, None, loss.data_ptr(), gw.data_ptr(), 0, st)
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(BC.WINDOWS):
        t0 = time.perf_counter()
        for _ in range(64):
            call()
        torch.cuda.synchronize()
        us.append(1e6 * (time.perf_counter() - t0) / 64)
    us.sort()
    return dict(us_per_launch=round(us[len(us) // 2], 3), us_min=round(us[0], 3), us_max=round(us[-1], 3), windows=BC.WINDOWS,
                launches_per_window=64, mean_loss=float(loss.mean()))


def child_step(spec):
    import torch

    import nerf_pytorch_amd as N
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    (cfg_c, _), (cfg_f, nf) = NETS[spec["coarse"]], NETS[spec["fine"]]
    mc, mf = N.FlexibleNeRFModel(**cfg_c).to(dev), N.FlexibleNeRFModel(**cfg_f).to(dev)
    e = N.TrainEngine(mc, mf, 64, nf, perturb=True, white_background=True, noise_std=0.0, overlap=spec["overlap"], **spec["engine"])
    rays, target = random_rays(torch, dev, RAYS)
    res = BC.timed(lambda: e.step(rays, target, lr=0.0), spec["steps"], spec["warmup"], count_kernels=False)
    if e.proposal_loss is not None:
        res["proposal_loss"] = float(e.proposal_loss)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--test-log")
    ap.add_argument("--timeout", type=int, default=120, help="seconds, per measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_proposal.json"))
    a = ap.parse_args()
    if a.child:
        spec = BC.child_spec(a.child)
        return BC.emit(TAG, child_kernel(spec) if spec["what"] == "kernel" else child_step(spec))
    out = dict(rays_per_step=RAYS, lr=0.0, windows=BC.WINDOWS)
    specs = [(("kernel_4096_rays_64+192",), dict(what="kernel", rays=RAYS, sc=64, sf=256))]
    streams = (("one_stream", False), ("two_streams", True))
    for net in NETS:
        steps = 10 if net == "8x256" else 40
        for sname, overlap in streams:
            for arm, kw in (("plain", {}), ("proposal", dict(proposal=1.0))):
                specs.append((("step", net, sname, arm), dict(what="step", coarse=net, fine=net, overlap=overlap, engine=kw, steps=steps,
                                                              warmup=5)))
    for sname, overlap in streams:
        specs.append((("mixed", sname, "8x256+8x256_plain"), dict(what="step", coarse="8x256", fine="8x256", overlap=overlap, engine={},
                                                                 steps=10, warmup=5)))
        specs.append((("mixed", sname, "4x64_proposer+8x256"), dict(what="step", coarse="4x64", fine="8x256", overlap=overlap, steps=10, warmup=5,
                                                                   engine=dict(proposal=1.0, coarse_photometric=False))))
    BC.run_specs(__file__, TAG, specs, out, a.timeout)
    if "stopped_at" not in out:
        for net in NETS:
            for sname, _ in streams:
                arms = out["step"][net][sname]
                arms["proposal_over_plain_pct"] = round(100.0 * (arms["proposal"]["ms"] / arms["plain"]["ms"] - 1.0), 2)
        for sname, _ in streams:
            arms = out["mixed"][sname]
            arms["proposer_over_plain_pct"] = round(100.0 * (arms["4x64_proposer+8x256"]["ms"] / arms["8x256+8x256_plain"]["ms"] - 1.0), 2)
    if a.test_log:
        BC.scrape_log(out, a.test_log, "capability: ")
    BC.write_out(out, a.out)


if __name__ == "__main__":
    main()
