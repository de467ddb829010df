"""CPU study behind the robust arm of tests/test_gpu_robust.py's capability test: the oracle's autograd (oracle/nerf_oracle.py) on the
setup of DESIGN.md 3.22 -- the teacher views of scripts/study_matte_weights.py (six 64 x 64 views of the lego-lowres fixture nets over
white; the 60-degree view held out, the 0, 40 and 80 degree views training two 4 x 64 students for 400 Adam steps of 1024 rays, lr 5e-3,
sigma noise 1.0), with a fixed random 30 % of every training view's pixels replaced by saturated random colours
(tests/robust_cases.py::corrupt; an independent draw per pixel and per view).

The MSE optimum at a pixel is then 0.7 C + 0.3 E[o]: the plain arm's PSNR against the CLEAN images is capped.  The L1 / Huber optimum is
the median, C.

  stage 1   plain at seeds 0, 1, 2 (its seed-to-seed spread is the margin), and at seed 0: l1, huber at three deltas, charbonnier 1e-3;
  stage 2   the best of stage 1's robust arms with trim = 0.6.

The rule, fixed here before any GPU run: the robust arm with the highest held-out PSNR against the clean view (`chosen`); it `wins`
when it beats the plain arm of its seed by more than the margin.  The losses are the definition restated in torch by
tests/robust_cases.py::robust_loss_torch.

    python scripts/study_robust.py --out profiles/r22_robust_study.json [--steps 400] [--jobs 8] [--rate 0.3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

import nerf_oracle as O  # noqa: E402
import robust_cases as R  # noqa: E402
import study_matte_weights as SM  # noqa: E402

HUBER_DELTAS = (0.05, 0.1, 0.2)
CHARBONNIER_EPS = 1e-3
TRIM = 0.6
STAGE1 = [("l1", 0.0), ("huber", HUBER_DELTAS[0]), ("huber", HUBER_DELTAS[1]), ("huber", HUBER_DELTAS[2]), ("charbonnier", CHARBONNIER_EPS)]


def arm(kind, param, trim, seed, steps, n_rays, rate, threads=0, lr=5e-3, noise_std=1.0):
    """kind None: the plain squared error."""
    if threads:
        torch.set_num_threads(threads)
    t0 = time.time()
    rays, white, _ = SM.teacher_views()
    train = list(SM.TRAIN)
    dirty, hit = R.corrupt(white[train], rate)
    pool_r, pool_t = rays[train].reshape(-1, rays.shape[-1]), dirty.reshape(-1, 3)
    par = [{k: v.requires_grad_(True) for k, v in O.init_params(SM.STUDENT, seed=2 * seed + i).items()} for i in (0, 1)]
    flat = [v for p in par for v in p.values()]
    m, v = [torch.zeros_like(t) for t in flat], [torch.zeros_like(t) for t in flat]
    gen = torch.Generator().manual_seed(seed)
    picks = torch.randint(0, pool_r.shape[0], (steps, n_rays), generator=torch.Generator().manual_seed(seed))
    finite = True
    for i in range(steps):
        r, t = pool_r[picks[i]], pool_t[picks[i]]
        o = SM.passes(r, par[0], par[1], SM.STUDENT, True, noise_std, gen, True)
        if kind is None:
            loss = ((o["rgb_c"] - t) ** 2).mean() + ((o["rgb_f"] - t) ** 2).mean()
        else:
            loss = sum(R.robust_loss_torch(o["rgb_" + tag], t, R.KINDS[kind], param, trim)[0] for tag in ("c", "f"))
        finite = finite and bool(torch.isfinite(loss.detach()))
        grads = torch.autograd.grad(loss, flat)
        with torch.no_grad():
            for q, g, mm, vv in zip(flat, grads, m, v):
                O.adam_step(q, g, mm, vv, i + 1, lr)
    with torch.no_grad():
        o = SM.passes(rays[SM.HELD_OUT], par[0], par[1], SM.STUDENT, False, 0.0, None, True)
        mse = float(((o["rgb_f"] - white[SM.HELD_OUT]).double() ** 2).mean())
    return dict(arm="plain" if kind is None else kind, param=param, trim=trim, seed=seed, psnr_clean=float(-10.0 * np.log10(max(mse, 1e-30))),
                final_loss=float(loss.detach()), finite=finite, corrupted=float(hit.float().mean()), seconds=round(time.time() - t0, 1))


def cap_db(rate):
    """The derivable cap of the plain arm: a model AT the MSE optimum 0.7 C + 0.3 E[o] (E[o] = 1/2 per channel) against the clean
    held-out view -- the PSNR of rate * (C - 1/2)."""
    _, white, _ = SM.teacher_views()
    mse = float(((rate * (white[SM.HELD_OUT].double() - 0.5)) ** 2).mean())
    return float(-10.0 * np.log10(mse))


def run_all(jobs, n_jobs):
    if n_jobs > 1 and len(jobs) > 1:
        import torch.multiprocessing as mp
        with mp.get_context("spawn").Pool(min(n_jobs, len(jobs))) as pool:
            return pool.starmap(arm, jobs)
    return [arm(*j) for j in jobs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--rate", type=float, default=R.CORRUPTION_RATE)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    tail = (a.steps, a.rays, a.rate)
    stage1 = [(None, 0.0, 1.0, seed) + tail + (1,) for seed in (0, 1, 2)] + [(k, p, 1.0, 0) + tail + (1,) for k, p in STAGE1]
    runs = run_all(stage1, a.jobs)
    for r in runs:
        print(r, flush=True)
    robust = [r for r in runs if r["arm"] != "plain" and r["finite"]]
    best = max(robust, key=lambda r: r["psnr_clean"])
    runs += run_all([(best["arm"], best["param"], TRIM, 0) + tail + (0,)], 1)
    print(runs[-1], flush=True)
    plain = [r["psnr_clean"] for r in runs if r["arm"] == "plain"]
    margin = max(plain) - min(plain)
    chosen = max((r for r in runs if r["arm"] != "plain" and r["finite"]), key=lambda r: r["psnr_clean"])
    with open(a.out, "w") as f:
        json.dump(dict(what="CPU study of the robust photometric losses under 30 % saturated outliers, with the oracle's autograd "
                            "(scripts/study_robust.py)", steps=a.steps, rays=a.rays, corruption_rate=a.rate,
                       rule="the robust arm with the highest held-out PSNR against the clean view; it wins when it beats the plain arm "
                            "of its seed by more than the plain arm's seed-to-seed spread",
                       plain_cap_db=cap_db(a.rate), margin_db=margin,
                       chosen=dict(kind=chosen["arm"], param=chosen["param"], trim=chosen["trim"]),
                       wins=bool(chosen["psnr_clean"] > plain[0] + margin), runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
