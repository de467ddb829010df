"""CPU study behind the weight of the ray-weight spread loss in tests/test_gpu_spread.py's capability test: the oracle's autograd
(oracle/nerf_oracle.py) on the capability setup of DESIGN.md 3.15 / 3.16 -- six 64 x 64 teacher views of the lego-lowres fixture nets
(dense oracle render, 64 + 64 samples, white background), the 60-degree view held out, two 4 x 64 students, 400 Adam steps of 1024
rays, lr 5e-3, sigma noise 1.0 -- once per weight lambda: total loss = coarse mse + fine mse + lambda (mean L_coarse + mean L_fine), L
restated in torch by tests/spread_cases.py::spread_of_weights.  Reports, on the held-out view (no perturbation, no noise): PSNR of the
fine map against the teacher and the mean fine-pass L.

    python scripts/study_spread_lambda.py --out profiles/r18_spread_lambda_study.json [--lambdas 0 0.01 0.1] [--seeds 0] [--steps 400]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import nerf_oracle as O  # noqa: E402
import spread_cases as S  # noqa: E402

ANGLES, HELD_OUT = (0.0, 20.0, 40.0, 60.0, 80.0, 100.0), 3
TEACHER = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
STUDENT = dict(TEACHER, hidden_size=64)
NC = NF = 64


def passes(rays, par_c, par_f, cfg, perturb, noise_std, gen):
    """Both passes of the oracle's render with the weights of both kept: (rgb_c, rgb_f, w_c, w_f, z_c, z_f)."""
    n = rays.shape[0]
    ro, rd = rays[:, :3], rays[:, 3:6]
    z = O.stratified_z(rays[:, 6:7], rays[:, 7:8], NC, False, perturb, torch.rand(n, NC, generator=gen) if perturb else None)
    nz = (lambda s: torch.randn(n, s, generator=gen)) if noise_std > 0 else (lambda s: None)
    raw_c = O.run_network(par_c, ro[:, None, :] + rd[:, None, :] * z[:, :, None], rays, cfg)
    rgb_c, _, _, w_c, _ = O.volume_render(raw_c, z, rd, noise_std, nz(NC), True)
    _, z_f = O.hierarchical_z(z, w_c, NF, det=not perturb, u=torch.rand(n, NF, generator=gen) if perturb else None)
    raw_f = O.run_network(par_f, ro[:, None, :] + rd[:, None, :] * z_f[:, :, None], rays, cfg)
    rgb_f, _, _, w_f, _ = O.volume_render(raw_f, z_f, rd, noise_std, nz(NC + NF), True)
    return rgb_c, rgb_f, w_c, w_f, z, z_f


def teacher_views():
    w = np.load(os.path.join(ROOT, "tests", "golden", "lego_lowres_weights.npz"))
    r = np.load(os.path.join(ROOT, "tests", "golden", "lego_lowres_render.npz"))
    par_c = {k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("c_")}
    par_f = {k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("f_")}
    focal = float(r["focal"]) * 64.0 / float(r["W"])
    pose0 = torch.from_numpy(r["pose"]).float()
    rays, rgb = [], []
    for deg in ANGLES:
        a = np.deg2rad(deg)
        rot = torch.tensor([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=torch.float32)
        ro, rd = O.get_ray_bundle(64, 64, focal, rot @ pose0[:3, :4])
        rows = O.pack_rays(ro, rd, 2.0, 6.0, rd)
        with torch.no_grad():
            rgb.append(passes(rows, par_c, par_f, TEACHER, False, 0.0, None)[1])
        rays.append(rows)
    return torch.stack(rays), torch.stack(rgb)


def arm(rays, rgb, lam, seed, steps, n_rays, lr=5e-3, noise_std=1.0):
    train = [i for i in range(len(ANGLES)) if i != HELD_OUT]
    pool_r, pool_t = rays[train].reshape(-1, rays.shape[-1]), rgb[train].reshape(-1, 3)
    par = [{k: v.requires_grad_(True) for k, v in O.init_params(STUDENT, seed=2 * seed + i).items()} for i in (0, 1)]
    flat = [v for p in par for v in p.values()]
    m, v = [torch.zeros_like(t) for t in flat], [torch.zeros_like(t) for t in flat]
    gen = torch.Generator().manual_seed(seed)
    picks = torch.randint(0, pool_r.shape[0], (steps, n_rays), generator=torch.Generator().manual_seed(seed))
    for i in range(steps):
        r, t = pool_r[picks[i]], pool_t[picks[i]]
        rgb_c, rgb_f, w_c, w_f, z_c, z_f = passes(r, par[0], par[1], STUDENT, True, noise_std, gen)
        loss = ((rgb_c - t) ** 2).mean() + ((rgb_f - t) ** 2).mean()
        if lam > 0:
            loss = loss + lam * (S.spread_of_weights(w_c, z_c, r).mean() + S.spread_of_weights(w_f, z_f, r).mean())
        grads = torch.autograd.grad(loss, flat)
        with torch.no_grad():
            for p, g, mm, vv in zip(flat, grads, m, v):
                O.adam_step(p, g, mm, vv, i + 1, lr)
    with torch.no_grad():
        _, rgb_f, _, w_f, _, z_f = passes(rays[HELD_OUT], par[0], par[1], STUDENT, False, 0.0, None)
        mse = float(((rgb_f - rgb[HELD_OUT]).double() ** 2).mean())
        spread = float(S.spread_of_weights(w_f, z_f, rays[HELD_OUT]).mean())
    return dict(lam=lam, seed=seed, psnr=float(-10.0 * np.log10(max(mse, 1e-30))), spread_fine=spread, final_loss=float(loss.detach()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--lambdas", type=float, nargs="+", default=[0.0, 0.01, 0.1])
    ap.add_argument("--seeds", type=int, nargs="+", default=[0])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rays", type=int, default=1024)
    a = ap.parse_args()
    rays, rgb = teacher_views()
    runs = []
    for seed in a.seeds:
        for lam in a.lambdas:
            t = time.time()
            runs.append(dict(arm(rays, rgb, lam, seed, a.steps, a.rays), seconds=round(time.time() - t, 1)))
            print(runs[-1], flush=True)
            with open(a.out, "w") as f:
                json.dump(dict(what="CPU study of the spread weight with the oracle's autograd (scripts/study_spread_lambda.py)",
                               steps=a.steps, rays=a.rays, runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
