"""CPU study behind the weights of the depth-prior terms in tests/test_gpu_depth_prior.py's capability test: the oracle's autograd
(oracle/nerf_oracle.py) on the few-view setup of DESIGN.md 3.19 -- six 64 x 64 teacher views of the lego-lowres fixture nets (dense
oracle render, 64 + 64 samples, white background), the 60-degree view held out, THREE of the other five (0, 40 and 80 degrees) training
two 4 x 64 students for 400 Adam steps of 1024 rays, lr 5e-3, sigma noise 1.0.  The prior: the teacher's fine-pass depth on a keyed 5 %
of the training views' pixels with teacher acc_fine > 0.9, sigma = 0.05, weight 1; an arm with a prior draws 256 of its 1024 rays from
those pixels.  Total loss = coarse mse + fine mse + a (mean E_c + mean E_f) + b (mean Tm_c + mean Tm_f), means over all rays of the
batch, E and Tm restated in torch by tests/depth_prior_cases.py::depth_terms_of_weights.  Reports, on the held-out view (no
perturbation, no noise): PSNR of the fine map against the teacher and the mean |student depth - teacher depth| of the fine pass over
the rays with teacher acc_fine > 0.9.

    python scripts/study_depth_prior_weights.py --out profiles/r19_depth_prior_study.json [--arms 0,0 0.1,0 1,0 0,0.01 0,0.1] [--steps 400]
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
import depth_prior_cases as D  # noqa: E402

ANGLES, HELD_OUT, TRAIN = (0.0, 20.0, 40.0, 60.0, 80.0, 100.0), 3, (0, 2, 4)
TEACHER = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
STUDENT = dict(TEACHER, hidden_size=64)
NC = NF = 64
PRIOR_FRACTION, PRIOR_SIGMA, PRIOR_KEY, DEPTH_RAYS, ACC_MIN = 0.05, 0.05, 1234, 256, 0.9


def passes(rays, par_c, par_f, cfg, perturb, noise_std, gen):
    """Both passes of the oracle's render: dict(rgb_c, rgb_f, w_c, w_f, z_c, z_f, acc_f, depth_f)."""
    n = rays.shape[0]
    ro, rd = rays[:, :3], rays[:, 3:6]
    z = O.stratified_z(rays[:, 6:7], rays[:, 7:8], NC, False, perturb, torch.rand(n, NC, generator=gen) if perturb else None)
    nz = (lambda s: torch.randn(n, s, generator=gen)) if noise_std > 0 else (lambda s: None)
    raw_c = O.run_network(par_c, ro[:, None, :] + rd[:, None, :] * z[:, :, None], rays, cfg)
    rgb_c, _, _, w_c, _ = O.volume_render(raw_c, z, rd, noise_std, nz(NC), True)
    _, z_f = O.hierarchical_z(z, w_c, NF, det=not perturb, u=torch.rand(n, NF, generator=gen) if perturb else None)
    raw_f = O.run_network(par_f, ro[:, None, :] + rd[:, None, :] * z_f[:, :, None], rays, cfg)
    rgb_f, _, acc_f, w_f, depth_f = O.volume_render(raw_f, z_f, rd, noise_std, nz(NC + NF), True)
    return dict(rgb_c=rgb_c, rgb_f=rgb_f, w_c=w_c, w_f=w_f, z_c=z, z_f=z_f, acc_f=acc_f, depth_f=depth_f)


def teacher_views():
    w = np.load(os.path.join(ROOT, "tests", "golden", "lego_lowres_weights.npz"))
    r = np.load(os.path.join(ROOT, "tests", "golden", "lego_lowres_render.npz"))
    par_c = {k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("c_")}
    par_f = {k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("f_")}
    focal = float(r["focal"]) * 64.0 / float(r["W"])
    pose0 = torch.from_numpy(r["pose"]).float()
    rays, rgb, acc, depth = [], [], [], []
    for deg in ANGLES:
        a = np.deg2rad(deg)
        rot = torch.tensor([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=torch.float32)
        ro, rd = O.get_ray_bundle(64, 64, focal, rot @ pose0[:3, :4])
        rows = O.pack_rays(ro, rd, 2.0, 6.0, rd)
        with torch.no_grad():
            out = passes(rows, par_c, par_f, TEACHER, False, 0.0, None)
        rays.append(rows)
        rgb.append(out["rgb_f"])
        acc.append(out["acc_f"])
        depth.append(out["depth_f"])
    return torch.stack(rays), torch.stack(rgb), torch.stack(acc), torch.stack(depth)


def arm(views, a, b, seed, steps, n_rays, lr=5e-3, noise_std=1.0):
    rays, rgb, acc, depth = views
    train = list(TRAIN)
    pool_r, pool_t = rays[train].reshape(-1, rays.shape[-1]), rgb[train].reshape(-1, 3)
    pool_acc, pool_d = acc[train].reshape(-1), depth[train].reshape(-1)
    keyed = torch.rand(pool_acc.shape[0], generator=torch.Generator().manual_seed(PRIOR_KEY)) < PRIOR_FRACTION
    has = keyed & (pool_acc > ACC_MIN)
    pool_p = torch.stack((torch.where(has, pool_d, torch.zeros_like(pool_d)), has.float(), torch.full_like(pool_d, PRIOR_SIGMA)), dim=1)
    pixels = torch.nonzero(has).reshape(-1)
    with_prior = a > 0 or b > 0
    par = [{k: v.requires_grad_(True) for k, v in O.init_params(STUDENT, seed=2 * seed + i).items()} for i in (0, 1)]
    flat = [v for p in par for v in p.values()]
    m, v = [torch.zeros_like(t) for t in flat], [torch.zeros_like(t) for t in flat]
    gen = torch.Generator().manual_seed(seed)
    pg = torch.Generator().manual_seed(seed)
    picks = torch.randint(0, pool_r.shape[0], (steps, n_rays), generator=pg)
    keyp = pixels[torch.randint(0, pixels.numel(), (steps, DEPTH_RAYS), generator=pg)]
    for i in range(steps):
        idx = torch.cat((picks[i, :n_rays - DEPTH_RAYS], keyp[i])) if with_prior else picks[i]
        r, t, p = pool_r[idx], pool_t[idx], pool_p[idx]
        o = passes(r, par[0], par[1], STUDENT, True, noise_std, gen)
        loss = ((o["rgb_c"] - t) ** 2).mean() + ((o["rgb_f"] - t) ** 2).mean()
        if with_prior:
            for w, z in ((o["w_c"], o["z_c"]), (o["w_f"], o["z_f"])):
                E, Tm = D.depth_terms_of_weights(w, z, r, p.numpy())
                loss = loss + a * E.mean() + b * Tm.mean()
        grads = torch.autograd.grad(loss, flat)
        with torch.no_grad():
            for q, g, mm, vv in zip(flat, grads, m, v):
                O.adam_step(q, g, mm, vv, i + 1, lr)
    with torch.no_grad():
        o = passes(rays[HELD_OUT], par[0], par[1], STUDENT, False, 0.0, None)
        mse = float(((o["rgb_f"] - rgb[HELD_OUT]).double() ** 2).mean())
        solid = acc[HELD_OUT] > ACC_MIN
        derr = float((o["depth_f"] - depth[HELD_OUT])[solid].abs().double().mean())
    return dict(a=a, b=b, seed=seed, psnr=float(-10.0 * np.log10(max(mse, 1e-30))), depth_err=derr, final_loss=float(loss.detach()),
                prior_pixels=int(pixels.numel()), finite=bool(np.isfinite(float(loss.detach()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--arms", nargs="+", default=["0,0", "0.1,0", "1,0", "0,0.01", "0,0.1"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--threads", type=int, default=0)
    a = ap.parse_args()
    if a.threads:
        torch.set_num_threads(a.threads)
    views = teacher_views()
    runs = []
    for spec in a.arms:
        wa, wb = (float(v) for v in spec.split(","))
        t = time.time()
        runs.append(dict(arm(views, wa, wb, a.seed, a.steps, a.rays), seconds=round(time.time() - t, 1)))
        print(runs[-1], flush=True)
        with open(a.out, "w") as f:
            json.dump(dict(what="CPU study of the depth-prior weights with the oracle's autograd (scripts/study_depth_prior_weights.py)",
                           steps=a.steps, rays=a.rays, runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
