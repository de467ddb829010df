"""CPU study behind `alpha_loss` of tests/test_gpu_matte.py's capability test: the oracle's autograd (oracle/nerf_oracle.py) on the
setup of DESIGN.md 3.21 -- six 64 x 64 teacher views of the lego-lowres fixture nets (dense oracle render, 64 + 64 samples, white
background), the 60-degree view held out, three of the other five (0, 40 and 80 degrees) training two 4 x 64 students for 400 Adam
steps of 1024 rays, lr 5e-3, sigma noise 1.0.  The RGBA targets: a = clamp(teacher acc_fine, 0, 1), C = clamp((rgb_white - (1 - a)) /
max(a, 1e-3), 0, 1).

  plain arm   the render composited onto white against a C + (1 - a): what the library did with RGBA data before alpha=.
  matte arms  the render without a background against the matte over a random background per ray and step (the definition restated
              in torch by tests/matte_cases.py::matte_terms), plus alpha_loss * mean (acc - a)^2 per net, alpha_loss in {0, 0.01, 0.1, 1}.

Reports, on the held-out view (no perturbation, no noise): PSNR over white of the fine map (rgb + 1 - acc against the teacher's white
render) and the mean |acc_fine - a|.  The rule, fixed here before any GPU run: of the matte arms whose PSNR is no lower than the plain
arm's minus 0.5 dB, the one with the lowest opacity error (`chosen` in the output).

    python scripts/study_matte_weights.py --out profiles/r21_matte_study.json [--arms plain 0 0.01 0.1 1] [--steps 400] [--jobs 5]
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
import matte_cases as M  # noqa: E402

ANGLES, HELD_OUT, TRAIN = (0.0, 20.0, 40.0, 60.0, 80.0, 100.0), 3, (0, 2, 4)
TEACHER = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
STUDENT = dict(TEACHER, hidden_size=64)
NC = NF = 64
PSNR_SLACK_DB = 0.5


def passes(rays, par_c, par_f, cfg, perturb, noise_std, gen, white):
    """Both passes of the oracle's render: dict(rgb_c, acc_c, rgb_f, acc_f)."""
    n = rays.shape[0]
    ro, rd = rays[:, :3], rays[:, 3:6]
    z = O.stratified_z(rays[:, 6:7], rays[:, 7:8], NC, False, perturb, torch.rand(n, NC, generator=gen) if perturb else None)
    nz = (lambda s: torch.randn(n, s, generator=gen)) if noise_std > 0 else (lambda s: None)
    raw_c = O.run_network(par_c, ro[:, None, :] + rd[:, None, :] * z[:, :, None], rays, cfg)
    rgb_c, _, acc_c, w_c, _ = O.volume_render(raw_c, z, rd, noise_std, nz(NC), white)
    _, z_f = O.hierarchical_z(z, w_c, NF, det=not perturb, u=torch.rand(n, NF, generator=gen) if perturb else None)
    raw_f = O.run_network(par_f, ro[:, None, :] + rd[:, None, :] * z_f[:, :, None], rays, cfg)
    rgb_f, _, acc_f, _, _ = O.volume_render(raw_f, z_f, rd, noise_std, nz(NC + NF), white)
    return dict(rgb_c=rgb_c, acc_c=acc_c, rgb_f=rgb_f, acc_f=acc_f)


def teacher_views():
    """(rays [6, 4096, 11], the teacher's white render [6, 4096, 3], RGBA targets [6, 4096, 4])."""
    w = np.load(os.path.join(ROOT, "tests", "golden", "lego_lowres_weights.npz"))
    r = np.load(os.path.join(ROOT, "tests", "golden", "lego_lowres_render.npz"))
    par_c = {k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("c_")}
    par_f = {k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("f_")}
    focal = float(r["focal"]) * 64.0 / float(r["W"])
    pose0 = torch.from_numpy(r["pose"]).float()
    rays, white, rgba = [], [], []
    for deg in ANGLES:
        a = np.deg2rad(deg)
        rot = torch.tensor([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=torch.float32)
        ro, rd = O.get_ray_bundle(64, 64, focal, rot @ pose0[:3, :4])
        rows = O.pack_rays(ro, rd, 2.0, 6.0, rd)
        with torch.no_grad():
            out = passes(rows, par_c, par_f, TEACHER, False, 0.0, None, True)
        alpha = out["acc_f"].clamp(0.0, 1.0)
        C = ((out["rgb_f"] - (1.0 - alpha)[:, None]) / alpha.clamp(min=1e-3)[:, None]).clamp(0.0, 1.0)
        rays.append(rows)
        white.append(out["rgb_f"])
        rgba.append(torch.cat((C, alpha[:, None]), dim=1))
    return torch.stack(rays), torch.stack(white), torch.stack(rgba)


def arm(spec, seed, steps, n_rays, threads=0, lr=5e-3, noise_std=1.0):
    if threads:
        torch.set_num_threads(threads)
    t0 = time.time()
    rays, white, rgba = teacher_views()
    plain = spec == "plain"
    lam = 0.0 if plain else float(spec)
    train = list(TRAIN)
    pool_r, pool_t = rays[train].reshape(-1, rays.shape[-1]), rgba[train].reshape(-1, 4)
    par = [{k: v.requires_grad_(True) for k, v in O.init_params(STUDENT, seed=2 * seed + i).items()} for i in (0, 1)]
    flat = [v for p in par for v in p.values()]
    m, v = [torch.zeros_like(t) for t in flat], [torch.zeros_like(t) for t in flat]
    gen = torch.Generator().manual_seed(seed)
    picks = torch.randint(0, pool_r.shape[0], (steps, n_rays), generator=torch.Generator().manual_seed(seed))
    bgen = torch.Generator().manual_seed(seed + 4)
    finite = True
    for i in range(steps):
        r, t = pool_r[picks[i]], pool_t[picks[i]]
        o = passes(r, par[0], par[1], STUDENT, True, noise_std, gen, plain)
        if plain:
            tw = t[:, 3:] * t[:, :3] + (1.0 - t[:, 3:])
            loss = ((o["rgb_c"] - tw) ** 2).mean() + ((o["rgb_f"] - tw) ** 2).mean()
        else:
            bg = torch.rand(n_rays, 3, generator=bgen)
            loss = 0.0
            for tag in ("c", "f"):
                photo, alpha, _ = M.matte_terms(o["rgb_" + tag], o["acc_" + tag], t, 0, bg)
                loss = loss + photo + lam * alpha
        finite = finite and bool(torch.isfinite(loss.detach()))
        grads = torch.autograd.grad(loss, flat)
        with torch.no_grad():
            for q, g, mm, vv in zip(flat, grads, m, v):
                O.adam_step(q, g, mm, vv, i + 1, lr)
    with torch.no_grad():
        o = passes(rays[HELD_OUT], par[0], par[1], STUDENT, False, 0.0, None, False)
        over_white = o["rgb_f"] + (1.0 - o["acc_f"])[:, None]
        mse = float(((over_white - white[HELD_OUT]).double() ** 2).mean())
        aerr = float((o["acc_f"] - rgba[HELD_OUT][:, 3]).abs().double().mean())
    return dict(arm=spec, seed=seed, psnr_over_white=float(-10.0 * np.log10(max(mse, 1e-30))), acc_err=aerr,
                final_loss=float(loss.detach()), finite=finite, seconds=round(time.time() - t0, 1))


def choose(runs):
    plain = [r for r in runs if r["arm"] == "plain"]
    matte = [r for r in runs if r["arm"] != "plain" and r["finite"]]
    if not plain or not matte:
        return None
    ok = [r for r in matte if r["psnr_over_white"] >= plain[0]["psnr_over_white"] - PSNR_SLACK_DB] or matte
    return float(min(ok, key=lambda r: r["acc_err"])["arm"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--arms", nargs="+", default=["plain", "0", "0.01", "0.1", "1"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--threads", type=int, default=0)
    a = ap.parse_args()
    jobs = [(spec, a.seed, a.steps, a.rays, a.threads) for spec in a.arms]
    if a.jobs > 1:
        import torch.multiprocessing as mp
        with mp.get_context("spawn").Pool(a.jobs) as pool:
            runs = pool.starmap(arm, jobs)
    else:
        runs = [arm(*j) for j in jobs]
    for r in runs:
        print(r, flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(what="CPU study of alpha_loss with the oracle's autograd (scripts/study_matte_weights.py)", steps=a.steps,
                       rays=a.rays, rule="lowest acc_err among the matte arms with psnr_over_white >= plain - %.1f dB" % PSNR_SLACK_DB,
                       chosen=choose(runs), runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
