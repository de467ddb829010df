"""What the engine-level GPU tests (test_gpu_views, _pose, _cameras, _localize, _intrinsics, _distortion, _exposure, _window,
_step_forms) build their scenes from: the device, the lego-lowres fixture nets and the small random ones, a stack of perturbed views,
the embedding functions, the draw queue, the engine-state snapshot, the step scene whose launch counts the step_launches*.json
fixtures record, and the 64 x 64 lego scene of the occupancy and spread tests.  A helper module, not a test module: no test module
imports another one."""
import os

import numpy as np
import pytest
import torch

from conftest import gold  # noqa: F401, I001 (first: outside pytest this is what puts the package and the oracle on sys.path)
import pose_vjp as P  # noqa: I001

CFG = dict(num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
CFG64 = dict(num_layers=4, hidden_size=64, skip_connect_every=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4)
STEP_LAUNCHES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_launches.json")
V, RAYS = 3, 256


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch.device("cuda", 0)


def lego(dev, precision="fp32"):
    import nerf_pytorch_amd as N
    w, r = gold("lego_lowres_weights.npz"), gold("lego_lowres_render.npz")
    mc, mf = N.FlexibleNeRFModel(**CFG), N.FlexibleNeRFModel(**CFG)
    mc.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("c_")})
    mf.load_state_dict({k[2:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("f_")})
    mc, mf = mc.to(dev), mf.to(dev)
    if precision != "fp32":
        mc.set_training_precision(precision), mf.set_training_precision(precision)
    return mc, mf, int(r["H"]), int(r["W"]), float(np.float32(r["focal"])), r["pose"].astype(np.float32)


def small(dev, seed=11):
    """Two frozen random 4x64 nets on the lego fixture's camera."""
    import nerf_pytorch_amd as N
    torch.manual_seed(seed)
    mc, mf = N.FlexibleNeRFModel(**CFG64).to(dev), N.FlexibleNeRFModel(**CFG64).to(dev)
    for p in list(mc.parameters()) + list(mf.parameters()):
        p.requires_grad_(False)
    _, _, H, W, focal, pose0 = lego(dev)
    return mc, mf, H, W, focal, pose0


AABB = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))


def lego64():
    """The lego-lowres fixture nets, the fixture pose cut to 64 x 64 rays with a random target, and ONE grid from from_models at its
    defaults."""
    import nerf_pytorch_amd as N
    dev = torch.device("cuda", 0)
    mc, mf = lego(dev)[:2]
    r = gold("lego_lowres_render.npz")
    H = W = 64
    focal = float(r["focal"]) * 64.0 / float(r["W"])     # (the file's fp64 focal, not lego()'s fp32 one)
    pose = torch.from_numpy(r["pose"]).to(dev)
    opts = N.make_options(64, 64, perturb=False, white_background=True, radiance_field_noise_std=0.0)
    pix = torch.arange(H * W, dtype=torch.int64, device=dev)
    ro, rd = N.get_rays_at_pixels(H, W, focal, pose[:3, :4], pix)
    rays = N.pack_rays(ro, rd, opts, H, W, focal)
    target = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    grid = N.OccupancyGrid.from_models(mc, mf, AABB)
    return dict(N=N, dev=dev, mc=mc, mf=mf, H=H, W=W, focal=focal, pose=pose, opts=opts, rays=rays, target=target, grid=grid)


def se3(xi):
    """4 x 4 transform of a twist-like 6-vector (rotation by Rodrigues' formula, translation as given)."""
    T = torch.zeros(4, 4, dtype=xi.dtype, device=xi.device)
    T = T + torch.nn.functional.pad(P.rodrigues(xi[:3]), (0, 1, 0, 1))
    T = T + torch.nn.functional.pad(xi[3:, None], (3, 0, 0, 1))
    T = T + torch.nn.functional.pad(torch.ones(1, 1, dtype=xi.dtype, device=xi.device), (3, 0, 3, 0))
    return T


def se3_exp(xi):
    """4 x 4 SE(3) exponential of a twist [w, v] in torch (fp32 here): the kernel's exponential restated per view -- series in th^2
    below 1e-2 (three terms: the first one left out is below 1e-10 of the sum), closed forms above."""
    w, v = xi[:3], xi[3:]
    x = (w * w).sum()
    small = x < 1e-2
    xs = torch.where(small, torch.ones_like(x), x)    # (no 0 / 0 in the branch torch.where does not select)
    th = torch.sqrt(xs)
    a = torch.where(small, 1 - x / 6 + x * x / 120, torch.sin(th) / th)
    b = torch.where(small, 0.5 - x / 24 + x * x / 720, (1 - torch.cos(th)) / xs)
    c = torch.where(small, 1 / 6 - x / 120 + x * x / 5040, (th - torch.sin(th)) / (xs * th))
    z = torch.zeros_like(x)
    K = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    eye = torch.eye(3, dtype=xi.dtype, device=xi.device)
    K2 = K @ K
    R, t = eye + a * K + b * K2, (eye + b * K + c * K2) @ v
    top = torch.cat([R, t[:, None]], 1)
    return torch.cat([top, torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=xi.dtype, device=xi.device)], 0)


def ex_ed():
    import nerf_pytorch_amd as N
    return N.get_embedding_function(10, True, True), N.get_embedding_function(4, True, True)


def views(pose0, dev, V, scale=0.05, seed=2):
    """V poses: the fixture pose times small se(3) offsets."""
    g = torch.Generator().manual_seed(seed)
    base = torch.from_numpy(pose0)
    return torch.stack([base @ se3(torch.randn(6, generator=g) * scale) for _ in range(V)]).to(dev).contiguous()


def queue_draws(draws):
    queue = list(draws)
    real = torch.rand, torch.randn
    torch.rand = lambda *a, **k: queue.pop(0)
    torch.randn = lambda *a, **k: queue.pop(0)
    return real


def state(eng):
    return [t.clone() for t in (eng.mc.flat_params, eng.mf.flat_params, eng.exp_avg, eng.exp_avg_sq, eng.grad, eng.packed_c, eng.packed_f)]


class Scene:
    """The step scene: the small nets, 8 + 8 samples, RAYS rays, V views, the dense backward."""

    def __init__(self):
        import nerf_pytorch_amd as N
        self.N, self.dev = N, dev()
        self.mc, self.mf, self.H, self.W, self.focal, pose0 = small(self.dev)
        self.opts = N.make_options(8, 8)
        self.imgs = torch.rand(V, self.H, self.W, 3, generator=torch.Generator().manual_seed(1)).to(self.dev)
        self.base = views(pose0, self.dev, V)

    def engine(self, **kw):
        return self.N.TrainEngine(self.mc, self.mf, 8, 8, perturb=True, white_background=True, noise_std=0.2, seed=3, lr=5e-4, rank=0,
                                  backward="dense", **kw)

    def table(self):
        return self.N.CameraTable(self.base, lr=2e-3)

    def intrinsics(self):
        return self.N.Intrinsics(self.H, self.W, self.focal * 1.02, learn="all", lr=1e-3, device=self.dev)

    def distortion(self):
        return self.N.Distortion((-0.05, 0.01, 0.0, 0.0), learn="radial", lr=1e-3, device=self.dev)

    def exposure(self):
        return self.N.Exposure(V, learn="affine", lr=1e-3, device=self.dev)

    def image_args(self):
        return (self.imgs[0], self.base[0], self.H, self.W, self.focal, self.opts, RAYS)

    def views_args(self, poses=True):
        return (self.imgs, self.base if poses else None, self.H, self.W, self.focal, self.opts, RAYS)


def form_launches(scene, forms, make_objects):
    """{form: {kernel name: launches}} of the second step of every form of `forms` ({form: step(*objects)}; the first step warms
    up), on fresh objects -- make_objects() -- for each."""
    out = {}
    for form, step in forms.items():
        objects = make_objects()
        step(*objects)
        with scene.N.LaunchProfile() as prof:
            step(*objects)
        out[form] = prof.counts()
    return out
