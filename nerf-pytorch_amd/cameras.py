"""Camera table: se(3) pose refinement composed, differentiated and stepped on the device.

pose[v] = base[v] @ Exp(xi[v]) -- a camera-frame perturbation; xi = [w (3), v (3)] and Exp the full SE(3) exponential (the
reference's lieutils.SE3.Exp, twist order [w, v]).  One launch composes every view (nerfhip_pose_table_fwd), one launch pulls
d(loss)/d(poses) back to the twists (nerfhip_pose_table_bwd), and the twists are stepped by the fused Adam kernel the nets use
(nerfhip_adam_step on the flat [V * 6] vector).

* ``se3_poses(xi, base)`` -- the drop-in form: an autograd node when `xi` requires grad, the same launch otherwise.
* ``CameraTable`` -- owns the twists, their Adam state and every buffer; ``TrainEngine.step_on_views(cameras=table)`` runs the joint
  field-and-camera step with no host work besides launches.
* ``Intrinsics`` -- the shared intrinsics (fx, fy, cx, cy) on the device, their log-focal parametrisation and its Adam state;
  ``TrainEngine.step_on_views(intrinsics=...)`` learns them next to the field and the poses.
* ``Distortion`` -- the shared lens distortion (k1, k2, p1, p2) on the device with its Adam state;
  ``TrainEngine.step_on_views(distortion=...)`` learns it next to the field, the poses and the intrinsics.
* ``Exposure`` -- a colour log-gain and offset per view and channel on the device with its Adam state: the photometric side of a real
  capture (auto-exposure, auto-white-balance); ``TrainEngine.step_on_views(exposure=...)`` learns it next to everything above,
  ``localize_on_views(exposure=...)`` fits it against frozen nets.
"""
import torch

from . import _lib as L
from .train_utils import _pose_table


def _base_table(base, num_views):
    if base.dim() != 3 or base.shape[0] != num_views or base.shape[1] < 3 or base.shape[2] < 4:
        raise RuntimeError("base must be a (V = %d, >=3, >=4) tensor (got shape %s)" % (num_views, tuple(base.shape)))
    return _pose_table(base, True)


def _twists(xi):
    if xi.dim() != 2 or xi.shape[1] != 6 or xi.shape[0] < 1:
        raise RuntimeError("xi must be a (V, 6) tensor of twists [w, v] (got shape %s)" % (tuple(xi.shape),))
    return xi.detach().float().contiguous()


def _compose(xi, base, out):
    with L.launch_on(xi, base, out) as st:
        L.get_lib().pose_table_fwd(xi.data_ptr(), base.data_ptr(), base.stride(0), base.stride(1), xi.shape[0], out.data_ptr(), st)
    return out


def _pull_back(xi, base, g_poses, active, out):
    with L.launch_on(xi, base, g_poses, active, out) as st:
        L.get_lib().pose_table_bwd(xi.data_ptr(), base.data_ptr(), base.stride(0), base.stride(1), xi.shape[0], g_poses.data_ptr(),
                                   active.data_ptr() if active is not None else None, out.data_ptr(), st)
    return out


class _Se3Poses(torch.autograd.Function):
    """se3_poses with its closed-form VJP: the gradient flows from the (V, 3, 4) poses to the twists; the base carries none.  The
    forward issues exactly the launch of the plain call."""

    @staticmethod
    def forward(ctx, xi, base):
        x, b = _twists(xi), _base_table(base, xi.shape[0])
        ctx.save_for_backward(xi, base)   # (the inputs themselves: changing one in place before the backward is an autograd error)
        return _compose(x, b, torch.empty((x.shape[0], 3, 4), dtype=torch.float32, device=x.device))

    @staticmethod
    def backward(ctx, g_poses):
        xi, base = ctx.saved_tensors
        x = _twists(xi)
        g = _pull_back(x, _base_table(base, x.shape[0]), g_poses.float().contiguous(), None, torch.empty_like(x))
        return g.to(xi.dtype), None


def se3_poses(xi, base):
    """poses (V, 3, 4) = base[:, :3, :4] @ Exp(xi): one launch.  xi: (V, 6) twists [w, v] on the device; base: (V, >=3, 4) (a strided
    slice of a larger table is read in place).  The result is directly a pose table of select_training_rays_views.  With `xi`
    requiring grad the poses are differentiable w.r.t. it (one more launch in the backward), so
    select_training_rays_views(..., poses=se3_poses(xi, base), ...) -> loss.backward() -> torch.optim.Adam([xi]) refines the
    cameras; `base` gets no gradient.  A view whose twist is exactly zero gets its base bit for bit."""
    if torch.is_grad_enabled() and xi.requires_grad:
        return _Se3Poses.apply(xi, base)
    x = _twists(xi)
    return _compose(x, _base_table(base, x.shape[0]), torch.empty((x.shape[0], 3, 4), dtype=torch.float32, device=x.device))


def check_device_vector(t, shape, dev, what=None):
    """Whether `t` is a contiguous float32 tensor of shape `shape` on `dev`; with `what` ("Owner: name") anything else raises."""
    ok = (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32 and tuple(t.shape) == tuple(shape)
          and t.is_contiguous())
    if not ok and what is not None:
        raise RuntimeError("%s must be a contiguous float32 (%s) tensor on %s" % (what, ", ".join(str(d) for d in shape), dev))
    return ok


class _AdamVector:
    """A learned device vector with its Adam state: the parameter `_param` ("xi" / "q" / "dist" / "expo"), its gradient buffer "g_" + _param,
    the two moments, step_count, lr, betas, eps; the state dict holds the parameter, the moments, `base` (where the vector is a
    perturbation of one) and the step count."""

    def _init_adam(self, shape, lr, betas, eps):
        self.lr, self.betas, self.eps = lr, betas, eps
        self.step_count = 0
        self._state = (self._param, "exp_avg", "exp_avg_sq", "base")
        for name in (self._param, "g_" + self._param, "exp_avg", "exp_avg_sq"):
            setattr(self, name, torch.zeros(shape, dtype=torch.float32, device=self.dev))

    def step(self, lr=None):
        """One Adam step of the parameter on the gradient the last backward() left: the fused kernel the nets use."""
        self.step_count += 1
        b1, b2 = self.betas
        p, g = getattr(self, self._param), getattr(self, "g_" + self._param)
        with L.launch_on(p, g) as st:
            self.lib.adam_step(p.data_ptr(), g.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), p.numel(),
                               self.lr if lr is None else lr, b1, b2, self.eps, self.step_count, 1.0, st)

    def state_dict(self):
        return dict({k: getattr(self, k).clone() for k in self._state}, step=self.step_count)

    def load_state_dict(self, state):
        for k in self._state:
            t = getattr(self, k)
            if tuple(state[k].shape) != tuple(t.shape):
                raise RuntimeError("%s.load_state_dict: %s has shape %s, %s holds %s"
                                   % (type(self).__name__, k, tuple(state[k].shape), self._holder, tuple(t.shape)))
            t.copy_(state[k])
        self.step_count = int(state["step"])


class CameraTable(_AdamVector):
    """The cameras of a capture under refinement: one twist per view on top of a fixed base pose, with the Adam state of the
    twists.  Every buffer is allocated here once; poses(), backward() and step() are one launch each on the current stream of the
    table's device, with no host synchronisation.

    base_poses: (V, >=3, 4) device tensor (copied).  active: None (every view is refined) or V booleans: an inactive view's
    gradient is exactly zero, so its twist stays where it is -- at zero its pose stays its base bit for bit (freezing one anchor
    view fixes the gauge of a joint refinement)."""
    _param, _holder = "xi", "the table"

    def __init__(self, base_poses, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, active=None):
        if not isinstance(base_poses, torch.Tensor) or not base_poses.is_cuda:
            raise RuntimeError("CameraTable needs the base poses on a CUDA (HIP) device (nerf_pytorch_amd has no CPU path)")
        if base_poses.dim() != 3 or base_poses.shape[0] < 1 or base_poses.shape[1] < 3 or base_poses.shape[2] != 4:
            raise RuntimeError("base_poses must be a (V, >=3, 4) tensor (got shape %s)" % (tuple(base_poses.shape),))
        self.lib = L.get_lib()
        self.dev = base_poses.device
        self.base = base_poses.detach()[:, :3, :4].float().contiguous().clone()
        self.num_views = v = self.base.shape[0]
        self._init_adam((v, 6), lr, betas, eps)
        self.g_poses, self._poses = (torch.zeros((v, 3, 4), dtype=torch.float32, device=self.dev) for _ in range(2))
        self.active = None
        if active is not None:
            a = torch.as_tensor(active, device=self.dev)
            if a.numel() != v:
                raise RuntimeError("active must hold one flag per view (%d), got %d" % (v, a.numel()))
            self.active = (a.reshape(v) != 0).to(torch.uint8).contiguous()

    def poses(self):
        """Composes base @ Exp(xi) into the table's own (V, 3, 4) buffer and returns it (overwritten by the next call)."""
        return _compose(self.xi, self.base, self._poses)

    def backward(self, g_poses=None):
        """d(loss)/d(xi) (the table's own (V, 6) buffer) from d(loss)/d(poses): `g_poses`, a contiguous float32 (V, 3, 4) device
        tensor, or None for the table's own `g_poses` buffer (the one step_on_views(cameras=...) fills)."""
        g = self.g_poses if g_poses is None else g_poses
        check_device_vector(g, (self.num_views, 3, 4), self.dev, "CameraTable: g_poses")
        return _pull_back(self.xi, self.base, g, self.active, self.g_xi)

    def pose_matrices(self):
        """The current poses as a detached (V, 4, 4) tensor (bottom row 0 0 0 1), e.g. for saving."""
        out = torch.zeros((self.num_views, 4, 4), dtype=torch.float32, device=self.dev)
        out[:, :3] = self.poses()
        out[:, 3, 3] = 1.0
        return out


_LEARN = {"focal": (True, (1, 0, 0, 0)), "focal_xy": (False, (1, 1, 0, 0)), "all": (False, (1, 1, 1, 1)), (): (False, (0, 0, 0, 0))}


class Intrinsics(_AdamVector):
    """The shared intrinsics (fx, fy, cx, cy) of a capture under refinement, resident on the device, with the Adam state of their
    parametrisation q: fx = fx0 exp(q0), fy = fy0 exp(q1) (exp(q0) when the focals are tied), cx = cx0 + q2, cy = cy0 + q3 -- the
    log-focal keeps the focal positive and makes Adam's step a relative one.  Every buffer is allocated here once; values(),
    backward() and step() are one launch each on the current stream of the device, with no host synchronisation, so a learned
    focal is never read back inside a step.

    focal: one number (fx = fy = focal, cx = float32(width / 2), cy = float32(height / 2): the camera of the scalar path, whose
    bits values() then gives while q is zero), or the four numbers (fx, fy, cx, cy).  learn: "focal" (one focal: fx and fy tied,
    the principal point fixed), "focal_xy" (fx and fy apart), "all", or () (nothing moves).  An entry that is not learned gets an
    exact zero gradient, so its q stays where it is.  The NDC constants of a forward-facing scene are fixed by the caller's
    `focal_length` and do not follow these values."""
    _param, _holder = "q", "the object"

    def __init__(self, height, width, focal, learn="focal", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, device=None):
        key = tuple(learn) if isinstance(learn, (list, tuple)) else learn
        if key not in _LEARN:
            raise RuntimeError('Intrinsics: learn must be "focal", "focal_xy", "all" or () (got %r)' % (learn,))
        self.dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("Intrinsics lives on a CUDA (HIP) device (nerf_pytorch_amd has no CPU path)")
        try:
            four = [float(v) for v in focal]
        except TypeError:
            f = float(focal)
            four = [f, f, float(torch.tensor(int(width) * 0.5, dtype=torch.float32)), float(torch.tensor(int(height) * 0.5, dtype=torch.float32))]
        if len(four) != 4 or not (four[0] > 0 and four[1] > 0):
            raise RuntimeError("Intrinsics: focal must be one positive number or (fx, fy, cx, cy) with positive focals (got %r)" % (focal,))
        self.lib = L.get_lib()
        self.height, self.width = int(height), int(width)
        self.learn = key
        self.tie_focal, mask = _LEARN[key]
        self._init_adam((4,), lr, betas, eps)
        self.base = torch.tensor(four, dtype=torch.float32).to(self.dev)
        self.mask = torch.tensor(mask, dtype=torch.uint8).to(self.dev)
        self.g_intr = torch.zeros(4, dtype=torch.float32, device=self.dev)
        self._values = self.base.clone()

    def values(self):
        """Evaluates (fx, fy, cx, cy) into the object's own buffer of 4 and returns it (overwritten by the next call): the
        `intrinsics` of select_training_rays / get_ray_bundle / render_pose_rows."""
        with L.launch_on(self.q, self.base, self._values) as st:
            self.lib.intrinsics_fwd(self.q.data_ptr(), self.base.data_ptr(), int(self.tie_focal), self._values.data_ptr(), st)
        return self._values

    def backward(self, g_intr=None):
        """d(loss)/d(q) (the object's own buffer) from d(loss)/d(fx, fy, cx, cy): `g_intr`, a contiguous float32 device tensor of
        4, or None for the object's own `g_intr` buffer (the one a step with intrinsics=... fills)."""
        g = self.g_intr if g_intr is None else g_intr
        check_device_vector(g, (4,), self.dev, "Intrinsics: g_intr")
        with L.launch_on(self.q, self.base, g, self.mask, self.g_q) as st:
            self.lib.intrinsics_bwd(self.q.data_ptr(), self.base.data_ptr(), int(self.tie_focal), g.data_ptr(), self.mask.data_ptr(),
                                    self.g_q.data_ptr(), st)
        return self.g_q

    def state_dict(self):
        return dict(super().state_dict(), learn=self.learn)

    def load_state_dict(self, state):
        if "learn" in state and (tuple(state["learn"]) if isinstance(state["learn"], (list, tuple)) else state["learn"]) != self.learn:
            raise RuntimeError("Intrinsics.load_state_dict: the state was saved with learn=%r, this object has learn=%r"
                               % (state["learn"], self.learn))
        super().load_state_dict(state)


_LEARN_DIST = {"radial": (1, 1, 0, 0), "all": (1, 1, 1, 1), (): (0, 0, 0, 0)}


class Distortion(_AdamVector):
    """The shared lens distortion (k1, k2, p1, p2) of a capture under refinement (COLMAP's OPENCV model, include/nerfhip.h), resident
    on the device, with its Adam state.  The coefficients are stepped directly -- there is no parametrisation between them and
    Adam --: the selection's VJP writes d(loss)/d(k1, k2, p1, p2) into `g_dist` (an entry that is not learned gets an exact zero
    there, so it stays where it is) and step() is the fused Adam kernel the nets use, on the four floats.  Every buffer is allocated
    here once; no host synchronisation.

    coeffs: the four starting values.  learn: "radial" (k1 and k2; the tangential p1 and p2 fixed), "all", or () (nothing moves)."""
    _param, _holder = "dist", "the object"

    def __init__(self, coeffs=(0.0, 0.0, 0.0, 0.0), learn="radial", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, device=None):
        key = tuple(learn) if isinstance(learn, (list, tuple)) else learn
        if key not in _LEARN_DIST:
            raise RuntimeError('Distortion: learn must be "radial", "all" or () (got %r)' % (learn,))
        self.dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("Distortion lives on a CUDA (HIP) device (nerf_pytorch_amd has no CPU path)")
        four = [float(v) for v in coeffs]
        if len(four) != 4:
            raise RuntimeError("Distortion: coeffs must be the four numbers (k1, k2, p1, p2) (got %r)" % (coeffs,))
        self.lib = L.get_lib()
        self.learn = key
        self._init_adam((4,), lr, betas, eps)
        self._state = ("dist", "exp_avg", "exp_avg_sq")
        self.dist.copy_(torch.tensor(four, dtype=torch.float32))
        self.mask = torch.tensor(_LEARN_DIST[key], dtype=torch.uint8).to(self.dev)

    def values(self):
        """(k1, k2, p1, p2): the object's own parameter of 4, the `distortion` of select_training_rays / get_ray_bundle /
        render_pose_rows (the kernels read it in place; no launch)."""
        return self.dist

    def state_dict(self):
        return dict(super().state_dict(), learn=self.learn)

    def load_state_dict(self, state):
        if "learn" in state and (tuple(state["learn"]) if isinstance(state["learn"], (list, tuple)) else state["learn"]) != self.learn:
            raise RuntimeError("Distortion.load_state_dict: the state was saved with learn=%r, this object has learn=%r"
                               % (state["learn"], self.learn))
        super().load_state_dict(state)


_LEARN_EXPO = {"affine": (1, 1, 1, 1, 1, 1), "gain": (1, 1, 1, 0, 0, 0), (): (0, 0, 0, 0, 0, 0)}


def exposure_grad(rgb_coarse, rgb_fine, target, inds, hw, table, grad_scale=1.0, mask=None, tmp=None, out=None):
    """nerfhip_exposure_bwd on the current stream of the tensors' device: d(loss_coarse + loss_fine)/d(table) (V x 6 float32) of
    the loss under the table (include/nerfhip.h), into `out` (or a new tensor).  rgb_*: contiguous float32 (n, 3) (rgb_fine may be
    None); target: (n, >= 3) rows of unit-stride floats; inds: the selection's int64 global indices; tmp: None, or a float32 scratch
    of at least nerfhip_exposure_grad_tmp_bytes(n, V) bytes.  Three launches, no host synchronisation."""
    lib = L.get_lib()
    if not isinstance(table, torch.Tensor) or not table.is_cuda or table.dim() != 2:
        raise RuntimeError("exposure_grad: table must be a (V, 6) tensor on a CUDA (HIP) device")
    dev, nv = table.device, table.shape[0]
    check_device_vector(table, (nv, 6), dev, "exposure_grad: table")
    if not isinstance(rgb_coarse, torch.Tensor) or rgb_coarse.dim() != 2:
        raise RuntimeError("exposure_grad: rgb_coarse must be a contiguous float32 (n, 3) tensor on %s" % dev)
    n = rgb_coarse.shape[0]
    check_device_vector(rgb_coarse, (n, 3), dev, "exposure_grad: rgb_coarse")
    if rgb_fine is not None:
        check_device_vector(rgb_fine, (n, 3), dev, "exposure_grad: rgb_fine")
    if not (isinstance(target, torch.Tensor) and target.device == dev and target.dtype == torch.float32 and target.dim() == 2
            and target.shape[0] == n and target.shape[1] >= 3 and target.stride(1) == 1):
        raise RuntimeError("exposure_grad: target must hold one row of >= 3 unit-stride float32 per ray (%d) on %s" % (n, dev))
    if not (isinstance(inds, torch.Tensor) and inds.device == dev and inds.dtype == torch.int64 and tuple(inds.shape) == (n,)
            and inds.is_contiguous()):
        raise RuntimeError("exposure_grad: inds must be a contiguous int64 (%d) tensor on %s" % (n, dev))
    if mask is not None and not (isinstance(mask, torch.Tensor) and mask.device == dev and mask.dtype == torch.uint8
                                 and tuple(mask.shape) == (nv, 6) and mask.is_contiguous()):
        raise RuntimeError("exposure_grad: mask must be a contiguous uint8 (%d, 6) tensor on %s" % (nv, dev))
    tb = lib.exposure_grad_tmp_bytes(n, nv)
    if tb < 0:
        raise RuntimeError("exposure_grad: %d rays over %d views is outside the kernel's limits" % (n, nv))
    if tmp is None:
        tmp = torch.empty(tb // 4 + 1, dtype=torch.float32, device=dev)
    elif not (isinstance(tmp, torch.Tensor) and tmp.device == dev and tmp.dtype == torch.float32 and tmp.is_contiguous()
              and tmp.numel() * 4 >= tb):
        raise RuntimeError("exposure_grad: tmp must be a contiguous float32 tensor of at least %d bytes on %s" % (tb, dev))
    if out is None:
        out = torch.empty((nv, 6), dtype=torch.float32, device=dev)
    else:
        check_device_vector(out, (nv, 6), dev, "exposure_grad: out")
    with L.launch_on(rgb_coarse, rgb_fine, target, inds, table, mask, tmp, out) as st:
        lib.exposure_bwd(rgb_coarse.data_ptr(), rgb_fine.data_ptr() if rgb_fine is not None else None, target.data_ptr(),
                         target.stride(0), n, float(grad_scale), inds.data_ptr(), int(hw), table.data_ptr(), nv,
                         mask.data_ptr() if mask is not None else None, tmp.data_ptr(), tmp.numel() * 4, out.data_ptr(), st)
    return out


class Exposure(_AdamVector):
    """The per-view exposure of a capture: row v of the (V, 6) table `expo` is (s_r, s_g, s_b, b_r, b_g, b_b), and a ray of view v
    is compared with its target as exp(s) * rgb + b per channel, coarse and fine alike (include/nerfhip.h).  Resident on the device
    with its Adam state; the table is stepped directly.  It sits behind the render, so its gradient needs no ray gradient:
    backward() is nerfhip_exposure_bwd (three launches) on the two rgb buffers, the targets and the selection's global indices, and
    step() is the fused Adam kernel the nets use.  Every buffer is allocated here (the scratch of backward() once per batch size that
    grows it); no host synchronisation.

    learn: "affine" (gain and offset), "gain" (the s columns only), or () (nothing moves).  anchor: views that stay at the
    identity -- their rows of `mask` are all zero, so their gradient is an exact zero --: one anchored view removes the global
    gain / offset ambiguity between the field and the table; anchor=() anchors none."""
    _param, _holder = "expo", "the object"

    def __init__(self, num_views, learn="affine", anchor=(0,), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, device=None):
        key = tuple(learn) if isinstance(learn, (list, tuple)) else learn
        if key not in _LEARN_EXPO:
            raise RuntimeError('Exposure: learn must be "affine", "gain" or () (got %r)' % (learn,))
        self.dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("Exposure lives on a CUDA (HIP) device (nerf_pytorch_amd has no CPU path)")
        self.num_views = v = int(num_views)
        if v < 1:
            raise RuntimeError("Exposure: num_views must be >= 1 (got %r)" % (num_views,))
        self.anchor = tuple(sorted(set(int(a) for a in anchor)))
        if any(a < 0 or a >= v for a in self.anchor):
            raise RuntimeError("Exposure: anchor views must be in 0 .. %d (got %r)" % (v - 1, anchor))
        self.lib = L.get_lib()
        self.learn = key
        self._init_adam((v, 6), lr, betas, eps)
        self._state = ("expo", "exp_avg", "exp_avg_sq")
        mask = torch.tensor(_LEARN_EXPO[key], dtype=torch.uint8).repeat(v, 1)
        if self.anchor:
            mask[list(self.anchor)] = 0
        self.mask = mask.to(self.dev).contiguous()
        self._tmp = None

    def values(self):
        """The (V, 6) table: the object's own parameter, the `table` of train_utils.exposure_mse_loss (the kernels read it in
        place; no launch)."""
        return self.expo

    def backward(self, rgb_coarse, rgb_fine, target, inds, hw, grad_scale=1.0):
        """d(loss)/d(expo) into the object's own `g_expo` (masked entries: exact zeros), from the rgb the nets rendered for the batch
        (rgb_fine may be None), its targets and its global indices `inds` (view = inds // hw)."""
        tb = self.lib.exposure_grad_tmp_bytes(rgb_coarse.shape[0], self.num_views)
        if tb >= 0 and (self._tmp is None or self._tmp.numel() * 4 < tb):
            self._tmp = torch.empty(tb // 4 + 1, dtype=torch.float32, device=self.dev)
        return exposure_grad(rgb_coarse, rgb_fine, target, inds, hw, self.expo, grad_scale, self.mask, self._tmp, self.g_expo)

    def apply(self, rgb, view):
        """exp(s) * rgb + b with row `view`, for an evaluation image rendered at that view: plain torch arithmetic on the device."""
        row = self.expo[int(view)]
        return rgb[..., :3] * torch.exp(row[:3]) + row[3:]

    def state_dict(self):
        return dict(super().state_dict(), learn=self.learn, anchor=self.anchor)

    def load_state_dict(self, state):
        if "learn" in state and (tuple(state["learn"]) if isinstance(state["learn"], (list, tuple)) else state["learn"]) != self.learn:
            raise RuntimeError("Exposure.load_state_dict: the state was saved with learn=%r, this object has learn=%r"
                               % (state["learn"], self.learn))
        if "anchor" in state and tuple(int(a) for a in state["anchor"]) != self.anchor:
            raise RuntimeError("Exposure.load_state_dict: the state was saved with anchor=%r, this object has anchor=%r"
                               % (tuple(state["anchor"]), self.anchor))
        super().load_state_dict(state)
