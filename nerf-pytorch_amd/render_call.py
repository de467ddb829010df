"""RenderCall: the one place that spells the fused render's entry points (include/nerfhip.h: nerfhip_render_fwd*, nerfhip_render_bwd*,
nerfhip_render_grad_rays, nerfhip_spread_loss on the render's workspace, and the size / region helpers that must be asked with the
same plans, cfg, n and layout).  ctypes only: addresses are integers or None -- what tensor.data_ptr() gives, and what the test
backends' ptr() gives --, and the library is passed in, so the emulator build is driven by the same code as the product.

A RenderCall fixes what every call of ONE render shares; the methods add what differs per call.  It owns no memory: whoever builds
it keeps the buffers alive for as long as the launches need them.
"""
import ctypes as C

from . import _lib as L


class RenderCall:
    def __init__(self, lib, plan_c, plan_f, cfg, rays, n, packed_c, packed_f, t_vals, u_det, rand=None, seed=0, ray_offset=0, layout=0,
                 ws=None, ws_bytes=0, regions=None):
        """cfg: a RenderCfg; rand: None (in-kernel draws) or the four addresses (t_rand, noise_coarse, u, noise_fine; any may be None);
        layout: the workspace layout -- 0 inference, 1 training with one set of backward buffers per net, 2 training with one shared
        set; ws / ws_bytes: the workspace (attributes: may be set once it is allocated); regions: a dict the region lookups are cached
        in -- pass one dict to every call of the same (plans, cfg, n, layout) and they are asked of the library once."""
        self.lib, self.plan_c, self.plan_f, self.cfg, self.rays, self.n = lib, plan_c, plan_f, cfg, rays, n
        self.t_vals, self.u_det, self.seed, self.ray_offset, self.layout = t_vals, u_det, seed, ray_offset, layout
        self.rand = (None,) * 4 if rand is None else tuple(rand)
        self._rr = None if rand is None else L.RenderRand(*self.rand)
        self.ws, self.ws_bytes = ws, ws_bytes
        self._regions = {} if regions is None else regions
        self._cfg_ref = C.byref(cfg)
        # (what every backward entry point starts with; the forwards put t_vals, u_det behind the packed images)
        self._head = (plan_c, plan_f, self._cfg_ref, rays, n, packed_c, packed_f)
        self._draws = (None if self._rr is None else C.byref(self._rr), seed, ray_offset)

    # ---- sizes (no workspace needed) ------------------------------------------------------------------------------------------------
    @staticmethod
    def _size(lib, nbytes):
        if nbytes < 0:
            raise L.NerfHipError(lib.last_error().decode())
        return nbytes

    @staticmethod
    def workspace_bytes(lib, plan_c, plan_f, cfg, n, layout):
        return RenderCall._size(lib, lib.render_workspace_bytes(plan_c, plan_f, C.byref(cfg), n, layout))

    @staticmethod
    def tmp_bytes(lib, plan_c, plan_f, cfg, n):
        """(bytes of the tmp of a backward with a ray gradient, bytes of the tmp of the frozen ray gradient)."""
        return (RenderCall._size(lib, lib.render_bwd_rays_tmp_bytes(plan_c, plan_f, C.byref(cfg), n)),
                RenderCall._size(lib, lib.render_grad_rays_tmp_bytes(plan_c, plan_f, C.byref(cfg), n)))

    @staticmethod
    def occ_tmp_bytes(lib, cfg, n):
        """Bytes of the list area of the culled forwards (its first four words: {kept, total} of the coarse, then of the fine pass)."""
        return RenderCall._size(lib, lib.render_occ_tmp_bytes(C.byref(cfg), n))

    # ---- the workspace ----------------------------------------------------------------------------------------------------------------
    def region(self, name):
        """(byte offset, bytes) of a region of the workspace ("z_coarse", "raw_fine", "bwd_scratch_coarse", ...)."""
        r = self._regions.get(name)
        if r is None:
            off, nb = C.c_int64(), C.c_int64()
            self.lib.render_workspace_region(self.plan_c, self.plan_f, self._cfg_ref, self.n, self.layout, name.encode(), C.byref(off),
                                             C.byref(nb))
            r = self._regions[name] = (off.value, nb.value)
        return r

    def stats_offset(self, net):
        """Byte offset in the workspace of the {kept, total} words a backward over a sample list of net "coarse" / "fine" leaves."""
        plan, samples = (self.plan_c, self.cfg.num_coarse) if net == "coarse" else (self.plan_f, self.cfg.num_coarse + self.cfg.num_fine)
        return self.region("bwd_scratch_" + net)[0] + self.lib.plan_bwd_stats_offset(plan, self.n * samples)

    # ---- the launches -----------------------------------------------------------------------------------------------------------------
    def forward(self, out, parts, stream, occ=None):
        """out: the eight map addresses in RenderOut's order; parts: NERFHIP_PART_* (None: the whole render through the plain
        nerfhip_render_fwd); occ: None, or (grid_c, grid_f, tmp, tmp_bytes) with the grids as OccGrid structs (or None) -- the culled
        forward: nerfhip_render_fwd_occ in layout 0, nerfhip_render_fwd_occ_train in the training layouts."""
        args = self._head + (self.t_vals, self.u_det) + self._draws + (C.byref(L.RenderOut(*out)), self.ws, self.ws_bytes, self.layout)
        if occ is None:
            if parts is None:
                return self.lib.render_fwd(*args, stream)
            return self.lib.render_fwd_parts(*args, parts, stream)
        grid_c, grid_f, tmp, tmp_bytes = occ
        fn = self.lib.render_fwd_occ if self.layout == 0 else self.lib.render_fwd_occ_train
        return fn(*args, parts, None if grid_c is None else C.byref(grid_c), None if grid_f is None else C.byref(grid_f), tmp, tmp_bytes,
                  stream)

    def backward(self, cot, g_params, parts, stream, g_weights=None, rays=None, frozen=False):
        """cot: the six cotangent addresses in RenderCotangents' order; g_params: (coarse, fine) flat gradient addresses; g_weights: None
        or the (coarse, fine) weight cotangents; rays: None or (flat_c, flat_f, tmp, tmp_bytes, g_rays) -- the ray gradient as well.
        The entry point:  nerfhip_render_bwd_parts    neither g_weights nor rays      nerfhip_render_bwd_parts_w   g_weights
                          nerfhip_render_bwd_rays     rays                            nerfhip_render_bwd_rays_w    both
                          nerfhip_render_grad_rays    frozen: needs rays, takes no g_weights, and g_params is not looked at.
        Layout 2 adds NERFHIP_PART_SHARED_BWD to parts."""
        if self.layout == 0:
            raise ValueError("RenderCall.backward: the forward ran in the inference layout, which keeps nothing for a backward")
        if self.layout == 2:
            parts |= L.PART_SHARED_BWD
        lib, head = self.lib, self._head + self._draws
        if frozen:
            if rays is None or g_weights is not None:
                raise ValueError("RenderCall.backward: frozen=True is the ray gradient alone: it needs rays=... and takes no g_weights")
            return lib.render_grad_rays(*head, C.byref(L.RenderCotangents(*cot)), self.ws, self.ws_bytes, parts, *rays, stream)
        if g_weights is None:
            g, parts_fn, rays_fn = L.RenderCotangents(*cot), lib.render_bwd_parts, lib.render_bwd_rays
        else:
            g, parts_fn, rays_fn = L.RenderCotangentsW(*cot, *g_weights), lib.render_bwd_parts_w, lib.render_bwd_rays_w
        args = head + (C.byref(g), self.ws, self.ws_bytes, g_params[0], g_params[1], parts)
        if rays is None:
            return parts_fn(*args, stream)
        return rays_fn(*args, *rays, stream)

    def backward_rgb(self, g_rgb_c, g_rgb_f, g_params, stream):
        """The convenience export nerfhip_render_bwd: both nets from their colour cotangents, on ONE shared set of backward buffers
        whatever the layout."""
        return self.lib.render_bwd(*self._head, *self._draws, g_rgb_c, g_rgb_f, self.ws, self.ws_bytes, g_params[0], g_params[1], stream)

    def spread(self, fine, scale, g_loss, loss, g_weights, stream):
        """nerfhip_spread_loss of one pass over the raw rows and depths its forward left in the workspace, with that pass's noise."""
        tag, S = ("fine", self.cfg.num_coarse + self.cfg.num_fine) if fine else ("coarse", self.cfg.num_coarse)
        return self.lib.spread_loss(self.ws + self.region("raw_" + tag)[0], self.ws + self.region("z_" + tag)[0], self.rays,
                                    self.cfg.ray_stride, self.n, S, self.cfg.noise_std, self.rand[3 if fine else 1], self.seed,
                                    3 if fine else 1, self.ray_offset, scale, g_loss, loss, g_weights, stream)

    def depth_prior(self, fine, prior, prior_stride, inds, prior_rows, w_expected, w_termination, scale, g_loss, loss, g_weights,
                    accumulate, stream):
        """nerfhip_depth_prior_loss of one pass over the same regions and with the same noise stream as `spread`.  prior: the table
        (rows of prior_stride floats: depth, weight, sigma); inds: None (ray r reads row r) or the int64 row index of every ray."""
        tag, S = ("fine", self.cfg.num_coarse + self.cfg.num_fine) if fine else ("coarse", self.cfg.num_coarse)
        return self.lib.depth_prior_loss(self.ws + self.region("raw_" + tag)[0], self.ws + self.region("z_" + tag)[0], self.rays,
                                         self.cfg.ray_stride, self.n, S, self.cfg.noise_std, self.rand[3 if fine else 1], self.seed,
                                         3 if fine else 1, self.ray_offset, prior, prior_stride, inds, prior_rows, w_expected,
                                         w_termination, scale, g_loss, loss, g_weights, int(bool(accumulate)), stream)

    def proposal(self, scale, g_loss, loss, g_weights, accumulate, stream):
        """nerfhip_proposal_loss over the raw rows and depths BOTH passes' forwards left in the workspace, each with its pass's noise:
        the per-ray interlevel loss and its gradient w.r.t. the coarse pass's weights (g_weights: [n, num_coarse])."""
        cfg = self.cfg
        if cfg.num_fine <= 0:
            raise ValueError("RenderCall.proposal: the interlevel loss needs a fine pass (num_fine > 0)")
        reg = lambda name: self.ws + self.region(name)[0]  # noqa: E731
        return self.lib.proposal_loss(reg("raw_coarse"), reg("z_coarse"), cfg.num_coarse, reg("raw_fine"), reg("z_fine"),
                                      cfg.num_coarse + cfg.num_fine, self.rays, cfg.ray_stride, self.n, cfg.noise_std, self.rand[1],
                                      self.rand[3], self.seed, self.ray_offset, scale, g_loss, loss, g_weights, int(bool(accumulate)),
                                      stream)
