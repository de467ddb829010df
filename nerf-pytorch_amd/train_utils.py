"""Drop-in for ``nerf/train_utils.py``: run_network, predict_and_render_radiance, run_one_iter_of_nerf with the
reference's signatures, defaults and return layout (nerf/train_utils.py:8-202).

When both networks are this package's FlexibleNeRFModel and the encoders come from this package's
get_embedding_function, predict_and_render_radiance runs the fused pipeline of libnerfhip.so (one C-ABI call forward,
one backward; encodings and activations never reach HBM).  Otherwise it composes the unit kernels exactly like the
reference composes its torch ops, so arbitrary user networks still work.

Random draws: made with torch.rand / torch.randn on the rays' device in the reference's order and shapes
(t_rand, coarse noise, u, fine noise per ray chunk), then handed to the kernels -- seeding torch reproduces a run.

Reference quirk kept on purpose: run_one_iter_of_nerf does not forward `mode` to predict_and_render_radiance
(train_utils.py:171-181), so rendering always reads options.nerf.train.* ; only the ray chunk size and the output
reshape honour `mode`.
"""
import contextlib
import ctypes as C
import math

import torch

from . import _lib as L
from . import backward_mode as BM
from .models import FlexibleNeRFModel
from .nerf_helpers import (EmbeddingFunction, _dist_vector, _intr_vector, get_minibatches, linspace01, ndc_rays,
                           sample_pdf_2 as sample_pdf)
from .render_call import RenderCall
from .volume_rendering_utils import volume_render_radiance_field


def run_network(network_fn, pts, ray_batch, chunksize, embed_fn, embeddirs_fn):
    """nerf/train_utils.py:8-25."""
    pts_flat = pts.reshape((-1, pts.shape[-1]))
    embedded = embed_fn(pts_flat)
    if embeddirs_fn is not None:
        viewdirs = ray_batch[..., None, -3:]
        input_dirs = viewdirs.expand(pts.shape)
        input_dirs_flat = input_dirs.reshape((-1, input_dirs.shape[-1]))
        embedded_dirs = embeddirs_fn(input_dirs_flat)
        embedded = torch.cat((embedded, embedded_dirs), dim=-1)
    batches = get_minibatches(embedded, chunksize=chunksize)
    preds = [network_fn(batch) for batch in batches]
    radiance_field = torch.cat(preds, dim=0)
    return radiance_field.reshape(list(pts.shape[:-1]) + [radiance_field.shape[-1]])


# ---- fused path -------------------------------------------------------------------------------------------------------
def _fusable(model_coarse, model_fine, enc_xyz, enc_dir, num_fine):
    if not isinstance(model_coarse, FlexibleNeRFModel):
        return False
    if num_fine > 0 and not isinstance(model_fine, FlexibleNeRFModel):
        return False
    models = [model_coarse] + ([model_fine] if num_fine > 0 else [])
    for m in models:
        c = m.cfg
        if not isinstance(enc_xyz, EmbeddingFunction):
            return False
        if (enc_xyz.num_encoding_functions, bool(enc_xyz.include_input), bool(enc_xyz.log_sampling)) != (
                c["num_encoding_fn_xyz"], c["include_input_xyz"], c["log_sampling_xyz"]):
            return False
        if c["use_viewdirs"]:
            if not isinstance(enc_dir, EmbeddingFunction):
                return False
            if (enc_dir.num_encoding_functions, bool(enc_dir.include_input), bool(enc_dir.log_sampling)) != (
                    c["num_encoding_fn_dir"], c["include_input_dir"], c["log_sampling_dir"]):
                return False
        elif enc_dir is not None:
            return False
    return True


class _FusedRender(torch.autograd.Function):
    """The fused pipeline as one autograd node.  Differentiable outputs: the colour, accumulation and depth maps of both
    passes (what any loss built on the reference's outputs can touch; disparity is derived from depth and acc by the
    caller in torch, so it is covered too).  Inputs with a gradient: the parameters of the two nets, passed one by one
    (they alias each model's flat buffer; backward returns each its slice of the flat gradient).

    With `rays_grad` the ray batch itself receives a gradient (pose optimisation: under autograd the reference
    differentiates pts = ro + rd * z, train_utils.py:67,107, and dists * ||rd||, volume_rendering_utils.py:24): columns
    0..5 (origin, direction) and 8..10 (viewdirs) of d(loss)/d(rays); near / far are constants of the ray.

    The workspace (activation stash, ~4.8 MB per ray for the 8x256 nets) is allocated per call from torch's caching
    allocator and owned by the autograd node: several nodes may be alive at once (run_one_iter_of_nerf renders a batch
    in ray chunks and backpropagates afterwards), so it must not be shared between calls.

    With the `spread` flag (the seventh entry of cfg_tuple) the node has two more differentiable outputs: the per-ray spread loss of
    each pass's ray weights (nerfhip_spread_loss; None for the fine pass without a fine net).  Its forward runs the kernel for the
    losses alone; its backward runs it again with the incoming per-ray cotangents as g_loss and hands the weight cotangents to the _w
    form of the render backward.  The flag is pinned at the forward, as the backward mode is.

    With prior rows (an optional eighth entry of cfg_tuple: a contiguous float32 (n, 3) tensor of (depth, weight, sigma)) the node has
    two more differentiable outputs behind those: the per-ray (E, Tm) of each pass, (n, 2) (nerfhip_depth_prior_loss; None for the fine
    pass without a fine net).  Its backward runs the kernel again with the incoming cotangents as g_loss -- accumulating behind the
    spread term where both are asked for -- and calls the _w form of the render backward.

    With the `proposal` flag (an optional ninth entry of cfg_tuple; needs a fine net) the node has one more differentiable output behind
    those: the per-ray interlevel loss (n) (nerfhip_proposal_loss), differentiable w.r.t. the COARSE net only.  Its backward runs the
    kernel again with the incoming cotangent as g_loss -- accumulating behind the coarse pass's spread and depth terms -- for the
    coarse weight cotangent of the _w render backward."""

    @staticmethod
    def forward(ctx, rays, model_c, model_f, cfg_tuple, rand, training, rays_grad, *params):
        lib = L.get_lib()
        nc, nf, perturb, lindisp, white, noise_std, spread = cfg_tuple[:7]
        prior = cfg_tuple[7] if len(cfg_tuple) > 7 else None
        proposal = bool(cfg_tuple[8]) if len(cfg_tuple) > 8 else False
        if proposal and nf <= 0:
            raise ValueError("proposal=True needs a fine net (num_fine > 0): the loss bounds the fine pass's weights")
        n, stride = rays.shape
        dev = rays.device
        cfg = L.RenderCfg(nc, nf, int(bool(perturb)), int(bool(lindisp)), int(bool(white)), float(noise_std), stride)
        # `training` (decided by the caller: grad mode is off inside Function.forward, and needs_input_grad ignores
        # torch.no_grad()): keep the activation stash for a backward
        # (inference -- no backward follows -- runs on each model's inference plan: fp32 unless set_inference_precision
        # chose the fp16-piece kernels)
        if training:  # (models with set_backward_compaction("auto") pick the mode of this pass from their last compacted backward)
            model_c._auto_choose_backward()
            if nf > 0:
                model_f._auto_choose_backward()
        plan_c = model_c._plan if training else model_c._inference_plan()
        plan_f = (model_f._plan if training else model_f._inference_plan()) if nf > 0 else None
        # (training layout 2: this node's backward runs the two nets one after the other on one stream, so they share one
        # set of backward buffers -- several nodes may be alive at once when a batch is rendered in ray chunks)
        layout = 2 if training else 0
        wsb = RenderCall.workspace_bytes(lib, plan_c, plan_f, cfg, n, layout)
        ws = torch.empty(wsb // 4 + 1, dtype=torch.float32, device=dev)
        ctx.set_materialize_grads(False)  # cotangents of outputs the loss never touched arrive as None, not as zeros
        names = ("rgb_coarse", "disp_coarse", "acc_coarse", "depth_coarse", "rgb_fine", "disp_fine", "acc_fine",
                 "depth_fine")
        bufs = {k: torch.empty((n, 3) if k.startswith("rgb") else (n,), dtype=torch.float32, device=dev) for k in names}
        packed_c = model_c._packed() if training else model_c._inference_packed()
        packed_f = (model_f._packed() if training else model_f._inference_packed()) if nf > 0 else None
        ctx.call = call = RenderCall(lib, plan_c, plan_f, cfg, rays.data_ptr(), n, packed_c.data_ptr(), _ptr(packed_f),
                                     linspace01(nc, dev).data_ptr(), linspace01(nf, dev).data_ptr() if nf > 0 else None,
                                     [_ptr(r) for r in rand], 0, 0, layout, ws.data_ptr(), wsb)
        with L.launch_on(rays, ws, packed_c, packed_f, *[r for r in rand if r is not None]) as st:
            call.forward([bufs[k].data_ptr() for k in names], None, st)
        # (the ray gradient multiplies by the weights of THIS forward: keep copies only if it will be asked for)
        # (... of the nets as they ran: theta_eff under an encoding window)
        flats = (model_c._theta_eff(copy=True), model_f._theta_eff(copy=True) if nf > 0 else None) if (training and rays_grad) else None
        # (the window is schedule state of the model: the node's backward windows its gradients as its forward was windowed)
        ctx.windows = (model_c._window_w, model_f._window_w if nf > 0 else None)
        ctx.keep = (rays, model_c, model_f, ws, flats)
        # (ctx.call holds addresses and plan handles: what else stands behind them, kept alive for the node's backward)
        ctx.alive = (rand, packed_c, packed_f, (model_c._plan_owner, model_f._plan_owner if nf > 0 else None) if training else None)
        # (the backward data flow is an option of the PLAN, and what this forward left in the workspace -- the general stash, nothing, the
        # register-image stash -- depends on it: the node's backward runs in the mode its forward ran in, whatever
        # set_backward_compaction was called with in between)
        ctx.bwd_modes = (lib.plan_bwd_compaction(plan_c), lib.plan_bwd_compaction(plan_f) if plan_f is not None else 0) if training else None
        # (... and with the frozen flag of its forward: set_frozen on both nets and a ray batch that wants a gradient -> the backward is
        # the ray gradient alone, nerfhip_render_grad_rays)
        ctx.frozen = bool(training and rays_grad and model_c.frozen and (nf == 0 or model_f.frozen))
        ctx.n_params = len(params)
        ctx.mark_non_differentiable(bufs["disp_coarse"], bufs["disp_fine"])
        ctx.spread = bool(spread)
        ctx.prior = prior
        ctx.proposal = proposal
        if not spread and prior is None and not proposal:
            return tuple(bufs[k] for k in names)
        if ctx.frozen:
            raise ValueError("spread=True, depth_prior=... or proposal=True on frozen nets (set_frozen) makes no sense: these losses regularise the nets")
        tail = ()
        if spread:
            sp = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2 if nf > 0 else 1)]
            with L.launch_on(rays, ws, *sp) as st:
                for fine, out_sp in enumerate(sp):   # (the losses alone, over the raw rows and depths the forward left in its workspace)
                    call.spread(fine, 1.0, None, out_sp.data_ptr(), None, st)
            tail += (sp[0], sp[1] if nf > 0 else None)
        if prior is not None:
            dp = [torch.empty((n, 2), dtype=torch.float32, device=dev) for _ in range(2 if nf > 0 else 1)]
            with L.launch_on(rays, ws, prior, *dp) as st:
                for fine, out_dp in enumerate(dp):
                    call.depth_prior(fine, prior.data_ptr(), 3, None, n, 1.0, 1.0, 1.0, None, out_dp.data_ptr(), None, False, st)
            tail += (dp[0], dp[1] if nf > 0 else None)
        if proposal:
            pl = torch.empty(n, dtype=torch.float32, device=dev)
            with L.launch_on(rays, ws, pl) as st:   # (the loss alone, over both passes' raw rows and depths)
                call.proposal(1.0, None, pl.data_ptr(), None, False, st)
            tail += (pl,)
        return tuple(bufs[k] for k in names) + tail

    @staticmethod
    def backward(ctx, g_rgb_c, g_disp_c, g_acc_c, g_depth_c, g_rgb_f, g_disp_f, g_acc_f, g_depth_f, *g_tail):
        call, lib = ctx.call, ctx.call.lib
        rays, model_c, model_f, ws, flats = ctx.keep
        if call.layout == 0:
            raise RuntimeError("fused render was run without gradient bookkeeping")
        n = rays.shape[0]
        dev = rays.device
        cfg = call.cfg
        nf = cfg.num_fine
        keep = [None if g is None else g.contiguous().float()
                for g in (g_rgb_c, g_acc_c, g_depth_c, g_rgb_f, g_acc_f, g_depth_f)]
        parts = 0
        g_tail = [None if g is None else g.contiguous().float() for g in g_tail]
        g_sp = (g_tail[:2] if ctx.spread else []) + [None, None]
        g_dp = (g_tail[2:4] if ctx.spread else g_tail[:2]) + [None, None] if ctx.prior is not None else [None, None]
        g_pp = g_tail[2 * (int(ctx.spread) + int(ctx.prior is not None))] if ctx.proposal else None
        if any(k is not None for k in keep[:3]) or g_sp[0] is not None or g_dp[0] is not None or g_pp is not None:
            parts |= L.PART_COARSE
        if nf > 0 and (any(k is not None for k in keep[3:]) or g_sp[1] is not None or g_dp[1] is not None):
            parts |= L.PART_FINE
        if ctx.frozen:
            return (_FusedRender._frozen_backward(ctx, keep, parts),) + (None,) * (6 + ctx.n_params)
        gpc = torch.zeros(model_c.num_flat_params, dtype=torch.float32, device=dev)
        gpf = torch.zeros(model_f.num_flat_params, dtype=torch.float32, device=dev) if nf > 0 else None
        g_rays = torch.zeros_like(rays) if flats is not None else None
        if parts:
            gw = [None, None]
            for fine in (0, 1):   # (the weight cotangents of the passes whose spread or depth losses a loss touched)
                if g_sp[fine] is not None or g_dp[fine] is not None or (not fine and g_pp is not None):
                    gw[fine] = torch.empty((n, cfg.num_coarse + (nf if fine else 0)), dtype=torch.float32, device=dev)
            g_weights = [_ptr(g) for g in gw] if (gw[0] is not None or gw[1] is not None) else None
            tmp = rays_args = None
            if g_rays is not None:
                tmpb = RenderCall.tmp_bytes(lib, call.plan_c, call.plan_f, cfg, n)[0]
                tmp = torch.empty(tmpb // 4 + 4, dtype=torch.float32, device=dev)
                rays_args = (flats[0].data_ptr(), _ptr(flats[1]), tmp.data_ptr(), tmpb, g_rays.data_ptr())
            # "auto" models read the {kept, total} words of their compacted backward; the two nets share one set of backward buffers
            # here (the fine pass runs first), so the passes are issued one by one with the copy in between -- the same launches in
            # the same order as the single call (not with a ray gradient: its second pass accumulates into the first one's)
            auto = [m for m in (model_c, model_f) if m is not None and m._backward_choice == "auto"]
            passes = [parts]
            if auto and g_rays is None and parts == (L.PART_COARSE | L.PART_FINE):
                passes = [L.PART_FINE, L.PART_COARSE]
            with _forward_modes(ctx), L.launch_on(rays, ws, gpc, gpf, tmp, *[k for k in keep if k is not None]) as st:
                for fine in (0, 1):
                    if g_sp[fine] is not None:
                        call.spread(fine, 1.0, g_sp[fine].data_ptr(), None, gw[fine].data_ptr(), st)
                    if g_dp[fine] is not None:   # (behind the spread term: added to the cotangent it wrote)
                        call.depth_prior(fine, ctx.prior.data_ptr(), 3, None, n, 1.0, 1.0, 1.0, g_dp[fine].data_ptr(), None,
                                         gw[fine].data_ptr(), g_sp[fine] is not None, st)
                if g_pp is not None:   # (behind the coarse pass's spread and depth terms: added to the cotangent they wrote)
                    call.proposal(1.0, g_pp.data_ptr(), None, gw[0].data_ptr(), g_sp[0] is not None or g_dp[0] is not None, st)
                for part in passes:
                    call.backward([_ptr(k) for k in keep], (gpc.data_ptr(), _ptr(gpf)), part, st, g_weights, rays_args)
                    # (the words in the shared buffers: the coarse net's behind a pass that ran it -- it runs last --, the fine net's
                    # only between the two passes)
                    model, net, mode = (model_c, "coarse", ctx.bwd_modes[0]) if part & L.PART_COARSE else (model_f, "fine", ctx.bwd_modes[1])
                    if (part & L.PART_COARSE or len(passes) == 2) and model in auto and mode in BM.BUILDS_LIST:
                        model._stats.request([("net", BM.stats_words(call, net, ws))], torch.cuda.current_stream(dev))
        model_c._window_grads(gpc, ctx.windows[0])
        if nf > 0:
            model_f._window_grads(gpf, ctx.windows[1])
        grads = model_c._split_flat(gpc) + (model_f._split_flat(gpf) if nf > 0 else ())
        return (g_rays,) + (None,) * 6 + grads

    @staticmethod
    def _frozen_backward(ctx, keep, parts):
        """d(loss)/d(rays) of a node whose nets were frozen at its forward: no parameter gradient exists anywhere."""
        call = ctx.call
        rays, _, _, ws, flats = ctx.keep
        g_rays = torch.zeros_like(rays)
        if not parts:
            return g_rays
        tmpb = RenderCall.tmp_bytes(call.lib, call.plan_c, call.plan_f, call.cfg, call.n)[1]
        tmp = torch.empty(tmpb // 4 + 4, dtype=torch.float32, device=rays.device)
        with _forward_modes(ctx), L.launch_on(rays, ws, tmp, *[k for k in keep if k is not None]) as st:
            call.backward([_ptr(k) for k in keep], None, parts, st, None,
                          (flats[0].data_ptr(), _ptr(flats[1]), tmp.data_ptr(), tmpb, g_rays.data_ptr()), frozen=True)
        return g_rays


def _ptr(t):
    return None if t is None else t.data_ptr()


@contextlib.contextmanager
def _forward_modes(ctx):
    """The plans of a _FusedRender node in the backward modes its forward ran in (ctx.bwd_modes), for the duration of its backward."""
    lib = ctx.call.lib
    pins = [(p, was, lib.plan_bwd_compaction(p)) for p, was in zip((ctx.call.plan_c, ctx.call.plan_f), ctx.bwd_modes) if p is not None]
    for plan, was, cur in pins:
        if was != cur:
            lib.plan_set_bwd_compaction(plan, was)
    try:
        yield
    finally:
        for plan, was, cur in pins:
            if was != cur:
                lib.plan_set_bwd_compaction(plan, cur)


def _check_prior_rows(depth_prior, n, dev):
    if (not isinstance(depth_prior, torch.Tensor) or depth_prior.device != dev or depth_prior.dtype != torch.float32
            or tuple(depth_prior.shape) != (n, 3)):
        raise ValueError("depth_prior must be a float32 (%d, 3) tensor of (depth, weight, sigma) rows on %s" % (n, dev))
    return depth_prior.detach().contiguous()


def _predict_fused(ray_batch, model_coarse, model_fine, opts, occupancy=None, spread=False, depth_prior=None, proposal=False):
    rays_grad = bool(ray_batch.requires_grad and torch.is_grad_enabled())
    rays = ray_batch.contiguous().float() if rays_grad else ray_batch.detach().contiguous().float()
    n = rays.shape[0]
    dev = rays.device
    nc, nf = opts.num_coarse, opts.num_fine
    perturb, noise_std = opts.perturb, opts.radiance_field_noise_std
    # the reference's draw order per ray chunk (train_utils.py:63, volume_rendering_utils.py:30, nerf_helpers.py:279,
    # volume_rendering_utils.py:30)
    t_rand = torch.rand((n, nc), dtype=torch.float32, device=dev) if perturb else None
    noise_c = torch.randn((n, nc), dtype=torch.float32, device=dev) if noise_std > 0.0 else None
    u = torch.rand((n, nf), dtype=torch.float32, device=dev) if (nf > 0 and not (perturb == 0.0)) else None
    noise_f = torch.randn((n, nc + nf), dtype=torch.float32, device=dev) if (nf > 0 and noise_std > 0.0) else None
    cfg_tuple = (nc, nf, bool(perturb), bool(opts.lindisp), bool(opts.white_background), float(noise_std))
    pc = model_coarse._ordered_params()
    pf = model_fine._ordered_params() if nf > 0 else []
    for m, ps in ((model_coarse, pc), (model_fine, pf)):
        if ps and m.frozen and any(p.requires_grad for p in ps):
            raise RuntimeError("a frozen model (set_frozen) has a parameter that requires grad: freeze the parameters "
                               "(p.requires_grad_(False)) or call set_frozen(False)")
    training = torch.is_grad_enabled() and (rays_grad or any(p.requires_grad for p in pc + pf))
    if occupancy is not None:
        if training:
            raise NotImplementedError(_OCC_TRAIN_MSG)
        from .occupancy import render_fwd_occ
        outs = render_fwd_occ(rays, model_coarse, model_fine if nf > 0 else None, cfg_tuple, (t_rand, noise_c, u, noise_f), occupancy)
        rgb_c, disp_c, acc_c, _, rgb_f, disp_f, acc_f, _ = outs
        return (rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f) if nf > 0 else (rgb_c, disp_c, acc_c, None, None, None)
    tail_cfg = (bool(spread),) if depth_prior is None else (bool(spread), _check_prior_rows(depth_prior, n, dev))
    if proposal:   # (the ninth entry; without it the tuple is what it always was)
        tail_cfg = (tail_cfg + (None,))[:2] + (True,)
    outs = _FusedRender.apply(rays, model_coarse, model_fine if nf > 0 else None, cfg_tuple + tail_cfg,
                              (t_rand, noise_c, u, noise_f), training, rays_grad, *pc, *pf)
    rgb_c, disp_c, acc_c, depth_c, rgb_f, disp_f, acc_f, depth_f = outs[:8]
    # (spread=True: the two per-ray spread losses; depth_prior: the two (n, 2) depth losses behind them; proposal=True: the per-ray
    # interlevel loss last)
    tail = tuple(outs[8:])
    if rgb_c.requires_grad:
        # disparity re-derived from the differentiable depth / accumulation maps with the reference's own torch ops
        # (volume_rendering_utils.py:46-48: same values as the kernel's, and autograd covers a loss on it)
        disp_c = 1.0 / torch.max(1e-10 * torch.ones_like(depth_c), depth_c / acc_c)
        if nf > 0:
            disp_f = 1.0 / torch.max(1e-10 * torch.ones_like(depth_f), depth_f / acc_f)
    if nf > 0:
        return (rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f) + tail
    return (rgb_c, disp_c, acc_c, None, None, None) + tail


_OCC_TRAIN_MSG = ("an occupancy grid culls the inference render only: pass occupancy= with mode=\"validation\" under torch.no_grad() "
                  "(the training forward and its backward run dense)")


def _predict_culled(ray_batch, model_coarse, model_fine, opts, encode_position_fn, encode_direction_fn, occupancy):
    """A ray chunk through the fused render with an occupancy grid (the caller has checked the mode)."""
    if not _fusable(model_coarse, model_fine, encode_position_fn, encode_direction_fn, opts.num_fine):
        raise NotImplementedError("an occupancy grid needs the fused render (FlexibleNeRFModel nets and their own embedding functions)")
    return _predict_fused(ray_batch, model_coarse, model_fine, opts, occupancy)


def predict_and_render_radiance(ray_batch, model_coarse, model_fine, options, mode="train", encode_position_fn=None,
                                encode_direction_fn=None, occupancy=None, spread=False, depth_prior=None, proposal=False):
    """nerf/train_utils.py:28-127.  Returns (rgb_coarse, disp_coarse, acc_coarse, rgb_fine, disp_fine, acc_fine).
    spread: True (train mode on the fused path only; anything else raises ValueError) -- the tuple gains two trailing tensors, the
    per-ray spread loss of each pass's ray weights (mip-NeRF 360's L_dist; include/nerfhip.h nerfhip_spread_loss): spread_coarse (n) and
    spread_fine (n; None without a fine net), both differentiable w.r.t. the nets.
    depth_prior: None, or the batch's prior rows, float32 (n, 3) of (depth, weight, sigma), weight 0 = no prior (train mode on the fused
    path only; anything else raises ValueError) -- the tuple gains two more trailing tensors, behind the spread pair when both are asked
    for: depth_loss_coarse (n, 2) and depth_loss_fine (n, 2; None without a fine net), each ray's (E, Tm) of include/nerfhip.h
    nerfhip_depth_prior_loss, differentiable w.r.t. the nets.
    proposal: True (train mode on the fused path with a fine net only; anything else raises ValueError) -- the tuple gains one more
    trailing tensor, behind the spread and depth tensors when those are asked for: proposal_loss (n), each ray's interlevel loss of
    include/nerfhip.h nerfhip_proposal_loss (mip-NeRF 360's L_prop), differentiable w.r.t. the COARSE net only.
    occupancy: None, or an occupancy.OccupancyGrid -- with mode="validation" and no gradient wanted, the samples in its empty cells
    skip the MLPs (nerfhip_render_fwd_occ) and the chunk's counts are added to the grid's view_counts; in train mode it raises
    NotImplementedError."""
    if not ray_batch.is_cuda:
        raise RuntimeError("predict_and_render_radiance needs CUDA (HIP) tensors: nerf_pytorch_amd has no CPU path")
    opts = getattr(options.nerf, mode)
    if spread and (mode != "train" or occupancy is not None
                   or not _fusable(model_coarse, model_fine, encode_position_fn, encode_direction_fn, opts.num_fine)):
        raise ValueError("spread=True needs mode=\"train\" on the fused render (FlexibleNeRFModel nets and their own embedding functions, "
                         "no occupancy grid)")
    if depth_prior is not None and (mode != "train" or occupancy is not None
                                    or not _fusable(model_coarse, model_fine, encode_position_fn, encode_direction_fn, opts.num_fine)):
        raise ValueError("depth_prior=... needs mode=\"train\" on the fused render (FlexibleNeRFModel nets and their own embedding "
                         "functions, no occupancy grid)")
    if proposal and (mode != "train" or occupancy is not None or opts.num_fine <= 0
                     or not _fusable(model_coarse, model_fine, encode_position_fn, encode_direction_fn, opts.num_fine)):
        raise ValueError("proposal=True needs mode=\"train\" on the fused render with a fine net (FlexibleNeRFModel nets and their own "
                         "embedding functions, num_fine > 0, no occupancy grid)")
    if occupancy is not None:
        if mode != "validation":
            raise NotImplementedError(_OCC_TRAIN_MSG)
        return _predict_culled(ray_batch, model_coarse, model_fine, opts, encode_position_fn, encode_direction_fn, occupancy)
    if _fusable(model_coarse, model_fine, encode_position_fn, encode_direction_fn, opts.num_fine):
        kw = {"proposal": True} if proposal else {}
        if depth_prior is None:
            return _predict_fused(ray_batch, model_coarse, model_fine, opts, spread=spread, **kw)
        return _predict_fused(ray_batch, model_coarse, model_fine, opts, spread=spread, depth_prior=depth_prior, **kw)

    # generic composition (arbitrary networks / encoders), mirroring the reference step by step
    lib = L.get_lib()
    num_rays = ray_batch.shape[0]
    rays = ray_batch.detach().contiguous().float()
    ro, rd = rays[..., :3], rays[..., 3:6]
    dev = rays.device
    nc = opts.num_coarse
    t_rand = torch.rand((num_rays, nc), dtype=torch.float32, device=dev) if opts.perturb else None
    z_vals = torch.empty((num_rays, nc), dtype=torch.float32, device=dev)
    with L.launch_on(rays, t_rand, z_vals) as st:
        lib.stratified_z(rays.data_ptr(), rays.shape[1], num_rays, linspace01(nc, dev).data_ptr(), nc,
                         int(bool(opts.lindisp)), int(bool(opts.perturb)), t_rand.data_ptr() if t_rand is not None else None,
                         0, 0, z_vals.data_ptr(), st)
    pts = ro[..., None, :] + rd[..., None, :] * z_vals[..., :, None]
    radiance_field = run_network(model_coarse, pts, ray_batch, opts.chunksize, encode_position_fn, encode_direction_fn)
    rgb_coarse, disp_coarse, acc_coarse, weights, _ = volume_render_radiance_field(
        radiance_field, z_vals, rd, radiance_field_noise_std=opts.radiance_field_noise_std,
        white_background=opts.white_background)
    rgb_fine, disp_fine, acc_fine = None, None, None
    if opts.num_fine > 0:
        z_vals_mid = 0.5 * (z_vals[..., 1:] + z_vals[..., :-1])
        z_samples = sample_pdf(z_vals_mid, weights[..., 1:-1].detach(), opts.num_fine, det=(opts.perturb == 0.0))
        z_vals, _ = torch.sort(torch.cat((z_vals, z_samples), dim=-1), dim=-1)
        pts = ro[..., None, :] + rd[..., None, :] * z_vals[..., :, None]
        radiance_field = run_network(model_fine, pts, ray_batch, opts.chunksize, encode_position_fn, encode_direction_fn)
        rgb_fine, disp_fine, acc_fine, _, _ = volume_render_radiance_field(
            radiance_field, z_vals, rd, radiance_field_noise_std=opts.radiance_field_noise_std,
            white_background=opts.white_background)
    return rgb_coarse, disp_coarse, acc_coarse, rgb_fine, disp_fine, acc_fine


class _PackRays(torch.autograd.Function):
    """rows [o d near far (v/||v||)] (train_utils.py:143-168) with the gradient autograd gives the reference:
    d(rays)/d(o) = I on columns 0..2, d/d(d) = I on columns 3..5, and the normalisation of the viewdirs columns,
    (g_v - u (u . g_v)) / ||v|| with u = v/||v||, w.r.t. the direction v the reference normalises -- the ray direction itself
    (blender branch) or the PRE-ndc direction (LLFF branch: `vsrc` is a different tensor from `rd` then)."""

    @staticmethod
    def forward(ctx, ro, rd, vsrc, near, far, use_view):
        n = rd.shape[0]
        rays = torch.empty((n, 11 if use_view else 8), dtype=torch.float32, device=rd.device)
        with L.launch_on(ro, rd, vsrc, rays) as st:
            L.get_lib().pack_rays(ro.data_ptr(), rd.data_ptr(), vsrc.data_ptr() if use_view else None, near, far, n,
                                  rays.data_ptr(), st)
        ctx.save_for_backward(vsrc)
        ctx.use_view = use_view
        return rays

    @staticmethod
    def backward(ctx, g):
        (vsrc,) = ctx.saved_tensors
        g_ro, g_rd, g_v = g[:, 0:3].contiguous(), g[:, 3:6].contiguous(), None
        if ctx.use_view:
            nrm = vsrc.norm(p=2, dim=-1, keepdim=True)
            u, gv = vsrc / nrm, g[:, 8:11]
            g_v = (gv - u * (u * gv).sum(-1, keepdim=True)) / nrm
        return g_ro, g_rd, g_v, None, None, None


def pack_rays(ray_origins, ray_directions, options, height=None, width=None, focal_length=None):
    """The ray packing of run_one_iter_of_nerf (nerf/train_utils.py:143-168): rows [o d near far (d/||d||)].
    Differentiable w.r.t. origins and directions (both branches, ndc_rays included) -- what pose optimisation needs."""
    lib = L.get_lib()
    want_grad = torch.is_grad_enabled() and (ray_origins.requires_grad or ray_directions.requires_grad)
    use_view = bool(options.nerf.use_viewdirs)
    if want_grad:
        ro = ray_origins.reshape(-1, 3).contiguous().float()
        rd_src = ray_directions.reshape(-1, 3).contiguous().float()
        rd = rd_src
        if options.dataset.no_ndc is False:  # (train_utils.py:156-160; viewdirs come from the pre-ndc directions: :146-150)
            ro, rd = ndc_rays(height, width, focal_length, 1.0, ro, rd_src)
        return _PackRays.apply(ro, rd, rd_src, float(options.dataset.near), float(options.dataset.far), use_view)
    rd_src = ray_directions.detach().reshape(-1, 3).contiguous().float()
    ro = ray_origins.detach().reshape(-1, 3).contiguous().float()
    rd = rd_src
    if options.dataset.no_ndc is False:
        ro, rd = ndc_rays(height, width, focal_length, 1.0, ro, rd_src)
    n = rd.shape[0]
    rays = torch.empty((n, 11 if use_view else 8), dtype=torch.float32, device=rd.device)
    with L.launch_on(ro, rd, rd_src, rays) as st:
        lib.pack_rays(ro.data_ptr(), rd.data_ptr(), rd_src.data_ptr() if use_view else None, float(options.dataset.near),
                      float(options.dataset.far), n, rays.data_ptr(), st)
    return rays


def _select_cfg(height, width, focal_length, options, channels, seed, step, first):
    f = float(focal_length)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).item()  # noqa: E731
    return L.SelectCfg(height=int(height), width=int(width), focal=f, near=float(options.dataset.near),
                       far=float(options.dataset.far), use_viewdirs=int(bool(options.nerf.use_viewdirs)),
                       ndc=int(options.dataset.no_ndc is False), ndc_near=1.0, ndc_cw=f32(-1.0 / (width / (2.0 * f))),
                       ndc_ch=f32(-1.0 / (height / (2.0 * f))), ndc_two_near=2.0, ndc_neg_two_near=-2.0,
                       channels=int(channels), seed=int(seed) & 0xFFFFFFFFFFFFFFFF, step=int(step), first=int(first))


def _pose_table(poses, views):
    """The pose(s) as the kernels read them: float32, unit column stride (and, with a view axis, rows and views that do not
    overlap); a table that is laid out otherwise is copied.  A 2-D pose is the table with no view axis (`views` False)."""
    if views and (poses.dim() != 3 or poses.shape[1] < 3 or poses.shape[2] < 4):
        raise RuntimeError("poses must be a (V, >=3, >=4) tensor (got shape %s)" % (tuple(poses.shape),))
    p = poses.detach().float()
    ok = p.stride(-1) == 1 and (not views or (p.stride(1) >= 4 and (p.shape[0] == 1 or p.stride(0) >= 2 * p.stride(1) + 4)))
    return p if ok else p.contiguous()


# (the camera model: 0 the scalar pin-hole, 1 device intrinsics, 2 lens distortion; a view axis?) -> the selection's entry point, its
# VJP's, the VJP's tmp-size function.  (The single view without intrinsics keeps its own VJP: two launches where the views form at
# V = 1 issues three.)
_SELECT_ENTRY = {(0, False): ("select_rays", "select_rays_bwd", "pose_grad_tmp_bytes"),
                 (0, True): ("select_rays_views", "select_rays_views_bwd", "pose_grad_views_tmp_bytes"),
                 (1, False): ("select_rays_views_intr", "select_rays_views_intr_bwd", "intr_grad_views_tmp_bytes"),
                 (1, True): ("select_rays_views_intr", "select_rays_views_intr_bwd", "intr_grad_views_tmp_bytes"),
                 (2, False): ("select_rays_views_dist", "select_rays_views_dist_bwd", "dist_grad_views_tmp_bytes"),
                 (2, True): ("select_rays_views_dist", "select_rays_views_dist_bwd", "dist_grad_views_tmp_bytes")}


def _camera_model(intr, dist):
    return 2 if dist is not None else (1 if intr is not None else 0)


def _table_args(poses, views, intr=None, dist=None):
    """The pose arguments of the entry points of _SELECT_ENTRY: (pointer, row stride) of the single pose, or -- with a view axis,
    `intr` or `dist`, whose pointers then lead (intr, or intr | NULL and dist) -- the table (num_views, pointer, view stride, row
    stride); a single pose is the table of one view."""
    if intr is None and dist is None and not views:
        return poses.data_ptr(), poses.stride(-2)
    head = () if intr is None else (intr.data_ptr(),)
    if dist is not None:
        head = (intr.data_ptr() if intr is not None else None, dist.data_ptr())
    if views:
        return head + (poses.shape[0], poses.data_ptr(), poses.stride(0), poses.stride(1))
    return head + (1, poses.data_ptr(), 0, poses.stride(-2))


def _select_launch(cfg, poses, images, select_inds, n, views, intr=None, dist=None):
    """nerfhip_select_rays (`poses` one pose, `images` one image) or, with a view axis, nerfhip_select_rays_views; with `intr` (the
    device intrinsics) nerfhip_select_rays_views_intr in both cases; with `dist` (the device distortion coefficients, with or
    without `intr`) nerfhip_select_rays_views_dist."""
    dev = poses.device
    rays = torch.empty((n, 11 if cfg.use_viewdirs else 8), dtype=torch.float32, device=dev)
    target = torch.empty((n, cfg.channels), dtype=torch.float32, device=dev) if images is not None else None
    used = torch.empty((n,), dtype=torch.int64, device=dev)
    fn = getattr(L.get_lib(), _SELECT_ENTRY[_camera_model(intr, dist), bool(views)][0])
    with L.launch_on(poses, images, select_inds, rays, intr, dist) as st:
        fn(C.byref(cfg), *_table_args(poses, views, intr, dist), images.data_ptr() if images is not None else None,
           select_inds.data_ptr() if select_inds is not None else None, n, rays.data_ptr(),
           target.data_ptr() if target is not None else None, used.data_ptr(), st)
    return rays, target, used


def _select_vjp(cfg, intr, poses, used, g_rays, g_rays_2, views, want_poses=True, want_intr=True, out=None, out_intr=None, dist=None,
                want_dist=True, out_dist=None, dist_mask=None):
    """The VJP entry point of _SELECT_ENTRY on the current stream: the triple (d(loss)/d(pose[:3, :4]) (3 x 4 float32; with a view
    axis V x 3 x 4), d(loss)/d(intr) (4 float32; None without `intr`), d(loss)/d(dist) (4 float32; None without `dist`)) of the rays
    the select call with `cfg` / `poses` / `intr` / `dist` made at the select indices `used`, from d(loss)/d(rays) rows g_rays
    (+ g_rays_2, added row by row).  With `intr` or `dist` an output that is not wanted is None and is not computed.  dist_mask: None,
    or 4 bytes on the device: a coefficient whose byte is 0 gets an exact zero."""
    lib = L.get_lib()
    model = _camera_model(intr, dist)
    _, fn, tmp_fn = _SELECT_ENTRY[model, bool(views)]
    n, nv = used.numel(), poses.shape[0] if views else 1
    tb = getattr(lib, tmp_fn)(*((n, nv) if views or model else (n,)))
    if tb < 0:
        raise RuntimeError("select_training_rays_views: %d rays over %d views is outside the kernel's limits" % (n, nv))
    mk = lambda *shape: torch.empty(shape, dtype=torch.float32, device=poses.device)  # noqa: E731
    tmp = mk(tb // 4 + 1)
    gp = gi = gd = None
    if not model or want_poses:
        gp = out if out is not None else mk(*((nv, 3, 4) if views else (3, 4)))
    if intr is not None and want_intr:
        gi = out_intr if out_intr is not None else mk(4)
    if dist is not None and want_dist:
        gd = out_dist if out_dist is not None else mk(4)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    outs = (ptr(gp), ptr(gi), ptr(gd), ptr(dist_mask))[:{0: 1, 1: 2, 2: 4}[model]]   # (what the model's VJP entry point takes)
    with L.launch_on(poses, used, g_rays, g_rays_2, tmp, gp, gi, gd, intr, dist, dist_mask) as st:
        getattr(lib, fn)(C.byref(cfg), *_table_args(poses, views, intr, dist), used.data_ptr(), n, g_rays.data_ptr(),
                         g_rays_2.data_ptr() if g_rays_2 is not None else None, g_rays.stride(0), tmp.data_ptr(), tb, *outs, st)
    return gp, gi, gd


class _SelectRays(torch.autograd.Function):
    """select_training_rays / select_training_rays_views with the pose VJP (nerfhip_select_rays_bwd / nerfhip_select_rays_views_bwd):
    the gradient flows from the rays to the [:3, :4] entries of the pose (of every pose of the table), with `intrinsics` to the four
    intrinsics and with `distortion` to the four coefficients (nerfhip_select_rays_views_intr_bwd / _dist_bwd: one call for all of
    them); targets and select indices carry none.  The forward issues exactly the launch of the plain call."""

    @staticmethod
    def forward(ctx, poses, intrinsics, distortion, cfg, images, select_inds, n, views):
        p = _pose_table(poses, views)
        k = None if intrinsics is None else _intr_vector(intrinsics, p.device, "select_training_rays")
        d = None if distortion is None else _dist_vector(distortion, p.device, "select_training_rays")
        rays, target, used = _select_launch(cfg, p, images, select_inds, n, views, k, d)
        ctx.keep = (cfg, p, used, views, k, d)
        ctx.poses_shape = (poses.shape, poses.dtype)
        ctx.intr_shape = None if intrinsics is None else intrinsics.shape
        ctx.dist_shape = None if distortion is None else distortion.shape
        ctx.mark_non_differentiable(*[t for t in (target, used) if t is not None])
        ctx.set_materialize_grads(False)
        return rays, target, used

    @staticmethod
    def backward(ctx, g_rays, _g_target, _g_used):
        if g_rays is None:
            return (None,) * 8
        cfg, p, used, views, k, d = ctx.keep
        g_rays = g_rays.contiguous().float()
        g34, gi, gd = _select_vjp(cfg, k, p, used, g_rays, None, views, ctx.needs_input_grad[0], ctx.needs_input_grad[1], dist=d,
                                  want_dist=ctx.needs_input_grad[2])
        gi = gi.reshape(ctx.intr_shape) if gi is not None else None
        gd = gd.reshape(ctx.dist_shape) if gd is not None else None
        g = None
        if g34 is not None:
            shape, dtype = ctx.poses_shape
            g = torch.zeros(shape, dtype=dtype, device=p.device)
            g[..., :3, :4] = g34.to(dtype)
        return g, gi, gd, None, None, None, None, None


def _select(cfg, poses, images, select_inds, n, views, intrinsics=None, distortion=None):
    if images is not None:
        images = images.detach().float().contiguous()
    if select_inds is not None:
        select_inds = torch.as_tensor(select_inds, dtype=torch.int64, device=poses.device).contiguous()
    if torch.is_grad_enabled() and (poses.requires_grad or (intrinsics is not None and intrinsics.requires_grad)
                                    or (isinstance(distortion, torch.Tensor) and distortion.requires_grad)):
        return _SelectRays.apply(poses, intrinsics, distortion, cfg, images, select_inds, n, views)
    k = None if intrinsics is None else _intr_vector(intrinsics, poses.device, "select_training_rays")
    d = None if distortion is None else _dist_vector(distortion, poses.device, "select_training_rays")
    return _select_launch(cfg, _pose_table(poses, views), images, select_inds, n, views, k, d)


def _check_out4(what, name, t, dev):
    if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (4,) or not t.is_contiguous() or t.device != dev):
        raise RuntimeError("%s: %s must be a contiguous float32 (4) tensor on %s" % (what, name, dev))


def _select_bwd(what, cfg, poses, select_inds, g_rays, g_rays_2, out, views, intrinsics=None, out_intrinsics=None, want_poses=True,
                distortion=None, out_distortion=None, distortion_mask=None):
    """The checks of g_rays / g_rays_2 / out (`what`: the public function, for the messages), then the VJP."""
    for name, g in (("g_rays", g_rays), ("g_rays_2", g_rays_2)):
        if g is not None and (g.dtype != torch.float32 or g.dim() != 2 or g.stride(1) != 1
                              or g.shape[1] < (11 if cfg.use_viewdirs else 8)):
            raise RuntimeError("%s: %s must be float32 rows of the ray layout (got %s, shape %s)" % (what, name, g.dtype, tuple(g.shape)))
    if g_rays_2 is not None and (g_rays_2.shape != g_rays.shape or g_rays_2.stride() != g_rays.stride()):
        raise RuntimeError("%s: g_rays_2 must have the layout of g_rays" % what)
    p = _pose_table(poses, views)
    shape = (p.shape[0], 3, 4) if views else (3, 4)
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous()):
        raise RuntimeError("%s: out must be a contiguous float32 (%s) tensor" % (what, ", ".join(str(d) for d in shape)))
    used = torch.as_tensor(select_inds, dtype=torch.int64, device=poses.device).contiguous()
    if not want_poses and ((intrinsics is None and distortion is None) or out is not None):
        raise RuntimeError("%s: want_poses=False asks for the intrinsics' (or the distortion's) gradient alone: it needs intrinsics "
                           "or distortion and excludes out" % what)
    if intrinsics is None and out_intrinsics is not None:
        raise RuntimeError("%s: out_intrinsics needs intrinsics" % what)
    if distortion is None:
        if out_distortion is not None or distortion_mask is not None:
            raise RuntimeError("%s: out_distortion and distortion_mask need distortion" % what)
        if intrinsics is None:
            return _select_vjp(cfg, None, p, used, g_rays, g_rays_2, views, out=out)[0]
    _check_out4(what, "out_intrinsics", out_intrinsics, p.device)
    k = None if intrinsics is None else _intr_vector(intrinsics, p.device, what)
    if distortion is None:
        return _select_vjp(cfg, k, p, used, g_rays, g_rays_2, views, want_poses=want_poses, out=out, out_intr=out_intrinsics)[:2]
    _check_out4(what, "out_distortion", out_distortion, p.device)
    if distortion_mask is not None and (not isinstance(distortion_mask, torch.Tensor) or distortion_mask.dtype != torch.uint8
                                        or tuple(distortion_mask.shape) != (4,) or distortion_mask.device != p.device):
        raise RuntimeError("%s: distortion_mask must be a uint8 (4) tensor on %s" % (what, p.device))
    return _select_vjp(cfg, k, p, used, g_rays, g_rays_2, views, want_poses=want_poses, out=out, out_intr=out_intrinsics,
                       dist=_dist_vector(distortion, p.device, what), out_dist=out_distortion, dist_mask=distortion_mask)


def select_training_rays(height, width, focal_length, pose, image, num_random_rays, options, select_inds=None, seed=0,
                         step=0, first=0, intrinsics=None, distortion=None):
    """The image branch of the training loop (train_nerf.py:210-227) fused with run_one_iter_of_nerf's ray packing
    (train_utils.py:143-168), in ONE launch: draws `num_random_rays` distinct pixels on the device (or takes the
    reference's `select_inds`, the flat indices it draws with np.random.choice), generates only those rays from `pose`
    (>= 3x4, device), and gathers their targets from `image` (H, W, 3|4).  Returns (rays (N, 8|11) -- feed them to
    predict_and_render_radiance or TrainEngine.step --, target (N, C), select_inds (N,)).
    With a `pose` that requires grad the rays are differentiable w.r.t. it (pose refinement, as the reference's torch
    arithmetic is): the backward runs the pose VJP kernel (select_training_rays_bwd).
    intrinsics: None, or a float32 device tensor (fx, fy, cx, cy) in pixels that replaces `focal_length` and the image centre in
    the pin-hole direction ((col - cx) / fx, -(row - cy) / fy, -1) -- read on the device, so a learned focal is never read back
    to the host.  `focal_length` still fixes the NDC constants, which do not follow `intrinsics`.  With `intrinsics` requiring
    grad the rays are differentiable w.r.t. it as well.
    distortion: None, or a float32 device tensor (k1, k2, p1, p2): the lens distortion of the capture (COLMAP's OPENCV model,
    include/nerfhip.h); the pin-hole direction is undistorted under it on the device, with or without `intrinsics`.  With
    `distortion` requiring grad the rays are differentiable w.r.t. it as well (the same node, the same one VJP call)."""
    channels = 3 if image is None else image.shape[-1]
    cfg = _select_cfg(height, width, focal_length, options, channels, seed, step, first)
    return _select(cfg, pose, image, select_inds, int(num_random_rays), False, intrinsics, distortion)


def select_training_rays_bwd(height, width, focal_length, pose, select_inds, g_rays, options, g_rays_2=None, out=None,
                             intrinsics=None, out_intrinsics=None, want_poses=True, distortion=None, out_distortion=None,
                             distortion_mask=None):
    """The pose VJP of select_training_rays without autograd: d(loss)/d(pose[:3, :4]) (3 x 4 float32 device tensor; written
    into `out` when given) of the rays select_training_rays(height, width, focal_length, pose, ..., options) made at
    `select_inds` (its third output), from d(loss)/d(rays) rows `g_rays` (+ `g_rays_2`, added row by row: e.g. the coarse and
    the fine net's parts that TrainEngine.forward_backward(ray_grad=...) leaves).  Enqueued on the current stream.
    With `intrinsics` (those of the forward) the result is the pair (d(loss)/d(pose[:3, :4]), d(loss)/d(intrinsics) (4 float32;
    written into `out_intrinsics` when given)), from one call; want_poses=False (with `intrinsics` only) leaves the pose gradient
    out -- it is not computed, and the first entry of the pair is None.
    With `distortion` (that of the forward) the result is the triple (pose gradient, d(loss)/d(intrinsics) -- None without
    `intrinsics` --, d(loss)/d(distortion) (4 float32; written into `out_distortion` when given)), from one call; distortion_mask:
    None, or a uint8 device tensor of 4: a coefficient whose byte is 0 gets an exact zero."""
    cfg = _select_cfg(height, width, focal_length, options, 3, 0, 0, 0)
    return _select_bwd("select_training_rays_bwd", cfg, pose, select_inds, g_rays, g_rays_2, out, False, intrinsics, out_intrinsics,
                       want_poses, distortion, out_distortion, distortion_mask)


def select_training_rays_views(height, width, focal_length, poses, images, num_random_rays, options, select_inds=None, seed=0,
                               step=0, first=0, intrinsics=None, distortion=None):
    """select_training_rays over a stack of views, in ONE launch: `num_random_rays` distinct (view, pixel) pairs drawn from all of
    `images` (V, H, W, 3|4; or None) with the rays of each generated from its own row of `poses` (V, >=3, 4; device; a strided
    slice of a larger table is read in place).  Intrinsics and options are shared by the views.  The indices (third output, and
    `select_inds` when given) are global: v * H * W + k, k the reference's flat select index in view v.  Returns (rays, target,
    select_inds) as select_training_rays does; every row equals the row that call makes for (poses[v], images[v], [k]).
    With `poses` requiring grad the rays are differentiable w.r.t. them: the backward runs the per-view pose VJP
    (select_training_rays_views_bwd), so every view with a ray in the batch gets its gradient from one step.
    intrinsics, distortion: as for select_training_rays (one (fx, fy, cx, cy) and one (k1, k2, p1, p2) for all views)."""
    channels = 3 if images is None else images.shape[-1]
    cfg = _select_cfg(height, width, focal_length, options, channels, seed, step, first)
    if images is not None and (images.dim() != 4 or images.shape[0] != poses.shape[0]
                               or tuple(images.shape[1:3]) != (cfg.height, cfg.width)):
        raise RuntimeError("select_training_rays_views: images must be (V, H, W, C) with V = %d, H = %d, W = %d (got %s)"
                           % (poses.shape[0], cfg.height, cfg.width, tuple(images.shape)))
    return _select(cfg, poses, images, select_inds, int(num_random_rays), True, intrinsics, distortion)


def select_training_rays_views_bwd(height, width, focal_length, poses, select_inds, g_rays, options, g_rays_2=None, out=None,
                                   intrinsics=None, out_intrinsics=None, want_poses=True, distortion=None, out_distortion=None,
                                   distortion_mask=None):
    """The per-view pose VJP of select_training_rays_views without autograd: d(loss)/d(poses[:, :3, :4]) (V x 3 x 4 float32 device
    tensor; written into `out` when given) from d(loss)/d(rays) rows `g_rays` (+ `g_rays_2`, added row by row) at the global
    `select_inds` of the forward.  Entry v is bit-identical to select_training_rays_bwd on the rays of view v alone (in batch
    order); a view without a ray gets zeros.  Enqueued on the current stream; no host synchronisation.
    With `intrinsics` the result is the pair (pose gradients, d(loss)/d(intrinsics)), as for select_training_rays_bwd: the
    intrinsics' gradient is one fixed-order sum over all rays of the batch, whatever their view; want_poses=False as there.
    With `distortion` the result is the triple (pose gradients, d(loss)/d(intrinsics) or None, d(loss)/d(distortion)), as there."""
    cfg = _select_cfg(height, width, focal_length, options, 3, 0, 0, 0)
    return _select_bwd("select_training_rays_views_bwd", cfg, poses, select_inds, g_rays, g_rays_2, out, True, intrinsics,
                       out_intrinsics, want_poses, distortion, out_distortion, distortion_mask)


class _ExposureLoss(torch.autograd.Function):
    """exposure_mse_loss as ONE node: the forward is the launch of nerfhip_mse_loss_views_fwd_bwd (which also leaves the two rgb
    cotangents), the backward hands those out scaled by the incoming cotangents and, for a table that requires grad, calls
    nerfhip_exposure_bwd."""

    @staticmethod
    def forward(ctx, rgb_coarse, rgb_fine, target, inds, hw, table):
        lib = L.get_lib()
        n = rgb_coarse.shape[0]
        rc = rgb_coarse.detach().float().contiguous()
        rf = None if rgb_fine is None else rgb_fine.detach().float().contiguous()
        tgt = target.detach().float()
        if tgt.dim() != 2 or tgt.shape[1] < 3 or tgt.stride(1) != 1:
            tgt = tgt[..., :3].reshape(n, 3).contiguous()
        tab = table.detach().float().contiguous()
        if tab.dim() != 2 or tab.shape[1] != 6:
            raise RuntimeError("exposure_mse_loss: table must be (V, 6) (got shape %s)" % (tuple(table.shape),))
        ind = inds.to(torch.int64).contiguous()
        mk = lambda *shape: torch.empty(shape, dtype=torch.float32, device=rc.device)  # noqa: E731
        gc, gf, loss = mk(n, 3), (mk(n, 3) if rf is not None else None), mk(3)
        with L.launch_on(rc, rf, tgt, ind, tab, gc, gf, loss) as st:
            lib.mse_loss_views_fwd_bwd(rc.data_ptr(), rf.data_ptr() if rf is not None else None, tgt.data_ptr(), tgt.stride(0), n, 1.0,
                                       ind.data_ptr(), int(hw), tab.data_ptr(), tab.shape[0], gc.data_ptr(),
                                       gf.data_ptr() if gf is not None else None, loss.data_ptr(), st)
        ctx.keep = (rc, rf, tgt, ind, int(hw), tab, gc, gf)
        ctx.dtypes = (rgb_coarse.dtype, None if rgb_fine is None else rgb_fine.dtype, table.dtype, tuple(table.shape))
        ctx.set_materialize_grads(False)
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g_lc, g_lf):
        rc, rf, tgt, ind, hw, tab, gc, gf = ctx.keep
        dt_c, dt_f, dt_t, tab_shape = ctx.dtypes
        need = ctx.needs_input_grad
        g_rc = g_rf = g_tab = None
        if need[0] and g_lc is not None:
            g_rc = (gc * g_lc).to(dt_c)
        if rf is not None and need[1] and g_lf is not None:
            g_rf = (gf * g_lf).to(dt_f)
        if need[5]:
            # the table gradient is linear in the two nets' terms.  `(coarse + fine).backward()` hands both outputs ONE cotangent
            # tensor: known equal without reading it, so one call (cotangent 1: the entry point's bits).  Two tensors may still be
            # equal; reading them would synchronise, so all three calls run and the device selects.
            from .cameras import exposure_grad
            zero = torch.zeros((), device=rc.device)
            a = zero if g_lc is None else g_lc
            b = zero if (g_lf is None or rf is None) else g_lf
            if rf is None:
                g_tab = exposure_grad(rc, None, tgt, ind, hw, tab) * a
            elif a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()):
                g_tab = exposure_grad(rc, rf, tgt, ind, hw, tab) * a
            else:
                g_tab = torch.where(a == b, exposure_grad(rc, rf, tgt, ind, hw, tab) * a,
                                    exposure_grad(rc, None, tgt, ind, hw, tab) * a + exposure_grad(rf, None, tgt, ind, hw, tab) * b)
            g_tab = g_tab.reshape(tab_shape).to(dt_t)
        return g_rc, g_rf, None, None, None, g_tab


def exposure_mse_loss(rgb_coarse, rgb_fine, target, inds, hw, table):
    """(coarse_mse, fine_mse) = (mse_loss(rgb_coarse', target), mse_loss(rgb_fine', target)) with rgb' = exp(s) * rgb + b under the
    per-view exposure `table` (V, 6) -- the drop-in for the two mse_loss lines of the reference's loop (train_nerf.py:244-258) on a
    batch drawn by select_training_rays_views: `inds` are the global indices it returned, hw = height * width.  rgb_fine=None is the
    coarse-only net (fine_mse is then 0).  One autograd node, one launch in the forward; the backward gives the kernel's rgb
    cotangents times the incoming cotangents (both 1, as in `(coarse + fine).backward()`: nerfhip_mse_loss_views_fwd_bwd's and
    nerfhip_exposure_bwd's bits; anything else costs one multiply per element on top), and fills `table.grad` when the table requires
    grad (Exposure.values() of an object stepped by hand, or a leaf of one's own optimiser).  No host synchronisation: when the two
    outputs get one and the same cotangent tensor, as `(coarse + fine).backward()` gives them, the table gradient is ONE
    nerfhip_exposure_bwd call; when they get two tensors it is three (both nets, and each net alone, scaled), selected on the device
    by whether the two cotangents are equal."""
    return _ExposureLoss.apply(rgb_coarse, rgb_fine, target, inds, hw, table)


class _MatteLoss(torch.autograd.Function):
    """matte_mse_loss as ONE node: the forward is the launch of nerfhip_matte_loss_fwd_bwd (which also leaves g_rgb and g_acc of the
    weighted total), the backward hands those out scaled by the incoming cotangent."""

    @staticmethod
    def forward(ctx, rgb, acc, target, mode, bg, lam_alpha, lam_entropy, seed, ray_offset):
        lib = L.get_lib()
        n = rgb.shape[0]
        r = rgb.detach().float().contiguous()
        a = acc.detach().float().reshape(n).contiguous()
        tgt = target.detach().float()
        if tgt.dim() != 2 or tgt.shape[1] < 4 or tgt.stride(1) != 1:
            tgt = tgt.reshape(n, -1).contiguous()
        if tgt.shape[1] < 4:
            raise ValueError("matte_mse_loss: target_rgba must hold rows of 4 floats (r, g, b, alpha) (got shape %s)" % (tuple(target.shape),))
        rows = None   # (a per-ray background)
        if isinstance(bg, torch.Tensor):
            rows = bg.detach().float().reshape(n, 3).contiguous()
        const = bg if isinstance(bg, tuple) else (0.0, 0.0, 0.0)
        mk = lambda *shape: torch.empty(shape, dtype=torch.float32, device=r.device)  # noqa: E731
        g_rgb, g_acc, loss = mk(n, 3), mk(n), mk(3)
        with L.launch_on(r, a, tgt, rows, g_rgb, g_acc, loss) as st:
            lib.matte_loss_fwd_bwd(r.data_ptr(), a.data_ptr(), tgt.data_ptr(), tgt.stride(0), n, mode, None if rows is None else rows.data_ptr(),
                                   int(isinstance(bg, str)), *const, int(seed) & 0xFFFFFFFFFFFFFFFF, int(ray_offset), lam_alpha, lam_entropy,
                                   1.0, g_rgb.data_ptr(), g_acc.data_ptr(), loss.data_ptr(), st)
        ctx.keep = (g_rgb, g_acc)
        ctx.meta = (rgb.dtype, acc.dtype, tuple(acc.shape))
        total = loss[0].clone()   # (no view of `parts`: an output of its own)
        if lam_alpha != 0.0:
            total = total + lam_alpha * loss[1]
        if lam_entropy != 0.0:
            total = total + lam_entropy * loss[2]
        ctx.mark_non_differentiable(loss)
        return total, loss

    @staticmethod
    def backward(ctx, g_total, _g_parts):
        g_rgb, g_acc = ctx.keep
        dt_r, dt_a, acc_shape = ctx.meta
        need = ctx.needs_input_grad
        return ((g_rgb * g_total).to(dt_r) if need[0] else None, (g_acc * g_total).reshape(acc_shape).to(dt_a) if need[1] else None,
                None, None, None, None, None, None, None)


def matte_mse_loss(rgb, acc, target_rgba, mode="matte", background="random", alpha_loss=0.0, opacity_entropy=0.0, seed=0, ray_offset=0):
    """(total, parts): the loss of ONE net's rgb (n, 3) and accumulated opacity acc (n) -- the rgb_* / acc_* outputs of
    run_one_iter_of_nerf -- against RGBA targets (n, >= 4; straight alpha), in place of one mse_loss line of the reference's loop
    (train_nerf.py:244-258); one call per net.  mode "matte": the squared error of rgb + (1 - acc) * b against a * C + (1 - a) * b
    over a per-ray background b -- background="random" (uniform draws keyed by seed and ray_offset + ray index), a constant
    (r, g, b), or an (n, 3) tensor -- plus alpha_loss * mean (acc - a)^2; mode "weight": alpha weights every pixel's squared error
    (a mask: 0 = ignore; background and alpha_loss do not apply).  Both: plus opacity_entropy * mean H(acc), the binary entropy.
    total is differentiable w.r.t. rgb and acc: one autograd node, one launch (nerfhip_matte_loss_fwd_bwd) in the forward, whose
    cotangents the backward hands out times the incoming cotangent; parts is the detached device tensor [3] = {photometric, alpha,
    entropy}, unscaled means."""
    if mode not in ("matte", "weight"):
        raise ValueError("matte_mse_loss: mode must be 'matte' or 'weight' (got %r)" % (mode,))
    if mode == "weight":
        if alpha_loss != 0.0:
            raise ValueError("matte_mse_loss: alpha_loss=%r with mode='weight': alpha is a per-pixel loss weight there, not an opacity"
                             % (alpha_loss,))
        background = (0.0, 0.0, 0.0)   # (not read)
    elif not isinstance(background, torch.Tensor) and background != "random":
        background = tuple(float(v) for v in background)
        if len(background) != 3:
            raise ValueError("matte_mse_loss: background must be 'random', three floats (r, g, b) or an (n, 3) tensor")
    return _MatteLoss.apply(rgb, acc, target_rgba, int(mode == "weight"), background, float(alpha_loss), float(opacity_entropy), seed,
                            ray_offset)


ROBUST_KINDS = {"l2": 0, "l1": 1, "huber": 2, "charbonnier": 3, "relative": 4}


class _RobustLoss(torch.autograd.Function):
    """robust_mse_loss as ONE node: the forward is the launch of nerfhip_robust_loss_fwd_bwd (which also leaves g_rgb), the backward
    hands that out scaled by the incoming cotangent."""

    @staticmethod
    def forward(ctx, rgb, target, kind, param, keep):
        lib = L.get_lib()
        n = rgb.shape[0]
        r = rgb.detach().float().contiguous()
        tgt = target.detach().float()
        if tgt.dim() != 2 or tgt.shape[1] < 3 or tgt.stride(1) != 1:
            tgt = tgt.reshape(n, -1).contiguous()
        if tgt.shape[1] < 3:
            raise ValueError("robust_mse_loss: target must hold rows of at least 3 floats (got shape %s)" % (tuple(target.shape),))
        mk = lambda *shape: torch.empty(shape, dtype=torch.float32, device=r.device)  # noqa: E731
        g_rgb, words = mk(n, 3), mk(3)
        tmp = mk(lib.robust_loss_tmp_bytes(n) // 4) if keep < 1.0 else None
        with L.launch_on(r, tgt, g_rgb, words, tmp) as st:
            lib.robust_loss_fwd_bwd(r.data_ptr(), tgt.data_ptr(), tgt.stride(0), n, kind, param, keep, 1.0, g_rgb.data_ptr(), None, None,
                                    words.data_ptr(), None if tmp is None else tmp.data_ptr(), 0 if tmp is None else 4 * tmp.numel(), st)
        ctx.keep = g_rgb
        ctx.meta = rgb.dtype
        loss, kept, tau = words[0].clone(), words[1].clone(), words[2].clone()   # (no views of `words`: outputs of their own)
        ctx.mark_non_differentiable(kept, tau)
        return loss, kept, tau

    @staticmethod
    def backward(ctx, g_loss, _g_kept, _g_tau):
        return (ctx.keep * g_loss).to(ctx.meta) if ctx.needs_input_grad[0] else None, None, None, None, None


def robust_mse_loss(rgb, target, kind="huber", param=0.1, trim=None):
    """(loss, (kept, tau)): the robust photometric loss of ONE net's rgb (n, 3) against target (n, >= 3), in place of one mse_loss line
    of the reference's loop (train_nerf.py:244-258); one call per net.  kind: "l2", "l1", "huber" (param = delta), "charbonnier"
    (param = eps) or "relative" (RawNeRF's (p - t) / (sg(p) + eps), param = eps) -- the definition is nerfhip_robust_loss_fwd_bwd's
    (include/nerfhip.h); trim: None, or the fraction of the rays that is kept by per-ray residual (the others get a zero gradient row;
    the divisor stays 3 n).  loss is differentiable w.r.t. rgb: one autograd node, one launch in the forward, whose cotangent the
    backward hands out times the incoming cotangent; kept (the kept fraction) and tau (the residual at the cut; +inf without a trim) are
    detached device scalars."""
    if kind not in ROBUST_KINDS:
        raise ValueError("robust_mse_loss: unknown kind %r (one of %s)" % (kind, ", ".join(sorted(ROBUST_KINDS))))
    k = ROBUST_KINDS[kind]
    if k >= 2 and not (isinstance(param, (int, float)) and not isinstance(param, bool) and param > 0.0 and math.isfinite(param)):
        raise ValueError("robust_mse_loss: param=%r: kind %r needs a finite parameter > 0" % (param, kind))
    if trim is not None and not (isinstance(trim, (int, float)) and not isinstance(trim, bool) and 0.0 < trim <= 1.0):
        raise ValueError("robust_mse_loss: trim must be None or a kept fraction in (0, 1] (got %r)" % (trim,))
    loss, kept, tau = _RobustLoss.apply(rgb, target, k, float(param) if k >= 2 else 0.0, 1.0 if trim is None else float(trim))
    return loss, (kept, tau)


def select_cached_training_rays(cache_dict, num_random_rays, options, select_inds=None, seed=0, step=0, first=0):
    """The cached branch (train_nerf.py:175-194): rows of cache_dict["ray_bundle"] (2, ., 3) and of
    cache_dict["target"][..., :3], both already on the device."""
    lib = L.get_lib()
    bundle = cache_dict["ray_bundle"]
    ro = bundle[0].reshape((-1, 3)).float().contiguous()
    rd = bundle[1].reshape((-1, 3)).float().contiguous()
    tgt = cache_dict["target"][..., :3].reshape((-1, 3)).float().contiguous()
    dev, n = ro.device, int(num_random_rays)
    cfg = _select_cfg(cache_dict["height"], cache_dict["width"], cache_dict["focal_length"], options, 3, seed, step, first)
    if select_inds is not None:
        select_inds = torch.as_tensor(select_inds, dtype=torch.int64, device=dev).contiguous()
    rays = torch.empty((n, 11 if cfg.use_viewdirs else 8), dtype=torch.float32, device=dev)
    target = torch.empty((n, 3), dtype=torch.float32, device=dev)
    used = torch.empty((n,), dtype=torch.int64, device=dev)
    with L.launch_on(ro, rd, tgt, select_inds, rays) as st:
        lib.select_cached_rays(C.byref(cfg), ro.data_ptr(), rd.data_ptr(), tgt.data_ptr(), ro.shape[0],
                               select_inds.data_ptr() if select_inds is not None else None, n, rays.data_ptr(),
                               target.data_ptr(), used.data_ptr(), st)
    return rays, target, used


def run_one_iter_of_nerf(height, width, focal_length, model_coarse, model_fine, ray_origins, ray_directions, options,
                         mode="train", encode_position_fn=None, encode_direction_fn=None, occupancy=None, spread=False, depth_prior=None,
                         proposal=False):
    """nerf/train_utils.py:130-202.  occupancy: see predict_and_render_radiance (mode="validation" only); the grid's view_counts
    are zeroed first, so that after the call they are the sums over every ray chunk of this call.
    spread: see predict_and_render_radiance (mode="train" only): two trailing per-ray tensors, spread_coarse and spread_fine.
    depth_prior: see predict_and_render_radiance (mode="train" only): one (depth, weight, sigma) row per ray, chunked with the rays; two
    more trailing tensors, depth_loss_coarse and depth_loss_fine (n, 2), behind the spread pair.
    proposal: see predict_and_render_radiance (mode="train" only): one more trailing per-ray tensor, proposal_loss, last."""
    if not ray_directions.is_cuda:
        raise RuntimeError("run_one_iter_of_nerf needs CUDA (HIP) tensors: nerf_pytorch_amd has no CPU path")
    if spread and mode != "train":
        raise ValueError("spread=True needs mode=\"train\"")
    if depth_prior is not None and mode != "train":
        raise ValueError("depth_prior=... needs mode=\"train\"")
    if proposal and mode != "train":
        raise ValueError("proposal=True needs mode=\"train\"")
    restore_shapes = [ray_directions.shape, ray_directions.shape[:-1], ray_directions.shape[:-1]]
    if model_fine:
        restore_shapes += restore_shapes
    rays = pack_rays(ray_origins, ray_directions, options, height, width, focal_length)
    batches = get_minibatches(rays, chunksize=getattr(options.nerf, mode).chunksize)
    if occupancy is not None:
        if mode != "validation":
            raise NotImplementedError(_OCC_TRAIN_MSG)
        occupancy.view_counts.zero_()
        # (the options block the dense call below reads: like the reference, this function renders under `mode`'s DEFAULT)
        pred = [_predict_culled(batch, model_coarse, model_fine, options.nerf.train, encode_position_fn, encode_direction_fn, occupancy)
                for batch in batches]
    else:
        extra = [{"spread": True} if spread else {} for _ in batches]
        if proposal:
            for kw in extra:
                kw["proposal"] = True
        if depth_prior is not None:
            if depth_prior.shape[0] != rays.shape[0]:
                raise ValueError("depth_prior must hold one row per ray (%d rays, %d rows)" % (rays.shape[0], depth_prior.shape[0]))
            for kw, rows in zip(extra, get_minibatches(depth_prior, chunksize=getattr(options.nerf, mode).chunksize)):
                kw["depth_prior"] = rows
        pred = [predict_and_render_radiance(batch, model_coarse, model_fine, options,
                                            encode_position_fn=encode_position_fn,
                                            encode_direction_fn=encode_direction_fn, **kw) for batch, kw in zip(batches, extra)]
    synthesized_images = list(zip(*pred))
    synthesized_images = [torch.cat(image, dim=0) if image[0] is not None else None for image in synthesized_images]
    if mode == "validation":
        synthesized_images = [image.view(shape) if image is not None else None
                              for (image, shape) in zip(synthesized_images, restore_shapes)]
        if model_fine:
            return tuple(synthesized_images)
        return tuple(synthesized_images + [None, None, None])
    return tuple(synthesized_images)
