"""TrainEngine: one NeRF training iteration (train_nerf.py:229-270) as a fixed graph of C-ABI calls on two HIP
streams, with no host synchronisation inside the step.  The reference runs everything sequentially
(nerf/train_utils.py:68-117 coarse then fine, train_nerf.py:244-261 loss, backward, optimiser); here

    main stream:  coarse forward --E1--> hierarchical sampling + fine forward -> fine loss -> fine backward
                  -> [all-reduce of the fine net's gradient, async] ------------------------------+
    side stream:           E1 -> coarse loss -> coarse backward --E2-->                           |
    main stream:                                            wait E2 -> [all-reduce coarse] -> wait both -> Adam -> re-pack

the coarse net's backward needs nothing from the fine pass, so it runs next to the fine forward/backward (fills the
tails of those launches), and with G > 1 ranks the fine net's gradient all-reduce (RCCL) is in flight while the coarse
backward still computes.  `overlap=False` gives the single-stream order (coarse+fine forward, loss, fine backward,
coarse backward) with the same collectives -- in both orders the fine net's all-reduce is launched before the coarse
backward.  Default: two streams for nets narrower than 256 (measured +3.5 %), one stream for 256-wide nets (-0.4 %).

Data parallelism (BASELINE config 3): one process per GPU, weights replicated, each rank renders its own N/G rays;
the only exchange is the all-reduce (sum) of the 2 x 595,844-float gradient (one collective per net), scaled by 1/G
inside the Adam kernel.  Every rank applies the identical update, so no parameter broadcast is needed after step 0.

Occupancy grid (`occupancy=`, one rank): from a warm-up on both forwards are nerfhip_render_fwd_occ_train through
the grid (main stream, one list area), the nets' backwards run in a mode that keeps no stash, and every few optimizer steps the
grid's density is updated from the images just packed.

Ray-weight spread loss (mip-NeRF 360's L_dist; `spread=`): a net with a weight lambda > 0 gets one nerfhip_spread_loss
launch between its loss and its backward, on the same stream, and the _w form of that backward; `spread_losses` reads the means.

Depth priors (DS-NeRF; `depth_loss=` and a step's `depth_prior=`): a net with a nonzero weight gets one
nerfhip_depth_prior_loss launch on the stream its backward runs on, behind the spread launch where there is one (then accumulating into
the same weight cotangent), ahead of the _w form of its backward; `depth_losses` reads the means.  A step without `depth_prior=` is
the step without the feature.

Interlevel proposal loss (mip-NeRF 360's L_prop; `proposal=` and `coarse_photometric=`): the coarse net's loss gains
lambda * mean_ray(L) -- one nerfhip_proposal_loss launch in the coarse net's pass, behind the spread and depth launches (accumulating
into their cotangent where either ran), ahead of the _w form of its backward.  The kernel reads the FINE pass's raw rows and depths:
on two streams the coarse net's pass starts behind the fine forward, and overlaps the fine backward only.  coarse_photometric=False
withholds the colour cotangent from the coarse backward: the coarse net learns from its weight losses alone.

RGBA targets (`alpha=`, `background=`, `alpha_loss=`, `opacity_entropy=`): with alpha="matte" or "weight" each net's
loss launch is nerfhip_matte_loss_fwd_bwd in place of nerfhip_mse_loss_fwd_bwd, on the same stream, and the g_acc it writes enters the
net's backward as the cotangent of the accumulated opacity, next to g_rgb (withheld with it under coarse_photometric=False);
`matte_losses` reads each net's {photometric, alpha, entropy}.  Without `alpha=` the fourth column of a target is ignored, as ever.

Robust photometric losses (`photometric=`, `trim=`): with either set each net's loss launch is
nerfhip_robust_loss_fwd_bwd in place of nerfhip_mse_loss_fwd_bwd, on the same stream, with the same grad_scale, into the same g_rgb
buffer and loss words; everything behind the launch is untouched.  Each net trims on its own residuals (no new wait between the
streams), and in a data-parallel step each rank trims its own shard: tau is a quantile of the rank's rays, not of the global batch.
`loss` holds the robust means, `robust_stats` each net's {kept fraction, tau}.  Without the keywords: the same launches, the same bits.
"""
import math

import torch

from . import _lib as L
from . import backward_mode as BM
from . import train_utils as TU
from .cameras import Distortion, Exposure, Intrinsics, check_device_vector
from .depth_prior import DepthPrior
from .nerf_helpers import linspace01
from .render_call import RenderCall
from .parallel import allreduce_gradients, shard_bounds


class TrainEngine:
    def __init__(self, model_coarse, model_fine, num_coarse, num_fine, perturb=True, lindisp=False, white_background=False,
                 noise_std=0.0, lr=5e-3, betas=(0.9, 0.999), eps=1e-8, seed=0, process_group=None, world_size=None,
                 rank=None, overlap=None, always_reduce=False, backward=None, window=None, total_steps=None, occupancy=None,
                 occupancy_warmup=256, occupancy_every=16, spread=None, depth_loss=None, proposal=None, coarse_photometric=True,
                 alpha=None, background=None, alpha_loss=None, opacity_entropy=None, photometric=None, trim=None):
        self.lib = L.get_lib()
        self.mc, self.mf = model_coarse, model_fine if num_fine > 0 else None
        self.dev = model_coarse.flat_params.device
        if self.dev.type != "cuda":
            raise RuntimeError("TrainEngine needs the models on a CUDA (HIP) device")
        self.view = bool(model_coarse.cfg["use_viewdirs"])
        self.stride = 11 if self.view else 8
        self.cfg = L.RenderCfg(num_coarse, num_fine, int(bool(perturb)), int(bool(lindisp)), int(bool(white_background)),
                               float(noise_std), self.stride)
        self.lr, self.betas, self.eps = lr, betas, eps
        self.seed = seed
        self.step_count = 0
        self.localize_count = 0   # localisation steps run (localize_on_image / localize_on_views): keys their selections and draws
        self.pg = process_group
        if world_size is None:
            world_size = torch.distributed.get_world_size(process_group) if torch.distributed.is_initialized() else 1
        if rank is None:
            rank = torch.distributed.get_rank(process_group) if torch.distributed.is_initialized() else 0
        self.world, self.rank = world_size, rank
        # the gradient collectives are issued when there is somebody to exchange with -- or always (always_reduce: a
        # one-rank group still goes through RCCL's work handles and stream ordering; the single-GPU test of that path)
        self._reduce = world_size > 1 or (bool(always_reduce) and torch.distributed.is_initialized())
        # one flat gradient / Adam-state buffer covering both nets: a single collective per step
        self.nc_params = model_coarse.num_flat_params
        self.nf_params = self.mf.num_flat_params if self.mf is not None else 0
        tot = self.nc_params + self.nf_params
        self.grad = torch.zeros(tot, dtype=torch.float32, device=self.dev)
        self.exp_avg = torch.zeros_like(self.grad)
        self.exp_avg_sq = torch.zeros_like(self.grad)
        self.loss = torch.zeros(3, dtype=torch.float32, device=self.dev)
        self._loss_c = torch.zeros(3, dtype=torch.float32, device=self.dev)
        self._loss_f = torch.zeros(3, dtype=torch.float32, device=self.dev)
        # two-stream graph: measured on MI355X (profiles/r02_overlap_ab.txt) +3.5 % for 128-wide nets (the short kernels'
        # tails fill), -0.4 % for 256-wide fp32 nets (every launch already fills the chip for milliseconds); the fp16-piece
        # plans at 256 wide (HBM- and latency-bound kernels that leave the matrix pipe idle half the time: room for a second
        # stream): +1.4 % dense, +6 % compacted, +7 % recomputed (profiles/r06_bench_trained_overlap1.json against
        # r06_bench_trained.json of round 6's first passes) -> default by width and arithmetic
        self.overlap = ((model_coarse.cfg["hidden_size"] <= 128 or getattr(model_coarse, "training_precision", "fp32") != "fp32")
                        if overlap is None else bool(overlap))
        self._side = None       # second HIP stream of this device (created on first use)
        self._ev = None
        self._pending = []      # in-flight gradient all-reduces of the current step
        self._ws = None
        self._ws_n = -1
        self.render_call = None   # the last step's render_call.RenderCall (addresses of that step's buffers; engine-owned workspace)
        self._bufs = None
        # buffers of a step with a ray gradient, sized in _ray_grad_bufs: the coarse net's part of d(loss)/d(rays) (forward_backward),
        # one backward tmp per net with its size in bytes, the step routine's own ray gradient (the fine net's part)
        self.ray_grad_coarse = self._ray_grad = None
        self._rg_tmp, self._rg_n, self._ray_grad_n = (None, None, 0), -1, -1
        # backward mode of the step: None -- whatever each model's set_backward_compaction says (default: dense); "dense" / "compact" /
        # "recompute" -- set on both models; "auto" -- chosen per net and per step from the zero-cotangent fraction the previous
        # compacted steps reported (read back asynchronously: no host synchronisation), see _choose_backward_modes
        self.backward = backward
        self._nets = tuple((name, m) for name, m in (("coarse", self.mc), ("fine", self.mf)) if m is not None)
        # occupancy grid in training (None: the step as it always was).  From step `occupancy_warmup` on the two
        # forwards are nerfhip_render_fwd_occ_train through `occupancy` (an occupancy.OccupancyGrid; both on the main stream, ONE
        # engine-owned list area), every net's backward runs in a mode whose training forward leaves no stash ("recompute", or
        # "fused_compact" where the net has the fused backward), and every `occupancy_every`-th optimizer_step -- during the warm-up
        # already -- updates the grid from the nets just packed (grid.update_density; a grid without a density is left as it is)
        self.occupancy, self.occupancy_warmup, self.occupancy_every = occupancy, int(occupancy_warmup), int(occupancy_every)
        self._occ_tmp, self._occ_tb = None, 0
        if occupancy is not None:
            if world_size > 1:
                raise NotImplementedError("TrainEngine: occupancy=... with world size %d is not implemented; run it with one rank"
                                          % world_size)
            if self.occupancy_every < 1 or self.occupancy_warmup < 0:
                raise ValueError("TrainEngine: occupancy_every must be >= 1 and occupancy_warmup >= 0")
            if occupancy.bits.device != self.dev:
                raise RuntimeError("TrainEngine: the occupancy grid lives on %s, the engine on %s" % (occupancy.bits.device, self.dev))
            if backward not in (None, "auto") and BM.parse(backward) not in (BM.RECOMPUTE, BM.FUSED_COMPACT):
                raise ValueError("TrainEngine: occupancy=... culls the training forward of a backward that keeps no stash and walks a "
                                 "sample list: backward must be None, 'auto', 'recompute' or 'fused_compact' (got %r)" % (backward,))
        if backward not in (None, "auto"):
            mode = BM.parse(backward)   # (ValueError for anything that is not a mode)
            for _, m in self._nets:
                m.set_backward_compaction(mode)
        # ray-weight spread loss (mip-NeRF 360's L_dist): None / 0 -- the step as it always was, launch for launch; a
        # float or (lambda_coarse, lambda_fine) -- a net with lambda > 0 adds lambda * mean_ray(L) to its loss: after its forward one
        # nerfhip_spread_loss on the stream its backward runs on, over the raw rows and depths the forward left in the workspace, then
        # the _w form of its backward with the engine-owned weight cotangent
        if spread is None:
            spread = (0.0, 0.0)
        elif isinstance(spread, (int, float)):
            spread = (float(spread), float(spread))
        else:
            spread = tuple(float(v) for v in spread)
        if len(spread) != 2 or not all(v >= 0.0 and math.isfinite(v) for v in spread):
            raise ValueError("TrainEngine: spread must be None, a finite weight >= 0 or a pair (coarse, fine) of them (got %r)" % (spread,))
        self.spread = (spread[0], spread[1] if self.mf is not None else 0.0)
        self._spread_bufs = None   # per net with lambda > 0: (weight cotangent [n, S], per-ray loss [n]), sized in _prepare
        # depth priors (DS-NeRF): None -- no term; (a, b) -- the weights of the expected-depth and the termination term
        # on both nets; ((a_c, b_c), (a_f, b_f)) -- per net.  A net's loss becomes mse + (1 / n) sum_rays (a E + b Tm) over ALL n rays of
        # a step that is given prior rows (depth_prior=...); a step without them is the step without the feature
        self.depth_loss = self._parse_depth_loss(depth_loss, self.mf is not None)
        self._depth_bufs = None    # per net with a nonzero weight: (weight cotangent [n, S], per-ray losses [n, 2]), sized in _prepare
        self._depth_ran = False    # whether the last step launched the depth kernel (depth_losses)
        self._depth_keep = None    # the last step's prior table and indices (alive until the next step: the launches read them)
        # interlevel proposal loss (mip-NeRF 360's L_prop): None / 0 -- the step as it always was, launch for launch; a
        # weight lambda > 0 -- the coarse net's loss gains lambda * mean_ray(L) of its weight histogram against the fine pass's weights
        # (a constant of the term: the fine net's gradient does not move)
        if proposal is None:
            proposal = 0.0
        if isinstance(proposal, bool) or not isinstance(proposal, (int, float)) or not (proposal >= 0.0 and math.isfinite(proposal)):
            raise ValueError("TrainEngine: proposal must be None or a finite weight >= 0 (got %r)" % (proposal,))
        if proposal > 0.0 and self.mf is None:
            raise ValueError("TrainEngine: proposal > 0 needs a fine net (num_fine > 0): the loss bounds the fine pass's weights")
        self.proposal = float(proposal)
        self._proposal_bufs = None   # (coarse weight cotangent [n, num_coarse], per-ray loss [n]), sized in _prepare
        # coarse_photometric=False: the coarse backward is given no colour cotangent (its MSE is still launched and reported); it needs
        # a weight loss on the coarse net, or that net would learn nothing
        self.coarse_photometric = bool(coarse_photometric)
        if not self.coarse_photometric and not (self.proposal > 0.0 or self.spread[0] > 0.0 or any(self.depth_loss[0])):
            raise ValueError("TrainEngine: coarse_photometric=False leaves the coarse net without any loss: give it proposal > 0 (or a "
                             "spread or depth weight on the coarse net)")
        # RGBA targets: None -- the fourth column of a target is ignored, the step as it always was; "matte" -- each
        # net's loss is taken over a per-ray background (`background`: "random", the default -- uniform draws keyed by the step's seed
        # and the global ray index --, or a constant (r, g, b)), with alpha_loss * mean (acc - a)^2 on top; "weight" -- alpha weights
        # every pixel's squared error.  Both: opacity_entropy * mean H(acc).  One nerfhip_matte_loss_fwd_bwd per net in place of
        # nerfhip_mse_loss_fwd_bwd; its g_acc enters the net's backward as the cotangent of the accumulated opacity
        self.alpha, self.background, self.alpha_loss, self.opacity_entropy = self._parse_alpha(
            alpha, background, alpha_loss, opacity_entropy, bool(white_background), self.mf is not None)
        # robust photometric losses: None -- the plain squared error, the step as it always was; `photometric`: "l1",
        # ("huber", delta), ("charbonnier", eps) or ("relative", eps); `trim`: the fraction of the batch's rays that is kept, by per-ray
        # residual (the others get a zero cotangent row); each may be a pair (coarse, fine).  When either is set, each net's loss launch
        # is nerfhip_robust_loss_fwd_bwd in place of nerfhip_mse_loss_fwd_bwd, on the same stream, into the same g_rgb and loss words;
        # each net trims on its own residuals, and in a data-parallel step each rank trims its own shard
        self.robust = self._parse_robust(photometric, trim, self.mf is not None)
        if self.robust is not None and self.alpha is not None:
            raise ValueError("TrainEngine: %s=... together with alpha=%r is not covered: the matte loss carries its own kernel"
                             % ("photometric" if photometric is not None else "trim", self.alpha))
        self._stats = BM.StatsReader(("coarse", "fine"))
        self._zero_frac = self._stats.frac   # last known fraction of all-zero d(loss)/d(raw) rows per net (updated in place)
        # steps run dense / compacted / recomputed / fused / fused over the list / fused over the stash, per net ("auto")
        self.backward_modes_used = {"coarse": [0, 0, 0, 0, 0, 0], "fine": [0, 0, 0, 0, 0, 0]}
        # coarse-to-fine encoding window (BARF; FlexibleNeRFModel.set_encoding_window), set on both nets for every step: None -- the
        # engine sets none (a window set on the models by hand is honoured); (start, end) in units of step_count / total_steps -- per
        # encoding alpha = (progress - start) / (end - start) * num_encoding_fn: closed up to `start`, fully open from `end` on;
        # or a callable step -> (alpha_xyz, alpha_dir)
        if window is not None and not callable(window):
            start, end = (float(v) for v in window)
            if not end > start or not total_steps or total_steps <= 0:
                raise ValueError("TrainEngine: window=(start, end) needs end > start and total_steps > 0 (got %r, total_steps=%r)"
                                 % (window, total_steps))
            window = (start, end)
        self.window, self.total_steps = window, total_steps
        self._set_window()
        self.t_vals = linspace01(num_coarse, self.dev)
        self.u_det = linspace01(num_fine, self.dev) if num_fine > 0 else None
        self.repack()

    @staticmethod
    def _parse_depth_loss(depth_loss, has_fine):
        bad = ValueError("TrainEngine: depth_loss must be None, a pair (a, b) of finite weights >= 0 (expected-depth, termination) or "
                         "a pair of such pairs (coarse, fine) (got %r)" % (depth_loss,))
        if depth_loss is None:
            return ((0.0, 0.0), (0.0, 0.0))
        try:
            d = tuple(depth_loss)
            if len(d) != 2:
                raise bad
            if all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in d):
                d = (d, d)
            d = tuple(tuple(float(v) for v in pair) for pair in d)
        except TypeError:
            raise bad from None
        if any(len(pair) != 2 or not all(v >= 0.0 and math.isfinite(v) for v in pair) for pair in d):
            raise bad
        return (d[0], d[1] if has_fine else (0.0, 0.0))

    @staticmethod
    def _parse_alpha(alpha, background, alpha_loss, opacity_entropy, white_background, has_fine):
        """-> (mode or None, None / "random" / (r, g, b), (alpha_loss coarse, fine), (opacity_entropy coarse, fine))."""
        if alpha not in (None, "matte", "weight"):
            raise ValueError("TrainEngine: alpha must be None, 'matte' or 'weight' (got %r)" % (alpha,))

        def pair(name, v):
            if v is None:
                return (0.0, 0.0)
            bad = ValueError("TrainEngine: %s must be a finite weight >= 0 or a pair (coarse, fine) of them (got %r)" % (name, v))
            if isinstance(v, bool):
                raise bad
            try:
                v = (float(v), float(v)) if isinstance(v, (int, float)) else tuple(float(x) for x in v)
            except (TypeError, ValueError):
                raise bad from None
            if len(v) != 2 or not all(x >= 0.0 and math.isfinite(x) for x in v):
                raise bad
            return v

        lam_a, lam_h = pair("alpha_loss", alpha_loss), pair("opacity_entropy", opacity_entropy)
        if alpha is None:   # (the parsed weights decide: 0, 0.0, (0, 0) and [0.0, 0.0] all ask for nothing)
            for name, given, asks in (("alpha_loss", alpha_loss, any(lam_a)), ("opacity_entropy", opacity_entropy, any(lam_h)),
                                      ("background", background, background is not None)):
                if asks:
                    raise ValueError("TrainEngine: %s=%r needs alpha='matte' or alpha='weight'" % (name, given))
            return None, None, (0.0, 0.0), (0.0, 0.0)
        if not has_fine:
            lam_a, lam_h = (lam_a[0], 0.0), (lam_h[0], 0.0)
        if alpha == "weight":
            if any(lam_a):
                raise ValueError("TrainEngine: alpha_loss=%r with alpha='weight': alpha is a per-pixel loss weight there, not an "
                                 "opacity (alpha_loss belongs to alpha='matte')" % (alpha_loss,))
            if background is not None:
                raise ValueError("TrainEngine: background=%r with alpha='weight': the weighted loss reads no background" % (background,))
            return alpha, None, lam_a, lam_h
        if white_background:
            raise ValueError("TrainEngine: alpha='matte' with white_background=True would composite twice (the render onto white, the "
                             "loss onto its background): use white_background=False and background=(1, 1, 1)")
        if background is None:
            background = "random"
        if not (isinstance(background, str) and background == "random"):
            try:
                background = tuple(float(x) for x in background)
            except (TypeError, ValueError):
                background = ()
            if len(background) != 3 or not all(math.isfinite(x) for x in background):
                raise ValueError("TrainEngine: background must be 'random' or three finite floats (r, g, b)")
        return alpha, background, lam_a, lam_h

    ROBUST_KINDS = {"l2": 0, "l1": 1, "huber": 2, "charbonnier": 3, "relative": 4}

    @classmethod
    def _parse_robust(cls, photometric, trim, has_fine):
        """-> None (neither keyword asks for anything), or ((kind, param, keep) of the coarse net, of the fine net)."""
        def number(v):
            return isinstance(v, (int, float)) and not isinstance(v, bool)

        def spec(v):
            """One net's `photometric` -> (kind, param)."""
            bad = ValueError("TrainEngine: photometric must be None, 'l1', ('huber', delta), ('charbonnier', eps) or ('relative', eps) "
                             "with a finite parameter > 0, or a pair (coarse, fine) of those (got %r)" % (photometric,))
            if v is None:
                return (0, 0.0)
            name, param = (v, None) if isinstance(v, str) else (tuple(v) if isinstance(v, (tuple, list)) and len(v) == 2 else (None, None))
            if not isinstance(name, str):
                raise bad
            if name not in cls.ROBUST_KINDS:
                raise ValueError("TrainEngine: photometric: unknown kind %r (one of %s)" % (name, ", ".join(sorted(cls.ROBUST_KINDS))))
            kind = cls.ROBUST_KINDS[name]
            if kind < 2:
                if param is not None:
                    raise bad
                return (kind, 0.0)
            if not number(param) or not (param > 0.0 and math.isfinite(param)):
                raise ValueError("TrainEngine: photometric=(%r, %r): the parameter must be a finite number > 0" % (name, param))
            return (kind, float(param))

        def keep_of(v):
            if v is None:
                return 1.0
            if not number(v) or not (0.0 < v <= 1.0):
                raise ValueError("TrainEngine: trim must be None, a kept fraction in (0, 1] or a pair (coarse, fine) of those (got %r)"
                                 % (trim,))
            return float(v)

        one = photometric is None or isinstance(photometric, str) or (
            isinstance(photometric, (tuple, list)) and len(photometric) == 2 and isinstance(photometric[0], str) and number(photometric[1]))
        if not one and not (isinstance(photometric, (tuple, list)) and len(photometric) == 2):
            spec(photometric)   # (raises)
        kinds = (spec(photometric),) * 2 if one else tuple(spec(v) for v in photometric)
        if trim is not None and not number(trim) and not (isinstance(trim, (tuple, list)) and len(trim) == 2):
            keep_of(trim)   # (raises)
        keeps = (keep_of(trim),) * 2 if trim is None or number(trim) else tuple(keep_of(v) for v in trim)
        if not has_fine:
            kinds, keeps = (kinds[0], (0, 0.0)), (keeps[0], 1.0)
        if all(k == (0, 0.0) for k in kinds) and all(k == 1.0 for k in keeps):
            return None
        return tuple(k + (kp,) for k, kp in zip(kinds, keeps))

    def window_alphas(self, step):
        """(alpha_xyz, alpha_dir) of the schedule at step `step` (None without one)."""
        if self.window is None:
            return None
        if callable(self.window):
            return tuple(self.window(step))
        start, end = self.window
        t = (step / float(self.total_steps) - start) / (end - start)
        return (t * self.mc.cfg["num_encoding_fn_xyz"], t * self.mc.cfg["num_encoding_fn_dir"])

    def _set_window(self):
        """Puts both nets under the schedule's window of the step about to run (step_count); True if that changed a window."""
        alphas = self.window_alphas(self.step_count)
        changed = False
        if alphas is not None:
            for _, m in self._nets:
                if m.encoding_window != alphas:
                    m.set_encoding_window(*alphas)
                    changed = True
        return changed

    def repack(self):
        # (under an encoding window each pack is preceded by the theta_eff kernel; the buffer it fills is what a step's ray gradient
        # multiplies by)
        self.packed_c = self.mc._packed(True)
        self.packed_f = self.mf._packed(True) if self.mf is not None else None

    def _prepare(self, n):
        if self._ws_n == n:
            return
        plan_f = self.mf._plan if self.mf is not None else None
        self._wsb = RenderCall.workspace_bytes(self.lib, self.mc._plan, plan_f, self.cfg, n, 1)
        self._ws = torch.empty(self._wsb // 4 + 1, dtype=torch.float32, device=self.dev)
        self._ws_n = n
        self._regions = {}   # (the workspace offsets the steps' RenderCalls look up: asked once per n)
        mk = lambda *s: torch.empty(s, dtype=torch.float32, device=self.dev)  # noqa: E731
        if self.occupancy is not None:   # (the list area of the culled forwards; its first four words: occupancy_counts)
            self._occ_tb = RenderCall.occ_tmp_bytes(self.lib, self.cfg, n)
            self._occ_tmp = torch.zeros(self._occ_tb // 4 + 64, dtype=torch.int32, device=self.dev)
        self._bufs = dict(rgb_c=mk(n, 3), rgb_f=mk(n, 3), g_c=mk(n, 3), g_f=mk(n, 3), disp_c=mk(n), acc_c=mk(n),
                          disp_f=mk(n), acc_f=mk(n))
        if self.alpha is not None:   # (the cotangents of the accumulated opacity: what the matte kernel writes)
            self._bufs.update(ga_c=mk(n), ga_f=mk(n))
        if self.robust is not None:   # (a trimming net's per-ray residuals: the selection's keys; one per net -- two streams)
            words = self.lib.robust_loss_tmp_bytes(n) // 4
            self._bufs.update({"rt_" + tag: mk(words) for tag, (_, _, keep) in zip("cf", self.robust) if keep < 1.0})
        if any(self.spread):   # (what the spread kernel writes)
            S = (self.cfg.num_coarse, self.cfg.num_coarse + self.cfg.num_fine)
            self._spread_bufs = {fine: (mk(n, S[fine]), torch.zeros(n, dtype=torch.float32, device=self.dev))
                                 for fine in (0, 1) if self.spread[fine] > 0.0}
        if any(any(w) for w in self.depth_loss):   # (what the depth kernel writes; the weight cotangent is the spread term's where it has one)
            S = (self.cfg.num_coarse, self.cfg.num_coarse + self.cfg.num_fine)
            self._depth_bufs = {fine: (self._spread_bufs[fine][0] if self.spread[fine] > 0.0 else mk(n, S[fine]),
                                       torch.zeros(n, 2, dtype=torch.float32, device=self.dev))
                                for fine in (0, 1) if any(self.depth_loss[fine])}
        if self.proposal > 0.0:   # (what the proposal kernel writes; the coarse weight cotangent is the spread / depth terms' where they have one)
            shared = (self._spread_bufs or {}).get(0) or (self._depth_bufs or {}).get(0)
            self._proposal_bufs = (shared[0] if shared else mk(n, self.cfg.num_coarse), torch.zeros(n, dtype=torch.float32, device=self.dev))

    def workspace_bytes(self):
        return 0 if self._ws is None else self._wsb

    def _check_inputs(self, rays, target):
        for name, t in (("rays", rays), ("target", target)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != self.dev:
                raise RuntimeError("TrainEngine: %s must be a tensor on %s (nerf_pytorch_amd has no CPU path)" % (name, self.dev))
            if t.dtype != torch.float32:
                raise RuntimeError("TrainEngine: %s must be float32 (got %s)" % (name, t.dtype))
            if t.dim() != 2:
                raise RuntimeError("TrainEngine: %s must be 2-D (got shape %s)" % (name, tuple(t.shape)))
        if rays.shape[1] != self.stride or not rays.is_contiguous():
            raise RuntimeError("TrainEngine: rays must be contiguous rows of %d floats (got shape %s, strides %s)"
                               % (self.stride, tuple(rays.shape), rays.stride()))
        if target.shape[0] != rays.shape[0] or target.shape[1] < 3 or target.stride(1) != 1:
            # e.g. target_s[..., :3] of an RGBA image is fine (row stride 4 is passed on), a transposed view is not
            raise RuntimeError("TrainEngine: target must hold one row of >= 3 unit-stride floats per ray (got shape %s, "
                               "strides %s)" % (tuple(target.shape), target.stride()))

    def _streams(self):
        main = torch.cuda.current_stream(self.dev)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
            self._ev = (torch.cuda.Event(), torch.cuda.Event())
        return main, self._side

    def _ray_grad_bufs(self, n, own=False):
        """Engine-owned buffers of a step of `n` rays with a ray gradient: the coarse net's part of d(loss)/d(rays) and one tmp per net
        (the two nets' backward chains may run at the same time on two streams); with `own`, the step routine's ray gradient as well."""
        mk = lambda *s: torch.empty(s, dtype=torch.float32, device=self.dev)  # noqa: E731
        if own and self._ray_grad_n != n:
            self._ray_grad, self._ray_grad_n = mk(n, self.stride), n
        if self._rg_n != n:
            plan_f = self.mf._plan if self.mf is not None else None
            # (one tmp serves both forms of the step: the trainable one's and the frozen one's, whichever is larger)
            tb = max(RenderCall.tmp_bytes(self.lib, self.mc._plan, plan_f, self.cfg, n))
            self.ray_grad_coarse = mk(n, self.stride) if self.mf is not None else None
            self._rg_tmp = (mk(tb // 4 + 4), mk(tb // 4 + 4) if self.mf is not None else None, tb)
            self._rg_n = n
        return self.ray_grad_coarse, self._rg_tmp

    def _no_pose_grad_across_ranks(self, what):
        if self.world > 1:
            raise NotImplementedError("TrainEngine: %s with world size %d is not implemented (the pose / ray gradient of a "
                                      "data-parallel step would need its own all-reduce); run it with one rank" % (what, self.world))

    def _check_depth_prior(self, depth_prior, n, frozen):
        """depth_prior= of a step -> (table, row stride, indices or None, rows): `rows` (n, 3) read ray by ray, or (P, inds) -- a
        DepthPrior and the int64 global index of every ray."""
        if not any(any(w) for w in self.depth_loss):
            raise ValueError("TrainEngine: depth_prior=... on an engine without depth_loss (construct it with depth_loss=(a, b))")
        if frozen:
            raise ValueError("TrainEngine: a frozen step (localize_*, the exposure fit) takes no depth prior: the frozen ray gradient "
                             "takes no weight cotangent")
        inds = None
        if isinstance(depth_prior, (tuple, list)):
            prior, inds = depth_prior
            if not isinstance(prior, DepthPrior):
                raise ValueError("TrainEngine: depth_prior=(P, inds) needs P as a DepthPrior (got %s)" % type(prior).__name__)
            table = prior.table
            if (not isinstance(inds, torch.Tensor) or inds.device != self.dev or inds.dtype != torch.int64 or tuple(inds.shape) != (n,)
                    or not inds.is_contiguous()):
                raise ValueError("TrainEngine: depth_prior=(P, inds) needs inds as a contiguous int64 (%d) tensor on %s" % (n, self.dev))
        else:
            table = depth_prior
            if not isinstance(table, torch.Tensor) or tuple(table.shape) != (n, 3):
                raise ValueError("TrainEngine: depth_prior must be a contiguous float32 (%d, 3) tensor on %s, or (DepthPrior, inds)"
                                 % (n, self.dev))
        if table.device != self.dev or table.dtype != torch.float32 or not table.is_contiguous():
            raise ValueError("TrainEngine: the depth prior rows must be contiguous float32 on %s" % (self.dev,))
        return table, table.shape[1], inds, table.shape[0]

    def forward_backward(self, rays, target, ray_offset=0, global_rays=None, draws=None, ray_grad=None, frozen=False, step=None,
                         exposure=None, depth_prior=None):
        """rays: (n, 8|11) packed rows on the device; target: (n, >=3), row stride free (an RGBA image's [..., :3] view
        works).  Leaves the summed-over-this-rank gradient in self.grad and {coarse_mse, fine_mse, sum} in self.loss
        (device); with world > 1 the gradient all-reduces are in flight when this returns (optimizer_step waits).
        global_rays: total rays of the step over all ranks when the shards are NOT equal -- this rank's cotangents are
        then weighted n * world / global_rays, so that the 1/world-scaled sum is the gradient of the global-batch mean.
        draws: None (production: in-kernel Philox draws keyed by (seed, step, global ray index)) or the reference's four
        draws as device tensors (t_rand (n, nc), noise_coarse (n, nc), u (n, nf), noise_fine (n, nc + nf); any may be
        None) -- e.g. made with torch.rand / torch.randn in the reference's order, to run the engine on exactly the random
        numbers another implementation consumed.
        ray_grad: None, or a contiguous float32 (n, 8|11) device tensor: the step then also computes d(loss)/d(rays) (the
        render backward with the ray gradient, nerfhip_render_bwd_rays; fused 64-wide backward modes run as mode 2 there).
        Its two parts land in two buffers: the fine net's in `ray_grad`, the coarse net's in the engine-owned
        `self.ray_grad_coarse` (a net with num_fine == 0: the whole of it in `ray_grad`); d(loss)/d(rays) is their sum, and
        train_utils.select_training_rays_bwd / step_on_image(pose_grad=...) add them row by row.  One rank only.
        frozen: True (needs ray_grad): the nets are left alone -- the backward is nerfhip_render_grad_rays, d(loss)/d(rays) without any
        parameter gradient: self.grad is not touched, no gradient is windowed or all-reduced; same streams, same two buffers.
        step: the counter the in-kernel draws are keyed by (default: step_count; the localisation steps pass localize_count).
        TrainEngine(backward="auto") is a policy of the training backward (its thresholds weigh the weight gradient's cost): a frozen
        step leaves each net in the mode its last training step chose and counts nothing in backward_modes_used.
        exposure: None, or (X, inds, hw): a cameras.Exposure on the engine's device, the int64 global indices of the batch (one per ray,
        what select_training_rays_views returned) and hw = height * width: both nets' losses are taken under X's per-view table
        (nerfhip_mse_loss_views_fwd_bwd in place of the plain loss launch, same streams), and after the two streams have joined
        X.backward(...) leaves d(loss)/d(table) in X.g_expo (three launches on the main stream, reading the engine's own rgb buffers).
        The exposure sits behind the render: it asks for no ray gradient.  With frozen=True and no ray_grad the step is the
        test-time fit: the two forwards, the two losses and the table gradient, no render backward.  One rank only.
        depth_prior: None, or the prior rows of the batch -- a contiguous float32 (n, 3) device tensor of (depth, weight, sigma), weight
        0 = no prior -- or (P, inds): a depth_prior.DepthPrior and the int64 global indices of the batch (what
        select_training_rays_views returned).  Needs TrainEngine(depth_loss=...); refused on a frozen step."""
        self._check_inputs(rays, target)
        dp = None if depth_prior is None else self._check_depth_prior(depth_prior, rays.shape[0], frozen)
        if self.alpha is not None:
            if target.shape[1] < 4:
                raise ValueError("TrainEngine: alpha=%r needs targets of 4 columns (r, g, b, alpha); got shape %s"
                                 % (self.alpha, tuple(target.shape)))
            if exposure is not None:
                raise ValueError("TrainEngine: exposure=... on an engine with alpha=%r is not covered: the loss under the exposure "
                                 "table reads no alpha" % (self.alpha,))
        if self.robust is not None and exposure is not None:
            raise ValueError("TrainEngine: exposure=... on an engine with photometric=... or trim=... is not covered: the loss under the "
                             "exposure table carries its own kernel")
        if frozen and any(self.spread):
            raise ValueError("TrainEngine: a frozen step (localize_*, the exposure fit) with spread > 0 makes no sense: the spread loss "
                             "regularises the nets, and a frozen step updates none")
        if frozen and self.proposal > 0.0:
            raise ValueError("TrainEngine: a frozen step (localize_*, the exposure fit) with proposal > 0 makes no sense: the proposal "
                             "loss trains the coarse net, and a frozen step updates none")
        if not self.coarse_photometric and not frozen and not (self.proposal > 0.0 or self.spread[0] > 0.0
                                                               or (dp is not None and any(self.depth_loss[0]))):
            raise ValueError("TrainEngine: coarse_photometric=False and a step without depth_prior=...: the coarse net's only loss is "
                             "its depth term, and this step has none")
        if self.occupancy is not None and (ray_grad is not None or frozen):
            raise NotImplementedError("TrainEngine: a step with a ray gradient (pose, camera, intrinsics or distortion gradients) or a "
                                      "frozen step (localize_*) is not implemented with occupancy=...: the ray gradient of the culled "
                                      "render is not covered")
        if frozen and ray_grad is None and exposure is None:
            raise RuntimeError("TrainEngine: forward_backward(frozen=True) computes the ray gradient alone: pass ray_grad=... "
                               "(or exposure=...: the fit of the exposure table alone)")
        ex_inds = ex_hw = None
        if exposure is not None:
            self._no_pose_grad_across_ranks("exposure")
            exposure, ex_inds, ex_hw = exposure
            self._check_exposure(exposure, None)
            if (not isinstance(ex_inds, torch.Tensor) or ex_inds.device != self.dev or ex_inds.dtype != torch.int64
                    or tuple(ex_inds.shape) != (rays.shape[0],) or not ex_inds.is_contiguous()):
                raise RuntimeError("TrainEngine: exposure=(X, inds, hw) needs inds as a contiguous int64 (%d) tensor on %s"
                                   % (rays.shape[0], self.dev))
            ex_hw = int(ex_hw)
        if ray_grad is not None:
            self._no_pose_grad_across_ranks("ray_grad")
            if not check_device_vector(ray_grad, rays.shape, self.dev):
                raise RuntimeError("TrainEngine: ray_grad must be a contiguous float32 tensor of the rays' shape %s on %s"
                                   % (tuple(rays.shape), self.dev))
        lib, n = self.lib, rays.shape[0]
        gscale = 1.0 if global_rays is None else float(n) * self.world / float(global_rays)
        culled = self._occupancy_active()
        if self.backward == "auto" and not frozen:
            self._choose_backward_modes()
        elif culled and self.backward is None:
            self._set_culled_modes(count=False)
        if self._set_window():   # (optimizer_step packed for this step already; only a step_count or schedule changed by hand gets here)
            self.repack()
        self._prepare(n)
        b = self._bufs
        nf = self.cfg.num_fine
        plan_f = self.mf._plan if self.mf is not None else None
        out = (b["rgb_c"].data_ptr(), b["disp_c"].data_ptr(), b["acc_c"].data_ptr(), None,
               b["rgb_f"].data_ptr() if nf > 0 else None, b["disp_f"].data_ptr() if nf > 0 else None,
               b["acc_f"].data_ptr() if nf > 0 else None, None)
        seed = self.seed + (self.step_count if step is None else step) * 0x9E3779B97F4A7C15 & 0xFFFFFFFFFFFFFFFF
        gc = self.grad[:self.nc_params]
        gf = self.grad[self.nc_params:] if nf > 0 else None
        tstride = target.stride(0)
        # (coarse_photometric=False: the coarse backward gets no colour cotangent -- a frozen step's ray gradient keeps it)
        matte = self.alpha is not None   # (then g_acc of the matte loss rides in the slot next to g_rgb, and is withheld with it)
        robust = self.robust is not None
        with_c = self.coarse_photometric or frozen
        cot_c = (b["g_c"].data_ptr() if with_c else None, b["ga_c"].data_ptr() if matte and with_c else None, None, None, None, None)
        cot_f = (None, None, None, b["g_f"].data_ptr() if nf > 0 else None, b["ga_f"].data_ptr() if matte and nf > 0 else None, None)
        if matte:
            bg = self.background
            matte_args = (int(self.alpha == "weight"), None, int(bg == "random")) + (bg if isinstance(bg, tuple) else (0.0, 0.0, 0.0))
        rand = None
        if draws is not None:
            shapes = ((n, self.cfg.num_coarse), (n, self.cfg.num_coarse), (n, nf), (n, self.cfg.num_coarse + nf))
            for d, shp in zip(draws, shapes):
                if d is not None and (d.device != self.dev or d.dtype != torch.float32 or tuple(d.shape) != shp or not d.is_contiguous()):
                    raise RuntimeError("TrainEngine: a random-draw tensor must be contiguous float32 %s on %s" % (shp, self.dev))
            self._draws = tuple(draws)  # (kept alive until the next step: the backward kernels read them again)
            rand = [None if d is None else d.data_ptr() for d in draws]
        # (the step's render: layout 1 -- the two nets' backwards may run at the same time --, the offsets of _prepare's workspace)
        call = self.render_call = RenderCall(lib, self.mc._plan, plan_f, self.cfg, rays.data_ptr(), n, self.packed_c.data_ptr(),
                                             self.packed_f.data_ptr() if nf > 0 else None, self.t_vals.data_ptr(),
                                             self.u_det.data_ptr() if nf > 0 else None, rand, seed, ray_offset, 1, self._ws.data_ptr(),
                                             self._wsb, self._regions)
        g_params = (gc.data_ptr(), gf.data_ptr() if gf is not None else None)
        tmp_c = tmp_f = g_rays_c = None
        if ray_grad is not None:
            g_rays_c, (tmp_c, tmp_f, tmpb) = self._ray_grad_bufs(n)
            if g_rays_c is None:
                g_rays_c = ray_grad
            # (the flat vectors as the nets run: theta_eff under an encoding window, as the last repack left it)
            pc_flat = self.mc._theta_eff(refresh=False).data_ptr()
            pf_flat = self.mf._theta_eff(refresh=False).data_ptr() if nf > 0 else None

        def net_pass(part, rgb, acc, g_rgb, g_acc, cot, loss, grad, model, tmp, g_rays, stream):
            """One net's loss, then its backward in the step's form, then its window gradients (behind its backward, ahead of its
            all-reduce), on `stream`.  With a spread weight: the spread kernel between the loss and the backward, and the backward's
            _w form."""
            fine = int(part == L.PART_FINE)
            g_weights = None
            if self.spread[fine] > 0.0:
                gw, sl = self._spread_bufs[fine]
                # (scale: lambda / n under the loss launch's grad_scale convention -- the total is the mse terms + lambda * mean_ray(L))
                call.spread(fine, self.spread[fine] * gscale / n, None, sl.data_ptr(), gw.data_ptr(), stream)
                g_weights = (None, gw.data_ptr()) if fine else (gw.data_ptr(), None)
            if dp is not None and any(self.depth_loss[fine]):
                gw, dl = self._depth_bufs[fine]
                a, bb = self.depth_loss[fine]
                # (scale: 1 / n under the same convention; behind a spread launch the term is added to the cotangent it wrote)
                call.depth_prior(fine, dp[0].data_ptr(), dp[1], None if dp[2] is None else dp[2].data_ptr(), dp[3], a, bb, gscale / n,
                                 None, dl.data_ptr(), gw.data_ptr(), self.spread[fine] > 0.0, stream)
                g_weights = (None, gw.data_ptr()) if fine else (gw.data_ptr(), None)
            if not fine and self.proposal > 0.0:
                gw, pl = self._proposal_bufs
                # (scale: lambda / n as for the spread term; behind a spread or depth launch the term is added to the cotangent it wrote.
                # Reads the fine pass's raw rows and depths: `stream` is behind the fine forward, and the fine backward only reads them)
                call.proposal(self.proposal * gscale / n, None, pl.data_ptr(), gw.data_ptr(), g_weights is not None, stream)
                g_weights = (gw.data_ptr(), None)
            if matte:   # (loss = {photometric, alpha, entropy} of this net; the background draws are the step's: seed, global ray index)
                lib.matte_loss_fwd_bwd(rgb.data_ptr(), acc.data_ptr(), target.data_ptr(), tstride, n, *matte_args, seed, ray_offset,
                                       self.alpha_loss[fine], self.opacity_entropy[fine], gscale, g_rgb.data_ptr(), g_acc.data_ptr(),
                                       loss.data_ptr(), stream)
            elif robust:   # (loss = {robust mean, kept fraction, tau} of this net; the net trims on its own residuals)
                kind, param, keep = self.robust[fine]
                rt = b.get("rt_f" if fine else "rt_c")
                lib.robust_loss_fwd_bwd(rgb.data_ptr(), target.data_ptr(), tstride, n, kind, param, keep, gscale, g_rgb.data_ptr(), None,
                                        None, loss.data_ptr(), None if rt is None else rt.data_ptr(), 0 if rt is None else 4 * rt.numel(),
                                        stream)
            elif exposure is None:
                lib.mse_loss_fwd_bwd(rgb.data_ptr(), None, target.data_ptr(), tstride, n, gscale, g_rgb.data_ptr(), None, loss.data_ptr(), stream)
            else:
                lib.mse_loss_views_fwd_bwd(rgb.data_ptr(), None, target.data_ptr(), tstride, n, gscale, ex_inds.data_ptr(), ex_hw,
                                           exposure.expo.data_ptr(), exposure.num_views, g_rgb.data_ptr(), None, loss.data_ptr(), stream)
            if ray_grad is None and frozen:   # (the fit of the exposure table alone: no render backward)
                return
            # (frozen: no parameter gradient -- the ray gradient alone)
            rays_args = None if ray_grad is None else (pc_flat, pf_flat, tmp.data_ptr(), tmpb, g_rays.data_ptr())
            call.backward(cot, g_params, part, stream, g_weights, rays_args, frozen)
            if not frozen:
                model._window_grads(grad, model._window_w, stream)

        occ = None
        if culled:   # (the grid's struct is read during the call; one list area serves both forwards: both run on the main stream)
            grid = self.occupancy._struct()
            occ = (grid, grid, self._occ_tmp.data_ptr(), self._occ_tb)
        fwd = lambda part, stream: call.forward(out, part, stream, occ)  # noqa: E731
        coarse = (L.PART_COARSE, b["rgb_c"], b["acc_c"], b["g_c"], b.get("ga_c"), cot_c, self._loss_c, gc, self.mc, tmp_c, g_rays_c)
        fine = (L.PART_FINE, b["rgb_f"], b["acc_f"], b["g_f"], b.get("ga_f"), cot_f, self._loss_f, gf, self.mf, tmp_f, ray_grad)
        self._pending = []
        self._depth_keep, self._depth_ran = dp, dp is not None
        with torch.cuda.device(self.dev):
            main, side = self._streams()
            st = main.cuda_stream
            two = self.overlap and nf > 0
            late = two and self.proposal > 0.0   # (the coarse net's pass reads the fine forward's rows: it overlaps the fine backward only)
            fwd(L.PART_COARSE, st)
            if two:
                e1, e2 = self._ev
            if two and not late:   # the coarse net's pass next to the fine forward and backward
                e1.record(main)
                side.wait_event(e1)
                net_pass(*coarse, side.cuda_stream)
                e2.record(side)
            if nf > 0:
                fwd(L.PART_FINE, st)
                if late:
                    e1.record(main)
                net_pass(*fine, st)
                if late:   # the coarse net's pass next to the fine backward
                    side.wait_event(e1)
                    net_pass(*coarse, side.cuda_stream)
                    e2.record(side)
                if self._reduce and not frozen:  # in flight while the coarse backward computes
                    self._pending.append(allreduce_gradients(gf, self.pg, async_op=True, single_rank=True))
            if two:
                main.wait_event(e2)
            else:
                net_pass(*coarse, st)
            if self._reduce and not frozen:
                self._pending.append(allreduce_gradients(gc, self.pg, async_op=True, single_rank=True))
            if nf > 0:
                torch.stack((self._loss_c[0], self._loss_f[0], self._loss_c[0] + self._loss_f[0]), out=self.loss)
            elif matte or robust:   # (the coarse net's words are {photometric, alpha, entropy} / {loss, kept fraction, tau})
                self.loss.zero_()
                self.loss[0::2] = self._loss_c[0]   # ({photometric_c, 0, sum}: no fine net, as the plain loss launch writes it)
            else:
                self.loss.copy_(self._loss_c)
            if self.backward == "auto" and not frozen:   # ({kept, total} of every net that ran over a list in the step just issued)
                self._stats.request(((name, self._stats_words(name)) for name, m in self._nets if m.backward_compaction in BM.BUILDS_LIST), main)
            if exposure is not None:   # (main stream, behind both nets' passes)
                exposure.backward(b["rgb_c"], b["rgb_f"] if nf > 0 else None, target, ex_inds, ex_hw, gscale)

    # ---- backward="auto" (the policy and its thresholds: backward_mode.choose) ----------------------------------------------------
    @staticmethod
    def _mode_for(frac, f16, fused=0):
        return BM.choose(frac, f16, fused)

    def _choose_backward_modes(self):
        """Sets each net's plan option for the step about to run.  The fractions come from the last compacted step whose two statistics
        words per net have arrived on the host (an asynchronous copy behind that step's backward; polled, never waited for); a net that
        runs dense produces none, so every backward_mode.PROBE_EVERY-th step runs compacted to look again."""
        self._stats.poll()
        if self._occupancy_active():   # (the culled forward fixes the modes; they are counted, and their statistics read, as ever)
            return self._set_culled_modes(count=True)
        probe = self.step_count % BM.PROBE_EVERY == 0
        for name, m in self._nets:
            mode = BM.choose(self._zero_frac[name], m.training_precision != "fp32", m.fused_backward_available(), probe)
            if m.backward_compaction != mode:
                m._apply_backward(mode)
            self.backward_modes_used[name][mode] += 1

    def _occupancy_active(self):
        """Whether the step about to run culls its samples through the grid (from step `occupancy_warmup` on)."""
        return self.occupancy is not None and self.step_count >= self.occupancy_warmup

    def _set_culled_modes(self, count):
        """The backward modes of a culled step (backward=None / "auto"): each net recomputes over its list -- in the fused kernel where
        it has one."""
        for name, m in self._nets:
            mode = BM.FUSED_COMPACT if m.fused_backward_available() else BM.RECOMPUTE
            if m.backward_compaction != mode:
                m._apply_backward(mode)
            if count:
                self.backward_modes_used[name][mode] += 1

    @property
    def occupancy_counts(self):
        """{kept_coarse, total_coarse, kept_fine, total_fine} of the last culled step's forwards: an int32 device view of the list
        area's first four words (no copy, no sync; zeros before the first culled step); None without a grid."""
        return None if self._occ_tmp is None else self._occ_tmp[:4]

    @property
    def spread_losses(self):
        """(coarse, fine): the mean over the last step's rays of each net's unscaled spread loss L, as device scalars formed on demand
        from the per-ray buffers the spread kernel wrote (no host synchronisation); None for a net without a spread weight or before
        the first step."""
        b = self._spread_bufs or {}
        return tuple(b[fine][1].mean() if fine in b else None for fine in (0, 1))

    @property
    def matte_losses(self):
        """(coarse, fine): each net's device tensor [3] = {photometric, alpha, entropy} of the last step (unscaled means, as
        nerfhip_matte_loss_fwd_bwd wrote them; no host synchronisation); fine is None without a fine net.  None without alpha=..."""
        if self.alpha is None:
            return None
        return (self._loss_c, self._loss_f if self.mf is not None else None)

    @property
    def robust_stats(self):
        """(coarse, fine): each net's device tensor [2] = {kept fraction, tau} of the last step's robust loss launch (views of the words
        nerfhip_robust_loss_fwd_bwd wrote; no host synchronisation; a net that does not trim reports {1, +inf}); fine is None without a
        fine net.  None without photometric= / trim=."""
        if self.robust is None:
            return None
        return (self._loss_c[1:3], self._loss_f[1:3] if self.mf is not None else None)

    @property
    def proposal_loss(self):
        """The mean over the last step's rays of the unscaled interlevel loss L, as a device scalar formed on demand from the per-ray
        buffer the proposal kernel wrote (no host synchronisation); None without a proposal weight or before the first step."""
        return None if self._proposal_bufs is None else self._proposal_bufs[1].mean()

    @property
    def depth_losses(self):
        """(coarse, fine): per net a device tensor (mean E, mean Tm) over ALL rays of the last step -- the unscaled expected-depth and
        termination losses the depth kernel wrote, formed on demand (no host synchronisation); None for a net without a weight, or
        when the last step was given no prior."""
        b = (self._depth_bufs or {}) if self._depth_ran else {}
        return tuple(b[fine][1].mean(dim=0) if fine in b else None for fine in (0, 1))

    def _stats_words(self, name):
        """The two statistics words of net `name` in the workspace of the last step."""
        return BM.stats_words(self.render_call, name, self._ws)

    def backward_sample_counts(self):
        """{"coarse": (kept, total), "fine": (kept, total)}: the sample points the last step's COMPACTED backward of each net kept
        (those whose d(loss)/d(raw) row is not all zero) and the sample points of that launch; None for a net whose
        set_backward_compaction is off.  Reads two words per net from the step's workspace: synchronises the device."""
        out = {"coarse": None, "fine": None}
        if self._ws is None:
            return out
        torch.cuda.synchronize(self.dev)
        for name, m in self._nets:
            if m.backward_compaction in BM.BUILDS_LIST:   # (the fused backward over every sample builds no list)
                out[name] = tuple(self._stats_words(name).tolist())
        return out

    def wait_gradients(self):
        """Orders this device's current stream behind the step's gradient all-reduces (no-op without collectives).

        Invariant the step relies on (nccl == RCCL): an asynchronous collective runs on the backend's own stream, which
        first waits for everything enqueued on the stream that was current when it was ISSUED (so the all-reduce of a
        net's gradient starts after that net's k_wgrad_reduce), and `work.wait()` does not block the host: it makes the
        stream that is current when it is CALLED wait for the collective.  Both the issue (forward_backward) and the wait
        happen with self.dev current and on self.dev's current stream -- the stream the Adam kernels are then launched on
        (optimizer_step) -- so Adam reads all-reduced gradients; the next step's kernels follow Adam on the same stream.
        gloo (the CPU / one-device tests) blocks the host in wait() instead: stronger, same result."""
        if not self._pending:
            return
        with torch.cuda.device(self.dev):
            for w in self._pending:
                if w is not None:
                    w.wait()
        self._pending = []

    def collective_times_ms(self, reps=20, warmup=3):
        """Diagnostic for the first real N-GPU run: what ONE gradient all-reduce of each net costs by itself -- the same
        buffers, the same process group, nothing else on the device -- as HIP events on the current stream around a
        synchronous collective (mean of `reps` after `warmup`).  In the step the fine net's all-reduce overlaps the coarse
        backward, so these are upper bounds of what the exchange adds.  Returns {"fine": ms, "coarse": ms} (None entries
        when there is no process group).  The step's pending collectives are waited for first and the live gradient is not
        touched (the transfers run on a zero-filled buffer of the same size)."""
        if not (torch.distributed.is_available() and torch.distributed.is_initialized()):
            return dict(fine=None, coarse=None)
        self.wait_gradients()  # (never next to the step's own collectives: they would reduce the same process group concurrently)
        out = {}
        # a zero-filled scratch of the gradient's size, NOT the live gradient: `warmup + reps` in-place SUM all-reduces multiply a
        # buffer by world^23 (inf / NaN on larger worlds); zeros stay zeros, and the transfer does not depend on the values
        scratch = torch.zeros_like(self.grad)
        with torch.cuda.device(self.dev):
            for name, sl in (("fine", scratch[self.nc_params:]), ("coarse", scratch[:self.nc_params])):
                if sl.numel() == 0:
                    out[name] = None
                    continue
                for _ in range(warmup):
                    allreduce_gradients(sl, self.pg, single_rank=True)
                torch.cuda.synchronize(self.dev)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    allreduce_gradients(sl, self.pg, single_rank=True)
                b.record()
                torch.cuda.synchronize(self.dev)
                out[name] = round(a.elapsed_time(b) / reps, 4)
        return out

    def optimizer_step(self, lr=None):
        lib = self.lib
        self.wait_gradients()
        self.step_count += 1
        lr = self.lr if lr is None else lr
        scale = 1.0 / self.world
        b1, b2 = self.betas
        n0 = self.nc_params
        with L.launch_on(self.grad, self.mc.flat_params) as st:
            lib.adam_step(self.mc.flat_params.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr(),
                          self.exp_avg_sq.data_ptr(), n0, lr, b1, b2, self.eps, self.step_count, scale, st)
            if self.mf is not None:
                lib.adam_step(self.mf.flat_params.data_ptr(), self.grad[n0:].data_ptr(), self.exp_avg[n0:].data_ptr(),
                              self.exp_avg_sq[n0:].data_ptr(), self.nf_params, lr, b1, b2, self.eps, self.step_count, scale,
                              st)
        self._set_window()   # (the window of the step that follows: its images are packed here)
        self.repack()
        g = self.occupancy
        if g is not None and g.density is not None and self.step_count % self.occupancy_every == 0:
            # (the engine's own plans and the images just packed: no second pack; on the stream of the step -- the next forward follows it)
            g.update_density(((self.mc._plan, self.packed_c), (self.mf._plan if self.mf is not None else None, self.packed_f)),
                             self.step_count // self.occupancy_every)

    def step(self, rays, target, ray_offset=0, lr=None, global_rays=None, draws=None, ray_grad=None, depth_prior=None):
        """One full training iteration.  Returns the device tensor {coarse_mse, fine_mse, sum} (no host sync).
        depth_prior: see forward_backward."""
        self.forward_backward(rays, target, ray_offset, global_rays, draws, ray_grad, depth_prior=depth_prior)
        self.optimizer_step(lr)
        return self.loss

    def step_on_image(self, image, pose, height, width, focal_length, options, num_random_rays, lr=None, global_rays=None,
                      pose_grad=None, intrinsics=None, distortion=None, exposure=None, depth_prior=None, depth_rays=0):
        """One whole iteration of the reference's loop body (train_nerf.py:210-270) on a resident training image:
        on-device selection of this rank's distinct pixels (ranks take disjoint slices of one permutation keyed by
        (seed, iteration)), their rays and targets, then `step`.  No host work besides launches.
        Weak scaling (default): every rank draws `num_random_rays` rays, the step covers world * num_random_rays.
        Strong scaling (`global_rays` = the step's total, BASELINE config 3: 8192 over 8 ranks): this rank takes its
        parallel.shard_bounds slice of the first `global_rays` positions; unequal shards are weighted (forward_backward).
        pose_grad: None, or a contiguous float32 (3, 4) tensor on the engine's device: the step also writes d(loss)/d(pose[:3, :4])
        into it (pose refinement: the render backward with the ray gradient, then the pose VJP of the selection on the main
        stream after the two streams joined, nerfhip_select_rays_bwd; still no host synchronisation).  The engine's Adam
        updates the nets as usual (lr=0 freezes them); a pose parametrisation of one's own takes the gradient with
        torch.autograd.backward(pose_expr[:3, :4], pose_grad).  One rank only.
        intrinsics: None, or a cameras.Intrinsics on the engine's device: the rays are generated from its (fx, fy, cx, cy), read on
        the device, and the step learns them -- see step_on_views.  `focal_length` must still be passed: it fixes the NDC constants.
        distortion: None, or a cameras.Distortion on the engine's device -- see step_on_views.
        exposure: refused -- a single image has no view axis for a per-view table: use step_on_views.
        depth_prior, depth_rays: a depth_prior.DepthPrior of ONE view -- see step_on_views."""
        self._no_exposure_on_image("step_on_image", exposure)
        if pose_grad is not None:
            self._no_pose_grad_across_ranks("pose_grad")
            self._check_pose_grads("pose_grad", pose_grad, (3, 4))
        return self._step_on_selection((height, width, focal_length, options), pose, image, False, num_random_rays, lr, global_rays,
                                       pose_grad, None, intrinsics, False, distortion, None, depth_prior, depth_rays)

    def step_on_views(self, images, poses, height, width, focal_length, options, num_random_rays, lr=None, global_rays=None,
                      pose_grads=None, cameras=None, intrinsics=None, distortion=None, exposure=None, depth_prior=None, depth_rays=0):
        """step_on_image over a resident stack of views: this rank's rays are drawn from ALL of `images` (V, H, W, 3|4) with the
        rays of each generated from its own row of `poses` (V, >=3, 4) -- train_utils.select_training_rays_views --, then `step`.
        Same rank slicing (first = rank * n, or the shard_bounds slice of `global_rays`) over the permutation of V * H * W, same
        ray_offset = first for the in-kernel draws, no host work besides launches.
        pose_grads: None, or a contiguous float32 (V, 3, 4) tensor on the engine's device: the step also writes
        d(loss)/d(poses[v, :3, :4]) of every view into it (zeros for a view without a ray in the batch): the render backward with
        the ray gradient, then nerfhip_select_rays_views_bwd on the main stream after the two streams joined; still no host
        synchronisation.  The engine's Adam updates the nets as usual (lr=0 freezes them).  One rank only.
        cameras: None, or a cameras.CameraTable on the engine's device (then `poses` must be None and `pose_grads` must not be
        given): the joint field-and-camera step -- the table composes its poses, the batch is drawn from them, the pose gradients
        land in the table's own buffer and are pulled back to its twists, the nets take their Adam step and the twists theirs (the
        table's own lr).  All of it on the main stream after the two streams joined; no host synchronisation.  One rank only.
        intrinsics: None, or a cameras.Intrinsics on the engine's device: the step learns the shared (fx, fy, cx, cy) next to the
        field (and the poses, when asked) -- intrinsics.values() -> selection from them -> forward_backward with the ray gradient ->
        ONE VJP call that fills the pose gradients (when asked) and intrinsics.g_intr -> cameras.backward() -> intrinsics.backward()
        -> the nets' Adam -> cameras.step() -> intrinsics.step().  Allowed with neither pose_grads nor cameras (it turns the ray
        gradient on).  `focal_length` must still be passed: it fixes the NDC constants, which do not follow the learned values.  One
        rank only.
        distortion: None, or a cameras.Distortion on the engine's device: the rays are undistorted under its (k1, k2, p1, p2), read on
        the device, and the step learns them, with or without `intrinsics` and `cameras`: the same ONE VJP call also fills
        distortion.g_dist, and distortion.step() follows intrinsics.step().  Alone it turns the ray gradient on.  One rank only.
        exposure: None, or a cameras.Exposure of V views on the engine's device: both losses are taken under its per-view colour gain
        and offset (forward_backward(exposure=...)) and the step learns the table: X.backward() after the two streams joined,
        X.step() last (after distortion.step()).  Alone or with any of the above.  It sits behind the render and does NOT turn the
        ray gradient on: alone, the step is selection, forward_backward, optimizer_step, X.step().  One rank only.
        depth_prior: None, or a depth_prior.DepthPrior of these V views on the engine's device (needs TrainEngine(depth_loss=...)): the
        selection's global indices are handed to the depth kernel, which reads each ray's prior row from the resident table.
        depth_rays: m rays of the batch drawn from the pixels that carry a prior (a sparse table gives a uniformly drawn batch almost
        none; DS-NeRF draws keypoint rays separately): the step's indices are the first n - m positions of the usual keyed permutation
        followed by P.pixels[j], j the positions rank * m ... rank * m + m - 1 of a second keyed permutation over len(P.pixels)
        (nerfhip_select_indices with the seed XORed with DEPTH_RAYS_KEY); 0 <= m <= min(n, len(P.pixels)); refused with global_rays.
        No host synchronisation."""
        return self._step_on_selection((height, width, focal_length, options), poses, images, True, num_random_rays, lr, global_rays,
                                       pose_grads, cameras, intrinsics, False, distortion, exposure, depth_prior, depth_rays)

    def localize_on_image(self, image, pose, height, width, focal_length, options, num_random_rays, pose_grad=None, intrinsics=None,
                          distortion=None, exposure=None):
        """step_on_image(pose_grad=...) for FROZEN nets (camera localisation against a trained field): the same selection, forward and
        pose VJP, with the render backward w.r.t. the rays alone (forward_backward(frozen=True)) and no optimizer step.  Nothing of
        the nets or their optimiser moves -- flat_params, exp_avg, exp_avg_sq, grad, the packed images and step_count are what they
        were, bit for bit --; the selection and the in-kernel draws are keyed by `localize_count`, which advances instead.
        pose_grad: a contiguous float32 (3, 4) tensor on the engine's device, overwritten with d(loss)/d(pose[:3, :4]).  One rank only.
        intrinsics: None, or a cameras.Intrinsics (see step_on_views): its values are learned against the frozen field; then
        pose_grad may be None.
        distortion: None, or a cameras.Distortion (see step_on_views), learned against the frozen field; then pose_grad may be None.
        exposure: refused -- a single image has no view axis for a per-view table: use localize_on_views."""
        self._no_exposure_on_image("localize_on_image", exposure)
        self._no_pose_grad_across_ranks("localize_on_image")
        if pose_grad is None and intrinsics is None and distortion is None:
            raise RuntimeError("TrainEngine: localize_on_image needs pose_grad=... or intrinsics=... (or distortion=...)")
        if pose_grad is not None:
            self._check_pose_grads("pose_grad", pose_grad, (3, 4))
        return self._step_on_selection((height, width, focal_length, options), pose, image, False, num_random_rays, None, None,
                                       pose_grad, None, intrinsics, True, distortion)

    def localize_on_views(self, images, poses, height, width, focal_length, options, num_random_rays, pose_grads=None, cameras=None,
                          intrinsics=None, distortion=None, exposure=None):
        """step_on_views for FROZEN nets (see localize_on_image): with pose_grads (V, 3, 4) the step writes d(loss)/d(poses[v, :3, :4])
        of every view; with cameras=T (then poses must be None and pose_grads must not be given) the table composes its poses, takes
        the gradients in its own buffer, pulls them back to its twists (T.backward()) and steps them (T.step()) -- the nets stay put.
        intrinsics: None, or a cameras.Intrinsics (see step_on_views): its values are learned against the frozen field, alone or
        together with the poses.  distortion: None, or a cameras.Distortion, in the same way.
        exposure: None, or a cameras.Exposure (see step_on_views), fitted against the frozen field.  Alone it is the test-time fit of
        a held-out view's exposure: the two forwards, the two losses under the table, the table gradient and X.step() -- no render
        backward at all.  One rank only."""
        self._no_pose_grad_across_ranks("localize_on_views")
        if cameras is None and pose_grads is None and intrinsics is None and distortion is None and exposure is None:
            raise RuntimeError("TrainEngine: localize_on_views needs pose_grads=..., cameras=... or intrinsics=... (or distortion=... "
                               "or exposure=...)")
        return self._step_on_selection((height, width, focal_length, options), poses, images, True, num_random_rays, None, None,
                                       pose_grads, cameras, intrinsics, True, distortion, exposure)

    def _resolve_cameras(self, poses, pose_grads, cameras):
        """(poses, pose_grads) of a step over views: the caller's, checked; or, with cameras=T, the table's composed poses and its own
        gradient buffer (then `poses` must be None and `pose_grads` must not be given).  One rank only where a pose gradient is asked."""
        if cameras is not None:
            if poses is not None:
                raise RuntimeError("TrainEngine: with cameras=... the poses come from the table: pass poses=None")
            if pose_grads is not None:
                raise RuntimeError("TrainEngine: cameras=... and pose_grads=... exclude each other (the table owns its gradient buffer)")
            self._no_pose_grad_across_ranks("cameras")
            if cameras.dev != self.dev:
                raise RuntimeError("TrainEngine: the camera table lives on %s, the engine on %s" % (cameras.dev, self.dev))
            return cameras.poses(), cameras.g_poses
        if pose_grads is not None:
            self._no_pose_grad_across_ranks("pose_grads")
            self._check_pose_grads("pose_grads", pose_grads, (poses.shape[0], 3, 4))
        return poses, pose_grads

    def _check_pose_grads(self, name, g, shape):
        check_device_vector(g, shape, self.dev, "TrainEngine: " + name)

    @staticmethod
    def _no_exposure_on_image(what, exposure):
        if exposure is not None:
            raise RuntimeError("TrainEngine: %s takes no exposure=...: a single image has no view axis for a per-view table (use "
                               "the _on_views form with a stack of one)" % what)

    def _check_exposure(self, exposure, num_views):
        """exposure=X of a step: a cameras.Exposure on the engine's device, of `num_views` views (None: not checked)."""
        if not isinstance(exposure, Exposure):
            raise RuntimeError("TrainEngine: exposure must be a cameras.Exposure (got %s)" % type(exposure).__name__)
        if exposure.dev != self.dev:
            raise RuntimeError("TrainEngine: the exposure table lives on %s, the engine on %s" % (exposure.dev, self.dev))
        if num_views is not None and exposure.num_views != num_views:
            raise RuntimeError("TrainEngine: the exposure table holds %d views, the step draws from %d" % (exposure.num_views, num_views))

    # the second permutation of depth_rays= is keyed by the engine's seed XOR this constant (the 64-bit golden-ratio constant's complement)
    DEPTH_RAYS_KEY = 0x61C8864680B583EB

    def _depth_select_inds(self, prior, n, m, first, count, population):
        """The step's indices under depth_rays=m (see step_on_views): two nerfhip_select_indices launches, a gather and a concatenation
        on the engine's device, no host synchronisation."""
        lib = self.lib
        seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        head = torch.empty(n - m, dtype=torch.int64, device=self.dev)
        pos = torch.empty(m, dtype=torch.int64, device=self.dev)
        with L.launch_on(prior.pixels, head, pos) as st:
            if n - m > 0:
                lib.select_indices(seed, int(count), population, first, n - m, head.data_ptr(), st)
            lib.select_indices(seed ^ self.DEPTH_RAYS_KEY, int(count), prior.pixels.numel(), self.rank * m, m, pos.data_ptr(), st)
            return torch.cat((head, prior.pixels[pos]))

    def _step_on_selection(self, scene, poses, images, views, num_random_rays, lr, global_rays, pose_grads, cameras, intrinsics, frozen,
                           distortion=None, exposure=None, depth_prior=None, depth_rays=0):
        """The step of step_on_image / step_on_views / localize_on_* behind their own argument checks.  scene: (height, width,
        focal_length, options); views: whether `poses` / `images` carry a view axis.  In launch order: the checks of intrinsics=I and
        distortion=D, then I.values() and D.values(); cameras=T checked, T.poses() (_resolve_cameras); this rank's slice of the
        step's permutation; the selection; `step` -- or, with any of pose_grads / cameras / intrinsics / distortion,
        forward_backward with the ray gradient, then on the main stream after the two streams joined ONE VJP call that fills
        `pose_grads` (when asked), I.g_intr and D.g_dist, T.backward(), I.backward(), optimizer_step, T.step(), I.step(), D.step().
        frozen (localize_on_*): the ray gradient alone and no optimizer_step; the selection and the draws are keyed by
        localize_count, which advances.  Without intrinsics (distortion) no intrinsics (distortion) keyword is passed on: the step
        reaches the entry points of the selection without them.
        exposure=X (views only): checked first, ahead of intrinsics and distortion; forward_backward takes (X, the selection's indices, height * width) --
        alone WITHOUT a ray gradient --, and X.step() comes last, after D.step()."""
        height, width, focal_length, options = scene
        kw, vjp_kw = {}, {}
        depth_rays = int(depth_rays)
        if depth_prior is None:
            if depth_rays:
                raise ValueError("TrainEngine: depth_rays=%d without depth_prior=..." % depth_rays)
        else:
            if not isinstance(depth_prior, DepthPrior):
                raise ValueError("TrainEngine: depth_prior must be a depth_prior.DepthPrior (got %s)" % type(depth_prior).__name__)
            self._check_depth_prior((depth_prior, torch.empty(0, dtype=torch.int64, device=self.dev)), 0, frozen)
            nviews = images.shape[0] if views else 1
            if (depth_prior.num_views, depth_prior.height, depth_prior.width) != (nviews, int(height), int(width)):
                raise ValueError("TrainEngine: the depth prior holds %d views of %d x %d, the step draws from %d of %d x %d"
                                 % (depth_prior.num_views, depth_prior.height, depth_prior.width, nviews, int(height), int(width)))
            if depth_rays and global_rays is not None:
                raise ValueError("TrainEngine: depth_rays=... and global_rays=... exclude each other")
            if not 0 <= depth_rays <= min(int(num_random_rays), depth_prior.pixels.numel() // self.world):
                raise ValueError("TrainEngine: depth_rays must lie in 0 ... min(num_random_rays, len(P.pixels)) (got %d; %d rays, %d "
                                 "pixels with a prior over %d ranks)" % (depth_rays, int(num_random_rays), depth_prior.pixels.numel(),
                                                                         self.world))
        if exposure is not None:
            self._no_pose_grad_across_ranks("exposure")
            self._check_exposure(exposure, images.shape[0] if isinstance(images, torch.Tensor) and images.dim() == 4 else None)
        if intrinsics is not None:
            if not isinstance(intrinsics, Intrinsics):
                raise RuntimeError("TrainEngine: intrinsics must be a cameras.Intrinsics (got %s)" % type(intrinsics).__name__)
            self._no_pose_grad_across_ranks("intrinsics")
            if intrinsics.dev != self.dev:
                raise RuntimeError("TrainEngine: the intrinsics live on %s, the engine on %s" % (intrinsics.dev, self.dev))
            kw = dict(intrinsics=intrinsics.values())
        if distortion is not None:
            if not isinstance(distortion, Distortion):
                raise RuntimeError("TrainEngine: distortion must be a cameras.Distortion (got %s)" % type(distortion).__name__)
            self._no_pose_grad_across_ranks("distortion")
            if distortion.dev != self.dev:
                raise RuntimeError("TrainEngine: the distortion lives on %s, the engine on %s" % (distortion.dev, self.dev))
            kw = dict(kw, distortion=distortion.values())
        if views:
            poses, pose_grads = self._resolve_cameras(poses, pose_grads, cameras)
        if intrinsics is not None or distortion is not None:   # (pose_grads None: no pose gradient is computed)
            vjp_kw = dict(kw, want_poses=pose_grads is not None)
        if intrinsics is not None:
            vjp_kw["out_intrinsics"] = intrinsics.g_intr
        if distortion is not None:
            vjp_kw.update(out_distortion=distortion.g_dist, distortion_mask=distortion.mask)
        if global_rays is None:
            n = int(num_random_rays)
            first = self.rank * n
        else:
            first, hi = shard_bounds(int(global_rays), self.rank, self.world)
            n = hi - first
        select = TU.select_training_rays_views if views else TU.select_training_rays
        count = self.localize_count if frozen else self.step_count
        if depth_rays:   # (the last depth_rays rays of the batch come from the pixels that carry a prior)
            population = int(height) * int(width) * (images.shape[0] if views else 1)
            kw = dict(kw, select_inds=self._depth_select_inds(depth_prior, n, depth_rays, first, count, population))
        with torch.no_grad():
            rays, target, used = select(height, width, focal_length, poses, images, n, options, seed=self.seed, step=count, first=first, **kw)
        want_rays = pose_grads is not None or intrinsics is not None or distortion is not None
        dkw = {} if depth_prior is None else dict(depth_prior=(depth_prior, used))
        if not want_rays and exposure is None:
            return self.step(rays, target, ray_offset=first, lr=lr, global_rays=global_rays, **dkw)
        ex = None if exposure is None else (exposure, used, int(height) * int(width))
        if want_rays:
            self._ray_grad_bufs(n, own=True)
        self.forward_backward(rays, target, first, global_rays, None, self._ray_grad if want_rays else None, frozen, count, ex, **dkw)
        if want_rays:
            vjp = TU.select_training_rays_views_bwd if views else TU.select_training_rays_bwd
            with torch.cuda.device(self.dev):
                vjp(height, width, focal_length, poses, used, self._ray_grad, options, self.ray_grad_coarse, out=pose_grads, **vjp_kw)
        if cameras is not None:
            cameras.backward()
        if intrinsics is not None:
            intrinsics.backward()
        if frozen:
            self.localize_count += 1
        else:
            self.optimizer_step(lr)
        if cameras is not None:
            cameras.step()
        if intrinsics is not None:
            intrinsics.step()
        if distortion is not None:
            distortion.step()
        if exposure is not None:
            exposure.step()
        return self.loss

    @staticmethod
    def lr_at(iteration, lr0=5e-3, lr_decay=250, lr_decay_factor=0.1):
        """train_nerf.py:264-270: lr0 * factor ** (i / (lr_decay * 1000))."""
        return lr0 * (lr_decay_factor ** (iteration / (lr_decay * 1000.0)))

    @staticmethod
    def psnr(loss_sum):
        v = float(loss_sum)
        return -10.0 * math.log10(v if v != 0 else 1e-5)
