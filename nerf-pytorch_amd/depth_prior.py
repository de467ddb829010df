"""DepthPrior: a device-resident table of sparse per-pixel depth priors (DS-NeRF, Deng et al. 2022) -- what a
structure-from-motion run leaves next to the cameras: a depth at some pixels of some views, each with a confidence.

The table is read ray by ray by nerfhip_depth_prior_loss (include/nerfhip.h) through the global pixel index the selection returns
(train_utils.select_training_rays_views' third output), so its rows are in SELECT-INDEX order: row g = v * H * W + col * H + row of
pixel (row, col) of view v -- the reference's flat select index k has row k % H and column k // H.  A row is (depth, weight, sigma);
weight 0 marks a pixel without a prior, and nothing else of such a row is interpreted.
"""
import torch


class DepthPrior:
    def __init__(self, depth, weight=None, sigma=0.05, device=None):
        """depth: (V, H, W) depths along the ray parameter t (for this library's pin-hole rays: the camera-space z-depth of a point);
        weight: (V, H, W) confidence weights c >= 0, None = 1 where `depth` is finite and > 0 (0 elsewhere); sigma: a float or
        (V, H, W), the standard deviation of the termination term.  ValueError for a pixel with c > 0 and a non-finite depth or
        sigma <= 0 (checked on the host, once).  device: where the table lives (default: depth's device)."""
        depth = torch.as_tensor(depth)
        if depth.dim() != 3:
            raise ValueError("DepthPrior: depth must be (V, H, W) (got shape %s)" % (tuple(depth.shape),))
        dev = depth.device if device is None else torch.device(device)
        d = depth.detach().to(torch.float32)
        if weight is None:
            w = (torch.isfinite(d) & (d > 0)).to(torch.float32)
        else:
            w = torch.as_tensor(weight).detach().to(torch.float32).to(d.device)
            if w.shape != d.shape:
                raise ValueError("DepthPrior: weight must have depth's shape %s (got %s)" % (tuple(d.shape), tuple(w.shape)))
        s = torch.as_tensor(sigma).detach().to(torch.float32).to(d.device)
        if s.dim() == 0:
            s = s.expand_as(d)
        elif s.shape != d.shape:
            raise ValueError("DepthPrior: sigma must be a number or have depth's shape %s (got %s)" % (tuple(d.shape), tuple(s.shape)))
        has = w > 0
        if bool((has & ~torch.isfinite(d)).any()):
            raise ValueError("DepthPrior: a pixel with weight > 0 has a non-finite depth")
        if bool((has & ~(s > 0)).any()):
            raise ValueError("DepthPrior: a pixel with weight > 0 has sigma <= 0 (or NaN)")
        self.num_views, self.height, self.width = (int(v) for v in d.shape)
        # (V, H, W) -> (V, W, H): row g = v H W + col H + row
        order = lambda t: t.transpose(1, 2).reshape(-1)  # noqa: E731
        self.table = torch.stack((order(d), order(w), order(s)), dim=1).contiguous().to(dev)
        self.pixels = torch.nonzero(self.table[:, 1] > 0).reshape(-1).contiguous()   # (ascending; int64)
        self.dev = self.table.device

    @classmethod
    def from_points(cls, num_views, height, width, view, row, col, depth, weight=1.0, sigma=0.05, device=None):
        """Scatters sparse keypoints (the COLMAP case: `weight` and `sigma` from the reprojection error, on the caller's side): point
        i is a depth at pixel (row[i], col[i]) of view[i].  weight, sigma: numbers or one per point.  ValueError for a pixel outside
        the views or named twice."""
        as_long = lambda t: torch.as_tensor(t).detach().to(torch.int64).reshape(-1).cpu()  # noqa: E731
        view, row, col = as_long(view), as_long(row), as_long(col)
        m = view.numel()
        as_f = lambda t: torch.as_tensor(t).detach().to(torch.float32).cpu().reshape(-1).expand(m) if torch.as_tensor(t).numel() in (1, m) else None  # noqa: E731
        d, w, s = as_f(depth), as_f(weight), as_f(sigma)
        if row.numel() != m or col.numel() != m or d is None or w is None or s is None:
            raise ValueError("DepthPrior.from_points: view, row, col, depth (and weight, sigma where given per point) must have one length")
        V, H, W = int(num_views), int(height), int(width)
        if m and bool(((view < 0) | (view >= V) | (row < 0) | (row >= H) | (col < 0) | (col >= W)).any()):
            raise ValueError("DepthPrior.from_points: a point lies outside the %d views of %d x %d pixels" % (V, H, W))
        flat = (view * H + row) * W + col
        if torch.unique(flat).numel() != m:
            raise ValueError("DepthPrior.from_points: a pixel is named twice")
        maps = [torch.zeros(V * H * W, dtype=torch.float32) for _ in range(3)]
        maps[2].fill_(1.0)   # (sigma of a pixel without a prior: never read)
        for t, v in zip(maps, (d, w, s)):
            t[flat] = v
        if device is None:
            device = torch.as_tensor(depth).device
        return cls(maps[0].reshape(V, H, W), maps[1].reshape(V, H, W), maps[2].reshape(V, H, W), device=device)

    def rows(self, select_inds):
        """The (n, 3) prior rows of a batch, gathered by the selection's global indices (what step(..., depth_prior=rows) takes)."""
        return self.table[select_inds.to(self.dev)].contiguous()
