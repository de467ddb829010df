"""Occupancy grid of the inference render: one bit per cell of a box around the scene, built once from the trained density
(Instant-NGP / NerfAcc / PlenOctrees style).  A sample whose point falls into an empty cell is never sent through the MLPs
(include/nerfhip.h "occupancy grid").

In training the grid is kept alive while the nets change: OccupancyGrid.for_training starts from an all-ones grid with a
zero density per cell, TrainEngine(..., occupancy=grid) culls its steps' samples through it from a warm-up on and calls
grid.update_density every few steps (decayed running maximum of the probed density, thresholded at min(threshold, mean density)).

    grid = OccupancyGrid.from_models(model_coarse, model_fine, aabb=((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)))
    with torch.no_grad():
        out, rows = render_pose_rows(H, W, focal, pose, model_coarse, model_fine, cfg, enc_xyz, enc_dir, occupancy=grid)
    kept_c, total_c, kept_f, total_f = grid.view_counts.tolist()   # of the whole view (the only host sync: whenever the caller asks)
"""
import ctypes as C

import torch

from . import _lib as L
from .render_call import RenderCall


def _aabb(aabb):
    lo, hi = aabb
    lo, hi = tuple(float(v) for v in lo), tuple(float(v) for v in hi)
    if len(lo) != 3 or len(hi) != 3 or not all(h > l for l, h in zip(lo, hi)):
        raise ValueError("aabb must be ((lo_x, lo_y, lo_z), (hi_x, hi_y, hi_z)) with hi > lo on every axis")
    return lo, hi


def _resolution(resolution):
    res = (int(resolution),) * 3 if isinstance(resolution, int) else tuple(int(r) for r in resolution)
    if len(res) != 3 or not all(1 <= r <= 512 for r in res) or (res[0] * res[1] * res[2]) % 32:
        raise ValueError("resolution: one or three values in 1 .. 512 whose product is a multiple of 32 (got %r)" % (resolution,))
    return res


class OccupancyGrid:
    """Device bits + box + resolution.  `bits`: int32 tensor of resolution product / 32 words; bit b of the grid (cell
    (i_z * res_y + i_y) * res_x + i_x) is bit b & 31 of word b >> 5.  `outside`: whether a point outside the box counts as
    occupied.  `last_counts`: int32 device tensor {kept_coarse, total_coarse, kept_fine, total_fine} of the last ray CHUNK that
    ran through this grid; `view_counts`: the same four, int64, summed on the device over every chunk since they were last zeroed --
    run_one_iter_of_nerf (and so render_pose_rows) zeroes them first, so after it they are the counts of the whole call.  Both are
    written by the device and read (.tolist()) whenever the caller wants them: no host sync of their own."""

    def __init__(self, bits, aabb, resolution, outside=False):
        self.aabb = _aabb(aabb)
        self.resolution = _resolution(resolution)
        self.outside = bool(outside)
        words = self.resolution[0] * self.resolution[1] * self.resolution[2] // 32
        if not bits.is_cuda:
            raise RuntimeError("OccupancyGrid needs a CUDA (HIP) tensor: nerf_pytorch_amd has no CPU path")
        if bits.dtype != torch.int32 or bits.numel() != words or not bits.is_contiguous():
            raise ValueError("bits: a contiguous int32 tensor of %d words" % words)
        self.bits = bits
        self.density = None     # fp32 [num_cells] on the device: the density grid of training (for_training / update_density), else None
        self.update_count = 0   # update_density calls so far: the next one probes with pass 1 + update_count mod 4095
        self._scratch = None    # update_density's buffers (second bits buffer, the two tmp areas), made on first use
        self.last_threshold = None   # after update_density: a device view of min(threshold, mean density) of that call
        self.last_counts = torch.zeros(4, dtype=torch.int32, device=bits.device)
        self.view_counts = torch.zeros(4, dtype=torch.int64, device=bits.device)

    # ---- C ABI ---------------------------------------------------------------------------------------------------------
    def _struct(self):
        g = L.OccGrid()
        g.bits = self.bits.data_ptr()
        g.lo = (C.c_float * 3)(*self.aabb[0])
        g.hi = (C.c_float * 3)(*self.aabb[1])
        g.res = (C.c_int * 3)(*self.resolution)
        g.outside = int(self.outside)
        return g

    @property
    def num_cells(self):
        return self.resolution[0] * self.resolution[1] * self.resolution[2]

    # ---- construction --------------------------------------------------------------------------------------------------
    @classmethod
    def from_models(cls, model_coarse, model_fine, aabb, resolution=128, passes=4, threshold=0.01, dilate=1, seed=0,
                    chunk_cells=1 << 20, outside=False):
        """The grid of two trained nets: a cell is occupied where either net's raw density exceeds `threshold` at the cell
        centre (pass 0) or at one of passes - 1 jittered probes, then dilated `dilate` times by one cell across faces.  The
        probes run through each net's inference plan, `chunk_cells` cells per launch (a multiple of 32: it bounds the scratch)."""
        lib = L.get_lib()
        res = _resolution(resolution)
        ncells = res[0] * res[1] * res[2]
        chunk = max(32, min(int(chunk_cells), ncells) // 32 * 32)
        dev = model_coarse._flat.device
        grid = cls(torch.zeros(ncells // 32, dtype=torch.int32, device=dev), aabb, res, outside)
        tb = int(lib.occ_update_tmp_bytes(chunk))
        tmp = torch.empty(tb // 4 + 64, dtype=torch.float32, device=dev)
        g = grid._struct()
        for model in (model_coarse, model_fine):
            if model is None:
                continue
            plan, packed = model._inference_plan(), model._inference_packed()
            with L.launch_on(grid.bits, tmp, packed) as st:
                for k in range(int(passes)):
                    for first in range(0, ncells, chunk):
                        lib.occ_update(plan, packed.data_ptr(), C.byref(g), float(threshold), k, int(seed), first,
                                       min(chunk, ncells - first), tmp.data_ptr(), tb, st)
        for _ in range(int(dilate)):
            out = torch.empty_like(grid.bits)
            with L.launch_on(grid.bits, out) as st:
                lib.occ_dilate(grid.bits.data_ptr(), out.data_ptr(), (C.c_int * 3)(*res), st)
            grid.bits = out
        return grid

    @classmethod
    def for_training(cls, aabb, resolution=128, outside=False, device="cuda"):
        """The grid a training run starts from: every bit set (nothing is culled until update_density has seen the nets) and a zero
        density per cell."""
        res = _resolution(resolution)
        ncells = res[0] * res[1] * res[2]
        grid = cls(torch.full((ncells // 32,), -1, dtype=torch.int32, device=device), aabb, res, outside)
        grid.density = torch.zeros(ncells, dtype=torch.float32, device=grid.bits.device)
        return grid

    def update_slab(self, step, fraction=0.25):
        """(first cell, cell count) of the slab update_density(step=...) probes: the grid is cut into ceil(1 / fraction) contiguous,
        32-aligned slabs and call `step` takes slab step mod that number -- any ceil(1 / fraction) consecutive steps cover the grid."""
        if not 0.0 < float(fraction) <= 1.0:
            raise ValueError("fraction must lie in (0, 1] (got %r)" % (fraction,))
        nslabs = int(-(-1.0 // float(fraction)))
        slab = -(-(self.num_cells // 32) // nslabs) * 32
        first = (int(step) % nslabs) * slab
        return min(first, self.num_cells), max(0, min(slab, self.num_cells - first))

    def update_density(self, plans_and_packed, step, decay=0.95, threshold=0.01, fraction=0.25, dilate=1, seed=0, chunk_cells=1 << 20):
        """One update of the density grid and, from it, of the bits (Instant-NGP's rule), on the current stream, with no host
        synchronisation.  plans_and_packed: (plan, packed image) pairs of the nets to probe (TrainEngine passes its own training
        plans and the images its optimizer step just packed).  step: the index of this update in the caller's schedule
        (TrainEngine: step_count // occupancy_every): it picks the slab of update_slab(step, fraction), one jittered probe per cell
        of it (pass 1 + update_count mod 4095 of nerfhip_occ_update's counter rule).  There
            density = max(density * decay, max over the nets of relu(sigma))            (nerfhip_occ_density_update)
        and then, over the whole grid, bit = density > min(threshold, mean(density)) (nerfhip_occ_density_bits), dilated `dilate`
        times across faces.  `bits` changes through `density` alone."""
        if self.density is None:
            raise RuntimeError("OccupancyGrid.update_density needs a density grid: build the grid with OccupancyGrid.for_training")
        lib = L.get_lib()
        first, count = self.update_slab(step, fraction)
        chunk = max(32, min(int(chunk_cells), max(count, 32)) // 32 * 32)
        res = (C.c_int * 3)(*self.resolution)
        dev = self.bits.device
        if self._scratch is None or self._scratch[0] != chunk:
            tb, bb = int(lib.occ_update_tmp_bytes(chunk)), int(lib.occ_density_bits_tmp_bytes(res))
            self._scratch = (chunk, torch.empty_like(self.bits), torch.empty(tb // 4 + 64, dtype=torch.float32, device=dev), tb,
                             torch.empty(bb // 4 + 64, dtype=torch.float32, device=dev), bb)
        _, alt, tmp, tb, btmp, bb = self._scratch
        g = self._struct()
        k = 1 + self.update_count % 4095
        nets = [(plan, packed) for plan, packed in plans_and_packed if plan is not None]
        with L.launch_on(self.bits, self.density, tmp, *[packed for _, packed in nets]) as st:
            for i, (plan, packed) in enumerate(nets):   # (the first net decays; the others only raise: the max over the nets)
                for c0 in range(first, first + count, chunk):
                    lib.occ_density_update(plan, packed.data_ptr(), C.byref(g), self.density.data_ptr(), float(decay) if i == 0 else 1.0,
                                           k, int(seed), c0, min(chunk, first + count - c0), tmp.data_ptr(), tb, st)
            cur, other = (self.bits, alt) if int(dilate) % 2 == 0 else (alt, self.bits)   # (the last write lands in self.bits)
            lib.occ_density_bits(self.density.data_ptr(), res, float(threshold), cur.data_ptr(), btmp.data_ptr(), bb, st)
            for _ in range(int(dilate)):
                lib.occ_dilate(cur.data_ptr(), other.data_ptr(), res, st)
                cur, other = other, cur
        self.last_threshold = btmp[:1]   # (a device view of min(threshold, mean density): no copy, no sync)
        self.update_count += 1

    def occupied_fraction(self):
        """Set cells / cells (a host sync)."""
        b = self.bits.view(torch.uint8)
        table = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64, device=b.device)
        return float(table[b.long()].sum().item()) / float(self.num_cells)

    # ---- checkpoints ---------------------------------------------------------------------------------------------------
    def state_dict(self):
        state = {"bits": self.bits.detach().cpu().clone(), "aabb": torch.tensor(self.aabb, dtype=torch.float32),
                 "resolution": torch.tensor(self.resolution, dtype=torch.int32), "outside": torch.tensor(int(self.outside))}
        if self.density is not None:   # (a grid of training: its density and the count its probes' pass numbers follow)
            state["density"] = self.density.detach().cpu().clone()
            state["update_count"] = torch.tensor(int(self.update_count))
        return state

    def load_state_dict(self, state):
        aabb = _aabb(tuple(tuple(float(v) for v in row) for row in state["aabb"].tolist()))
        res = _resolution(tuple(int(v) for v in state["resolution"].tolist()))
        bits = state["bits"].to(device=self.bits.device, dtype=torch.int32).contiguous()
        if bits.numel() != res[0] * res[1] * res[2] // 32:
            raise ValueError("state_dict: %d words of bits for resolution %r" % (bits.numel(), res))
        density = None
        if "density" in state:
            density = state["density"].to(device=self.bits.device, dtype=torch.float32).contiguous()
            if density.numel() != res[0] * res[1] * res[2]:
                raise ValueError("state_dict: %d density values for resolution %r" % (density.numel(), res))
        self.aabb, self.resolution, self.outside, self.bits = aabb, res, bool(int(state["outside"])), bits
        self.density, self.update_count, self._scratch = density, int(state.get("update_count", 0)), None
        return self

    @classmethod
    def from_state_dict(cls, state, device):
        res = tuple(int(v) for v in state["resolution"].tolist())
        g = cls(torch.zeros(res[0] * res[1] * res[2] // 32, dtype=torch.int32, device=device),
                tuple(tuple(float(v) for v in row) for row in state["aabb"].tolist()), res)
        return g.load_state_dict(state)


def render_fwd_occ(rays, model_c, model_f, cfg_tuple, rand, grid):
    """nerfhip_render_fwd_occ on a ray chunk (train_utils._predict_fused with a grid; inference only): the eight maps of the
    fused render, and grid.last_counts <- the chunk's kept / total sample counts."""
    lib = L.get_lib()
    nc, nf, perturb, lindisp, white, noise_std = cfg_tuple
    n, stride = rays.shape
    dev = rays.device
    from .nerf_helpers import linspace01
    cfg = L.RenderCfg(nc, nf, int(bool(perturb)), int(bool(lindisp)), int(bool(white)), float(noise_std), stride)
    plan_c = model_c._inference_plan()
    plan_f = model_f._inference_plan() if nf > 0 else None
    wsb = RenderCall.workspace_bytes(lib, plan_c, plan_f, cfg, n, 0)
    tb = RenderCall.occ_tmp_bytes(lib, cfg, n)
    ws = torch.empty(wsb // 4 + 1, dtype=torch.float32, device=dev)
    tmp = torch.empty(tb // 4, dtype=torch.int32, device=dev)
    names = ("rgb_coarse", "disp_coarse", "acc_coarse", "depth_coarse", "rgb_fine", "disp_fine", "acc_fine", "depth_fine")
    bufs = {k: torch.empty((n, 3) if k.startswith("rgb") else (n,), dtype=torch.float32, device=dev) for k in names}
    packed_c = model_c._inference_packed()
    packed_f = model_f._inference_packed() if nf > 0 else None
    call = RenderCall(lib, plan_c, plan_f, cfg, rays.data_ptr(), n, packed_c.data_ptr(), packed_f.data_ptr() if nf > 0 else None,
                      linspace01(nc, dev).data_ptr(), linspace01(nf, dev).data_ptr() if nf > 0 else None,
                      [None if r is None else r.data_ptr() for r in rand], 0, 0, 0, ws.data_ptr(), wsb)
    g = grid._struct()
    if n > 0:
        tmp[:4].zero_()  # (a pass that does not run -- num_fine == 0 -- leaves its pair untouched)
        with L.launch_on(rays, ws, tmp, grid.bits, packed_c, packed_f, *[r for r in rand if r is not None]) as st:
            call.forward([bufs[k].data_ptr() for k in names], L.PART_COARSE | L.PART_FINE, st, (g, g, tmp.data_ptr(), tb))
        grid.last_counts = tmp[:4]  # (a view of the chunk's list area: no copy, no sync)
        grid.view_counts += grid.last_counts
    return tuple(bufs[k] for k in names)
