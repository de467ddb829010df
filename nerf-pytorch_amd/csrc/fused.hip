// fused.hip -- predict_and_render_radiance (nerf/train_utils.py:28-127) as a fixed pipeline of kernels on one stream:
//   stratified depths -> coarse MLP (encodes in registers) -> compositing -> inverse-CDF + merge -> fine MLP ->
//   compositing, and the matching backward.  Nothing of size (N*S, 90) or (N*S, 256) is materialised for inference;
//   a training forward additionally writes the activation stash the weight-gradient GEMM consumes.
#include "nh_mlp.h"
#include "nh_raygrad.h"

namespace {

// one net's regions of the workspace (byte offsets)
struct NetSpace {
    int64_t z, raw, weights, stash;  // (weights: the coarse net's only -- the fine depths are drawn from them)
    // backward buffers, one set per net: the coarse and the fine backward chains are independent and may run on
    // different streams (nerfhip_render_bwd_parts)
    int64_t g_raw, scratch, scratch_bytes;
    int64_t gnorm;  // dL/d||rd|| per ray of the net's compositing backward (read by the ray-gradient pass)
};
struct Workspace {
    NetSpace c, f;
    int64_t total;
};

int64_t align_up(int64_t v) { return (v + 255) & ~(int64_t)255; }

// training: 0 = inference; 1 = training, one set of backward buffers per net (the two backward chains may then run on
// different streams: nerfhip_render_bwd_parts); 2 = training, the two nets SHARE one set of backward buffers (their
// backward chains must run one after the other on one stream -- what nerfhip_render_bwd does; a parts call says so with
// NERFHIP_PART_SHARED_BWD).  The forward's regions do not depend on that choice: they are laid out first.
Workspace layout(nerfhip_plan* pc, nerfhip_plan* pf, const nerfhip_render_cfg* cfg, int64_t n, int training) {
    Workspace w;
    memset(&w, 0, sizeof(w));
    const int64_t nc = cfg->num_coarse, nf = cfg->num_fine, sf = nc + nf;
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        int64_t o = off;
        off = align_up(off + bytes);
        return o;
    };
    w.c.z = take(n * nc * 4);
    w.c.raw = take(n * nc * 16);
    w.c.weights = take(n * nc * 4);
    if (nf > 0) {
        w.f.z = take(n * sf * 4);
        w.f.raw = take(n * sf * 16);
    }
    if (training) {
        w.c.gnorm = take(n * 4);
        if (nf > 0) w.f.gnorm = take(n * 4);
        w.c.stash = take(nerfhip_plan_stash_bytes(pc, n * nc));
        if (nf > 0) w.f.stash = take(nerfhip_plan_stash_bytes(pf, n * sf));
        w.c.scratch_bytes = nh_mlp_bwd_scratch_bytes(pc, n * nc);
        if (nf > 0) w.f.scratch_bytes = nh_mlp_bwd_scratch_bytes(pf, n * sf);
        if (training == 2 && nf > 0) {
            w.c.g_raw = w.f.g_raw = take(n * sf * 16);
            w.c.scratch = w.f.scratch = take(w.c.scratch_bytes > w.f.scratch_bytes ? w.c.scratch_bytes : w.f.scratch_bytes);
        } else {
            w.c.g_raw = take(n * nc * 16);
            w.c.scratch = take(w.c.scratch_bytes);
            if (nf > 0) {
                w.f.g_raw = take(n * sf * 16);
                w.f.scratch = take(w.f.scratch_bytes);
            }
        }
    }
    w.total = off;
    return w;
}

int check_cfg(nerfhip_plan* pc, nerfhip_plan* pf, const nerfhip_render_cfg* cfg) {
    NH_REQUIRE(pc && cfg, "render: plan/cfg is NULL");
    NH_REQUIRE(cfg->num_coarse >= 3 || (cfg->num_coarse >= 1 && cfg->num_fine == 0), "render: num_coarse too small");
    NH_REQUIRE(cfg->num_fine >= 0, "render: num_fine < 0");
    NH_REQUIRE(cfg->num_fine == 0 || pf, "render: num_fine > 0 needs a fine plan");
    NH_REQUIRE(cfg->ray_stride >= (pc->view ? 11 : 8), "render: ray_stride too small for use_viewdirs");
    NH_REQUIRE(!pf || pf->view == pc->view, "render: coarse/fine use_viewdirs mismatch");
    return NERFHIP_OK;
}

// what the passes of one call share
struct Call {
    const nerfhip_render_cfg* cfg;
    const float* rays;
    int64_t n;
    uint64_t seed, ray_offset;
    char* ws;
    nerfhip_stream_t stream;
};

// one net's pass through the pipeline: the coarse and the fine net take the same steps (forward_pass, backward_pass) with these
struct Pass {
    nerfhip_plan* plan;
    const float* packed;
    NhMlpInput in;        // the rays and the net's depths (the caller of forward_pass has put them into the z region); in.S per ray
    uint32_t rng_stream;  // of the compositing noise
    const float* noise;   // ... or the caller's
    NetSpace w;
    // the backward's: the net's cotangents, its gradient buffer, its flat parameters (the ray gradient reads them)
    const float *g_rgb, *g_depth, *g_acc;
    const float* g_weights;  // [n, in.S] cotangent of the ray weights, or NULL (the _w entry points: backward_pass alone reads it)
    float* g_params;
    const float* params;
};

Pass net_pass(const Call& c, bool fine, nerfhip_plan* plan, const float* packed, const nerfhip_render_rand* rnd, const Workspace& w) {
    Pass p;
    memset(&p, 0, sizeof(p));
    p.plan = plan;
    p.packed = packed;
    p.rng_stream = fine ? 3u : 1u;
    if (rnd) p.noise = fine ? rnd->noise_fine : rnd->noise_coarse;
    p.w = fine ? w.f : w.c;
    p.in.mode = 1;
    p.in.rays = c.rays;
    p.in.ray_stride = c.cfg->ray_stride;
    p.in.z = (const float*)(c.ws + p.w.z);
    p.in.S = c.cfg->num_coarse + (fine ? c.cfg->num_fine : 0);
    return p;
}

// the occupancy grid of one pass of nerfhip_render_fwd_occ and the sample list it is culled through
struct OccPass {
    const nerfhip_occ_grid* grid;
    NhCompact list;
};

// MLP over the pass's depths -> compositing.  (a training forward leaves in the stash what the plan's backward will read there:
// nh_mlp_forward_training)
// occ: mark / list / empty rows (nh_occ_list) -> the MLP over the listed samples alone, each result at its sample's own raw row -> the
// same compositing.  With `training` too (nerfhip_render_fwd_occ_train): the caller has checked that this plan's training forward
// leaves nothing in the stash, so the listed inference forward is that training forward on the kept samples
int forward_pass(const Call& c, const Pass& p, int training, float* rgb, float* disp, float* acc, float* weights, float* depth,
                 const OccPass* occ = nullptr) {
    const int64_t M = c.n * p.in.S;
    float* raw = (float*)(c.ws + p.w.raw);
    int rc;
    if (occ) {
        rc = nh_occ_list(occ->grid, c.rays, c.cfg->ray_stride, p.in.z, p.in.S, M, raw, occ->list, c.stream);
        if (rc) return rc;
        rc = nh_mlp_forward_listed(p.plan, p.packed, p.in, M, raw, occ->list, c.stream);
    } else {
        rc = training ? nh_mlp_forward_training(p.plan, p.packed, p.in, M, raw, (float*)(c.ws + p.w.stash), c.stream)
                      : nh_mlp_forward(p.plan, p.packed, p.in, M, raw, nullptr, c.stream);
    }
    if (rc) return rc;
    return nerfhip_volume_render_fwd(raw, p.in.z, c.rays + 3, c.cfg->ray_stride, c.n, p.in.S, c.cfg->noise_std, p.noise, c.seed,
                                     p.rng_stream, c.ray_offset, c.cfg->white_background, rgb, disp, acc, weights, depth, c.stream);
}

// compositing backward -> MLP backward (by the plan's data flow, nh_bwd_flow: it is told whether its d(pre-activation) images will
// be read) -> with g_rays: d(loss)/d(rays) of the pass, overwriting g_rays or accumulating into it: dL/d(encoded input) from the
// images the MLP backward just left in the scratch (nerfhip_mlp_bwd_input), then the positional encoding's backward and
// pts = ro + rd * z (nh_ray_grad)
int backward_pass(const Call& c, const Pass& q, void* tmp, int64_t tmp_bytes, float* g_rays, int accumulate) {
    nerfhip_plan* p = q.plan;
    const int64_t M = c.n * q.in.S;
    float* g_raw = (float*)(c.ws + q.w.g_raw);
    float* scratch = (float*)(c.ws + q.w.scratch);
    float* g_norm = g_rays ? (float*)(c.ws + q.w.gnorm) : nullptr;
    int rc = nh_volume_render_bwd((const float*)(c.ws + q.w.raw), q.in.z, c.rays + 3, c.cfg->ray_stride, c.n, q.in.S, c.cfg->noise_std,
                                  q.noise, c.seed, q.rng_stream, c.ray_offset, c.cfg->white_background, q.g_rgb, q.g_depth, q.g_acc, q.g_weights,
                                  g_raw, g_norm, c.stream);
    if (rc) return rc;
    rc = nh_mlp_backward(p, q.packed, &q.in, g_raw, M, (float*)(c.ws + q.w.stash), scratch, q.w.scratch_bytes, q.g_params,
                         g_rays != nullptr, c.stream);
    if (rc || !g_rays) return rc;
    const int64_t need = M * (int64_t)(p->Dx + p->Dd) * 4;
    NH_REQUIRE(q.params && tmp && tmp_bytes >= need, "render_bwd: the ray gradient needs the flat parameters and %lld bytes of tmp",
               (long long)need);
    rc = nerfhip_mlp_bwd_input(p, q.params, M, scratch, (float*)tmp, c.stream);
    if (rc) return rc;
    return nh_ray_grad(c.rays, c.cfg->ray_stride, c.n, q.in.z, q.in.S, (const float*)tmp, p->Dx, p->Dd, p->cfg.include_input_xyz ? 1 : 0,
                       (p->view && p->cfg.include_input_dir) ? 1 : 0, p->cfg.num_encoding_fn_xyz, p->view ? p->cfg.num_encoding_fn_dir : 0,
                       p->freqs_xyz, p->freqs_dir, g_norm, g_rays, accumulate, c.stream);
}

// The frozen form of backward_pass (nerfhip_render_grad_rays): compositing backward -> list / recomputation / data gradient
// (nh_mlp_backward_data: no weight gradient, no reduce, none of the weight gradient's bookkeeping) -> per-sample point and view
// gradients on the MFMAs (nh_raygrad.h) -> their sum per ray, overwriting g_rays or accumulating into it
int grad_rays_pass(const Call& c, const Pass& q, void* tmp, int64_t tmp_bytes, float* g_rays, int accumulate) {
    nerfhip_plan* p = q.plan;
    const int64_t M = c.n * q.in.S;
    float* g_raw = (float*)(c.ws + q.w.g_raw);
    float* scratch = (float*)(c.ws + q.w.scratch);
    float* g_norm = (float*)(c.ws + q.w.gnorm);
    const int64_t need = nh_point_grad_tmp_bytes(p, M);
    NH_REQUIRE(q.params && tmp && tmp_bytes >= need, "render_grad_rays: the ray gradient needs the flat parameters and %lld bytes of tmp",
               (long long)need);
    int rc = nh_volume_render_bwd((const float*)(c.ws + q.w.raw), q.in.z, c.rays + 3, c.cfg->ray_stride, c.n, q.in.S, c.cfg->noise_std,
                                  q.noise, c.seed, q.rng_stream, c.ray_offset, c.cfg->white_background, q.g_rgb, q.g_depth, q.g_acc, nullptr,
                                  g_raw, g_norm, c.stream);
    if (rc) return rc;
    NhBwdData d;
    rc = nh_mlp_backward_data(p, q.packed, &q.in, g_raw, M, (float*)(c.ws + q.w.stash), scratch, q.w.scratch_bytes, true, false, c.stream, &d);
    if (rc) return rc;
    // (need_images: nh_bwd_flow resolves no fused flow, so the data-gradient chain has just written the images read below)
    NH_REQUIRE(!d.f.fused, "render_grad_rays: the fused backward leaves no d(pre-activation) images");
    rc = nh_point_grad(p, q.params, M, scratch, d.cx, c.rays, c.cfg->ray_stride, q.in.z, q.in.S, (float*)tmp, c.stream);
    if (rc) return rc;
    return nh_ray_grad_sum(c.rays, c.cfg->ray_stride, c.n, q.in.z, q.in.S, (p->view && p->Dd > 0) ? 1 : 0, (const float*)tmp, g_norm, g_rays,
                           accumulate, c.stream);
}

}  // namespace

extern "C" int64_t nerfhip_render_workspace_bytes(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine,
                                                  const nerfhip_render_cfg* cfg, int64_t n_rays, int training) {
    if (check_cfg(plan_coarse, plan_fine, cfg) != NERFHIP_OK || n_rays < 0) return -1;
    return layout(plan_coarse, plan_fine, cfg, n_rays, training).total;
}

extern "C" int nerfhip_render_workspace_region(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine,
                                               const nerfhip_render_cfg* cfg, int64_t n_rays, int training, const char* name,
                                               int64_t* offset, int64_t* bytes) {
    int rc = check_cfg(plan_coarse, plan_fine, cfg);
    if (rc) return rc;
    NH_REQUIRE(name && offset && bytes && n_rays >= 0, "render_workspace_region: bad arguments");
    const Workspace w = layout(plan_coarse, plan_fine, cfg, n_rays, training);
    // (training layouts: each net's backward scratch -- nerfhip_plan_bwd_stats_offset points into it)
    // (... and the d(loss)/d(raw) rows its compositing backward writes)
    static const char* const names[2][5] = {{"z_coarse", "raw_coarse", "weights_coarse", "bwd_scratch_coarse", "bwd_g_raw_coarse"},
                                            {"z_fine", "raw_fine", nullptr, "bwd_scratch_fine", "bwd_g_raw_fine"}};
    for (int fine = 0; fine < 2; ++fine) {
        const NetSpace& s = fine ? w.f : w.c;
        const int64_t M = n_rays * (cfg->num_coarse + (fine ? cfg->num_fine : 0));
        const int64_t off[5] = {s.z, s.raw, s.weights, s.scratch, s.g_raw}, size[5] = {M * 4, M * 16, M * 4, s.scratch_bytes, M * 16};
        for (int i = 0; i < 5; ++i)
            if (names[fine][i] && strcmp(name, names[fine][i]) == 0) {
                NH_REQUIRE(!fine || cfg->num_fine > 0, "render_workspace_region: %s needs num_fine > 0", name);
                NH_REQUIRE(training || strncmp(name, "bwd_", 4) != 0, "render_workspace_region: %s exists in a training layout only", name);
                *offset = off[i];
                *bytes = size[i];
                return NERFHIP_OK;
            }
    }
    NH_REQUIRE(false, "render_workspace_region: unknown region '%s'", name);
}

// nerfhip_render_fwd_parts, and -- occ_c / occ_f: the passes' grids and lists, checked by the caller -- nerfhip_render_fwd_occ and
// nerfhip_render_fwd_occ_train
static int render_fwd(nerfhip_plan_t pc, nerfhip_plan_t pf, const nerfhip_render_cfg* cfg, const float* rays, int64_t n,
                      const float* packed_c, const float* packed_f, const float* t_vals, const float* u_det,
                      const nerfhip_render_rand* rnd, uint64_t seed, uint64_t ray_offset, const nerfhip_render_out* out, void* workspace,
                      int64_t workspace_bytes, int training, int parts, nerfhip_stream_t stream, const OccPass* occ_c,
                      const OccPass* occ_f) {
    int rc = check_cfg(pc, pf, cfg);
    if (rc) return rc;
    NH_REQUIRE(rays && packed_c && t_vals && out && workspace && n >= 0, "render_fwd: bad arguments");
    NH_REQUIRE(parts >= 1 && parts <= 3, "render_fwd: parts must be a combination of NERFHIP_PART_COARSE | NERFHIP_PART_FINE");
    NH_REQUIRE(cfg->num_fine == 0 || packed_f, "render_fwd: packed_fine is NULL");
    if (n == 0) return NERFHIP_OK;
    // (the regions a forward touches are the same in both training layouts; the size is checked against the layout the caller
    // names -- 1: one set of backward buffers per net, 2: shared -- so that an undersized workspace for the backward it intends
    // is refused here, not at backward time)
    NH_REQUIRE(training >= 0 && training <= 2, "render_fwd: training must be 0, 1 (two sets of backward buffers) or 2 (shared)");
    const Workspace w = layout(pc, pf, cfg, n, training);
    NH_REQUIRE(workspace_bytes >= w.total, "render_fwd: workspace too small (%lld < %lld)", (long long)workspace_bytes,
               (long long)w.total);
    const Call c = {cfg, rays, n, seed, ray_offset, (char*)workspace, stream};
    float* z_c = (float*)(c.ws + w.c.z);
    float* w_c = (float*)(c.ws + w.c.weights);
    if (parts & NERFHIP_PART_COARSE) {
        rc = nerfhip_stratified_z(rays, cfg->ray_stride, n, t_vals, cfg->num_coarse, cfg->lindisp, cfg->perturb, rnd ? rnd->t_rand : nullptr,
                                  seed, ray_offset, z_c, stream);
        if (rc) return rc;
        rc = forward_pass(c, net_pass(c, false, pc, packed_c, rnd, w), training, out->rgb_coarse, out->disp_coarse, out->acc_coarse, w_c,
                          out->depth_coarse, occ_c);
        if (rc) return rc;
    }
    if (cfg->num_fine > 0 && (parts & NERFHIP_PART_FINE)) {
        const int det = cfg->perturb ? 0 : 1;  // det = (perturb == 0.0), nerf/train_utils.py:101
        const float* u = rnd ? rnd->u : nullptr;
        NH_REQUIRE(!det || u || u_det, "render_fwd: perturb == 0 needs u_det");
        rc = nerfhip_hierarchical_z(z_c, w_c, n, cfg->num_coarse, u, det, u_det, cfg->num_fine, seed, ray_offset, nullptr,
                                    (float*)(c.ws + w.f.z), stream);
        if (rc) return rc;
        // (only the coarse compositing writes its weights: the fine depths were drawn from them)
        rc = forward_pass(c, net_pass(c, true, pf, packed_f, rnd, w), training, out->rgb_fine, out->disp_fine, out->acc_fine, nullptr,
                          out->depth_fine, occ_f);
        if (rc) return rc;
    }
    return NERFHIP_OK;
}

extern "C" int nerfhip_render_fwd_parts(nerfhip_plan_t pc, nerfhip_plan_t pf, const nerfhip_render_cfg* cfg,
                                        const float* rays, int64_t n, const float* packed_c, const float* packed_f,
                                        const float* t_vals, const float* u_det, const nerfhip_render_rand* rnd,
                                        uint64_t seed, uint64_t ray_offset, const nerfhip_render_out* out, void* workspace,
                                        int64_t workspace_bytes, int training, int parts, nerfhip_stream_t stream) {
    return render_fwd(pc, pf, cfg, rays, n, packed_c, packed_f, t_vals, u_det, rnd, seed, ray_offset, out, workspace, workspace_bytes,
                      training, parts, stream, nullptr, nullptr);
}

// tmp of nerfhip_render_fwd_occ: one list area (nh_compact_view) for the larger pass -- the two passes run one after the other and
// share its counts and list; the area's first 16 words are the statistics: words 0, 1 the coarse pass's {kept, total}, words 2, 3 the
// fine pass's (each pass's NhCompact::stats points at its own pair)
extern "C" int64_t nerfhip_render_occ_tmp_bytes(const nerfhip_render_cfg* cfg, int64_t n) {
    if (!cfg || n < 0 || cfg->num_coarse < 1 || cfg->num_fine < 0) return -1;
    const int64_t m = n * ((int64_t)cfg->num_coarse + cfg->num_fine);
    return nh_compact_ints(m > 0 ? m : 1) * 4;
}

// what nerfhip_render_fwd_occ and nerfhip_render_fwd_occ_train share: the checks of the grids, the plans and tmp, then render_fwd with
// one list area behind both passes.  training != 0 (the _train entry point): a pass that runs must be one whose training forward
// leaves nothing in the stash (nh_bwd_flow: recompute, no register-image stash) -- that forward IS the inference forward, so the
// listed one stands in for it, and the plan's backward recomputes from the forward's input over its own list
static int render_fwd_occ_any(const char* what, nerfhip_plan_t pc, nerfhip_plan_t pf, const nerfhip_render_cfg* cfg, const float* rays,
                              int64_t n, const float* packed_c, const float* packed_f, const float* t_vals, const float* u_det,
                              const nerfhip_render_rand* rnd, uint64_t seed, uint64_t ray_offset, const nerfhip_render_out* out,
                              void* workspace, int64_t workspace_bytes, int training, int parts, const nerfhip_occ_grid* grid_c,
                              const nerfhip_occ_grid* grid_f, void* tmp, int64_t tmp_bytes, nerfhip_stream_t stream) {
    int rc;
    NH_REQUIRE(parts >= 1 && parts <= 3, "%s: parts must be a combination of NERFHIP_PART_COARSE | NERFHIP_PART_FINE", what);
    NH_REQUIRE(n >= 0, "%s: bad arguments", what);
    const bool coarse_runs = (parts & NERFHIP_PART_COARSE) != 0, fine_runs = cfg->num_fine > 0 && (parts & NERFHIP_PART_FINE);
    for (int fine = 0; fine < 2; ++fine) {
        if (!(fine ? fine_runs : coarse_runs)) continue;
        const nerfhip_occ_grid* g = fine ? grid_f : grid_c;
        nerfhip_plan* p = fine ? pf : pc;
        NH_REQUIRE(g, "%s: grid_%s is NULL", what, fine ? "fine" : "coarse");
        if ((rc = nh_occ_check(g, what)) != 0 || (rc = nh_mlp_listed_check(p, what)) != 0) return rc;
        if (training) {
            const NhBwdFlow f = nh_bwd_flow(p, n * ((int64_t)cfg->num_coarse + (fine ? cfg->num_fine : 0)), true, false);
            NH_REQUIRE(f.recompute && !f.reg_image,
                       "%s: the %s plan's training forward leaves a stash (backward mode %d of nerfhip_plan_set_bwd_compaction, or an "
                       "inference-only plan, or too many sample points for the recomputing flow): the culled training forward works "
                       "with modes 2 (recompute), 3 (fused) and 4 (fused over the list)",
                       what, fine ? "fine" : "coarse", p->bwd_compact);
        }
    }
    const int64_t m_max = n * ((int64_t)cfg->num_coarse + cfg->num_fine);
    NH_REQUIRE(m_max < ((int64_t)1 << 31), "%s: at most 2^31 - 1 sample points per pass (got %lld)", what, (long long)m_max);
    const int64_t need = nerfhip_render_occ_tmp_bytes(cfg, n);
    NH_REQUIRE(tmp && tmp_bytes >= need, "%s: tmp too small (%lld < %lld)", what, (long long)tmp_bytes, (long long)need);
    OccPass oc, of;
    oc.grid = grid_c;
    oc.list = nh_compact_view((int*)tmp, m_max > 0 ? m_max : 1);
    of.grid = grid_f;
    of.list = oc.list;
    of.list.stats = oc.list.stats + 2;
    return render_fwd(pc, pf, cfg, rays, n, packed_c, packed_f, t_vals, u_det, rnd, seed, ray_offset, out, workspace, workspace_bytes,
                      training, parts, stream, &oc, &of);
}

extern "C" int nerfhip_render_fwd_occ(nerfhip_plan_t pc, nerfhip_plan_t pf, const nerfhip_render_cfg* cfg, const float* rays,
                                      int64_t n, const float* packed_c, const float* packed_f, const float* t_vals,
                                      const float* u_det, const nerfhip_render_rand* rnd, uint64_t seed, uint64_t ray_offset,
                                      const nerfhip_render_out* out, void* workspace, int64_t workspace_bytes, int training,
                                      int parts, const nerfhip_occ_grid* grid_c, const nerfhip_occ_grid* grid_f, void* tmp,
                                      int64_t tmp_bytes, nerfhip_stream_t stream) {
    int rc = check_cfg(pc, pf, cfg);
    if (rc) return rc;
    NH_REQUIRE(training == 0,
               "render_fwd_occ: an occupancy grid culls the inference render only (training = %d): the training forward and its backward "
               "run dense",
               training);
    return render_fwd_occ_any("render_fwd_occ", pc, pf, cfg, rays, n, packed_c, packed_f, t_vals, u_det, rnd, seed, ray_offset, out,
                              workspace, workspace_bytes, 0, parts, grid_c, grid_f, tmp, tmp_bytes, stream);
}

extern "C" int nerfhip_render_fwd_occ_train(nerfhip_plan_t pc, nerfhip_plan_t pf, const nerfhip_render_cfg* cfg, const float* rays,
                                            int64_t n, const float* packed_c, const float* packed_f, const float* t_vals,
                                            const float* u_det, const nerfhip_render_rand* rnd, uint64_t seed, uint64_t ray_offset,
                                            const nerfhip_render_out* out, void* workspace, int64_t workspace_bytes, int training,
                                            int parts, const nerfhip_occ_grid* grid_c, const nerfhip_occ_grid* grid_f, void* tmp,
                                            int64_t tmp_bytes, nerfhip_stream_t stream) {
    int rc = check_cfg(pc, pf, cfg);
    if (rc) return rc;
    NH_REQUIRE(training == 1 || training == 2,
               "render_fwd_occ_train: training must be 1 (two sets of backward buffers) or 2 (shared), got %d", training);
    return render_fwd_occ_any("render_fwd_occ_train", pc, pf, cfg, rays, n, packed_c, packed_f, t_vals, u_det, rnd, seed, ray_offset, out,
                              workspace, workspace_bytes, training, parts, grid_c, grid_f, tmp, tmp_bytes, stream);
}

extern "C" int nerfhip_render_fwd(nerfhip_plan_t pc, nerfhip_plan_t pf, const nerfhip_render_cfg* cfg, const float* rays,
                                  int64_t n, const float* packed_c, const float* packed_f, const float* t_vals,
                                  const float* u_det, const nerfhip_render_rand* rnd, uint64_t seed, uint64_t ray_offset,
                                  const nerfhip_render_out* out, void* workspace, int64_t workspace_bytes, int training,
                                  nerfhip_stream_t stream) {
    return nerfhip_render_fwd_parts(pc, pf, cfg, rays, n, packed_c, packed_f, t_vals, u_det, rnd, seed, ray_offset, out,
                                    workspace, workspace_bytes, training, NERFHIP_PART_COARSE | NERFHIP_PART_FINE, stream);
}

extern "C" int64_t nerfhip_render_bwd_rays_tmp_bytes(nerfhip_plan_t pc, nerfhip_plan_t pf, const nerfhip_render_cfg* cfg,
                                                     int64_t n) {
    if (check_cfg(pc, pf, cfg) != NERFHIP_OK || n < 0) return -1;
    int64_t b = n * cfg->num_coarse * (int64_t)(pc->Dx + pc->Dd) * 4;
    if (cfg->num_fine > 0) {
        const int64_t f = n * (cfg->num_coarse + cfg->num_fine) * (int64_t)(pf->Dx + pf->Dd) * 4;
        if (f > b) b = f;
    }
    return b;
}

// nerfhip_render_bwd_rays / _parts and their _w forms: gw_c / gw_f are the cotangents of the two passes' ray weights (NULL = none; a
// weight cotangent alone is enough for a pass to run)
static int render_bwd(nerfhip_plan_t pc, nerfhip_plan_t pf, const nerfhip_render_cfg* cfg, const float* rays, int64_t n,
                      const float* packed_c, const float* packed_f, const nerfhip_render_rand* rnd, uint64_t seed, uint64_t ray_offset,
                      const nerfhip_render_cotangents* g, const float* gw_c, const float* gw_f, void* workspace,
                      int64_t workspace_bytes, float* g_params_c, float* g_params_f, int parts, const float* params_c,
                      const float* params_f, void* tmp, int64_t tmp_bytes, float* g_rays, nerfhip_stream_t stream) {
    int rc = check_cfg(pc, pf, cfg);
    if (rc) return rc;
    NH_REQUIRE(rays && packed_c && g && workspace && n > 0, "render_bwd: bad arguments");
    const int shared = parts & NERFHIP_PART_SHARED_BWD;
    parts &= ~NERFHIP_PART_SHARED_BWD;
    NH_REQUIRE(parts >= 1 && parts <= 3, "render_bwd: parts must be a combination of NERFHIP_PART_COARSE | NERFHIP_PART_FINE");
    const Workspace w = layout(pc, pf, cfg, n, shared ? 2 : 1);
    NH_REQUIRE(workspace_bytes >= w.total, "render_bwd: workspace too small (%lld < %lld)", (long long)workspace_bytes,
               (long long)w.total);
    const Call c = {cfg, rays, n, seed, ray_offset, (char*)workspace, stream};
    int wrote_rays = 0;  // the first pass that runs overwrites g_rays, the second accumulates
    if (cfg->num_fine > 0 && (parts & NERFHIP_PART_FINE)) {
        NH_REQUIRE(packed_f && g_params_f && (g->g_rgb_fine || g->g_acc_fine || g->g_depth_fine || gw_f),
                   "render_bwd: fine arguments missing");
        Pass fine = net_pass(c, true, pf, packed_f, rnd, w);
        fine.g_rgb = g->g_rgb_fine, fine.g_depth = g->g_depth_fine, fine.g_acc = g->g_acc_fine;
        fine.g_weights = gw_f;
        fine.g_params = g_params_f, fine.params = params_f;
        rc = backward_pass(c, fine, tmp, tmp_bytes, g_rays, wrote_rays);
        if (rc) return rc;
        wrote_rays = g_rays != nullptr;
    }
    if (parts & NERFHIP_PART_COARSE) {
        NH_REQUIRE(g_params_c && (g->g_rgb_coarse || g->g_acc_coarse || g->g_depth_coarse || gw_c),
                   "render_bwd: coarse arguments missing");
        Pass coarse = net_pass(c, false, pc, packed_c, rnd, w);
        coarse.g_rgb = g->g_rgb_coarse, coarse.g_depth = g->g_depth_coarse, coarse.g_acc = g->g_acc_coarse;
        coarse.g_weights = gw_c;
        coarse.g_params = g_params_c, coarse.params = params_c;
        rc = backward_pass(c, coarse, tmp, tmp_bytes, g_rays, wrote_rays);
        if (rc) return rc;
    }
    return NERFHIP_OK;
}

extern "C" int nerfhip_render_bwd_rays(nerfhip_plan_t pc, nerfhip_plan_t pf, const nerfhip_render_cfg* cfg, const float* rays,
                                       int64_t n, const float* packed_c, const float* packed_f, const nerfhip_render_rand* rnd,
                                       uint64_t seed, uint64_t ray_offset, const nerfhip_render_cotangents* g, void* workspace,
                                       int64_t workspace_bytes, float* g_params_c, float* g_params_f, int parts,
                                       const float* params_c, const float* params_f, void* tmp, int64_t tmp_bytes,
                                       float* g_rays, nerfhip_stream_t stream) {
    return render_bwd(pc, pf, cfg, rays, n, packed_c, packed_f, rnd, seed, ray_offset, g, nullptr, nullptr, workspace, workspace_bytes,
                      g_params_c, g_params_f, parts, params_c, params_f, tmp, tmp_bytes, g_rays, stream);
}

extern "C" int nerfhip_render_bwd_parts(nerfhip_plan_t pc, nerfhip_plan_t pf, const nerfhip_render_cfg* cfg,
                                        const float* rays, int64_t n, const float* packed_c, const float* packed_f,
                                        const nerfhip_render_rand* rnd, uint64_t seed, uint64_t ray_offset,
                                        const nerfhip_render_cotangents* g, void* workspace, int64_t workspace_bytes,
                                        float* g_params_c, float* g_params_f, int parts, nerfhip_stream_t stream) {
    return render_bwd(pc, pf, cfg, rays, n, packed_c, packed_f, rnd, seed, ray_offset, g, nullptr, nullptr, workspace, workspace_bytes,
                      g_params_c, g_params_f, parts, nullptr, nullptr, nullptr, 0, nullptr, stream);
}

// the _w forms: the same routine with the weight cotangents of the extended struct (its first six members are
// nerfhip_render_cotangents, in order)
extern "C" int nerfhip_render_bwd_rays_w(nerfhip_plan_t pc, nerfhip_plan_t pf, const nerfhip_render_cfg* cfg, const float* rays,
                                         int64_t n, const float* packed_c, const float* packed_f, const nerfhip_render_rand* rnd,
                                         uint64_t seed, uint64_t ray_offset, const nerfhip_render_cotangents_w* g, void* workspace,
                                         int64_t workspace_bytes, float* g_params_c, float* g_params_f, int parts,
                                         const float* params_c, const float* params_f, void* tmp, int64_t tmp_bytes,
                                         float* g_rays, nerfhip_stream_t stream) {
    NH_REQUIRE(g, "render_bwd: bad arguments");
    const nerfhip_render_cotangents g6 = {g->g_rgb_coarse, g->g_acc_coarse, g->g_depth_coarse, g->g_rgb_fine, g->g_acc_fine, g->g_depth_fine};
    return render_bwd(pc, pf, cfg, rays, n, packed_c, packed_f, rnd, seed, ray_offset, &g6, g->g_weights_coarse, g->g_weights_fine,
                      workspace, workspace_bytes, g_params_c, g_params_f, parts, params_c, params_f, tmp, tmp_bytes, g_rays, stream);
}

extern "C" int nerfhip_render_bwd_parts_w(nerfhip_plan_t pc, nerfhip_plan_t pf, const nerfhip_render_cfg* cfg,
                                          const float* rays, int64_t n, const float* packed_c, const float* packed_f,
                                          const nerfhip_render_rand* rnd, uint64_t seed, uint64_t ray_offset,
                                          const nerfhip_render_cotangents_w* g, void* workspace, int64_t workspace_bytes,
                                          float* g_params_c, float* g_params_f, int parts, nerfhip_stream_t stream) {
    return nerfhip_render_bwd_rays_w(pc, pf, cfg, rays, n, packed_c, packed_f, rnd, seed, ray_offset, g, workspace, workspace_bytes,
                                     g_params_c, g_params_f, parts, nullptr, nullptr, nullptr, 0, nullptr, stream);
}

extern "C" int nerfhip_render_bwd(nerfhip_plan_t pc, nerfhip_plan_t pf, const nerfhip_render_cfg* cfg, const float* rays,
                                  int64_t n, const float* packed_c, const float* packed_f, const nerfhip_render_rand* rnd,
                                  uint64_t seed, uint64_t ray_offset, const float* g_rgb_c, const float* g_rgb_f,
                                  void* workspace, int64_t workspace_bytes, float* g_params_c, float* g_params_f,
                                  nerfhip_stream_t stream) {
    NH_REQUIRE(g_rgb_c && g_params_c, "render_bwd: bad arguments");
    nerfhip_render_cotangents g = {g_rgb_c, nullptr, nullptr, g_rgb_f, nullptr, nullptr};
    return nerfhip_render_bwd_parts(pc, pf, cfg, rays, n, packed_c, packed_f, rnd, seed, ray_offset, &g, workspace,
                                    workspace_bytes, g_params_c, g_params_f,
                                    NERFHIP_PART_COARSE | NERFHIP_PART_FINE | NERFHIP_PART_SHARED_BWD, stream);
}

extern "C" int64_t nerfhip_render_grad_rays_tmp_bytes(nerfhip_plan_t pc, nerfhip_plan_t pf, const nerfhip_render_cfg* cfg,
                                                      int64_t n) {
    if (check_cfg(pc, pf, cfg) != NERFHIP_OK || n < 0) return -1;
    int64_t b = nh_point_grad_tmp_bytes(pc, n * cfg->num_coarse);
    if (cfg->num_fine > 0) {
        const int64_t f = nh_point_grad_tmp_bytes(pf, n * (cfg->num_coarse + cfg->num_fine));
        if (f > b) b = f;
    }
    return b;
}

// nerfhip_render_bwd_rays for frozen nets: d(loss)/d(rays) alone -- no parameter gradient is computed, stored or applied
extern "C" int nerfhip_render_grad_rays(nerfhip_plan_t pc, nerfhip_plan_t pf, const nerfhip_render_cfg* cfg, const float* rays,
                                        int64_t n, const float* packed_c, const float* packed_f, const nerfhip_render_rand* rnd,
                                        uint64_t seed, uint64_t ray_offset, const nerfhip_render_cotangents* g, void* workspace,
                                        int64_t workspace_bytes, int parts, const float* params_c, const float* params_f, void* tmp,
                                        int64_t tmp_bytes, float* g_rays, nerfhip_stream_t stream) {
    int rc = check_cfg(pc, pf, cfg);
    if (rc) return rc;
    NH_REQUIRE(n >= 0, "render_grad_rays: bad arguments");
    if (n == 0) return NERFHIP_OK;
    NH_REQUIRE(rays && packed_c && g && workspace, "render_grad_rays: bad arguments");
    NH_REQUIRE(g_rays, "render_grad_rays: g_rays is NULL");
    NH_REQUIRE(tmp, "render_grad_rays: tmp is NULL");
    const int shared = parts & NERFHIP_PART_SHARED_BWD;
    parts &= ~NERFHIP_PART_SHARED_BWD;
    NH_REQUIRE(parts >= 1 && parts <= 3, "render_grad_rays: parts must be a combination of NERFHIP_PART_COARSE | NERFHIP_PART_FINE");
    const bool fine_runs = cfg->num_fine > 0 && (parts & NERFHIP_PART_FINE), coarse_runs = (parts & NERFHIP_PART_COARSE) != 0;
    NH_REQUIRE((!coarse_runs || params_c) && (!fine_runs || params_f), "render_grad_rays: the flat parameters (params) are NULL");
    NH_REQUIRE((!coarse_runs || nh_prec_level(pc->precision) != 1) && (!fine_runs || nh_prec_level(pf->precision) != 1),
               "render_grad_rays: an f16x3 plan is inference-only");
    const Workspace w = layout(pc, pf, cfg, n, shared ? 2 : 1);
    NH_REQUIRE(workspace_bytes >= w.total, "render_grad_rays: workspace too small (%lld < %lld)", (long long)workspace_bytes,
               (long long)w.total);
    const Call c = {cfg, rays, n, seed, ray_offset, (char*)workspace, stream};
    int wrote_rays = 0;  // the first pass that runs overwrites g_rays, the second accumulates
    if (fine_runs) {
        NH_REQUIRE(packed_f && (g->g_rgb_fine || g->g_acc_fine || g->g_depth_fine), "render_grad_rays: fine arguments missing");
        Pass fine = net_pass(c, true, pf, packed_f, rnd, w);
        fine.g_rgb = g->g_rgb_fine, fine.g_depth = g->g_depth_fine, fine.g_acc = g->g_acc_fine;
        fine.params = params_f;
        rc = grad_rays_pass(c, fine, tmp, tmp_bytes, g_rays, wrote_rays);
        if (rc) return rc;
        wrote_rays = 1;
    }
    if (coarse_runs) {
        NH_REQUIRE(g->g_rgb_coarse || g->g_acc_coarse || g->g_depth_coarse, "render_grad_rays: coarse arguments missing");
        Pass coarse = net_pass(c, false, pc, packed_c, rnd, w);
        coarse.g_rgb = g->g_rgb_coarse, coarse.g_depth = g->g_depth_coarse, coarse.g_acc = g->g_acc_coarse;
        coarse.params = params_c;
        rc = grad_rays_pass(c, coarse, tmp, tmp_bytes, g_rays, wrote_rays);
        if (rc) return rc;
    }
    return NERFHIP_OK;
}
