// dataio.hip -- the stages either side of the render path:
//   * training-ray selection: draw N distinct pixels, generate ONLY those rays, pack them, gather their target
//     colours (train_nerf.py:210-227, cached branch :175-194) -- one launch instead of a host permutation of the
//     whole image, a full-image get_ray_bundle and three fancy-index gathers;
//   * its backward to the pose (pose refinement): d(loss)/d(rays) -> d(loss)/d(c2w[:3, :4]), a fixed-order reduction;
//   * both over a stack of views (one batch spread over V images and V poses; one gradient per pose, each reduced in the
//     single-view order over its own rays): the selection is ONE kernel for one image, a stack of views and the cached bundle,
//     and both forms of the backward end in ONE sum kernel;
//   * the camera table: one se(3) twist per view composed onto a base pose, and its VJP (the parametrisation pose refinement steps);
//   * 8-bit output: cast_to_image / cast_to_disparity_image (eval_nerf.py:23-36).
// Everything here is HBM/latency-bound byte and index work: one thread per ray / pixel, coalesced rows.
#include "nh_host.h"
#include "nh_rays.h"

// ---- keyed permutation of [0, population) ----------------------------------------------------------------------------
// The reference draws np.random.choice(population, N, replace=False): a uniformly random N-subset in random order.
// Here: positions first..first+n-1 of a keyed pseudo-random permutation of [0, population) -- a 6-round balanced
// Feistel network over the smallest even number of bits covering the population, cycle-walked back into range
// (a bijection by construction, so the indices are distinct; ranks take disjoint position ranges of the SAME
// permutation).  Round keys: Philox4x32-10 of (seed, step), streams 4 and 5.
struct NhPerm {
    uint32_t k[6];
    uint32_t half, mask;
    uint64_t population;
};
NH_DEVICE NhPerm nh_perm_key(uint64_t seed, uint64_t step, uint64_t population) {
    NhPerm p;
    nh_u4 a = nh_philox(seed, step, 4u);
    nh_u4 b = nh_philox(seed, step, 5u);
    p.k[0] = a.x, p.k[1] = a.y, p.k[2] = a.z, p.k[3] = a.w, p.k[4] = b.x, p.k[5] = b.y;
    uint32_t bits = 2;
    while (bits < 64 && ((uint64_t)1 << bits) < population) bits += 2;
    p.half = bits / 2;
    p.mask = (uint32_t)(((uint64_t)1 << p.half) - 1);
    p.population = population;
    return p;
}
NH_DEVICE uint64_t nh_perm_at(const NhPerm& p, uint64_t x) {
    do {
        uint32_t l = (uint32_t)(x >> p.half), r = (uint32_t)x & p.mask;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            uint32_t h = r ^ p.k[i];
            h *= 0x85EBCA6Bu;
            h ^= h >> 13;
            h *= 0xC2B2AE35u;
            h ^= h >> 16;
            uint32_t t = l ^ (h & p.mask);
            l = r;
            r = t;
        }
        x = ((uint64_t)l << p.half) | r;
    } while (x >= p.population);
    return x;
}

NH_KERNEL void k_select_indices(uint64_t seed, uint64_t step, uint64_t population, int64_t first, int64_t n,
                                int64_t* __restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    NhPerm p = nh_perm_key(seed, step, population);
    out[i] = (int64_t)nh_perm_at(p, (uint64_t)(first + i));
}

extern "C" int nerfhip_select_indices(uint64_t seed, uint64_t step, int64_t population, int64_t first, int64_t n,
                                      int64_t* out, nerfhip_stream_t stream) {
    NH_REQUIRE(n >= 0 && first >= 0 && population >= 0 && population <= ((int64_t)1 << 32) && (n == 0 || out),
               "select_indices: bad arguments");
    NH_REQUIRE(first + n <= population, "select_indices: first + n exceeds the population (sampling is without replacement)");
    if (n == 0) return NERFHIP_OK;
    NH_LAUNCH(k_select_indices, nh_ceil_div(n, 256), 256, 0, stream, seed, step, (uint64_t)population, first, n, out);
    return nh_launch_status("select_indices");
}

// ---- fused selection -> rays -> packed rows + target gather ----------------------------------------------------------
// poses != NULL: image branch (rays generated for the selected pixels only) over a stack of num_views views; else cached
// branch (rows of the stored ray bundle).  The rest is run_one_iter_of_nerf's prologue (train_utils.py:143-168): viewdirs
// from the pre-NDC directions, optional ndc_rays with near = 1.0, [o d near far viewdirs] rows.
// Image branch, population V * H * W: global index g = v * (H * W) + k addresses view v and the reference's flat select index
// k of that view.  Pose of view v: poses + v * view_stride, row stride ld; image of view v: targets + v * H * W * channels.
// Intrinsics, near / far, NDC and viewdirs are shared by all views.  One view (nerfhip_select_rays; the views entry point
// at V = 1): g is k itself, nothing is divided out.  intr (device, fx fy cx cy; nerfhip_select_rays_views_intr) replaces the
// camera of (s.height, s.width, s.focal) in the pin-hole direction -- and nowhere else: the NDC constants stay ndc's.  dist (device,
// k1 k2 p1 p2; nerfhip_select_rays_views_dist) undistorts that direction (nh_undistort); NULL skips the solve.
NH_KERNEL void k_select_rays(nerfhip_select_cfg s, NhNdc ndc, const float* __restrict__ intr, const float* __restrict__ dist,
                             const float* __restrict__ poses, int64_t view_stride, int ld, int num_views,
                             const float* __restrict__ cached_o, const float* __restrict__ cached_d,
                             const float* __restrict__ targets, uint64_t population,
                             const int64_t* __restrict__ inds_in, int64_t n, float* __restrict__ rays,
                             float* __restrict__ target_out, int64_t* __restrict__ inds_out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t k;
    if (inds_in) {
        k = inds_in[i];
    } else {
        NhPerm p = nh_perm_key(s.seed, s.step, population);
        k = (int64_t)nh_perm_at(p, (uint64_t)(s.first + i));
    }
    if (inds_out) inds_out[i] = k;
    float o[3], d[3], v[3];
    int64_t pix;  // position of the target pixel: row-major, view by view
    if (poses) {
        int64_t view = 0, base = 0;
        if (num_views > 1) {
            const int64_t hw = (int64_t)s.height * s.width;
            view = k / hw, base = view * hw;
            k -= base;
        }
        // coords = stack(meshgrid_xy(arange(H), arange(W)), -1).reshape(-1, 2): entry k is (k % H, k / H), used as
        // (row, col) -- train_nerf.py:214-225
        int64_t row = k % s.height, col = k / s.height;
        float f[4];
        nh_intrinsics(intr, s.height, s.width, s.focal, f);
        nh_camera_ray(f, dist, poses + view * view_stride, ld, row, col, o, d);
        pix = base + row * s.width + col;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[c] = cached_o[k * 3 + c];
            d[c] = cached_d[k * 3 + c];
        }
        pix = k;
    }
    v[0] = d[0], v[1] = d[1], v[2] = d[2];
    if (s.ndc) nh_ndc_ray(ndc, o, d);
    nh_write_ray_row(rays + i * (s.use_viewdirs ? 11 : 8), o, d, s.near, s.far, s.use_viewdirs ? v : nullptr);
    if (targets) {
        for (int c = 0; c < s.channels; ++c) target_out[i * s.channels + c] = targets[pix * s.channels + c];
    }
}

static NhNdc ndc_of(const nerfhip_select_cfg* cfg) {
    return NhNdc{cfg->ndc_near, cfg->ndc_cw, cfg->ndc_ch, cfg->ndc_two_near, cfg->ndc_neg_two_near};
}

// the checks and the launch of the three selection entry points (`what`: the entry point, for the messages)
static int select_launch(const char* what, const nerfhip_select_cfg* cfg, const float* intr, const float* dist, int num_views,
                         const float* poses, int64_t view_stride, int ld, const float* co, const float* cd, const float* targets,
                         int64_t population, const int64_t* inds, int64_t n, float* rays, float* target_out, int64_t* inds_out,
                         nerfhip_stream_t stream) {
    NH_REQUIRE(cfg && n >= 0 && (n == 0 || rays), "%s: bad arguments", what);
    NH_REQUIRE(!targets || (target_out && cfg->channels >= 1 && cfg->channels <= 4), "%s: bad target arguments", what);
    NH_REQUIRE(population >= 0 && population <= ((int64_t)1 << 32), "%s: bad population", what);
    NH_REQUIRE(inds || (cfg->first >= 0 && cfg->first + n <= population),
               "%s: first + n exceeds the population (sampling is without replacement)", what);
    if (n == 0) return NERFHIP_OK;
    NH_LAUNCH(k_select_rays, nh_ceil_div(n, 256), 256, 0, stream, *cfg, ndc_of(cfg), intr, dist, poses, view_stride, ld, num_views, co,
              cd, targets, (uint64_t)population, inds, n, rays, target_out, inds_out);
    return nh_launch_status(what);
}

// the layout of a table of num_views poses (`name`: "pose" or "base", the parameters' prefix, for the messages)
static int table_check(int num_views, int64_t view_stride, int ld, const char* name, const char* what) {
    NH_REQUIRE(num_views >= 1 && num_views <= NERFHIP_MAX_VIEWS, "%s: num_views must be 1 .. %d (got %d)", what, NERFHIP_MAX_VIEWS,
               num_views);
    NH_REQUIRE(ld >= 4, "%s: %s_ld must be >= 4 (got %d)", what, name, ld);
    NH_REQUIRE(num_views == 1 || view_stride >= 2 * (int64_t)ld + 4,
               "%s: %s_view_stride %lld cannot hold the 3 rows of a pose at row stride %d", what, name, (long long)view_stride, ld);
    return NERFHIP_OK;
}

// what both views entry points ask of the pose table
static int views_check(const nerfhip_select_cfg* cfg, int num_views, const float* poses, int64_t view_stride, int ld,
                       const char* what) {
    NH_REQUIRE(cfg && poses && cfg->height > 0 && cfg->width > 0, "%s: bad arguments", what);
    int rc = table_check(num_views, view_stride, ld, "pose", what);
    if (rc) return rc;
    NH_REQUIRE((int64_t)num_views * cfg->height * cfg->width <= ((int64_t)1 << 32), "%s: num_views * height * width exceeds 2^32", what);
    return NERFHIP_OK;
}

extern "C" int nerfhip_select_rays(const nerfhip_select_cfg* cfg, const float* c2w, int c2w_ld, const float* image,
                                   const int64_t* select_inds, int64_t n, float* rays, float* target,
                                   int64_t* inds_out, nerfhip_stream_t stream) {
    NH_REQUIRE(cfg && c2w && c2w_ld >= 4 && cfg->height > 0 && cfg->width > 0, "select_rays: bad arguments");
    return select_launch("select_rays", cfg, nullptr, nullptr, 1, c2w, 0, c2w_ld, nullptr, nullptr, image,
                         (int64_t)cfg->height * cfg->width, select_inds, n, rays, target, inds_out, stream);
}

extern "C" int nerfhip_select_cached_rays(const nerfhip_select_cfg* cfg, const float* ray_origins,
                                          const float* ray_directions, const float* targets, int64_t population,
                                          const int64_t* select_inds, int64_t n, float* rays, float* target,
                                          int64_t* inds_out, nerfhip_stream_t stream) {
    NH_REQUIRE(cfg && ray_origins && ray_directions, "select_cached_rays: bad arguments");
    return select_launch("select_cached_rays", cfg, nullptr, nullptr, 0, nullptr, 0, 0, ray_origins, ray_directions, targets,
                         population, select_inds, n, rays, target, inds_out, stream);
}

extern "C" int nerfhip_select_rays_views(const nerfhip_select_cfg* cfg, int num_views, const float* poses,
                                         int64_t pose_view_stride, int pose_ld, const float* images, const int64_t* select_inds,
                                         int64_t n, float* rays, float* target, int64_t* inds_out, nerfhip_stream_t stream) {
    int rc = views_check(cfg, num_views, poses, pose_view_stride, pose_ld, "select_rays_views");
    if (rc) return rc;
    return select_launch("select_rays_views", cfg, nullptr, nullptr, num_views, poses, pose_view_stride, pose_ld, nullptr, nullptr,
                         images, (int64_t)num_views * cfg->height * cfg->width, select_inds, n, rays, target, inds_out, stream);
}

extern "C" int nerfhip_select_rays_views_intr(const nerfhip_select_cfg* cfg, const float* intr, int num_views, const float* poses,
                                              int64_t pose_view_stride, int pose_ld, const float* images,
                                              const int64_t* select_inds, int64_t n, float* rays, float* target, int64_t* inds_out,
                                              nerfhip_stream_t stream) {
    const char* what = "select_rays_views_intr";
    NH_REQUIRE(intr, "%s: intr must not be NULL", what);
    int rc = views_check(cfg, num_views, poses, pose_view_stride, pose_ld, what);
    if (rc) return rc;
    return select_launch(what, cfg, intr, nullptr, num_views, poses, pose_view_stride, pose_ld, nullptr, nullptr, images,
                         (int64_t)num_views * cfg->height * cfg->width, select_inds, n, rays, target, inds_out, stream);
}

extern "C" int nerfhip_select_rays_views_dist(const nerfhip_select_cfg* cfg, const float* intr, const float* dist, int num_views,
                                              const float* poses, int64_t pose_view_stride, int pose_ld, const float* images,
                                              const int64_t* select_inds, int64_t n, float* rays, float* target, int64_t* inds_out,
                                              nerfhip_stream_t stream) {
    const char* what = "select_rays_views_dist";
    NH_REQUIRE(dist, "%s: dist must not be NULL", what);
    int rc = views_check(cfg, num_views, poses, pose_view_stride, pose_ld, what);
    if (rc) return rc;
    return select_launch(what, cfg, intr, dist, num_views, poses, pose_view_stride, pose_ld, nullptr, nullptr, images,
                         (int64_t)num_views * cfg->height * cfg->width, select_inds, n, rays, target, inds_out, stream);
}

// ---- pose VJP: d(loss)/d(c2w[:3, :4]) from d(loss)/d(rays) (what autograd gives the reference's pose) --------------------
// get_ray_bundle is linear in the pose: d = c2w[:3, :3] dc, o = c2w[:3, 3] (nh_pinhole_ray), so ray r contributes
// g_c2w[c][k] += g_d[c] dc[k] (k < 3) and g_c2w[c][3] += g_o[c].  The select form first runs the packing and NDC backward of
// the ray's row in registers (viewdir normalisation, nh_ndc_ray_vjp), recomputing the pre-NDC ray from the pose.
// Reduction without atomics, in an order that depends on n only (bit-reproducible run to run and machine to machine):
// k_pose_vjp_part -- G(n) = min(ceil(n / 256), 1024) workgroups of 256 threads; thread t of workgroup b sums rays
// i = b * 256 + t + q * 256 G (q = 0, 1, ...) in q order, each wave combines its lanes by an xor butterfly, lane 0 of each wave
// hands its 12 sums to LDS and the workgroup's sums of its 4 waves (in wave order) go to tmp[b][12]; k_pose_vjp_sum -- one
// workgroup (per view: the views form below runs the same kernel), wave j sums tmp[p][j] over p = lane, lane + 64, ... in p order,
// then an xor butterfly.
namespace {

constexpr int PV_THREADS = 256, PV_MAX_WGS = 1024;

// G(n) (constexpr: for the host and for the kernels)
constexpr int64_t pv_wgs(int64_t n) {
    return n <= 0 ? 0 : ((n + PV_THREADS - 1) / PV_THREADS < PV_MAX_WGS ? (n + PV_THREADS - 1) / PV_THREADS : PV_MAX_WGS);
}

struct PoseVjpArgs {
    nerfhip_select_cfg s;
    NhNdc ndc;
    const float* intr;        // select form: the device intrinsics (fx fy cx cy), or NULL: the camera of (s.height, s.width, s.focal)
    const float* dist;        // select form: the device distortion coefficients (k1 k2 p1 p2), or NULL: the pin-hole camera
    int select;               // 1: select form (row k % height, col k / height; packing / NDC backward); 0: bundle form
    const float* c2w;         // select form only (the pre-NDC ray)
    int ld;
    const int64_t* inds;      // select indices / linear pixel ids (row * width + col), or NULL: ray i is pixel i
    int64_t n;
    const float* g_a;         // select form: d(loss)/d(rays) rows; bundle form: d(loss)/d(origins) [n, 3] or NULL
    const float* g_b;         // select form: a second set of rows, added (may be NULL); bundle form: d/d(directions) or NULL
    int g_stride;
    float* tmp;               // [G][12] workgroup partials
};

PoseVjpArgs select_vjp_args(const nerfhip_select_cfg* cfg, const float* c2w, int ld, const int64_t* inds, int64_t n,
                            const float* g_rays, const float* g_rays_2, int g_rays_stride, void* tmp) {
    PoseVjpArgs a;
    memset(&a, 0, sizeof(a));
    a.s = *cfg, a.ndc = ndc_of(cfg);
    a.select = 1, a.c2w = c2w, a.ld = ld, a.inds = inds, a.n = n, a.g_a = g_rays, a.g_b = g_rays_2;
    a.g_stride = g_rays_stride, a.tmp = (float*)tmp;
    return a;
}

// this ray's camera direction dc under the intrinsics f (undistorted under a.dist), and the cotangents go / gd of its pre-NDC
// origin / direction (ray i of the batch, k: its select index / linear pixel id)
// c2w: the ray's pose (select form only)
NH_DEVICE void pose_vjp_ray_cot(const PoseVjpArgs& a, const float* f, const float* __restrict__ c2w, int64_t i, int64_t k, float* dc,
                                float* go, float* gd) {
    int64_t row, col;
    if (a.select) {
        row = k % a.s.height, col = k / a.s.height;  // (k_select_rays)
    } else {
        row = k / a.s.width, col = k % a.s.width;    // (k_ray_bundle)
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) go[c] = 0.f, gd[c] = 0.f;
    nh_camera_dir(f, a.dist, row, col, dc);
    if (a.select) {
        const float* ga = a.g_a + i * a.g_stride;
        const float* gb = a.g_b ? a.g_b + i * a.g_stride : nullptr;
        float gr[11];
        const int cols = a.s.use_viewdirs ? 11 : 8;
        for (int c = 0; c < cols; ++c) gr[c] = gb ? ga[c] + gb[c] : ga[c];  // (columns 6, 7: near / far carry no gradient)
        float o[3], d[3];
        nh_rotate_ray(dc, c2w, a.ld, o, d);
        if (a.s.ndc) {
            nh_ndc_ray_vjp(a.ndc, o, d, gr, gr + 3, go, gd);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) go[c] = gr[c], gd[c] = gr[3 + c];
        }
        if (a.s.use_viewdirs) {  // v / ||v|| of the pre-NDC direction (nh_write_ray_row): (g_v - u (u . g_v)) / ||v||, u = v / ||v||
            const float nrm = sqrtf(fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0])));
            const float u0 = d[0] / nrm, u1 = d[1] / nrm, u2 = d[2] / nrm;
            const float dot = u0 * gr[8] + u1 * gr[9] + u2 * gr[10];
            gd[0] = gd[0] + (gr[8] - u0 * dot) / nrm;
            gd[1] = gd[1] + (gr[9] - u1 * dot) / nrm;
            gd[2] = gd[2] + (gr[10] - u2 * dot) / nrm;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (a.g_a) go[c] = a.g_a[i * 3 + c];
            if (a.g_b) gd[c] = a.g_b[i * 3 + c];
        }
    }
}
// this ray's 12 terms: t[c * 4 + k] = g_d[c] dc[k] (k < 3), t[c * 4 + 3] = g_o[c]
NH_DEVICE void pose_vjp_ray_at(const PoseVjpArgs& a, int64_t i, int64_t k, float* t) {
    float f[4], dc[3], go[3], gd[3];
    nh_intrinsics(a.intr, a.s.height, a.s.width, a.s.focal, f);
    pose_vjp_ray_cot(a, f, a.c2w, i, k, dc, go, gd);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        t[c * 4 + 0] = gd[c] * dc[0];
        t[c * 4 + 1] = gd[c] * dc[1];
        t[c * 4 + 2] = gd[c] * dc[2];
        t[c * 4 + 3] = go[c];
    }
}
NH_DEVICE void pose_vjp_ray(const PoseVjpArgs& a, int64_t i, float* t) { pose_vjp_ray_at(a, i, a.inds ? a.inds[i] : i, t); }

// the NS sums of a workgroup from its threads' sums: xor butterfly per wave, then the 4 waves in wave order -> dst[NS]
// (NS = 12: a pose; NS = 4: the intrinsics)
template <int NS>
NH_DEVICE void pv_block_sum(float* acc, float (*s_part)[NS], float* dst) {
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j] = nh_wave_sum(acc[j]);
    const int wave = nh_wave_in_block();
    if (nh_lane() == 0) {
#pragma unroll
        for (int j = 0; j < NS; ++j) s_part[wave][j] = acc[j];
    }
    nh_block_sync();
    if (threadIdx.x < NS) {
        float v = s_part[0][threadIdx.x];
        for (int w = 1; w < PV_THREADS / 64; ++w) v += s_part[w][threadIdx.x];
        dst[threadIdx.x] = v;
    }
}

NH_KERNEL void k_pose_vjp_part(PoseVjpArgs a) {
    NH_SHARED float s_part[PV_THREADS / 64][12];
    float acc[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[j] = 0.0f;
    const int64_t step = (int64_t)gridDim.x * PV_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * PV_THREADS + threadIdx.x; i < a.n; i += step) {
        float t[12];
        pose_vjp_ray(a, i, t);
#pragma unroll
        for (int j = 0; j < 12; ++j) acc[j] += t[j];
    }
    pv_block_sum<12>(acc, s_part, a.tmp + (int64_t)blockIdx.x * 12);
}

// workgroup `view` (NS waves) sums its partials part[slot0 .. slot0 + wgs - 1][NS] into g[view][NS].  Single view (cnt == NULL): one
// workgroup, the first `wgs` partials.  Views: the G(cnt[view]) partials from slot off[view] / 256 + view (k_pose_views_part).
// (profile names: the pose instantiation keeps "k_pose_vjp_sum", the one the existing records and scripts filter on; <4> is "k_intr_vjp_sum")
template <int NS>
NH_KERNEL void k_pose_vjp_sum(const float* __restrict__ part, int wgs, const int* __restrict__ cnt, const int* __restrict__ off,
                              float* __restrict__ g) {
    const int j = nh_wave_in_block(), lane = nh_lane(), view = (int)blockIdx.x;
    int64_t slot0 = 0;
    if (cnt) wgs = (int)pv_wgs(cnt[view]), slot0 = off[view] / PV_THREADS + view;
    float v = 0.0f;
    for (int q = lane; q < wgs; q += 64) v += part[(slot0 + q) * NS + j];
    v = nh_wave_sum(v);
    if (lane == 0) g[(int64_t)view * NS + j] = v;
}

int pose_vjp_launch(const PoseVjpArgs& a, int64_t tmp_bytes, float* g_c2w, nerfhip_stream_t stream, const char* what) {
    const int64_t wgs = pv_wgs(a.n);
    NH_REQUIRE(tmp_bytes >= wgs * 12 * (int64_t)sizeof(float) && (wgs == 0 || a.tmp),
               "%s: tmp must hold nerfhip_pose_grad_tmp_bytes(n) = %lld bytes", what, (long long)(wgs * 12 * sizeof(float)));
    if (wgs > 0) {
        NH_LAUNCH(k_pose_vjp_part, wgs, PV_THREADS, 0, stream, a);
        int rc = nh_launch_status(what);
        if (rc) return rc;
    }
    NH_LAUNCH_NAMED("k_pose_vjp_sum", k_pose_vjp_sum<12>, 1, 12 * 64, 0, stream, (const float*)a.tmp, (int)wgs, (const int*)nullptr, (const int*)nullptr,
              g_c2w);  // (n == 0: zeros)
    return nh_launch_status(what);
}

// ---- the pose VJP over a stack of views -----------------------------------------------------------------------------------
// g_poses[v] = the single-view result for pose v on the rays of view v alone, in ascending batch position -- bit for bit: the n_v
// rays of a view are ranked (a stable counting sort of the batch by view) and then summed along the single-view tree with n = n_v.
// Three launches whose grids depend on (n, V) only; integer bookkeeping only between them; no atomics:
//   k_pose_views_group -- workgroup v: off[v] = rays of views < v, cnt[v] = n_v (one scan of the n indices; view membership is two
//       compares against v H W, no division), then a second scan ranks view v's rays in batch order (prefix sums over the wave and
//       the 4 waves, PVG_PER consecutive rays per thread) and writes their batch positions to list[off[v] + rank];
//   k_pose_views_part -- floor(n / 256) + V workgroups; view v owns the slots slot0(v) = off[v] / 256 + v ... + G(n_v) - 1 (disjoint:
//       G(n_v) <= ceil(n_v / 256) <= floor((off[v] + n_v) / 256) - floor(off[v] / 256) + 1); workgroup w finds its (v, b) by bisection
//       over slot0, and is partial b of view v: k_pose_vjp_part's loop and sums over list positions b 256 + t + q 256 G(n_v);
//   k_pose_vjp_sum -- V workgroups: workgroup v sums view v's G(n_v) partials (none: exact zeros).
constexpr int PVG_PER = 4;

struct PoseViewsArgs {
    PoseVjpArgs a;        // c2w: the pose table; inds: GLOBAL indices v H W + k; tmp: the slots' partials [floor(n / 256) + V][12]
    int num_views;
    int64_t view_stride, hw;
    int *cnt, *off, *list;  // [V], [V], [n]
};

NH_DEVICE int wave_sum_i(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += nh_shfl_xor_i(v, m);
    return v;
}

NH_KERNEL void k_pose_views_group(PoseViewsArgs p) {
    NH_SHARED int s_less[PV_THREADS / 64], s_eq[PV_THREADS / 64], s_tot[PV_THREADS / 64];
    const int lane = nh_lane(), wave = nh_wave_in_block();
    const int n = (int)p.a.n;
    const int64_t lo = (int64_t)blockIdx.x * p.hw, hi = lo + p.hw;
    int less = 0, eq = 0;
    for (int i = (int)threadIdx.x; i < n; i += PV_THREADS) {
        const int64_t g = p.a.inds[i];
        less += g < lo ? 1 : 0;
        eq += (g >= lo && g < hi) ? 1 : 0;
    }
    less = wave_sum_i(less), eq = wave_sum_i(eq);
    if (lane == 0) s_less[wave] = less, s_eq[wave] = eq;
    nh_block_sync();
    int off = 0, cnt = 0;
    for (int w = 0; w < PV_THREADS / 64; ++w) off += s_less[w], cnt += s_eq[w];
    if (threadIdx.x == 0) p.off[blockIdx.x] = off, p.cnt[blockIdx.x] = cnt;
    // ranks in batch order: chunks of 256 * PVG_PER rays, thread t holds PVG_PER consecutive ones
    int done = 0;
    for (int base = 0; base < n && done < cnt; base += PV_THREADS * PVG_PER) {
        const int i0 = base + (int)threadIdx.x * PVG_PER;
        int flags = 0, c = 0;
#pragma unroll
        for (int e = 0; e < PVG_PER; ++e) {
            if (i0 + e < n) {
                const int64_t g = p.a.inds[i0 + e];
                if (g >= lo && g < hi) flags |= 1 << e, ++c;
            }
        }
        int incl = c;  // inclusive prefix sum of c over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = nh_shfl_i(incl, lane - d < 0 ? 0 : lane - d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_tot[wave] = incl;
        nh_block_sync();
        int r = off + done + incl - c, total = 0;
        for (int w = 0; w < PV_THREADS / 64; ++w) {
            if (w < wave) r += s_tot[w];
            total += s_tot[w];
        }
#pragma unroll
        for (int e = 0; e < PVG_PER; ++e)
            if (flags & (1 << e)) p.list[r++] = i0 + e;
        done += total;
        nh_block_sync();  // (s_tot is rewritten by the next chunk)
    }
}

NH_KERNEL void k_pose_views_part(PoseViewsArgs p) {
    NH_SHARED float s_part[PV_THREADS / 64][12];
    const int w = (int)blockIdx.x;
    int v = 0, top = p.num_views - 1;  // the last view whose first slot is <= w (slot0 is strictly increasing, slot0(0) = 0)
    while (v < top) {
        const int mid = (v + top + 1) >> 1;
        if (p.off[mid] / PV_THREADS + mid <= w)
            v = mid;
        else
            top = mid - 1;
    }
    const int off = p.off[v], nv = p.cnt[v];
    const int b = w - (off / PV_THREADS + v), wgs = (int)pv_wgs(nv);
    if (b >= wgs) return;  // (a slot no view uses; the whole workgroup leaves)
    PoseVjpArgs a = p.a;
    a.c2w = p.a.c2w + (int64_t)v * p.view_stride;
    const int64_t g0 = (int64_t)v * p.hw;
    float acc[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[j] = 0.0f;
    const int step = wgs * PV_THREADS;
    for (int r = b * PV_THREADS + (int)threadIdx.x; r < nv; r += step) {
        const int64_t i = p.list[off + r];
        float t[12];
        pose_vjp_ray_at(a, i, a.inds[i] - g0, t);
#pragma unroll
        for (int j = 0; j < 12; ++j) acc[j] += t[j];
    }
    pv_block_sum<12>(acc, s_part, p.a.tmp + (int64_t)w * 12);
}

int64_t pv_views_words(int64_t n, int num_views, int64_t* slots) {
    *slots = n / PV_THREADS + num_views;
    return *slots * 12 + 2 * (int64_t)num_views + n;
}

// ---- the VJP w.r.t. the shared intrinsics (fx, fy, cx, cy) -------------------------------------------------------------------------
// dc = ((col - cx) / fx, -(row - cy) / fy, -1) and d = R dc: with g_dc[k] = sum_c g_d[c] R[c][k] (g_d: pose_vjp_ray_cot's, the cotangent
// of the pre-NDC direction), ray i contributes
//     g_fx += -g_dc[0] dc[0] / fx,   g_fy += -g_dc[1] dc[1] / fy,   g_cx += -g_dc[0] / fx,   g_cy += g_dc[1] / fy.
// The intrinsics enter through the pin-hole direction only: the NDC constants are those of cfg and carry no gradient.  The intrinsics
// are shared by the views, so this is ONE sum over all n rays in batch order -- the single-view tree above (k_pose_vjp_part's loop,
// pv_block_sum<4>, k_pose_vjp_sum<4>) with four sums in place of twelve; each ray reads the pose of its own view, inds[i] / (H W).  No
// grouping, no atomics: the order depends on n only.  An index outside [0, V H W) contributes nothing (as it belongs to no view above).
// Under lens distortion (p.a.dist) dc is the undistorted direction and the four terms come from nh_undistort_vjp; dist = 0 gives the
// pin-hole terms' bits.
// ray i's camera direction dc and the cotangent of its x and y, g_dc = R^T g_d; false: the index belongs to no view (dropped)
NH_DEVICE bool intr_vjp_ray_gdc(const PoseViewsArgs& p, const float* f, int64_t population, int64_t i, int64_t* row, int64_t* col,
                                float* dc, float* gdc) {
    const int64_t g = p.a.inds[i];
    if (g < 0 || g >= population) return false;
    const int64_t view = p.num_views > 1 ? g / p.hw : 0;
    const float* __restrict__ c2w = p.a.c2w + view * p.view_stride;
    const int64_t k = g - view * p.hw;
    *row = k % p.a.s.height, *col = k / p.a.s.height;
    float go[3], gd[3];
    pose_vjp_ray_cot(p.a, f, c2w, i, k, dc, go, gd);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        float v = gd[0] * c2w[j];
        v = v + gd[1] * c2w[p.a.ld + j];
        v = v + gd[2] * c2w[2 * p.a.ld + j];
        gdc[j] = v;
    }
    return true;
}
// ray i's terms under distortion (nh_undistort_vjp at the ray's solution): those of the coefficients and / or of the intrinsics
NH_DEVICE void dist_vjp_ray_terms(const float* f, const float* kp, int64_t row, int64_t col, const float* dc,
                                  const float* gdc, float* t_dist, float* t_intr) {
    float pin[3];
    nh_pinhole_cam(f[0], f[1], f[2], f[3], row, col, pin);  // the observed point (xd, yd) = (pin[0], -pin[1])
    nh_undistort_vjp(kp, f, dc[0], -dc[1], pin[0], -pin[1], gdc[0], -gdc[1], t_dist, t_intr);
}

NH_KERNEL void k_intr_vjp_part(PoseViewsArgs p, float* __restrict__ part) {
    NH_SHARED float s_part[PV_THREADS / 64][4];
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, f[4], kp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    nh_intrinsics(p.a.intr, p.a.s.height, p.a.s.width, p.a.s.focal, f);
    if (p.a.dist) kp[0] = p.a.dist[0], kp[1] = p.a.dist[1], kp[2] = p.a.dist[2], kp[3] = p.a.dist[3];
    const int64_t population = (int64_t)p.num_views * p.hw;
    const int64_t step = (int64_t)gridDim.x * PV_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * PV_THREADS + threadIdx.x; i < p.a.n; i += step) {
        int64_t row, col;
        float dc[3], gdc[2];
        if (!intr_vjp_ray_gdc(p, f, population, i, &row, &col, dc, gdc)) continue;
        if (p.a.dist) {
            float t[4];
            dist_vjp_ray_terms(f, kp, row, col, dc, gdc, nullptr, t);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += t[j];
        } else {
            acc[0] += -(gdc[0] * dc[0]) / f[0];
            acc[1] += -(gdc[1] * dc[1]) / f[1];
            acc[2] += -gdc[0] / f[0];
            acc[3] += gdc[1] / f[1];
        }
    }
    pv_block_sum<4>(acc, s_part, part + (int64_t)blockIdx.x * 4);
}

// ---- the VJP w.r.t. the shared distortion coefficients (k1, k2, p1, p2) -------------------------------------------------------------
// The same ONE sum over all n rays in batch order along the single-view tree, with nh_undistort_vjp's four coefficient terms.  mask
// (device, one byte per coefficient, or NULL = all): a masked entry's partial is an exact zero in every workgroup, so its sum is one.
NH_KERNEL void k_dist_vjp_part(PoseViewsArgs p, const unsigned char* __restrict__ mask, float* __restrict__ part) {
    NH_SHARED float s_part[PV_THREADS / 64][4];
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, f[4];
    nh_intrinsics(p.a.intr, p.a.s.height, p.a.s.width, p.a.s.focal, f);
    const float kp[4] = {p.a.dist[0], p.a.dist[1], p.a.dist[2], p.a.dist[3]};
    const int64_t population = (int64_t)p.num_views * p.hw;
    const int64_t step = (int64_t)gridDim.x * PV_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * PV_THREADS + threadIdx.x; i < p.a.n; i += step) {
        int64_t row, col;
        float dc[3], gdc[2], t[4];
        if (!intr_vjp_ray_gdc(p, f, population, i, &row, &col, dc, gdc)) continue;
        dist_vjp_ray_terms(f, kp, row, col, dc, gdc, t, nullptr);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += t[j];
    }
    if (mask) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (!mask[j]) acc[j] = 0.0f;
    }
    pv_block_sum<4>(acc, s_part, part + (int64_t)blockIdx.x * 4);
}

// every form of the views VJP: g_poses (the three launches above), g_intr (two launches) and / or g_dist (two launches); intr == NULL:
// cfg's camera; dist == NULL: no lens distortion (then g_dist is NULL too)
int views_bwd(const char* what, const nerfhip_select_cfg* cfg, const float* intr, const float* dist, int num_views, const float* poses,
              int64_t pose_view_stride, int pose_ld, const int64_t* inds, int64_t n, const float* g_rays, const float* g_rays_2,
              int g_rays_stride, void* tmp, int64_t need, int64_t tmp_bytes, const char* need_name, float* g_poses, float* g_intr,
              float* g_dist, const unsigned char* dist_mask, nerfhip_stream_t stream) {
    int rc = views_check(cfg, num_views, poses, pose_view_stride, pose_ld, what);
    if (rc) return rc;
    NH_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && (n == 0 || (inds && g_rays)), "%s: bad arguments", what);
    NH_REQUIRE(g_rays_stride >= (cfg->use_viewdirs ? 11 : 8), "%s: g_rays_stride must cover the %d columns of a ray row", what,
               cfg->use_viewdirs ? 11 : 8);
    NH_REQUIRE(tmp_bytes >= need && (need == 0 || tmp), "%s: tmp must hold %s(n, num_views) = %lld bytes", what, need_name,
               (long long)need);
    PoseViewsArgs p;
    memset(&p, 0, sizeof(p));
    int64_t slots = 0, words = 0;
    if (n > 0) {
        words = pv_views_words(n, num_views, &slots);
        p.a = select_vjp_args(cfg, poses, pose_ld, inds, n, g_rays, g_rays_2, g_rays_stride, tmp);
        p.a.intr = intr, p.a.dist = dist;
        p.num_views = num_views, p.view_stride = pose_view_stride, p.hw = (int64_t)cfg->height * cfg->width;
        p.cnt = (int*)tmp + slots * 12, p.off = p.cnt + num_views, p.list = p.off + num_views;
    }
    if (g_poses) {
        if (n > 0) {
            NH_LAUNCH(k_pose_views_group, num_views, PV_THREADS, 0, stream, p);
            rc = nh_launch_status(what);
            if (rc) return rc;
            NH_LAUNCH(k_pose_views_part, slots, PV_THREADS, 0, stream, p);
            rc = nh_launch_status(what);
            if (rc) return rc;
        }
        NH_LAUNCH_NAMED("k_pose_vjp_sum", k_pose_vjp_sum<12>, num_views, 12 * 64, 0, stream, (const float*)p.a.tmp, 0, (const int*)p.cnt, (const int*)p.off,
                  g_poses);  // (n == 0: cnt is NULL, zeros)
        rc = nh_launch_status(what);
        if (rc) return rc;
    }
    if (g_intr) {
        float* part = n > 0 ? (float*)tmp + words : nullptr;  // [G(n)][4], behind the pose VJP's words
        const int64_t wgs = pv_wgs(n);
        if (wgs > 0) {
            NH_LAUNCH(k_intr_vjp_part, wgs, PV_THREADS, 0, stream, p, part);
            rc = nh_launch_status(what);
            if (rc) return rc;
        }
        NH_LAUNCH_NAMED("k_intr_vjp_sum", k_pose_vjp_sum<4>, 1, 4 * 64, 0, stream, (const float*)part, (int)wgs, (const int*)nullptr, (const int*)nullptr,
                  g_intr);  // (n == 0: zeros)
        rc = nh_launch_status(what);
        if (rc) return rc;
    }
    if (g_dist) {
        const int64_t wgs = pv_wgs(n);
        float* part = n > 0 ? (float*)tmp + words + wgs * 4 : nullptr;  // [G(n)][4], behind the intrinsics' partials
        if (wgs > 0) {
            NH_LAUNCH(k_dist_vjp_part, wgs, PV_THREADS, 0, stream, p, dist_mask, part);
            rc = nh_launch_status(what);
            if (rc) return rc;
        }
        NH_LAUNCH_NAMED("k_dist_vjp_sum", k_pose_vjp_sum<4>, 1, 4 * 64, 0, stream, (const float*)part, (int)wgs, (const int*)nullptr,
                        (const int*)nullptr, g_dist);  // (n == 0: zeros)
        rc = nh_launch_status(what);
    }
    return rc;
}

// ---- the gradient of the per-view exposure table (nerfhip_exposure_bwd) ---------------------------------------------------------------
// expo [V][6] = (s_r s_g s_b b_r b_g b_b) per view sits behind the render: p' = exp(s) p + b (k_mse_loss_views, elementwise.hip), so
// its gradient needs the two rgb buffers, the targets and the batch's global indices, and no ray gradient.  Row v is ONE sum over view
// v's rays in ascending batch position along the single-view tree with n = n_v -- the pose VJP's scheme over views: the same grouping
// launch (k_pose_views_group: off, cnt, the stable per-view list), k_pose_views_part's slots with six thread sums in list order,
// pv_block_sum<6>, then k_pose_vjp_sum<6> with V workgroups.  An index outside [0, V hw) is in no view's list: dropped.
// Per ray of the list and channel c, in this order, every operation one fp32 rounding unless said (e, b: the view's, once per thread):
//     e = (float)exp((double)s)                                       (one fp64 exp, then the final rounding)
//     coarse:  q = e * p;  d = (q + b) - t;  dk = d * k;  acc_s[c] += dk * q;  acc_b[c] += dk
//     fine (when given): the same on the fine rgb, added after the coarse term
// with k = 2 / (3 n) * grad_scale formed as k_mse_loss forms it.  mask (device, [V][6] bytes, or NULL = all learned): a masked
// entry's partial is an exact zero in every workgroup of its view, so its sum is one.
struct ExpoArgs {
    const float *rc, *rf, *tgt;   // rf may be NULL
    int tstride;
    int64_t n;
    float grad_scale;
    const float* expo;
    const unsigned char* mask;
    float* part;                  // the slots' partials [floor(n / 256) + V][6]
};

NH_KERNEL void k_expo_part(PoseViewsArgs p, ExpoArgs x) {
    NH_SHARED float s_part[PV_THREADS / 64][6];
    const int w = (int)blockIdx.x;
    int v = 0, top = p.num_views - 1;  // the last view whose first slot is <= w (k_pose_views_part)
    while (v < top) {
        const int mid = (v + top + 1) >> 1;
        if (p.off[mid] / PV_THREADS + mid <= w)
            v = mid;
        else
            top = mid - 1;
    }
    const int off = p.off[v], nv = p.cnt[v];
    const int b = w - (off / PV_THREADS + v), wgs = (int)pv_wgs(nv);
    // (a slot no view uses; the whole workgroup leaves.  b < 0: indices below 0 count as "less" for every view, so with 256 or more of
    // them view 0's first slot is above 0 and the workgroups below it belong to nobody)
    if (b < 0 || b >= wgs) return;
    const float k = 2.0f / (float)(3 * x.n) * x.grad_scale;
    float e[3], o[3], acc[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        e[c] = (float)exp((double)x.expo[(int64_t)v * 6 + c]);
        o[c] = x.expo[(int64_t)v * 6 + 3 + c];
        acc[c] = 0.0f, acc[3 + c] = 0.0f;
    }
    const int step = wgs * PV_THREADS;
    for (int r = b * PV_THREADS + (int)threadIdx.x; r < nv; r += step) {
        const int64_t i = p.list[off + r];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t = x.tgt[i * x.tstride + c];
            float q = e[c] * x.rc[i * 3 + c];
            float dk = ((q + o[c]) - t) * k;
            acc[c] += dk * q;
            acc[3 + c] += dk;
            if (x.rf) {
                q = e[c] * x.rf[i * 3 + c];
                dk = ((q + o[c]) - t) * k;
                acc[c] += dk * q;
                acc[3 + c] += dk;
            }
        }
    }
    if (x.mask) {
#pragma unroll
        for (int j = 0; j < 6; ++j)
            if (!x.mask[(int64_t)v * 6 + j]) acc[j] = 0.0f;
    }
    pv_block_sum<6>(acc, s_part, x.part + (int64_t)w * 6);
}

}  // namespace

extern "C" int64_t nerfhip_exposure_grad_tmp_bytes(int64_t n, int num_views) {
    if (n < 0 || n >= ((int64_t)1 << 31) || num_views < 1 || num_views > NERFHIP_MAX_VIEWS) return -1;
    return (int64_t)sizeof(float) * (6 * (n / PV_THREADS + num_views) + 2 * (int64_t)num_views + n);
}

extern "C" int nerfhip_exposure_bwd(const float* rgb_coarse, const float* rgb_fine, const float* target, int target_stride, int64_t n,
                                    float grad_scale, const int64_t* inds, int64_t hw, const float* expo, int num_views,
                                    const unsigned char* mask, void* tmp, int64_t tmp_bytes, float* g_expo, nerfhip_stream_t stream) {
    const char* what = "exposure_bwd";
    int rc = nh_exposure_check(what, inds, n, hw, expo, num_views);
    if (rc) return rc;
    NH_REQUIRE(g_expo && (n == 0 || (rgb_coarse && target)), "%s: bad arguments", what);
    NH_REQUIRE(target_stride >= 3, "%s: target_stride must be >= 3 (got %d)", what, target_stride);
    const int64_t need = nerfhip_exposure_grad_tmp_bytes(n, num_views);
    NH_REQUIRE(tmp && tmp_bytes >= need, "%s: tmp must hold nerfhip_exposure_grad_tmp_bytes(n, num_views) = %lld bytes", what,
               (long long)need);
    PoseViewsArgs p;
    memset(&p, 0, sizeof(p));
    const int64_t slots = n / PV_THREADS + num_views;
    float* part = (float*)tmp;
    if (n > 0) {
        p.a.inds = inds, p.a.n = n;
        p.num_views = num_views, p.hw = hw;
        p.cnt = (int*)tmp + slots * 6, p.off = p.cnt + num_views, p.list = p.off + num_views;
        ExpoArgs x = {rgb_coarse, rgb_fine, target, target_stride, n, grad_scale, expo, mask, part};
        NH_LAUNCH(k_pose_views_group, num_views, PV_THREADS, 0, stream, p);
        rc = nh_launch_status(what);
        if (rc) return rc;
        NH_LAUNCH(k_expo_part, slots, PV_THREADS, 0, stream, p, x);
        rc = nh_launch_status(what);
        if (rc) return rc;
    }
    NH_LAUNCH_NAMED("k_expo_sum", k_pose_vjp_sum<6>, num_views, 6 * 64, 0, stream, (const float*)part, 0, (const int*)p.cnt,
                    (const int*)p.off, g_expo);  // (n == 0: cnt is NULL, zeros)
    return nh_launch_status(what);
}

extern "C" int64_t nerfhip_pose_grad_views_tmp_bytes(int64_t n, int num_views) {
    int64_t slots;
    if (n < 0 || n >= ((int64_t)1 << 31) || num_views < 1 || num_views > NERFHIP_MAX_VIEWS) return -1;
    return n == 0 ? 0 : pv_views_words(n, num_views, &slots) * (int64_t)sizeof(float);
}

extern "C" int64_t nerfhip_intr_grad_views_tmp_bytes(int64_t n, int num_views) {
    const int64_t b = nerfhip_pose_grad_views_tmp_bytes(n, num_views);
    return b < 0 ? -1 : b + pv_wgs(n) * 4 * (int64_t)sizeof(float);
}

extern "C" int nerfhip_select_rays_views_intr_bwd(const nerfhip_select_cfg* cfg, const float* intr, int num_views, const float* poses,
                                                  int64_t pose_view_stride, int pose_ld, const int64_t* inds, int64_t n,
                                                  const float* g_rays, const float* g_rays_2, int g_rays_stride, void* tmp,
                                                  int64_t tmp_bytes, float* g_poses, float* g_intr, nerfhip_stream_t stream) {
    const char* what = "select_rays_views_intr_bwd";
    NH_REQUIRE(intr, "%s: intr must not be NULL", what);
    NH_REQUIRE(g_poses || g_intr, "%s: g_poses and g_intr must not both be NULL", what);
    return views_bwd(what, cfg, intr, nullptr, num_views, poses, pose_view_stride, pose_ld, inds, n, g_rays, g_rays_2, g_rays_stride,
                     tmp, nerfhip_intr_grad_views_tmp_bytes(n, num_views), tmp_bytes, "nerfhip_intr_grad_views_tmp_bytes", g_poses,
                     g_intr, nullptr, nullptr, stream);
}

extern "C" int64_t nerfhip_dist_grad_views_tmp_bytes(int64_t n, int num_views) {
    const int64_t b = nerfhip_intr_grad_views_tmp_bytes(n, num_views);
    return b < 0 ? -1 : b + pv_wgs(n) * 4 * (int64_t)sizeof(float);
}

extern "C" int nerfhip_select_rays_views_dist_bwd(const nerfhip_select_cfg* cfg, const float* intr, const float* dist, int num_views,
                                                  const float* poses, int64_t pose_view_stride, int pose_ld, const int64_t* inds,
                                                  int64_t n, const float* g_rays, const float* g_rays_2, int g_rays_stride, void* tmp,
                                                  int64_t tmp_bytes, float* g_poses, float* g_intr, float* g_dist,
                                                  const unsigned char* dist_mask, nerfhip_stream_t stream) {
    const char* what = "select_rays_views_dist_bwd";
    NH_REQUIRE(dist, "%s: dist must not be NULL", what);
    NH_REQUIRE(g_poses || g_intr || g_dist, "%s: g_poses, g_intr and g_dist must not all be NULL", what);
    return views_bwd(what, cfg, intr, dist, num_views, poses, pose_view_stride, pose_ld, inds, n, g_rays, g_rays_2, g_rays_stride, tmp,
                     nerfhip_dist_grad_views_tmp_bytes(n, num_views), tmp_bytes, "nerfhip_dist_grad_views_tmp_bytes", g_poses, g_intr,
                     g_dist, dist_mask, stream);
}

extern "C" int nerfhip_select_rays_views_bwd(const nerfhip_select_cfg* cfg, int num_views, const float* poses,
                                             int64_t pose_view_stride, int pose_ld, const int64_t* inds, int64_t n,
                                             const float* g_rays, const float* g_rays_2, int g_rays_stride, void* tmp,
                                             int64_t tmp_bytes, float* g_poses, nerfhip_stream_t stream) {
    const char* what = "select_rays_views_bwd";
    NH_REQUIRE(g_poses, "%s: bad arguments", what);
    return views_bwd(what, cfg, nullptr, nullptr, num_views, poses, pose_view_stride, pose_ld, inds, n, g_rays, g_rays_2, g_rays_stride,
                     tmp, nerfhip_pose_grad_views_tmp_bytes(n, num_views), tmp_bytes, "nerfhip_pose_grad_views_tmp_bytes", g_poses,
                     nullptr, nullptr, nullptr, stream);
}

extern "C" int64_t nerfhip_pose_grad_tmp_bytes(int64_t n) { return n < 0 ? -1 : pv_wgs(n) * 12 * (int64_t)sizeof(float); }

extern "C" int nerfhip_ray_bundle_bwd(int height, int width, float focal, const int64_t* pixels, int64_t n,
                                      const float* g_ray_origins, const float* g_ray_directions, void* tmp, int64_t tmp_bytes,
                                      float* g_c2w, nerfhip_stream_t stream) {
    NH_REQUIRE(height > 0 && width > 0 && n >= 0 && g_c2w && (n == 0 || g_ray_origins || g_ray_directions),
               "ray_bundle_bwd: bad arguments");
    NH_REQUIRE(pixels || n == (int64_t)height * width, "ray_bundle_bwd: n must be height*width when pixels is NULL");
    PoseVjpArgs a;
    memset(&a, 0, sizeof(a));
    a.s.height = height, a.s.width = width, a.s.focal = focal;
    a.select = 0, a.inds = pixels, a.n = n, a.g_a = g_ray_origins, a.g_b = g_ray_directions, a.g_stride = 3;
    a.tmp = (float*)tmp;
    return pose_vjp_launch(a, tmp_bytes, g_c2w, stream, "ray_bundle_bwd");
}

extern "C" int nerfhip_select_rays_bwd(const nerfhip_select_cfg* cfg, const float* c2w, int c2w_ld, const int64_t* inds,
                                       int64_t n, const float* g_rays, const float* g_rays_2, int g_rays_stride, void* tmp,
                                       int64_t tmp_bytes, float* g_c2w, nerfhip_stream_t stream) {
    NH_REQUIRE(cfg && c2w && c2w_ld >= 4 && cfg->height > 0 && cfg->width > 0 && n >= 0 && g_c2w && (n == 0 || (inds && g_rays)),
               "select_rays_bwd: bad arguments");
    NH_REQUIRE(g_rays_stride >= (cfg->use_viewdirs ? 11 : 8), "select_rays_bwd: g_rays_stride must cover the %d columns of a ray row",
               cfg->use_viewdirs ? 11 : 8);
    return pose_vjp_launch(select_vjp_args(cfg, c2w, c2w_ld, inds, n, g_rays, g_rays_2, g_rays_stride, tmp), tmp_bytes, g_c2w, stream,
                           "select_rays_bwd");
}

// ---- camera table: pose[v] = base[v] Exp(xi[v]) and its VJP (se(3) pose refinement) ---------------------------------------------------
// xi = [w (3), v (3)]; Exp the SE(3) exponential: R = I + c1 W + c2 W^2, t = (I + c2 W + c3 W^2) v, W = hat(w), x = |w|^2 and
//     c_n(x) = sum_k (-1)^k x^k / (2k + n)!      (c0 = cos, c1 = sin th / th, c2 = (1 - cos th) / th^2, c3 = (th - sin th) / th^3)
// with  c_n = 1 / n! - x c_{n+2}  and  d c_n / dx = -(c_{n+1} - n c_{n+2}) / 2.  One thread per view and a few hundred flops each: the
// arithmetic runs in fp64 (inputs and outputs are fp32), so what is left of the error is the last rounding -- and, in the closed form,
// what nh_sincos hands over.
//   x < PT_SERIES_BELOW (= 10 > pi^2: every twist of the principal domain |w| <= pi): c4 and c5 from their power series (PT_TERMS terms,
//       the first one left out < 1e-17 at x = 10), c3, c2, c1 from the recurrence upwards; no square root, no division, and x = 0 gives
//       1 / n! exactly -- the generators' derivative.
//   x >= PT_SERIES_BELOW (a twist that wraps round): th = sqrt(x), (s, c) = nh_sincos of the fp32 head of th / 2, corrected to first
//       order for its fp64 tail; sin th = 2 s c and 1 - cos th = 2 s^2 keep their relative accuracy at every multiple of pi; c3, c4, c5
//       from the recurrence downwards (x >= 10: 1 / n! - c_n does not cancel below 0.4 / n!).
constexpr double PT_SERIES_BELOW = 10.0;
constexpr int PT_TERMS = 13;
constexpr int PT_THREADS = 256;

namespace {

template <int N>
NH_DEVICE double pt_series(double x) {  // n! c_n(x) = 1 - x / ((n + 1)(n + 2)) (1 - x / ((n + 3)(n + 4)) (1 - ...))
    double s = 1.0;
#pragma unroll
    for (int k = PT_TERMS; k >= 1; --k) s = 1.0 - x * (1.0 / (double)((2 * k + N - 1) * (2 * k + N))) * s;
    return s;
}

// c[n] = c_n(x), n = 1 .. 5
NH_DEVICE void pt_coefs(double x, double* c) {
    if (x < PT_SERIES_BELOW) {
        c[5] = pt_series<5>(x) * (1.0 / 120.0);
        c[4] = pt_series<4>(x) * (1.0 / 24.0);
        c[3] = 1.0 / 6.0 - x * c[5];
        c[2] = 0.5 - x * c[4];
        c[1] = 1.0 - x * c[3];
    } else {
        const double th = sqrt(x), h = 0.5 * th;
        const float hh = (float)h, hl = (float)(h - (double)hh);
        float sf, cf;
        nh_sincos(hh, &sf, &cf);
        const double s = (double)sf + (double)cf * (double)hl, cc = (double)cf - (double)sf * (double)hl;
        c[1] = 2.0 * s * cc / th;
        c[2] = 2.0 * s * s / x;
        c[3] = (1.0 - c[1]) / x;
        c[4] = (0.5 - c[2]) / x;
        c[5] = (1.0 / 6.0 - c[3]) / x;
    }
}

struct PoseTableArgs {
    const float *xi, *base;  // [V][6]; 3 rows of ld floats at base + v * view_stride
    int64_t view_stride;
    int ld, num_views;
};

// the twist and the base of view v; returns whether the twist is exactly zero
NH_DEVICE bool pt_load(const PoseTableArgs& p, int v, double* w, double* u, const float** base) {
    const float* xi = p.xi + (int64_t)v * 6;
    bool zero = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = xi[k], b = xi[3 + k];
        w[k] = (double)a, u[k] = (double)b;
        zero = zero && a == 0.0f && b == 0.0f;
    }
    *base = p.base + (int64_t)v * p.view_stride;
    return zero;
}

NH_KERNEL void k_pose_table_fwd(PoseTableArgs p, float* __restrict__ poses) {
    const int v = (int)(blockIdx.x * PT_THREADS + threadIdx.x);
    if (v >= p.num_views) return;
    double w[3], u[3], c[6];
    const float* b;
    const bool zero = pt_load(p, v, w, u, &b);
    float* out = poses + (int64_t)v * 12;
    if (zero) {  // Exp(0) = I: the base itself, bit for bit (signed zeros included)
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) out[4 * i + j] = b[(int64_t)i * p.ld + j];
        return;
    }
    const double x = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    pt_coefs(x, c);
    const double W[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
    double D[3][3], t[3];  // D = R - I; t = V v
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double w2 = w[i] * w[j] - (i == j ? x : 0.0);  // (W^2)[i][j]
            D[i][j] = c[1] * W[i][j] + c[2] * w2;
            q += (c[2] * W[i][j] + c[3] * w2) * u[j];
        }
        t[i] = u[i] + q;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double r0 = (double)b[(int64_t)i * p.ld], r1 = (double)b[(int64_t)i * p.ld + 1], r2 = (double)b[(int64_t)i * p.ld + 2];
#pragma unroll
        for (int j = 0; j < 3; ++j) out[4 * i + j] = (float)(((r0 * D[0][j] + r1 * D[1][j]) + r2 * D[2][j]) + (j == 0 ? r0 : j == 1 ? r1 : r2));
        out[4 * i + 3] = (float)(((r0 * t[0] + r1 * t[1]) + r2 * t[2]) + (double)b[(int64_t)i * p.ld + 3]);
    }
}

// d(loss)/d(xi[v]) from d(loss)/d(poses[v]): G = base_R^T g_R and gt = base_R^T g_t are the cotangents of R and t;
//   <H, a W + b W^2> has the w-gradient  2 w (a' <H, W> + b' <H, W^2>) + a ax(H) + b ((H + H^T) w - 2 w tr H),
//   <H, W> = w . ax(H),  <H, W^2> = w^T H w - x tr H,  ax(H) = (H21 - H12, H02 - H20, H10 - H01),
// once with H = G, (a, b) = (c1, c2) and once with H = gt v^T, (a, b) = (c2, c3); d/dv = V^T gt.
NH_KERNEL void k_pose_table_bwd(PoseTableArgs p, const float* __restrict__ g_poses, const unsigned char* __restrict__ active,
                                float* __restrict__ g_xi) {
    const int v = (int)(blockIdx.x * PT_THREADS + threadIdx.x);
    if (v >= p.num_views) return;
    float* out = g_xi + (int64_t)v * 6;
    if (active && !active[v]) {
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k] = 0.0f;
        return;
    }
    double w[3], u[3], c[6];
    const float* b;
    pt_load(p, v, w, u, &b);
    const float* g = g_poses + (int64_t)v * 12;
    double G[3][3], gt[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double b0 = (double)b[k], b1 = (double)b[(int64_t)p.ld + k], b2 = (double)b[2 * (int64_t)p.ld + k];
#pragma unroll
        for (int j = 0; j < 3; ++j) G[k][j] = b0 * (double)g[j] + b1 * (double)g[4 + j] + b2 * (double)g[8 + j];
        gt[k] = b0 * (double)g[3] + b1 * (double)g[7] + b2 * (double)g[11];
    }
    const double x = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    pt_coefs(x, c);
    const double d1 = -0.5 * (c[2] - c[3]), d2 = -0.5 * (c[3] - 2.0 * c[4]), d3 = -0.5 * (c[4] - 3.0 * c[5]);  // d c_n / dx
    // rotation: H = G
    const double ax[3] = {G[2][1] - G[1][2], G[0][2] - G[2][0], G[1][0] - G[0][1]};
    const double tr = G[0][0] + G[1][1] + G[2][2];
    double hw[3], wHw = 0.0;  // (H + H^T) w
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        hw[k] = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) hw[k] += (G[k][j] + G[j][k]) * w[j];
        wHw += 0.5 * hw[k] * w[k];
    }
    const double w_ax = w[0] * ax[0] + w[1] * ax[1] + w[2] * ax[2];
    // translation: H = gt v^T
    const double at[3] = {u[1] * gt[2] - u[2] * gt[1], u[2] * gt[0] - u[0] * gt[2], u[0] * gt[1] - u[1] * gt[0]};  // v x gt
    const double wg = w[0] * gt[0] + w[1] * gt[1] + w[2] * gt[2], wu = w[0] * u[0] + w[1] * u[1] + w[2] * u[2];
    const double gu = gt[0] * u[0] + gt[1] * u[1] + gt[2] * u[2];
    const double w_at = w[0] * at[0] + w[1] * at[1] + w[2] * at[2];
    const double through_x = 2.0 * ((d1 * w_ax + d2 * (wHw - x * tr)) + (d2 * w_at + d3 * (wg * wu - x * gu)));
    const double wxg[3] = {w[1] * gt[2] - w[2] * gt[1], w[2] * gt[0] - w[0] * gt[2], w[0] * gt[1] - w[1] * gt[0]};  // w x gt
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double rot = c[1] * ax[k] + c[2] * (hw[k] - 2.0 * w[k] * tr);
        const double tra = c[2] * at[k] + c[3] * ((gt[k] * wu + u[k] * wg) - 2.0 * w[k] * gu);
        out[k] = (float)(w[k] * through_x + (rot + tra));
        out[3 + k] = (float)(gt[k] + (c[3] * (w[k] * wg - x * gt[k]) - c[2] * wxg[k]));
    }
}

}  // namespace

extern "C" int nerfhip_pose_table_fwd(const float* xi, const float* base, int64_t base_view_stride, int base_ld, int num_views,
                                      float* poses, nerfhip_stream_t stream) {
    const char* what = "pose_table_fwd";
    NH_REQUIRE(xi && base, "%s: xi and base must not be NULL", what);
    int rc = table_check(num_views, base_view_stride, base_ld, "base", what);
    if (rc) return rc;
    NH_REQUIRE(poses, "%s: poses must not be NULL", what);
    const PoseTableArgs p = {xi, base, base_view_stride, base_ld, num_views};
    NH_LAUNCH(k_pose_table_fwd, nh_ceil_div(num_views, PT_THREADS), PT_THREADS, 0, stream, p, poses);
    return nh_launch_status(what);
}

extern "C" int nerfhip_pose_table_bwd(const float* xi, const float* base, int64_t base_view_stride, int base_ld, int num_views,
                                      const float* g_poses, const unsigned char* active, float* g_xi, nerfhip_stream_t stream) {
    const char* what = "pose_table_bwd";
    NH_REQUIRE(xi && base, "%s: xi and base must not be NULL", what);
    int rc = table_check(num_views, base_view_stride, base_ld, "base", what);
    if (rc) return rc;
    NH_REQUIRE(g_poses && g_xi, "%s: g_poses and g_xi must not be NULL", what);
    const PoseTableArgs p = {xi, base, base_view_stride, base_ld, num_views};
    NH_LAUNCH(k_pose_table_bwd, nh_ceil_div(num_views, PT_THREADS), PT_THREADS, 0, stream, p, g_poses, active, g_xi);
    return nh_launch_status(what);
}

// ---- 8-bit output stage (eval_nerf.py:23-36) ---------------------------------------------------------------------------
// float -> uint8 exactly as the reference's host conversion behaves on x86-64: truncate towards zero to a 32-bit
// integer, keep the low byte (NaN / out-of-range -> the "integer indefinite" 0x80000000 -> 0).
NH_DEVICE uint8_t nh_to_u8(float v) {
    int32_t q;
    if (v != v || v >= 2147483648.0f || v < -2147483648.0f)
        q = (int32_t)0x80000000u;
    else
        q = (int32_t)v;
    return (uint8_t)((uint32_t)q & 0xFFu);
}

// cast_to_image: torchvision ToPILImage of a float CHW tensor = pic.mul(255).byte() -> HWC bytes.  in: [pixels,
// in_channels] (the first 3 are used, as the caller slices rgb[..., :3]); out: [pixels, 3] uint8.
NH_KERNEL void k_cast_to_image(const float* __restrict__ in, int in_channels, int64_t pixels, uint8_t* __restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels * 3) return;
    int64_t p = i / 3;
    int c = (int)(i - p * 3);
    out[i] = nh_to_u8(in[p * in_channels + c] * 255.0f);
}

extern "C" int nerfhip_cast_to_image(const float* rgb, int in_channels, int64_t pixels, uint8_t* out,
                                     nerfhip_stream_t stream) {
    NH_REQUIRE(pixels >= 0 && in_channels >= 3 && (pixels == 0 || (rgb && out)), "cast_to_image: bad arguments");
    if (pixels == 0) return NERFHIP_OK;
    NH_LAUNCH(k_cast_to_image, nh_ceil_div(pixels * 3, 256), 256, 0, stream, rgb, in_channels, pixels, out);
    return nh_launch_status("cast_to_image");
}

// cast_to_disparity_image: (t - min) / (max - min), clamp(0,1) * 255, astype(uint8).  torch's min()/max() propagate
// NaN, so a single NaN pixel (acc == 0) turns the whole reference image into zeros -- reproduced.
// Pass 1: one workgroup reduces min / max / any-NaN into scratch[0..2]; pass 2: the map.
NH_KERNEL void k_disparity_range(const float* __restrict__ t, int64_t n, float* __restrict__ scratch) {
    NH_SHARED float s_lo[16], s_hi[16], s_nan[16];
    float lo = INFINITY, hi = -INFINITY, bad = 0.0f;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        float v = t[i];
        if (v != v) {
            bad = 1.0f;
        } else {
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        lo = fminf(lo, nh_shfl_xor(lo, m));
        hi = fmaxf(hi, nh_shfl_xor(hi, m));
        bad = fmaxf(bad, nh_shfl_xor(bad, m));
    }
    int wave = nh_wave_in_block(), lane = nh_lane();
    if (lane == 0) s_lo[wave] = lo, s_hi[wave] = hi, s_nan[wave] = bad;
    nh_block_sync();
    if (threadIdx.x == 0) {
        int waves = (int)(blockDim.x >> 6);
        for (int w = 1; w < waves; ++w) {
            lo = fminf(lo, s_lo[w]);
            hi = fmaxf(hi, s_hi[w]);
            bad = fmaxf(bad, s_nan[w]);
        }
        scratch[0] = lo;
        scratch[1] = hi;
        scratch[2] = bad;
    }
}
NH_KERNEL void k_disparity_image(const float* __restrict__ t, int64_t n, const float* __restrict__ scratch,
                                 uint8_t* __restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float lo = scratch[0], hi = scratch[1];
    if (scratch[2] != 0.0f) lo = hi = NAN;
    float v = (t[i] - lo) / (hi - lo);
    v = v != v ? v : fminf(fmaxf(v, 0.0f), 1.0f);  // torch.clamp keeps NaN
    out[i] = nh_to_u8(v * 255.0f);
}

extern "C" int nerfhip_cast_to_disparity_image(const float* disparity, int64_t pixels, float* scratch3, uint8_t* out,
                                               nerfhip_stream_t stream) {
    NH_REQUIRE(pixels >= 0 && (pixels == 0 || (disparity && out && scratch3)), "cast_to_disparity_image: bad arguments");
    if (pixels == 0) return NERFHIP_OK;
    NH_LAUNCH(k_disparity_range, 1, 1024, 0, stream, disparity, pixels, scratch3);
    NH_LAUNCH(k_disparity_image, nh_ceil_div(pixels, 256), 256, 0, stream, disparity, pixels, scratch3, out);
    return nh_launch_status("cast_to_disparity_image");
}
