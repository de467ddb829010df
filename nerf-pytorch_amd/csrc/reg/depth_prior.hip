// depth_prior.hip -- depth priors (DS-NeRF, Deng et al. 2022): the expected-depth and ray-termination losses of one compositing pass
// against a per-ray prior row (D, c, sigma), and their gradient w.r.t. the ray weights: the cotangent `g_weights` that
// k_volume_render_bwd takes.  The definition is in include/nerfhip.h (nerfhip_depth_prior_loss).
//
// k_spread_loss's shape (reg/spread.hip): one wavefront owns one ray and walks its samples in chunks of 64, one per lane.  Walk 1 runs
// front to back: the transmittance (the fp64 product scan of k_volume_render_bwd's pass 1, so w is the compositing's own weight bit for
// bit), each lane's fp64 sums of w z and of the termination term over its samples of every chunk, w per sample into LDS.  The two sums
// are then added across the wave (a butterfly: a fixed order, no atomics), which gives d^ and both losses.  Walk 2 forms the gradient
// from the stored w -- dE/dw needs d^, so nothing can be written before the first walk has ended.  A ray without a prior (c > 0 false,
// or its index outside the table) leaves before anything but its index and its c is read.
#include "../nh_host.h"
#include "../nh_render.h"

#define NH_DEPTH_PRIOR_EPS 1e-5

// sample i of a ray with depths zr: its depth and k_i delta_i, fp64 from the fp32 depths (inv = 1 / (2 sigma^2))
NH_DEVICE void nh_depth_prior_sample(const float* __restrict__ zr, int s, int i, double far, double D, double inv, double* zi,
                                     double* kd) {
    const double zd = (double)zr[i];
    double delta;
    if (i + 1 < s) {
        delta = (double)zr[i + 1] - zd;
    } else {
        delta = far - zd;  // the last sample owns [z_{S-1}, far]
        if (!(delta > 0.0)) delta = 0.0;
    }
    const double u = zd - D;
    *zi = zd;
    *kd = exp(-(u * u) * inv) * delta;
}

NH_KERNEL void k_depth_prior_loss(const float* __restrict__ raw, const float* __restrict__ z, const float* __restrict__ rays,
                                  int ray_stride, int64_t n, int s, float noise_std, const float* __restrict__ noise, uint64_t seed,
                                  uint32_t rng_stream, uint64_t ray_offset, const float* __restrict__ prior, int64_t prior_stride,
                                  const int64_t* __restrict__ inds, int64_t prior_rows, float w_expected, float w_termination,
                                  float scale, const float* __restrict__ g_loss, float* __restrict__ loss,
                                  float* __restrict__ g_weights, int accumulate) {
    NH_DYN_LDS(lds_raw);
    float* sW = (float*)lds_raw;  // [s] the ray's weights
    const int64_t ray = blockIdx.x;
    const int lane = nh_lane();
    const int64_t row = inds ? inds[ray] : ray;
    float c = 0.0f;
    if (row >= 0 && row < prior_rows) c = prior[row * prior_stride + 1];
    if (!(c > 0.0f)) {  // no prior (c = NaN included): both losses 0; the gradient row zero, or -- accumulating -- left as it is
        if (loss && lane == 0) {
            loss[ray * 2] = 0.0f;
            loss[ray * 2 + 1] = 0.0f;
        }
        if (g_weights && !accumulate)
            for (int i = lane; i < s; i += 64) g_weights[ray * s + i] = 0.0f;
        return;
    }
    const double D = (double)prior[row * prior_stride], sg = (double)prior[row * prior_stride + 2];
    const double inv = 1.0 / (2.0 * sg * sg);
    const float* rr = rays + ray * ray_stride;
    const float* zr = z + ray * s;
    const double far = (double)rr[7];
    const float dx = rr[3], dy = rr[4], dz = rr[5];
    const float norm = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));  // as k_volume_render_fwd / _bwd form it
    // walk 1, front to back: transmittance, weights, the two sums
    double carry = 1.0, dsum = 0.0, tsum = 0.0;
    for (int base = 0; base < s; base += 64) {
        const int i = base + lane;
        const bool valid = i < s;
        RenderSample q;
        q.alpha = 0.f;
        q.b = 1.f;
        if (valid) q = nh_render_sample(raw, z, ray, s, i, norm, noise_std, noise, seed, rng_stream, ray_offset);
        double p = (double)q.b;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            double o = nh_shfl_up_d(p, d);
            if (lane >= d) p *= o;
        }
        double excl = nh_shfl_up_d(p, 1);
        if (lane == 0) excl = 1.0;
        const float T = (float)(carry * excl);
        carry *= nh_shfl_d(p, 63);
        if (valid) {
            const float w = q.alpha * T;
            sW[i] = w;
            double zi, kd;
            nh_depth_prior_sample(zr, s, i, far, D, inv, &zi, &kd);
            dsum += (double)w * zi;
            tsum += -log((double)w + NH_DEPTH_PRIOR_EPS) * kd;
        }
    }
    const double dhat = nh_wave_sum_d(dsum);
    const double err = dhat - D;
    if (loss) {
        const double tm = nh_wave_sum_d(tsum);
        if (lane == 0) {
            loss[ray * 2] = (float)((double)c * err * err);
            loss[ray * 2 + 1] = (float)((double)c * tm);
        }
    }
    if (!g_weights) return;
    nh_block_sync();
    // walk 2: the gradient.  A term whose weight is exactly 0 is left out (not 0 * inf)
    const bool on_e = w_expected != 0.0f, on_t = w_termination != 0.0f;
    const double ge = on_e ? (double)w_expected * (g_loss ? (double)g_loss[ray * 2] : 1.0) * 2.0 * (double)c * err : 0.0;
    const double gt = on_t ? (double)w_termination * (g_loss ? (double)g_loss[ray * 2 + 1] : 1.0) * (double)c : 0.0;
    for (int i = lane; i < s; i += 64) {
        double d = 0.0;
        if (on_e) d = ge * (double)zr[i];
        if (on_t) {
            double zi, kd;
            nh_depth_prior_sample(zr, s, i, far, D, inv, &zi, &kd);
            d -= gt * kd / ((double)sW[i] + NH_DEPTH_PRIOR_EPS);
        }
        const float v = (float)((double)scale * d);
        const int64_t g = ray * s + i;
        g_weights[g] = accumulate ? g_weights[g] + v : v;
    }
}

extern "C" int nerfhip_depth_prior_loss(const float* raw, const float* z, const float* rays, int ray_stride, int64_t n, int s,
                                        float noise_std, const float* noise, uint64_t seed, uint32_t rng_stream, uint64_t ray_offset,
                                        const float* prior, int64_t prior_stride, const int64_t* inds, int64_t prior_rows,
                                        float w_expected, float w_termination, float scale, const float* g_loss, float* loss,
                                        float* g_weights, int accumulate, nerfhip_stream_t stream) {
    NH_REQUIRE(n >= 0, "depth_prior_loss: n < 0");
    if (n == 0) return NERFHIP_OK;  // empty input: nothing to launch, pointers may be NULL
    NH_REQUIRE(raw && z && rays && prior, "depth_prior_loss: raw, z, rays or prior is NULL");
    NH_REQUIRE(ray_stride >= 8, "depth_prior_loss: ray_stride must be at least 8 (far is column 7)");
    NH_REQUIRE(prior_stride >= 3, "depth_prior_loss: prior_stride must be at least 3 (a row is depth, weight, sigma)");
    NH_REQUIRE(prior_rows >= 0, "depth_prior_loss: prior_rows < 0");
    NH_REQUIRE(s >= 1 && s <= 8192, "depth_prior_loss: 1 to 8192 samples per ray (got %d)", s);
    NH_REQUIRE(loss || g_weights, "depth_prior_loss: both outputs are NULL");
    const size_t lds = ((size_t)s * 4 + 7) & ~(size_t)7;
    NH_LAUNCH(k_depth_prior_loss, n, 64, lds, stream, raw, z, rays, ray_stride, n, s, noise_std, noise, seed, rng_stream, ray_offset,
              prior, prior_stride, inds, prior_rows, w_expected, w_termination, scale, g_loss, loss, g_weights, accumulate);
    return nh_launch_status("depth_prior_loss");
}
