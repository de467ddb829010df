// spread.hip -- the ray-weight spread loss (mip-NeRF 360's L_dist, Barron et al. 2022, eq. 15) of one compositing pass and its
// gradient w.r.t. the ray weights: the cotangent `g_weights` that k_volume_render_bwd takes.  (In this library "distortion" is the
// lens; this regulariser is the SPREAD of a ray's weights.)  The definition is in include/nerfhip.h (nerfhip_spread_loss).
//
// One wavefront owns one ray and walks its samples in chunks of 64, one per lane, as render.hip does.  With m ascending,
//     sum_i sum_j w_i w_j |m_i - m_j| = 2 sum_i w_i (m_i W_<i - WM_<i),
//     dL/dw_i = 2 [m_i (W_<i - W_>i) - (WM_<i - WM_>i)] + (2/3) w_i delta_i,
// so prefix and suffix sums of w and w m do the work of the S^2 double sum in O(S).  Walk 1 runs front to back: the transmittance
// (the fp64 product scan of k_volume_render_bwd's pass 1, so w is the compositing's own weight bit for bit), W_<, WM_< and the
// loss; it leaves w per sample and (W_<, WM_<) per chunk in LDS.  Walk 2 runs back to front carrying W_> and WM_>, rebuilds the
// in-chunk prefix from the chunk's stored carry and writes the gradient.  Every sum is fp64 in a fixed lane and chunk order (no
// atomics); each result is rounded to fp32 once.
#include "../nh_host.h"
#include "../nh_render.h"

// the normalised interval of sample i: midpoint and width, fp64 from the fp32 depths (zr: the ray's depths)
NH_DEVICE void nh_spread_interval(const float* __restrict__ zr, int s, int i, double near, double inv, double* m, double* delta) {
    const double si = ((double)zr[i] - near) * inv;
    double ei;
    if (i + 1 < s)
        ei = ((double)zr[i + 1] - near) * inv;
    else
        ei = si > 1.0 ? si : 1.0;  // the last sample owns [z_{S-1}, far]
    *m = 0.5 * (si + ei);
    *delta = ei - si;
}

NH_KERNEL void k_spread_loss(const float* __restrict__ raw, const float* __restrict__ z, const float* __restrict__ rays,
                             int ray_stride, int64_t n, int s, float noise_std, const float* __restrict__ noise, uint64_t seed,
                             uint32_t rng_stream, uint64_t ray_offset, float scale, const float* __restrict__ g_loss,
                             float* __restrict__ loss, float* __restrict__ g_weights) {
    NH_DYN_LDS(lds_raw);
    const int nchunks = (s + 63) / 64;
    float* sW = (float*)lds_raw;                                          // [s] the ray's weights
    double* sPW = (double*)(lds_raw + (((size_t)s * 4 + 7) & ~(size_t)7));  // [nchunks] W_< at the chunk's first sample
    double* sPM = sPW + nchunks;                                          // [nchunks] WM_< there
    const int64_t ray = blockIdx.x;
    const int lane = nh_lane();
    const float* rr = rays + ray * ray_stride;
    const float* zr = z + ray * s;
    const float near = rr[6], far = rr[7];
    if (!(far > near)) {  // inv = 0: no interval to spread over -- L = 0 and a zero gradient, exactly
        if (loss && lane == 0) loss[ray] = 0.0f;
        if (g_weights)
            for (int i = lane; i < s; i += 64) g_weights[ray * s + i] = 0.0f;
        return;
    }
    const double inv = 1.0 / ((double)far - (double)near);
    const float dx = rr[3], dy = rr[4], dz = rr[5];
    const float norm = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));  // as k_volume_render_fwd / _bwd form it
    // walk 1, front to back: transmittance, weights, prefix sums, loss
    double carry = 1.0, cW = 0.0, cM = 0.0, lsum = 0.0;
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
        float w = 0.0f;
        double m = 0.0, delta = 0.0;
        if (valid) {
            w = q.alpha * T;
            sW[i] = w;
            nh_spread_interval(zr, s, i, (double)near, inv, &m, &delta);
        }
        double iw = (double)w, im = (double)w * m;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            double ow = nh_shfl_up_d(iw, d), om = nh_shfl_up_d(im, d);
            if (lane >= d) {
                iw += ow;
                im += om;
            }
        }
        double ew = nh_shfl_up_d(iw, 1), em = nh_shfl_up_d(im, 1);
        if (lane == 0) {
            ew = 0.0;
            em = 0.0;
            sPW[base >> 6] = cW;
            sPM[base >> 6] = cM;
        }
        const double Wl = cW + ew, Ml = cM + em;
        if (valid) lsum += 2.0 * (double)w * (m * Wl - Ml) + (double)w * (double)w * delta / 3.0;
        cW += nh_shfl_d(iw, 63);
        cM += nh_shfl_d(im, 63);
    }
    if (loss) {
        const double L = nh_wave_sum_d(lsum);
        if (lane == 0) loss[ray] = (float)L;
    }
    if (!g_weights) return;
    nh_block_sync();
    const double scale_ray = (double)scale * (g_loss ? (double)g_loss[ray] : 1.0);
    // walk 2, back to front: suffix sums, the gradient
    double sfW = 0.0, sfM = 0.0;
    for (int ch = nchunks - 1; ch >= 0; --ch) {
        const int i = ch * 64 + lane;
        const bool valid = i < s;
        float w = 0.0f;
        double m = 0.0, delta = 0.0;
        if (valid) {
            w = sW[i];
            nh_spread_interval(zr, s, i, (double)near, inv, &m, &delta);
        }
        const double vw = (double)w, vm = (double)w * m;
        double iw = vw, im = vm;  // inclusive prefix within the chunk
        double jw = vw, jm = vm;  // inclusive suffix within the chunk
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            double ow = nh_shfl_up_d(iw, d), om = nh_shfl_up_d(im, d);
            if (lane >= d) {
                iw += ow;
                im += om;
            }
            double pw = nh_shfl_down_d(jw, d), pm = nh_shfl_down_d(jm, d);
            if (lane + d < 64) {
                jw += pw;
                jm += pm;
            }
        }
        double ew = nh_shfl_up_d(iw, 1), em = nh_shfl_up_d(im, 1);
        double aw = nh_shfl_down_d(jw, 1), am = nh_shfl_down_d(jm, 1);
        if (lane == 0) {
            ew = 0.0;
            em = 0.0;
        }
        if (lane == 63) {
            aw = 0.0;
            am = 0.0;
        }
        const double Wl = sPW[ch] + ew, Ml = sPM[ch] + em;  // sums over j < i
        const double Wg = sfW + aw, Mg = sfM + am;          // sums over j > i
        sfW += nh_shfl_d(jw, 0);
        sfM += nh_shfl_d(jm, 0);
        if (valid) {
            const double d = 2.0 * (m * (Wl - Wg) - (Ml - Mg)) + (2.0 / 3.0) * (double)w * delta;
            g_weights[ray * s + i] = (float)(scale_ray * d);
        }
    }
}

extern "C" int nerfhip_spread_loss(const float* raw, const float* z, const float* rays, int ray_stride, int64_t n, int s,
                                   float noise_std, const float* noise, uint64_t seed, uint32_t rng_stream, uint64_t ray_offset,
                                   float scale, const float* g_loss, float* loss, float* g_weights, nerfhip_stream_t stream) {
    NH_REQUIRE(n >= 0, "spread_loss: n < 0");
    if (n == 0) return NERFHIP_OK;  // empty input: nothing to launch, pointers may be NULL
    NH_REQUIRE(raw && z && rays, "spread_loss: raw, z or rays is NULL");
    NH_REQUIRE(ray_stride >= 8, "spread_loss: ray_stride must be at least 8 (near and far are columns 6 and 7)");
    NH_REQUIRE(s >= 1 && s <= 8192, "spread_loss: 1 to 8192 samples per ray (got %d)", s);
    NH_REQUIRE(loss || g_weights, "spread_loss: both outputs are NULL");
    const size_t lds = (((size_t)s * 4 + 7) & ~(size_t)7) + (size_t)((s + 63) / 64) * 16;
    NH_LAUNCH(k_spread_loss, n, 64, lds, stream, raw, z, rays, ray_stride, n, s, noise_std, noise, seed, rng_stream, ray_offset, scale,
              g_loss, loss, g_weights);
    return nh_launch_status("spread_loss");
}
