// proposal.hip -- the interlevel proposal loss (mip-NeRF 360's L_prop, Barron et al. 2022, eq. 13) of one ray's two compositing passes
// and its gradient w.r.t. the COARSE pass's ray weights: the cotangent `g_weights_coarse` that k_volume_render_bwd takes.  The fine
// weights are constants of the term (a stop-gradient).  The definition is in include/nerfhip.h (nerfhip_proposal_loss).
//
// k_spread_loss's shape (reg/spread.hip): one wavefront owns one ray and walks samples in chunks of 64, one per lane; both passes'
// weights are the compositing's own bit for bit (nh_render_sample and the fp64 product scan of k_volume_render_bwd's pass 1).
//   walk 1, coarse pass: the coarse edges e^_0..e^_Sc (fp32) and the prefix W^[k] = sum_{j<k} w^_j into LDS -- as an unevaluated
//                        sum of two doubles (error-free additions): B_i is a difference of two prefixes, r_i divides by w_i + eps,
//                        and behind an opaque sample a plain fp64 prefix near 1 would leave B_i of a 1e-9 weight with an absolute
//                        error of 1e-16, which eps = 2^-23 turns into 1e-9 of r_i.  R needs no such care: every r_i <= 0, so
//                        max_j |g_j| >= max_i |r_i| >= |R| / Sf.
//   walk 2, fine pass:   each lane binary-searches the coarse edges for lo_i, hi_i; B_i = W^[hi+1] - W^[lo]; the loss term and
//                        r_i = -2 max(0, w_i - B_i) / (w_i + eps); lo, hi and the fp64 prefix R[k] = sum_{i<k} r_i into LDS.
//   walk 3, coarse pass: lo and hi are non-decreasing, so the fine samples whose range holds j are contiguous: lane j binary-searches
//                        for the first i with hi_i >= j and the last with lo_i <= j; g_j = R[last+1] - R[first].
// Every sum is fp64 in a fixed lane and chunk order (no atomics); each output is rounded to fp32 once.  Every search runs a fixed
// number of steps over a clamped index range, so no depth row -- sorted or not, NaN or not -- takes an access out of the ray's LDS.
#include "../nh_host.h"
#include "../nh_render.h"

#define NH_PROPOSAL_EPS 1.1920928955078125e-07  // 2^-23 (multinerf's eps)
#define NH_PROPOSAL_MAX_SAMPLES 4096             // s_coarse + s_fine: 20 / 12 bytes of LDS per coarse / fine sample, 80 KiB at most

// the weights of 64 samples of one pass (lane i - base), 0 beyond the ray's end; `carry` is the transmittance ahead of the chunk
NH_DEVICE float nh_proposal_weight(const float* __restrict__ raw, const float* __restrict__ z, int64_t ray, int s, int i, float norm,
                                   float noise_std, const float* __restrict__ noise, uint64_t seed, uint32_t rng_stream,
                                   uint64_t ray_offset, int lane, double* carry) {
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
    const float T = (float)(*carry * excl);
    *carry *= nh_shfl_d(p, 63);
    return valid ? q.alpha * T : 0.0f;
}

// (hi, lo) + (bh, bl) as an unevaluated sum of two doubles: Knuth's two-sum of the high parts, the low parts added to its error term
NH_DEVICE void nh_dd_add(double* hi, double* lo, double bh, double bl) {
    const double s = *hi + bh;
    const double t = s - *hi;
    double e = (*hi - (s - t)) + (bh - t);
    e += *lo + bl;
    *hi = s + e;
    *lo = e - (*hi - s);
}

// the inclusive sum over the lanes up to this one, in two doubles
NH_DEVICE void nh_proposal_scan_dd(double* hi, double* lo, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double oh = nh_shfl_up_d(*hi, d), ol = nh_shfl_up_d(*lo, d);
        if (lane >= d) nh_dd_add(hi, lo, oh, ol);
    }
}

// the inclusive fp64 sum over the lanes up to this one
NH_DEVICE double nh_proposal_scan(double v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        double o = nh_shfl_up_d(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

NH_KERNEL void k_proposal_loss(const float* __restrict__ raw_c, const float* __restrict__ z_c, int sc, const float* __restrict__ raw_f,
                               const float* __restrict__ z_f, int sf, const float* __restrict__ rays, int ray_stride, int64_t n,
                               float noise_std, const float* __restrict__ noise_c, const float* __restrict__ noise_f, uint64_t seed,
                               uint64_t ray_offset, float scale, const float* __restrict__ g_loss, float* __restrict__ loss,
                               float* __restrict__ g_weights, int accumulate) {
    NH_DYN_LDS(lds_raw);
    double* sWh = (double*)lds_raw;              // [sc + 1] W^[k] = sum_{j<k} w^_j: the high part
    double* sWl = sWh + (sc + 1);                // [sc + 1] ... and the low part
    double* sR = sWl + (sc + 1);                 // [sf + 1] R[k]  = sum_{i<k} r_i
    float* sE = (float*)(sR + (sf + 1));         // [sc + 1] the coarse edges
    unsigned short* sLo = (unsigned short*)(sE + (sc + 1));  // [sf]
    unsigned short* sHi = sLo + sf;                          // [sf]
    const int64_t ray = blockIdx.x;
    const int lane = nh_lane();
    const float* rr = rays + ray * ray_stride;
    const float* zc = z_c + ray * sc;
    const float* zf = z_f + ray * sf;
    const float far = rr[7];
    const float dx = rr[3], dy = rr[4], dz = rr[5];
    const float norm = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));  // as k_volume_render_fwd / _bwd form it
    // walk 1: the coarse pass (noise stream 1)
    double carry = 1.0, cWh = 0.0, cWl = 0.0;
    for (int base = 0; base < sc; base += 64) {
        const int j = base + lane;
        const float w = nh_proposal_weight(raw_c, z_c, ray, sc, j, norm, noise_std, noise_c, seed, 1u, ray_offset, lane, &carry);
        double ih = (double)w, il = 0.0;
        nh_proposal_scan_dd(&ih, &il, lane);
        if (j < sc) {
            double ph = cWh, pl = cWl;
            nh_dd_add(&ph, &pl, ih, il);
            sWh[j + 1] = ph;
            sWl[j + 1] = pl;
            sE[j] = zc[j];
        }
        nh_dd_add(&cWh, &cWl, nh_shfl_d(ih, 63), nh_shfl_d(il, 63));
    }
    if (lane == 0) {
        const float last = zc[sc - 1];
        sWh[0] = 0.0;
        sWl[0] = 0.0;
        sE[sc] = far > last ? far : last;  // the last sample owns [z_last, max(far, z_last)]
    }
    nh_block_sync();
    // walk 2: the fine pass (noise stream 3)
    carry = 1.0;
    double cR = 0.0, lsum = 0.0;
    const float zf_last = zf[sf - 1];
    const float ef_last = far > zf_last ? far : zf_last;
    for (int base = 0; base < sf; base += 64) {
        const int i = base + lane;
        const float w = nh_proposal_weight(raw_f, z_f, ray, sf, i, norm, noise_std, noise_f, seed, 3u, ray_offset, lane, &carry);
        double r = 0.0;
        if (i < sf) {
            const float e0 = zf[i], e1 = i + 1 < sf ? zf[i + 1] : ef_last;
            // lo = min(#{k in 1..sc : e^_k <= e0}, sc - 1): the first k in [1, sc] with e^_k > e0, less one
            int a = 1, b = sc + 1;
#pragma unroll 1
            for (int it = 0; it < 13; ++it) {
                const int m = (a + b) >> 1;
                if (a < b) {
                    if (sE[m] <= e0)
                        a = m + 1;
                    else
                        b = m;
                }
            }
            int lo = a - 1;
            if (lo > sc - 1) lo = sc - 1;
            // hi = max(#{k in 0..sc-1 : e^_k < e1} - 1, lo): the first k in [0, sc) with e^_k >= e1, less one
            a = 0;
            b = sc;
#pragma unroll 1
            for (int it = 0; it < 13; ++it) {
                const int m = (a + b) >> 1;
                if (a < b) {
                    if (sE[m] < e1)
                        a = m + 1;
                    else
                        b = m;
                }
            }
            int hi = a - 1;
            if (hi < lo) hi = lo;
            sLo[i] = (unsigned short)lo;
            sHi[i] = (unsigned short)hi;
            const double wd = (double)w;
            const double B = (sWh[hi + 1] - sWh[lo]) + (sWl[hi + 1] - sWl[lo]);
            double d = wd - B;
            if (!(d > 0.0) && d == d) d = 0.0;  // max(0, .), NaN kept
            const double den = wd + NH_PROPOSAL_EPS;
            lsum += d * d / den;
            r = -2.0 * d / den;
        }
        if (g_weights) {
            const double incl = nh_proposal_scan(r, lane);
            if (i < sf) sR[i + 1] = cR + incl;
            cR += nh_shfl_d(incl, 63);
        }
    }
    if (loss) {
        const double L = nh_wave_sum_d(lsum);
        if (lane == 0) loss[ray] = (float)L;
    }
    if (!g_weights) return;
    if (lane == 0) sR[0] = 0.0;
    nh_block_sync();
    // walk 3: the coarse pass's gradient
    const double scale_ray = (double)scale * (g_loss ? (double)g_loss[ray] : 1.0);
    for (int j = lane; j < sc; j += 64) {
        // first: the first i in [0, sf) with hi_i >= j (sf: none)
        int a = 0, b = sf;
#pragma unroll 1
        for (int it = 0; it < 13; ++it) {
            const int m = (a + b) >> 1;
            if (a < b) {
                if ((int)sHi[m] < j)
                    a = m + 1;
                else
                    b = m;
            }
        }
        const int first = a;
        // last: the first i in [0, sf) with lo_i > j, less one (-1: none)
        a = 0;
        b = sf;
#pragma unroll 1
        for (int it = 0; it < 13; ++it) {
            const int m = (a + b) >> 1;
            if (a < b) {
                if ((int)sLo[m] <= j)
                    a = m + 1;
                else
                    b = m;
            }
        }
        const int last = a - 1;
        const double d = last >= first ? sR[last + 1] - sR[first] : 0.0;
        const float v = (float)(scale_ray * d);
        const int64_t g = ray * sc + j;
        g_weights[g] = accumulate ? g_weights[g] + v : v;
    }
}

extern "C" int nerfhip_proposal_loss(const float* raw_coarse, const float* z_coarse, int s_coarse, const float* raw_fine,
                                     const float* z_fine, int s_fine, const float* rays, int ray_stride, int64_t n, float noise_std,
                                     const float* noise_coarse, const float* noise_fine, uint64_t seed, uint64_t ray_offset,
                                     float scale, const float* g_loss, float* loss, float* g_weights_coarse, int accumulate,
                                     nerfhip_stream_t stream) {
    NH_REQUIRE(n >= 0, "proposal_loss: n < 0");
    if (n == 0) return NERFHIP_OK;  // empty input: nothing to launch, pointers may be NULL
    NH_REQUIRE(raw_coarse && z_coarse && raw_fine && z_fine && rays, "proposal_loss: raw_coarse, z_coarse, raw_fine, z_fine or rays is NULL");
    NH_REQUIRE(ray_stride >= 8, "proposal_loss: ray_stride must be at least 8 (far is column 7)");
    NH_REQUIRE(s_coarse >= 1 && s_fine >= 1, "proposal_loss: at least 1 sample per ray in each pass (got %d, %d)", s_coarse, s_fine);
    NH_REQUIRE(s_coarse <= NH_PROPOSAL_MAX_SAMPLES && s_fine <= NH_PROPOSAL_MAX_SAMPLES && s_coarse + s_fine <= NH_PROPOSAL_MAX_SAMPLES,
               "proposal_loss: s_coarse + s_fine may be at most %d samples per ray (got %d + %d)", NH_PROPOSAL_MAX_SAMPLES, s_coarse, s_fine);
    NH_REQUIRE(loss || g_weights_coarse, "proposal_loss: both outputs are NULL");
    // W^ (two doubles) and R (one), one more than the samples each; the coarse edges (fp32, one more); lo and hi (16 bits each).  A
    // binary search over at most 4097 entries ends within the kernel's 13 steps.  Above 64 KiB (s_coarse > ~2000) the launch needs the
    // kernel's dynamic-LDS limit raised: a CU has 160 KiB
    const size_t lds = (size_t)(s_coarse + 1) * 20 + (size_t)(s_fine + 1) * 8 + (((size_t)s_fine * 4 + 7) & ~(size_t)7);
    if (lds > 65536) {
        const int rc = nh_lds_limit(k_proposal_loss, (NH_PROPOSAL_MAX_SAMPLES + 1) * 20 + 64);
        if (rc != NERFHIP_OK) return rc;
    }
    NH_LAUNCH(k_proposal_loss, n, 64, lds, stream, raw_coarse, z_coarse, s_coarse, raw_fine, z_fine, s_fine, rays, ray_stride, n,
              noise_std, noise_coarse, noise_fine, seed, ray_offset, scale, g_loss, loss, g_weights_coarse, accumulate);
    return nh_launch_status("proposal_loss");
}
