// robust.hip -- the photometric loss of one compositing pass under a robust kind (l2, l1, Huber, Charbonnier, RawNeRF's relative error)
// with an optional trim of the batch's largest per-ray residuals, and its cotangent `g_rgb` for the fused backward.  The definition is
// in include/nerfhip.h (nerfhip_robust_loss_fwd_bwd).
//
// k_mse_loss's shape (elementwise.hip): one workgroup of 1024 threads, fp64 sums in a fixed order, no atomics.  Three phases:
//   1. the per-ray walk (only with a trim, or where resid_out / mask_out are asked for): thread t takes the rays t, t + 1024, ...
//      and forms e_r = (float) sum_c rho(d_c) into tmp (and resid_out);
//   2. the selection (only with a trim): tau, the kk-th smallest e_r.  A non-negative float's bits order as unsigned integers, so tau
//      is the largest T with |{r : bits(e_r) < T}| <= kk - 1, found one bit per round from bit 30 down: 31 block-wide counts (integer
//      wave sums, 16 words of LDS, one barrier a round over two alternating rows).  Exact and independent of scheduling.  A thread
//      counts the rays it wrote in phase 1; the first NH_ROBUST_KREG of them stay in registers (all of them up to 4096 rays), so that
//      a round reads no memory.  A NaN residual's key is the quiet NaN's (it sorts behind +inf), and !(NaN > tau) keeps its ray;
//   3. the plain kernel's element walk under the mask m_r = !(e_r > tau) read back from tmp: thread t takes the elements t, t + 1024,
//      ... of the [n][3] colours -- mse_loss_body<false>'s element-to-thread assignment, and with it the plain kernel's wave sums,
//      block sums and final division (kind 0 without a trim is the plain kernel bit for bit).
#include <math.h>

#include "../nh_host.h"

#define NH_ROBUST_KREG 4
#define NH_ROBUST_NAN_KEY 0x7fc00000u

enum { NH_ROBUST_L2 = 0, NH_ROBUST_L1 = 1, NH_ROBUST_HUBER = 2, NH_ROBUST_CHARBONNIER = 3, NH_ROBUST_RELATIVE = 4 };

// rho(d) in fp64 from the fp32 d (p: the rendered colour, read by the relative kind only)
NH_DEVICE double nh_robust_rho(int kind, float d, float p, float param) {
    const double x = (double)d, a = fabs(x), q = (double)param;
    switch (kind) {
        case NH_ROBUST_L1: return a;
        case NH_ROBUST_HUBER: return a <= q ? x * x : q * (2.0 * a - q);
        case NH_ROBUST_CHARBONNIER: return sqrt(x * x + q * q) - q;
        case NH_ROBUST_RELATIVE: {
            const double s = (double)p + q;
            return (x * x) / (s * s);
        }
        default: return x * x;
    }
}

// h(d) = psi(d) / 2, formed in fp64 and rounded to fp32 once (a NaN d stays a NaN in every kind)
NH_DEVICE float nh_robust_h(int kind, float d, float p, float param) {
    const double x = (double)d, q = (double)param;
    switch (kind) {
        case NH_ROBUST_L1: return d > 0.0f ? 0.5f : (d < 0.0f ? -0.5f : d);
        case NH_ROBUST_HUBER: return fabs(x) <= q ? d : (d > 0.0f ? param : (d < 0.0f ? -param : d));
        case NH_ROBUST_CHARBONNIER: return (float)(0.5 * x / sqrt(x * x + q * q));
        case NH_ROBUST_RELATIVE: {
            const double s = (double)p + q;
            return (float)(x / (s * s));
        }
        default: return d;
    }
}

// the per-ray residual e_r, non-negative (or NaN)
NH_DEVICE float nh_robust_residual(const float* __restrict__ rgb, const float* __restrict__ tgt, int tstride, int64_t r, int kind,
                                   float param) {
    double e = 0.0;
    for (int c = 0; c < 3; ++c) {
        const float p = rgb[r * 3 + c];
        e += nh_robust_rho(kind, p - tgt[r * tstride + c], p, param);
    }
    return (float)e;
}

NH_DEVICE unsigned nh_robust_key(float e) {
    unsigned u;
    memcpy(&u, &e, 4);
    return e != e ? NH_ROBUST_NAN_KEY : u;
}

// the sum of v over the workgroup, in every thread (row: 16 words of LDS that no thread still reads)
NH_DEVICE int64_t nh_robust_block_count(int v, int* row) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += nh_shfl_xor_i(v, m);
    if (nh_lane() == 0) row[nh_wave_in_block()] = v;
    nh_block_sync();
    int64_t s = 0;
    const int nw = (int)(blockDim.x >> 6);
    for (int i = 0; i < nw; ++i) s += row[i];
    return s;
}

NH_KERNEL void k_robust_loss(const float* __restrict__ rgb, const float* __restrict__ tgt, int tstride, int64_t n, int kind, float param,
                             int64_t kk, float grad_scale, float* __restrict__ g_rgb, float* __restrict__ resid_out,
                             unsigned char* __restrict__ mask_out, float* __restrict__ loss_out, float* __restrict__ tmp) {
    NH_SHARED double red[16];
    NH_SHARED int cnt[2][16];
    const float k = 2.0f / (float)(3 * n) * grad_scale;  // as k_mse_loss forms it
    const bool trim = kk > 0;
    const int64_t step = blockDim.x;
    float tau = INFINITY;
    int64_t kept = n;
    if (trim || resid_out || mask_out) {
        // phase 1: per ray
        unsigned kreg[NH_ROBUST_KREG];
#pragma unroll
        for (int j = 0; j < NH_ROBUST_KREG; ++j) kreg[j] = 0xffffffffu;  // (no ray: below no candidate)
        for (int64_t r = threadIdx.x, j = 0; r < n; r += step, ++j) {
            const float e = nh_robust_residual(rgb, tgt, tstride, r, kind, param);
            if (trim) tmp[r] = e;
            if (resid_out) resid_out[r] = e;
            if (mask_out && !trim) mask_out[r] = 1;
#pragma unroll
            for (int u = 0; u < NH_ROBUST_KREG; ++u)
                if (j == u) kreg[u] = nh_robust_key(e);
        }
        if (trim) {
            // phase 2: the kk-th smallest key, one bit a round
            unsigned T = 0u;
            for (int bit = 30; bit >= 0; --bit) {
                const unsigned c = T | (1u << bit);
                int mine = 0;
#pragma unroll
                for (int u = 0; u < NH_ROBUST_KREG; ++u) mine += kreg[u] < c ? 1 : 0;
                for (int64_t r = (int64_t)threadIdx.x + NH_ROBUST_KREG * step; r < n; r += step) mine += nh_robust_key(tmp[r]) < c ? 1 : 0;
                if (nh_robust_block_count(mine, cnt[bit & 1]) <= kk - 1) T = c;
            }
            memcpy(&tau, &T, 4);
            int mine = 0;
            for (int64_t r = threadIdx.x; r < n; r += step) {
                const int m = !(tmp[r] > tau);
                mine += m;
                if (mask_out) mask_out[r] = (unsigned char)m;
            }
            kept = nh_robust_block_count(mine, cnt[1]);  // (round 0 used row 0; this barrier also orders tmp ahead of phase 3)
        }
    }
    // phase 3: the plain kernel's elements in the plain kernel's order
    double sp = 0.0;
    for (int64_t i = threadIdx.x; i < n * 3; i += step) {
        const int64_t r = i / 3;
        const int c = (int)(i % 3);
        const float t = tgt[r * tstride + c];
        const float p = rgb[i];
        const float d = p - t;
        const bool m = !trim || !(tmp[r] > tau);
        if (m) sp += nh_robust_rho(kind, d, p, param);
        if (g_rgb) g_rgb[i] = m ? nh_robust_h(kind, d, p, param) * k : 0.0f;
    }
    sp = nh_wave_sum_d(sp);
    const int w = nh_wave_in_block();
    if (nh_lane() == 0) red[w] = sp;
    nh_block_sync();
    if (threadIdx.x == 0) {
        double a = 0.0;
        const int nw = (int)(blockDim.x >> 6);
        for (int i = 0; i < nw; ++i) a += red[i];
        loss_out[0] = (float)(a / (double)(3 * n));
        loss_out[1] = (float)((double)kept / (double)n);
        loss_out[2] = tau;
    }
}

extern "C" int64_t nerfhip_robust_loss_tmp_bytes(int64_t n) { return n > 0 ? 4 * n : 0; }

extern "C" int nerfhip_robust_loss_fwd_bwd(const float* rgb, const float* target, int target_stride, int64_t n, int kind, float param,
                                           float keep, float grad_scale, float* g_rgb, float* resid_out, unsigned char* mask_out,
                                           float* loss_out, void* tmp, int64_t tmp_bytes, nerfhip_stream_t stream) {
    NH_REQUIRE(n > 0 && n < ((int64_t)1 << 31), "robust_loss: n must be positive and below 2^31 (got %lld)", (long long)n);
    NH_REQUIRE(target_stride >= 3, "robust_loss: target_stride must be at least 3 (got %d)", target_stride);
    NH_REQUIRE(rgb, "robust_loss: rgb is NULL");
    NH_REQUIRE(target, "robust_loss: target is NULL");
    NH_REQUIRE(loss_out, "robust_loss: loss_out is NULL");
    NH_REQUIRE(kind >= NH_ROBUST_L2 && kind <= NH_ROBUST_RELATIVE,
               "robust_loss: kind must be 0 (l2), 1 (l1), 2 (huber), 3 (charbonnier) or 4 (relative) (got %d)", kind);
    NH_REQUIRE(kind < NH_ROBUST_HUBER || (isfinite(param) && param > 0.0f),
               "robust_loss: param (huber's delta, charbonnier's and relative's eps) must be finite and positive");
    NH_REQUIRE(keep > 0.0f && keep <= 1.0f, "robust_loss: keep must lie in (0, 1]");
    int64_t kk = 0;  // (0: no trim)
    if (keep < 1.0f) {
        NH_REQUIRE(tmp, "robust_loss: tmp is NULL (keep < 1 needs nerfhip_robust_loss_tmp_bytes(n) bytes)");
        NH_REQUIRE(((uintptr_t)tmp & 3u) == 0, "robust_loss: tmp must be aligned to 4 bytes");
        NH_REQUIRE(tmp_bytes >= nerfhip_robust_loss_tmp_bytes(n), "robust_loss: tmp_bytes is %lld, keep < 1 needs %lld", (long long)tmp_bytes,
                   (long long)nerfhip_robust_loss_tmp_bytes(n));
        kk = (int64_t)ceil((double)keep * (double)n);
        kk = kk < 1 ? 1 : (kk > n ? n : kk);
    }
    NH_LAUNCH(k_robust_loss, 1, 1024, 0, stream, rgb, target, target_stride, n, kind, param, kk, grad_scale, g_rgb, resid_out, mask_out,
              loss_out, (float*)tmp);
    return nh_launch_status("robust_loss");
}
