// matte.hip -- the loss of one compositing pass against RGBA targets: the photometric term over a per-ray background (matte mode) or
// under a per-pixel weight (weight mode), the squared error of the accumulated opacity against alpha, and the binary entropy of the
// accumulated opacity; with the cotangents `g_rgb` and `g_acc` that the fused backward takes.  The definition is in include/nerfhip.h
// (nerfhip_matte_loss_fwd_bwd).
//
// k_mse_loss's shape (elementwise.hip): one workgroup of 1024 threads, fp64 sums in a fixed order, no atomics.  Walk 1 is the plain
// kernel's: thread t takes the elements t, t + 1024, ... of the [n][3] colours, so that the photometric sum has mse_loss_body<false>'s
// element-to-thread assignment, and with it the plain kernel's wave sums, block sums and final division (weight mode with a == 1
// everywhere is the plain kernel bit for bit).  Walk 2 is per ray: thread t takes the rays t, t + 1024, ...; it forms the ray's three
// colour cotangents again (the same operations on the same inputs: the same bits, so no exchange between the threads that own a ray's
// three channels in walk 1 is needed) and from them g_acc, and adds the ray's alpha and entropy terms to its sums.
#include <math.h>

#include "../nh_host.h"

#define NH_MATTE_RNG_STREAM 4u  // (nerfhip.h: stream id 4 = background colour)
#define NH_MATTE_EPS 1e-6

// alpha as read: clamped to [0, 1]; a NaN stays a NaN (both comparisons are false)
NH_DEVICE float nh_matte_alpha(const float* __restrict__ tgt, int tstride, int64_t r) {
    const float a = tgt[r * tstride + 3];
    return a < 0.0f ? 0.0f : (a > 1.0f ? 1.0f : a);
}

// background colour c of ray r
NH_DEVICE float nh_matte_bg(const float* __restrict__ bg, int bg_random, float bg_r, float bg_g, float bg_b, uint64_t seed,
                            uint64_t ray_offset, int64_t r, int c) {
    if (bg) return bg[r * 3 + c];
    if (bg_random) return nh_rand_uniform(seed, NH_MATTE_RNG_STREAM, 3 * (ray_offset + (uint64_t)r) + (uint64_t)c);
    return c == 0 ? bg_r : (c == 1 ? bg_g : bg_b);
}

// the colour residual of (ray r, channel c) in matte mode: both composites in fp64 from the fp32 inputs, their difference rounded once
NH_DEVICE float nh_matte_residual(float p, float acc, float C, float a, float b) {
    const double t = (double)a * (double)C + (1.0 - (double)a) * (double)b;
    const double q = (double)p + (1.0 - (double)acc) * (double)b;
    return (float)(q - t);
}

NH_KERNEL void k_matte_loss(const float* __restrict__ rgb, const float* __restrict__ acc, const float* __restrict__ tgt, int tstride,
                            int64_t n, int mode, const float* __restrict__ bg, int bg_random, float bg_r, float bg_g, float bg_b,
                            uint64_t seed, uint64_t ray_offset, float lam_alpha, float lam_entropy, float grad_scale,
                            float* __restrict__ g_rgb, float* __restrict__ g_acc, float* __restrict__ loss_out) {
    NH_SHARED double red[3][16];
    const float k = 2.0f / (float)(3 * n) * grad_scale;  // as k_mse_loss forms it
    const bool matte = mode == 0;
    // walk 1: the photometric sum and g_rgb, the plain kernel's elements in the plain kernel's order
    double sp = 0.0;
    for (int64_t i = threadIdx.x; i < n * 3; i += blockDim.x) {
        const int64_t r = i / 3;
        const int c = (int)(i % 3);
        const float t = tgt[r * tstride + c];
        const float a = nh_matte_alpha(tgt, tstride, r);
        if (matte) {
            const float b = nh_matte_bg(bg, bg_random, bg_r, bg_g, bg_b, seed, ray_offset, r, c);
            const float d = nh_matte_residual(rgb[i], acc[r], t, a, b);
            sp += (double)d * (double)d;
            if (g_rgb) g_rgb[i] = d * k;
        } else {
            const float d = rgb[i] - t;
            sp += (double)a * ((double)d * (double)d);
            if (g_rgb) g_rgb[i] = (d * k) * a;
        }
    }
    // walk 2: per ray -- g_acc, the alpha and the entropy sums.  A term whose weight is exactly 0 is left out (not 0 * inf)
    const bool on_a = lam_alpha != 0.0f, on_h = lam_entropy != 0.0f;
    const double ka = 2.0 * (double)lam_alpha / (double)n * (double)grad_scale;
    const double kh = (double)lam_entropy / (double)n * (double)grad_scale;
    double sa = 0.0, sh = 0.0;
    for (int64_t r = threadIdx.x; r < n; r += blockDim.x) {
        const float a = nh_matte_alpha(tgt, tstride, r);
        const double av = (double)acc[r];
        const double da = av - (double)a;
        if (matte) sa += da * da;
        const bool below = av < NH_MATTE_EPS, above = av > 1.0 - NH_MATTE_EPS;
        const double x = below ? NH_MATTE_EPS : (above ? 1.0 - NH_MATTE_EPS : av);  // (a NaN stays a NaN)
        sh += -(x * log(x) + (1.0 - x) * log(1.0 - x));
        if (!g_acc) continue;
        double g = 0.0;
        if (matte) {
            for (int c = 0; c < 3; ++c) {
                const float b = nh_matte_bg(bg, bg_random, bg_r, bg_g, bg_b, seed, ray_offset, r, c);
                const float d = nh_matte_residual(rgb[r * 3 + c], acc[r], tgt[r * tstride + c], a, b);
                g -= (double)(d * k) * (double)b;
            }
            if (on_a) g += ka * da;
        }
        if (on_h && !(below || above)) g += kh * log((1.0 - x) / x);
        g_acc[r] = (float)g;
    }
    sp = nh_wave_sum_d(sp);
    sa = nh_wave_sum_d(sa);
    sh = nh_wave_sum_d(sh);
    const int w = nh_wave_in_block();
    if (nh_lane() == 0) {
        red[0][w] = sp;
        red[1][w] = sa;
        red[2][w] = sh;
    }
    nh_block_sync();
    if (threadIdx.x == 0) {
        double p = 0.0, a = 0.0, h = 0.0;
        const int nw = (int)(blockDim.x >> 6);
        for (int i = 0; i < nw; ++i) {
            p += red[0][i];
            a += red[1][i];
            h += red[2][i];
        }
        loss_out[0] = (float)(p / (double)(3 * n));
        loss_out[1] = (float)(a / (double)n);
        loss_out[2] = (float)(h / (double)n);
    }
}

extern "C" int nerfhip_matte_loss_fwd_bwd(const float* rgb, const float* acc, const float* target, int target_stride, int64_t n,
                                          int mode, const float* bg, int bg_random, float bg_r, float bg_g, float bg_b, uint64_t seed,
                                          uint64_t ray_offset, float lam_alpha, float lam_entropy, float grad_scale, float* g_rgb,
                                          float* g_acc, float* loss_out, nerfhip_stream_t stream) {
    NH_REQUIRE(n > 0, "matte_loss: n must be positive (got %lld)", (long long)n);
    NH_REQUIRE(target_stride >= 4, "matte_loss: target_stride must be at least 4 (a row is r, g, b, alpha; got %d)", target_stride);
    NH_REQUIRE(rgb, "matte_loss: rgb is NULL");
    NH_REQUIRE(acc, "matte_loss: acc is NULL");
    NH_REQUIRE(target, "matte_loss: target is NULL");
    NH_REQUIRE(loss_out, "matte_loss: loss_out is NULL");
    NH_REQUIRE(mode == 0 || mode == 1, "matte_loss: mode must be 0 (matte) or 1 (weight) (got %d)", mode);
    NH_REQUIRE(isfinite(lam_alpha) && lam_alpha >= 0.0f, "matte_loss: lam_alpha must be finite and not negative");
    NH_REQUIRE(isfinite(lam_entropy) && lam_entropy >= 0.0f, "matte_loss: lam_entropy must be finite and not negative");
    NH_REQUIRE(mode == 0 || lam_alpha == 0.0f, "matte_loss: lam_alpha must be 0 in weight mode (alpha is a loss weight there, not an opacity)");
    NH_LAUNCH(k_matte_loss, 1, 1024, 0, stream, rgb, acc, target, target_stride, n, mode, bg, bg_random, bg_r, bg_g, bg_b, seed,
              ray_offset, lam_alpha, lam_entropy, grad_scale, g_rgb, g_acc, loss_out);
    return nh_launch_status("matte_loss");
}
