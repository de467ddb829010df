// nh_render.h -- the per-sample quantities of the compositing, shared by the kernels that form the ray weights (render.hip,
// reg/spread.hip): one definition, so that every one of them sees the same alpha bit for bit.
#pragma once
#include "nh_device.h"

struct RenderSample {
    float alpha, b, e, dist, sig_in;
};

// per-sample quantities of lines :17-39 of the reference
NH_DEVICE RenderSample nh_render_sample(const float* __restrict__ raw, const float* __restrict__ z, int64_t ray, int s,
                                        int i, float norm, float noise_std, const float* __restrict__ noise,
                                        uint64_t seed, uint32_t rng_stream, uint64_t ray_offset) {
    RenderSample r;
    int64_t g = ray * s + i;
    float zi = z[g];
    float d = (i + 1 < s) ? (z[g + 1] - zi) : 1e10f;
    r.dist = d * norm;
    float nz = 0.0f;
    if (noise_std > 0.0f) {
        float dr = noise ? noise[g] : nh_rand_normal(seed, rng_stream, (ray_offset + (uint64_t)ray) * (uint64_t)s + i);
        nz = dr * noise_std;
    }
    r.sig_in = raw[g * 4 + 3] + nz;
    float sigma = r.sig_in > 0.0f ? r.sig_in : 0.0f;
    if (r.sig_in != r.sig_in) sigma = r.sig_in;  // relu propagates NaN
    r.e = expf(-sigma * r.dist);
    r.alpha = 1.0f - r.e;
    r.b = 1.0f - r.alpha + 1e-10f;
    return r;
}
