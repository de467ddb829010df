// nh_rays.h -- per-ray device arithmetic shared by the unit kernels (elementwise.hip), the fused training-ray selection and
// the pose VJP (dataio.hip), so that they produce identical bits.
#pragma once
#include "nh_device.h"

// get_ray_bundle (nerf/nerf_helpers.py:67-110)
// camera-space direction of pixel (row, col) under the intrinsics (fx, fy, cx, cy), in pixels: ((col - cx)/fx, -(row - cy)/fy, -1)
NH_DEVICE void nh_pinhole_cam(float fx, float fy, float cx, float cy, int64_t row, int64_t col, float* dc) {
    float ii = (float)col;  // x
    float jj = (float)row;  // y
    dc[0] = (ii - cx) / fx;
    dc[1] = -(jj - cy) / fy;
    dc[2] = -1.0f;
}
// the reference's camera: one focal, the principal point at the centre of a height x width image -- ((col - W/2)/f, -(row - H/2)/f, -1)
NH_DEVICE void nh_pinhole_cam(int height, int width, float focal, int64_t row, int64_t col, float* dc) {
    nh_pinhole_cam(focal, focal, (float)(width * 0.5), (float)(height * 0.5), row, col, dc);
}
// the four intrinsics of a call: intr (device, fx fy cx cy) when given, else the reference's camera of (height, width, focal)
NH_DEVICE void nh_intrinsics(const float* __restrict__ intr, int height, int width, float focal, float* f) {
    if (intr) {
        f[0] = intr[0], f[1] = intr[1], f[2] = intr[2], f[3] = intr[3];
    } else {
        f[0] = focal, f[1] = focal, f[2] = (float)(width * 0.5), f[3] = (float)(height * 0.5);
    }
}
// one pin-hole ray: d = c2w[:3, :3] dc, o = c2w[:3, 3]
NH_DEVICE void nh_pinhole_ray(const float* f, const float* __restrict__ c2w, int ld, int64_t row, int64_t col, float* o, float* d) {
    float dc[3];
    nh_pinhole_cam(f[0], f[1], f[2], f[3], row, col, dc);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = dc[0] * c2w[c * ld + 0];
        v = v + dc[1] * c2w[c * ld + 1];
        v = v + dc[2] * c2w[c * ld + 2];
        d[c] = v;
        o[c] = c2w[c * ld + 3];
    }
}
NH_DEVICE void nh_pinhole_ray(int height, int width, float focal, const float* __restrict__ c2w, int ld, int64_t row,
                              int64_t col, float* o, float* d) {
    float f[4];
    nh_intrinsics(nullptr, height, width, focal, f);
    nh_pinhole_ray(f, c2w, ld, row, col, o, d);
}

// ndc_rays (nerf/nerf_helpers.py:170-197)
struct NhNdc {
    float near, cw, ch, two_near, neg_two_near;
};
NH_DEVICE void nh_ndc_ray(const NhNdc& k, float* o, float* d) {
    float ox = o[0], oy = o[1], oz = o[2];
    float dx = d[0], dy = d[1], dz = d[2];
    float t = -(k.near + oz) / dz;
    ox = ox + t * dx;
    oy = oy + t * dy;
    oz = oz + t * dz;
    o[0] = k.cw * ox / oz;
    o[1] = k.ch * oy / oz;
    o[2] = 1.0f + k.two_near / oz;
    d[0] = k.cw * (dx / dz - ox / oz);
    d[1] = k.ch * (dy / dz - oy / oz);
    d[2] = k.neg_two_near / oz;
}

// Vector-Jacobian product of nh_ndc_ray at the pre-NDC ray (o, d): the chain rule through its statements in reverse order,
// which is what autograd does to nerf/nerf_helpers.py:170-197 (t = -(near + oz)/dz; p = o + t d; the six outputs are rational
// in p, d).  gO / gD: cotangents of the NDC origin / direction; g_o / g_d: those of the pre-NDC origin / direction.
NH_DEVICE void nh_ndc_ray_vjp(const NhNdc& k, const float* o, const float* d, const float* gO, const float* gD, float* g_o,
                              float* g_d) {
    const float ox = o[0], oy = o[1], oz = o[2];
    const float dx = d[0], dy = d[1], dz = d[2];
    const float gO0 = gO[0], gO1 = gO[1], gO2 = gO[2];
    const float gD0 = gD[0], gD1 = gD[1], gD2 = gD[2];
    const float t = -(k.near + oz) / dz;
    const float px = ox + t * dx, py = oy + t * dy, pz = oz + t * dz;
    const float ipz = 1.0f / pz, idz = 1.0f / dz;
    // outputs -> p, d
    const float ax = k.cw * (gO0 - gD0), ay = k.ch * (gO1 - gD1);  // d/d(px/pz), d/d(py/pz)
    float gpx = ax * ipz, gpy = ay * ipz;
    float gpz = -(ax * px + ay * py + k.two_near * gO2 + k.neg_two_near * gD2) * ipz * ipz;
    float gdx = k.cw * gD0 * idz, gdy = k.ch * gD1 * idz;
    float gdz = -(k.cw * gD0 * dx + k.ch * gD1 * dy) * idz * idz;
    // p = o + t d
    const float gt = gpx * dx + gpy * dy + gpz * dz;
    gdx += t * gpx;
    gdy += t * gpy;
    gdz += t * gpz;
    // t = -(near + oz) / dz
    gpz += -gt * idz;                         // (g wrt oz: through p and through t)
    gdz += gt * (k.near + oz) * idz * idz;
    g_o[0] = gpx;
    g_o[1] = gpy;
    g_o[2] = gpz;
    g_d[0] = gdx;
    g_d[1] = gdy;
    g_d[2] = gdz;
}

// one row of the packed ray batch (nerf/train_utils.py:143-168)
NH_DEVICE void nh_write_ray_row(float* r, const float* o, const float* d, float near, float far, const float* vsrc) {
    r[0] = o[0];
    r[1] = o[1];
    r[2] = o[2];
    r[3] = d[0];
    r[4] = d[1];
    r[5] = d[2];
    r[6] = near;
    r[7] = far;
    if (vsrc) {
        float x = vsrc[0], y = vsrc[1], z = vsrc[2];
        float nrm = sqrtf(fmaf(z, z, fmaf(y, y, x * x)));  // torch's CPU norm(p=2) is this fma chain (bit-exact)
        r[8] = x / nrm;
        r[9] = y / nrm;
        r[10] = z / nrm;
    }
}

