// nh_rays.h -- per-ray device arithmetic shared by the unit kernels (elementwise.hip), the fused training-ray selection and
// the camera VJPs (dataio.hip: pose, intrinsics, lens distortion), so that they produce identical bits.
#pragma once
#include "../../include/nerfhip.h"
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
// a ray from its camera direction: d = c2w[:3, :3] dc, o = c2w[:3, 3]
NH_DEVICE void nh_rotate_ray(const float* dc, const float* __restrict__ c2w, int ld, float* o, float* d) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = dc[0] * c2w[c * ld + 0];
        v = v + dc[1] * c2w[c * ld + 1];
        v = v + dc[2] * c2w[c * ld + 2];
        d[c] = v;
        o[c] = c2w[c * ld + 3];
    }
}

// ---- lens distortion (include/nerfhip.h: COLMAP's OPENCV model, kp = (k1, k2, p1, p2)) ---------------------------------------------
// (Fx, Fy) = F(x, y; kp), the distorted image of the normalised point (x, y) (y down), and F's Jacobian [[a, b], [b, d]], which is
// symmetric for this model.  With r2 = x^2 + y^2, rad = 1 + k1 r2 + k2 r2^2 and dr = 2 (k1 + 2 k2 r2) (so that d rad / dx = dr x):
//     Fx = x rad + 2 p1 x y + p2 (r2 + 2 x^2),              Fy = y rad + p1 (r2 + 2 y^2) + 2 p2 x y,
//     a = rad + dr x^2 + 2 p1 y + 6 p2 x,     b = dr x y + 2 p1 x + 2 p2 y,     d = rad + dr y^2 + 6 p1 y + 2 p2 x.
// kp = 0: every product with a coefficient is a zero, so F is (x, y) and J is I, exactly.
NH_DEVICE void nh_distort(const float* kp, float x, float y, float* Fx, float* Fy, float* a, float* b, float* d) {
    const float k1 = kp[0], k2 = kp[1], p1 = kp[2], p2 = kp[3];
    const float xx = x * x, yy = y * y, xy = x * y;
    const float r2 = xx + yy;
    const float rad = (1.0f + k1 * r2) + k2 * (r2 * r2);
    const float dr = 2.0f * (k1 + (2.0f * k2) * r2);
    *Fx = (x * rad + (2.0f * p1) * xy) + p2 * (r2 + 2.0f * xx);
    *Fy = (y * rad + p1 * (r2 + 2.0f * yy)) + (2.0f * p2) * xy;
    *a = ((rad + dr * xx) + (2.0f * p1) * y) + (6.0f * p2) * x;
    *b = (dr * xy + (2.0f * p1) * x) + (2.0f * p2) * y;
    *d = ((rad + dr * yy) + (6.0f * p1) * y) + (2.0f * p2) * x;
}
// the undistorted point (x, y) of the observed (xd, yd): Newton's iteration on F(x, y) = (xd, yd) from (xd, yd), with the analytic
// Jacobian, NERFHIP_UNDISTORT_ITERS steps on every ray -- no data-dependent exit, so a ray's bits depend on its inputs only.  kp = 0:
// the residual is an exact zero and J is I, so every step is x - 0 and (xd, yd) comes back bit for bit.
NH_DEVICE void nh_undistort(const float* kp, float xd, float yd, float* x, float* y) {
    float px = xd, py = yd;
    for (int it = 0; it < NERFHIP_UNDISTORT_ITERS; ++it) {
        float Fx, Fy, a, b, d;
        nh_distort(kp, px, py, &Fx, &Fy, &a, &b, &d);
        const float rx = Fx - xd, ry = Fy - yd;
        const float det = a * d - b * b;
        px = px - (d * rx - b * ry) / det;
        py = py - (a * ry - b * rx) / det;
    }
    *x = px, *y = py;
}
// The gradient through the solve by the implicit-function theorem (nothing is back-propagated through the iterations): (x, y) the
// solution, (xd, yd) the observed point under the intrinsics f, (g0, g1) the cotangent of (x, y); lambda = J^-T (g0, g1) at the
// solution.  t_dist: the ray's terms of d(loss)/d(k1, k2, p1, p2); t_intr: those of d(loss)/d(fx, fy, cx, cy), in the operation order
// of the pin-hole terms (kp = 0: lambda is (g0, g1) and they are the pin-hole terms bit for bit).  Either may be NULL.
NH_DEVICE void nh_undistort_vjp(const float* kp, const float* f, float x, float y, float xd, float yd, float g0, float g1,
                                float* t_dist, float* t_intr) {
    float Fx, Fy, a, b, d;
    nh_distort(kp, x, y, &Fx, &Fy, &a, &b, &d);
    const float det = a * d - b * b;
    const float l0 = (d * g0 - b * g1) / det, l1 = (a * g1 - b * g0) / det;
    if (t_dist) {
        const float xx = x * x, yy = y * y, xy2 = 2.0f * (x * y);
        const float r2 = xx + yy;
        const float lp = l0 * x + l1 * y;
        t_dist[0] = -(r2 * lp);
        t_dist[1] = -((r2 * r2) * lp);
        t_dist[2] = -(l0 * xy2 + l1 * (r2 + 2.0f * yy));
        t_dist[3] = -(l0 * (r2 + 2.0f * xx) + l1 * xy2);
    }
    if (t_intr) {
        t_intr[0] = -(l0 * xd) / f[0];
        t_intr[1] = -(l1 * yd) / f[1];
        t_intr[2] = -l0 / f[0];
        t_intr[3] = -l1 / f[1];
    }
}
// the camera direction of pixel (row, col): the pin-hole one, undistorted under dist (device, k1 k2 p1 p2) when given -- (x, -y, -1)
NH_DEVICE void nh_camera_dir(const float* f, const float* __restrict__ dist, int64_t row, int64_t col, float* dc) {
    nh_pinhole_cam(f[0], f[1], f[2], f[3], row, col, dc);
    if (dist) {
        const float kp[4] = {dist[0], dist[1], dist[2], dist[3]};
        float x, y;
        nh_undistort(kp, dc[0], -dc[1], &x, &y);
        dc[0] = x;
        dc[1] = -y;
    }
}
// one ray of the camera (f, dist)
NH_DEVICE void nh_camera_ray(const float* f, const float* __restrict__ dist, const float* __restrict__ c2w, int ld, int64_t row,
                             int64_t col, float* o, float* d) {
    float dc[3];
    nh_camera_dir(f, dist, row, col, dc);
    nh_rotate_ray(dc, c2w, ld, o, d);
}
// one pin-hole ray
NH_DEVICE void nh_pinhole_ray(const float* f, const float* __restrict__ c2w, int ld, int64_t row, int64_t col, float* o, float* d) {
    nh_camera_ray(f, nullptr, c2w, ld, row, col, o, d);
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

