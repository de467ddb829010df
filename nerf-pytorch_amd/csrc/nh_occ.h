// nh_occ.h -- the occupancy grid on the device (include/nerfhip.h "occupancy grid"): the sample point and its cell, in ONE place.
#pragma once
#include "nh_device.h"

// nerfhip_occ_grid as the kernels take it by value: inv_a = res_a / (hi_a - lo_a), formed once on the host in fp32
struct NhOccGrid {
    const uint32_t* bits;
    float lo[3], inv[3];
    int res[3];
    int outside;
};

// the point the MLP kernels encode for a sample of a packed ray row (mlp16.hip / mlp_f16w.hip / mlp64r.hip: pts = ro + rd * z)
NH_DEVICE void nh_occ_point(const float* rr, float zz, float* px, float* py, float* pz) {
    *px = rr[0] + rr[3] * zz;
    *py = rr[1] + rr[4] * zz;
    *pz = rr[2] + rr[5] * zz;
}

// 1: the cell of point p is occupied.  i_a = (int)floorf((p_a - lo_a) * inv_a); outside the box (i_a < 0 or i_a >= res_a -- decided on
// the floored float, which no conversion can overflow): g.outside; a NaN coordinate: occupied
NH_DEVICE int nh_occ_test(const NhOccGrid& g, float px, float py, float pz) {
    if (px != px || py != py || pz != pz) return 1;
    const float fx = floorf((px - g.lo[0]) * g.inv[0]), fy = floorf((py - g.lo[1]) * g.inv[1]), fz = floorf((pz - g.lo[2]) * g.inv[2]);
    if (!(fx >= 0.0f && fx < (float)g.res[0] && fy >= 0.0f && fy < (float)g.res[1] && fz >= 0.0f && fz < (float)g.res[2]))
        return g.outside ? 1 : 0;
    const unsigned b = ((unsigned)(int)fz * (unsigned)g.res[1] + (unsigned)(int)fy) * (unsigned)g.res[0] + (unsigned)(int)fx;
    return (int)((g.bits[b >> 5] >> (b & 31u)) & 1u);
}
