// nh_raygrad.h -- kernels and launches of fused.hip's frozen ray gradient, included by fused.hip alone (a header, not a translation
// unit of its own: the product's list of .hip files is pinned by tests/test_host_abi.py).
// d(loss)/d(rays) of a render backward whose nets are frozen (nerfhip_render_grad_rays, fused.hip), from the
// d(pre-activation) images the data-gradient chain left in the backward scratch, without the [M][Dx + Dd] temporary of
// nerfhip_mlp_bwd_input:
//   k_point_grad_pack  the weight slices that multiply the encoded input (layer1, every skip layer's trailing Dx columns,
//                      layers_dir.0's trailing Dd columns), gathered from the flat vector into transposed, zero-padded
//                      [slot][unit] images -- one contiguous LDS copy each;
//   k_point_grad       per image row: G_enc = sum over terms of P_term . W_term on v_mfma_f32_16x16x4_f32, the positional
//                      encoding's VJP on the accumulators, one 32-byte store {g_p[3], g_v[3], 0, 0} per sample;
//   k_ray_grad_sum     one wavefront per ray: the sum over its samples, in k_ray_grad's order (render.hip).
//
// Layout (DESIGN.md section 2's vocabulary).  A wave owns 16 image rows; lane l = (j = l & 15: row, g = l >> 4: k-group).
// B operand: the lane's own 16-byte load of units 16 q + 4 g .. + 3 of its row, element s used in k-step s; A operand:
// Wt[slot 16 t + j][the same four units] from LDS.  Accumulator register c of tile t in lane (j, g) is then slot
// 16 t + 4 g + c of row j: a lane holds whole QUADS of slots, and the slots are numbered so that a quad is
//   {sin, cos of pair 2 Q, sin, cos of pair 2 Q + 1},  pair p = (frequency p / 3, axis p % 3),  Q < ceil(3 L / 2),
// followed (include_input) by one quad {x, y, z, -}; slots beyond carry zero weights.  The VJP of a quad needs nothing from
// another lane; the four k-groups of a row are then added by two nh_shfl_xor steps (16, 32) in a fixed order.
// INVARIANT: a sample's eight floats depend only on its image row, its ray and its depth -- never on the slot of the
// wave tile, the workgroup or the launch geometry that computed them (every sum is a fixed chain over that row alone).
#pragma once
#include "nh_mlp.h"

namespace {

constexpr int NH_PG_MAX_TERMS = 2 * (NH_MAX_LAYERS + 2);  // (as nerfhip_mlp_bwd_input: 512-wide nets have one term per 256-row half)
constexpr int NH_PG_TX = 4, NH_PG_TD = 2;                 // 16-slot tiles of the xyz / direction encodings ...
constexpr int NH_PG_TX_EXT = 7, NH_PG_TD_EXT = 4;         // ... and with the extended encoding registers (L_xyz <= 16, L_dir <= 10)
constexpr int NH_PG_WAVES = 8, NH_PG_ROWS = 16 * NH_PG_WAVES;
constexpr int NH_PG_LDS_BUDGET = 160 * 1024;

struct PGTerm {
    int64_t img_off;  // floats from the scratch to the term's d(pre-activation) region
    int64_t wt_off;   // floats from the weight images' base to this term's [slots][stride] image
    int64_t w_off;    // flat offset of the weight tensor's row of the term's first unit
    int a_rows;       // floats per image row
    int nu, nq;       // real units; 16-unit chunks (the last one masked beyond nu)
    int stride;       // floats per slot row of the image: 16 nq + 4 (the + 4 spreads the lanes' 16-byte reads over the banks)
    int wt_floats;    // slots * stride, rounded up to whole 1-KiB wave copies
    int lds_off;      // floats from the LDS base (resident images), 0 when streamed
    int w_ld, col0;   // the tensor's column count, its first column that multiplies the encoding
    int dir;          // 0: an xyz term, 1: the direction term
};

struct PointGradArgs {
    PGTerm t[NH_PG_MAX_TERMS];
    int nterms, resident;
    const float* scratch;
    const float* wt;      // the weight images (k_point_grad_pack)
    const float* pairf;   // frequency of pair p: [8 TX] xyz, then [8 TD] direction (0: no such pair)
    int qin_x, qin_d;     // quad of the include_input columns, or -1
    int64_t M;
    const int* cidx;      // compacted images: row r belongs to sample cidx[r], r < cstats[NH_CSTAT_ACTIVE]
    const int* cstats;
    const float* rays;
    int ray_stride, view;
    const float* z;
    int S;
    float* out;           // [M][8]
};

struct PackArgs {
    PGTerm t[NH_PG_MAX_TERMS];
    int nterms, slots_x, slots_d;
    int64_t total;        // floats of all images
    const float* params;
    float* wt;
    float* pairf_out;
    int npairf;
    int col_x[16 * NH_PG_TX_EXT], col_d[16 * NH_PG_TD_EXT];  // slot -> column of the encoding, or -1
    float pairf[8 * (NH_PG_TX_EXT + NH_PG_TD_EXT)];
};

NH_KERNEL void k_point_grad_pack(PackArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < a.npairf) a.pairf_out[idx] = a.pairf[idx];
    if (idx >= a.total) return;
    int k = 0;
    while (k + 1 < a.nterms && idx >= a.t[k + 1].wt_off) ++k;
    const PGTerm& t = a.t[k];
    const int e = (int)(idx - t.wt_off);
    const int slot = e / t.stride, u = e - slot * t.stride;
    float v = 0.0f;
    if (slot < (t.dir ? a.slots_d : a.slots_x) && u < t.nu) {
        const int c = t.dir ? a.col_d[slot] : a.col_x[slot];
        if (c >= 0) v = a.params[t.w_off + (int64_t)u * t.w_ld + t.col0 + c];
    }
    a.wt[idx] = v;
}

NH_KERNEL void k_point_grad_zero(float* out, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) nh_store4(out + 4 * i, 0.0f, 0.0f, 0.0f, 0.0f);
}

// one term's image -> LDS: whole 1-KiB wave copies (the image is padded to them)
NH_DEVICE void pg_stage(const PointGradArgs& a, const PGTerm& t, float* dst, int wave, int lane) {
    const int bytes = t.wt_floats * 4;
    const NhDmaSrc src = nh_dma_src(a.wt + t.wt_off, (unsigned)bytes);
    for (int off = wave * 1024; off < bytes; off += NH_PG_WAVES * 1024) nh_dma16(src, lane * 16, off, dst + off / 4);
}

// acc[t] += Wt[16 t + j][u] * P[row j][u] over the term's units
template <int T>
NH_DEVICE void pg_gemm(f32x4 (&acc)[T], const float* dp, const float* w, const PGTerm& t, int g) {
    for (int q = 0; q < t.nq; ++q) {
        float4 b = *(const float4*)(dp + 16 * q);
        if (16 * q + 16 > t.nu) {  // (the padded rows of a region are not multiplied)
            const int u = 16 * q + 4 * g;
            b.x = u < t.nu ? b.x : 0.0f;
            b.y = u + 1 < t.nu ? b.y : 0.0f;
            b.z = u + 2 < t.nu ? b.z : 0.0f;
            b.w = u + 3 < t.nu ? b.w : 0.0f;
        }
        float4 av[T];
#pragma unroll
        for (int i = 0; i < T; ++i) av[i] = *(const float4*)(w + (size_t)(16 * i) * t.stride + 16 * q);
#pragma unroll
        for (int i = 0; i < T; ++i) acc[i] = nh_mfma16(av[i].x, b.x, acc[i]);
#pragma unroll
        for (int i = 0; i < T; ++i) acc[i] = nh_mfma16(av[i].y, b.y, acc[i]);
#pragma unroll
        for (int i = 0; i < T; ++i) acc[i] = nh_mfma16(av[i].z, b.z, acc[i]);
#pragma unroll
        for (int i = 0; i < T; ++i) acc[i] = nh_mfma16(av[i].w, b.w, acc[i]);
    }
}

// the positional encoding's VJP on the quads this lane holds: dL/dv_c += f (cos(f v_c) g_sin - sin(f v_c) g_cos), + the raw columns
template <int T>
NH_DEVICE void pg_vjp(const f32x4 (&acc)[T], const float (&fq)[T][2], int qin, int g, float v0, float v1, float v2, float* o0,
                      float* o1, float* o2) {
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if (4 * t + g == qin) {
            s0 += acc[t][0];
            s1 += acc[t][1];
            s2 += acc[t][2];
        } else {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int axis = (8 * t + 2 * g + e) % 3;
                const float v = axis == 0 ? v0 : (axis == 1 ? v1 : v2);
                float sn, cs;
                nh_sincos(v * fq[t][e], &sn, &cs);
                const float d = fq[t][e] * (cs * acc[t][2 * e] - sn * acc[t][2 * e + 1]);
                s0 += axis == 0 ? d : 0.0f;
                s1 += axis == 1 ? d : 0.0f;
                s2 += axis == 2 ? d : 0.0f;
            }
        }
    }
    *o0 = s0, *o1 = s1, *o2 = s2;
}

NH_DEVICE float pg_sum_groups(float v) {
    v += nh_shfl_xor(v, 16);
    v += nh_shfl_xor(v, 32);
    return v;
}

template <int TX, int TD>
NH_KERNEL void NH_LB(64 * NH_PG_WAVES, 2) k_point_grad(PointGradArgs a) {
    NH_DYN_LDS(lds_raw);
    float* const lds = (float*)lds_raw;
    const int lane = nh_lane(), wave = nh_wave_in_block(), j = lane & 15, g = lane >> 4;
    const int64_t rows = a.cidx ? (int64_t)nh_uload_i32(a.cstats, NH_CSTAT_ACTIVE) : a.M;
    const int64_t nblk = (rows + NH_PG_ROWS - 1) / NH_PG_ROWS;
    if ((int64_t)blockIdx.x >= nblk) return;  // (workgroups behind the list: before LDS is touched)
    float fx[TX][2], fd[TD][2];
#pragma unroll
    for (int t = 0; t < TX; ++t) fx[t][0] = a.pairf[8 * t + 2 * g], fx[t][1] = a.pairf[8 * t + 2 * g + 1];
#pragma unroll
    for (int t = 0; t < TD; ++t) fd[t][0] = a.pairf[8 * TX + 8 * t + 2 * g], fd[t][1] = a.pairf[8 * TX + 8 * t + 2 * g + 1];
    if (a.resident) {
        for (int k = 0; k < a.nterms; ++k) pg_stage(a, a.t[k], lds + a.t[k].lds_off, wave, lane);
        nh_wait_vmem();
        nh_block_sync();
    }
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t r = blk * NH_PG_ROWS + wave * 16 + j;  // (rows up to the next multiple of 128 exist in every region)
        f32x4 ax[TX], ad[TD];
#pragma unroll
        for (int t = 0; t < TX; ++t) ax[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < TD; ++t) ad[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int k = 0; k < a.nterms; ++k) {
            const PGTerm& t = a.t[k];
            if (!a.resident) {  // streamed: one term's image at a time, behind a barrier
                nh_block_sync();
                pg_stage(a, t, lds, wave, lane);
                nh_wait_vmem();
                nh_block_sync();
            }
            const float* const w = lds + t.lds_off + (size_t)j * t.stride + 4 * g;
            const float* const dp = a.scratch + t.img_off + (size_t)r * (size_t)t.a_rows + 4 * g;
            if (t.dir)
                pg_gemm<TD>(ad, dp, w, t, g);
            else
                pg_gemm<TX>(ax, dp, w, t, g);
        }
        const bool live = r < rows;
        const int64_t m = live ? (a.cidx ? (int64_t)a.cidx[r] : r) : 0;
        const float* const rr = a.rays + (size_t)(m / a.S) * a.ray_stride;
        const float zz = a.z[m];
        // pts = ro + rd * z, as the forward forms it
        const float px = rr[0] + rr[3] * zz, py = rr[1] + rr[4] * zz, pz = rr[2] + rr[5] * zz;
        float gp0, gp1, gp2, gv0 = 0.0f, gv1 = 0.0f, gv2 = 0.0f;
        pg_vjp<TX>(ax, fx, a.qin_x, g, px, py, pz, &gp0, &gp1, &gp2);
        if (a.view) pg_vjp<TD>(ad, fd, a.qin_d, g, rr[8], rr[9], rr[10], &gv0, &gv1, &gv2);
        gp0 = pg_sum_groups(gp0), gp1 = pg_sum_groups(gp1), gp2 = pg_sum_groups(gp2);
        gv0 = pg_sum_groups(gv0), gv1 = pg_sum_groups(gv1), gv2 = pg_sum_groups(gv2);
        if (live && g == 0) {
            float* const o = a.out + m * 8;
            nh_store4(o, gp0, gp1, gp2, gv0);
            nh_store4(o + 4, gv1, gv2, 0.0f, 0.0f);
        }
    }
}

struct RaySumArgs {
    const float* rays;
    int stride;
    const float* z;
    int S, view;
    const float* pg;  // [n * S][8]
    const float* g_norm;
    float* g_rays;
    int accumulate;
};

// k_ray_grad's sum and tail (render.hip) over the [M][8] buffer: the same lane walk, the same tree
NH_KERNEL void k_ray_grad_sum(RaySumArgs a) {
    const int64_t ray = blockIdx.x;
    const int lane = nh_lane();
    const float* rr = a.rays + ray * a.stride;
    const float d[3] = {rr[3], rr[4], rr[5]};
    float go[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f}, gv[3] = {0.f, 0.f, 0.f};
    for (int i = lane; i < a.S; i += 64) {
        const int64_t m = ray * a.S + i;
        const float zz = a.z[m];
        const float4 p = *(const float4*)(a.pg + m * 8), q = *(const float4*)(a.pg + m * 8 + 4);
        const float gp[3] = {p.x, p.y, p.z}, gq[3] = {p.w, q.x, q.y};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            go[c] += gp[c];
            gd[c] += gp[c] * zz;
            if (a.view) gv[c] += gq[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        go[c] = nh_wave_sum(go[c]);
        gd[c] = nh_wave_sum(gd[c]);
        gv[c] = nh_wave_sum(gv[c]);
    }
    if (lane == 0) {
        float* out = a.g_rays + ray * a.stride;
        const float norm = sqrtf(fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0])));
        const float gn = a.g_norm ? a.g_norm[ray] : 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float dirterm = gd[c] + (norm > 0.0f ? gn * d[c] / norm : 0.0f);
            if (a.accumulate) {
                out[c] += go[c];
                out[3 + c] += dirterm;
                if (a.view) out[8 + c] += gv[c];
            } else {
                out[c] = go[c];
                out[3 + c] = dirterm;
                if (a.view) out[8 + c] = gv[c];
            }
        }
        if (!a.accumulate) {
            out[6] = 0.0f;
            out[7] = 0.0f;
            for (int c = (a.view ? 11 : 8); c < a.stride; ++c) out[c] = 0.0f;
        }
    }
}

// slot -> column of one encoding ([x | sin(f0 x) | cos(f0 x) | sin(f1 x) | ...], nerf/nerf_helpers.py:130-157) and the pair
// frequencies, for `tiles` 16-slot tiles; returns the include_input quad (or -1)
int pg_slots(int L, bool inc, const float* freqs, int tiles, int* col, float* pairf) {
    const int npairs = 3 * L, nqp = (npairs + 1) / 2, qin = inc ? nqp : -1;
    for (int s = 0; s < 16 * tiles; ++s) {
        const int Q = s >> 2, c = s & 3, p = 2 * Q + (c >> 1);
        col[s] = -1;
        if (Q < nqp && p < npairs) col[s] = (inc ? 3 : 0) + 6 * (p / 3) + ((c & 1) ? 3 : 0) + p % 3;
        if (Q == qin && c < 3) col[s] = c;
    }
    for (int p = 0; p < 8 * tiles; ++p) pairf[p] = p < npairs ? freqs[p / 3] : 0.0f;
    return qin;
}

struct PGLayout {
    PGTerm t[NH_PG_MAX_TERMS];
    int nterms;
    bool ext, resident;
    int lds_bytes;
    int64_t wt_floats;  // all images
};

// the term list nerfhip_mlp_bwd_input builds (mlp.hip), with each term's weight image and its place in LDS
PGLayout pg_layout(const nerfhip_plan* p, int64_t M) {
    PGLayout y;
    memset(&y, 0, sizeof(y));
    const int H = p->H, Lx = p->cfg.num_encoding_fn_xyz, Ld = p->view ? p->cfg.num_encoding_fn_dir : 0;
    const bool dir = p->view && p->Dd > 0;
    auto quads = [](int L, bool inc) { return (3 * L + 1) / 2 + (inc ? 1 : 0); };
    y.ext = quads(Lx, p->cfg.include_input_xyz) > 4 * NH_PG_TX || (dir && quads(Ld, p->cfg.include_input_dir) > 4 * NH_PG_TD);
    const int slots_x = 16 * (y.ext ? NH_PG_TX_EXT : NH_PG_TX), slots_d = 16 * (y.ext ? NH_PG_TD_EXT : NH_PG_TD);
    const int64_t nt = nh_ceil_div(M, 128) * 4;
    auto add = [&](const NhRegion& R, int nu, int tensor, int col0, int is_dir) {
        for (int u0 = 0; u0 < nu; u0 += 256) {
            PGTerm& t = y.t[y.nterms++];
            t.img_off = 32 * nt * (R.row_prefix + u0);
            t.a_rows = R.rows;
            t.nu = nu - u0 < 256 ? nu - u0 : 256;
            t.nq = (t.nu + 15) / 16;
            t.stride = 16 * t.nq + 4;
            t.wt_floats = (int)(nh_ceil_div((int64_t)(is_dir ? slots_d : slots_x) * t.stride, 256) * 256);
            t.w_ld = p->tensors[tensor].cols;
            t.w_off = p->tensors[tensor].off + (int64_t)u0 * t.w_ld;
            t.col0 = col0;
            t.dir = is_dir;
            t.wt_off = y.wt_floats;
            y.wt_floats += t.wt_floats;
        }
    };
    add(p->grad.P[0], H, p->t_layer1_w, 0, 0);
    for (int i = 0; i < p->L - 1; ++i)
        if (p->is_skip(i)) add(p->grad.P[i + 1], H, p->t_xyz_w[i], H, 0);
    if (dir) add(p->grad.PDIR, H / 2, p->t_dir_w, H, 1);
    y.resident = y.wt_floats * 4 <= NH_PG_LDS_BUDGET;
    int largest = 0;
    for (int k = 0; k < y.nterms; ++k) {
        y.t[k].lds_off = y.resident ? (int)y.t[k].wt_off : 0;
        if (y.t[k].wt_floats > largest) largest = y.t[k].wt_floats;
    }
    y.lds_bytes = y.resident ? (int)y.wt_floats * 4 : largest * 4;
    return y;
}

constexpr int NH_PG_PAIRF = 8 * (NH_PG_TX_EXT + NH_PG_TD_EXT);

}  // namespace

// tmp of one pass over M sample points: the [M][8] buffer, the weight images, the pair frequencies
static int64_t nh_point_grad_tmp_bytes(const nerfhip_plan* p, int64_t M) {
    return (M * 8 + pg_layout(p, M).wt_floats + NH_PG_PAIRF) * (int64_t)sizeof(float);
}

// per sample {dL/d(point)[3], dL/d(viewdir)[3], 0, 0} into tmp[M][8] from the d(pre-activation) images in `scratch` (cx: their list, or
// NULL: sample order) and the flat parameters; tmp also takes the transposed weight slices
static int nh_point_grad(nerfhip_plan* p, const float* params, int64_t M, const float* scratch, const NhCompact* cx, const float* rays,
                  int ray_stride, const float* z, int S, float* tmp, nerfhip_stream_t stream) {
    NH_REQUIRE(p && params && scratch && rays && z && tmp && M > 0 && S > 0, "point_grad: bad arguments");
    NH_REQUIRE(p->freqs_set, "point_grad: nerfhip_plan_set_freqs has not been called");
    const PGLayout y = pg_layout(p, M);
    NH_REQUIRE(y.lds_bytes <= NH_PG_LDS_BUDGET, "point_grad: a weight slice of %d bytes does not fit the LDS", y.lds_bytes);
    float* const out = tmp;
    float* const wt = tmp + M * 8;
    float* const pairf = wt + y.wt_floats;
    const int tx = y.ext ? NH_PG_TX_EXT : NH_PG_TX, td = y.ext ? NH_PG_TD_EXT : NH_PG_TD;
    const bool dir = p->view && p->Dd > 0;
    PackArgs k;
    memset(&k, 0, sizeof(k));
    memcpy(k.t, y.t, sizeof(k.t));
    k.nterms = y.nterms;
    k.slots_x = 16 * tx, k.slots_d = 16 * td;
    k.total = y.wt_floats;
    k.params = params;
    k.wt = wt;
    k.pairf_out = pairf;
    k.npairf = 8 * (tx + td);
    const int qin_x = pg_slots(p->cfg.num_encoding_fn_xyz, p->cfg.include_input_xyz != 0, p->freqs_xyz, tx, k.col_x, k.pairf);
    const int qin_d = pg_slots(dir ? p->cfg.num_encoding_fn_dir : 0, dir && p->cfg.include_input_dir, p->freqs_dir, td, k.col_d, k.pairf + 8 * tx);
    NH_LAUNCH(k_point_grad_pack, nh_ceil_div(y.wt_floats, 256), 256, 0, stream, k);
    int rc = nh_launch_status("point_grad_pack");
    if (rc) return rc;
    PointGradArgs a;
    memset(&a, 0, sizeof(a));
    memcpy(a.t, y.t, sizeof(a.t));
    a.nterms = y.nterms;
    a.resident = y.resident ? 1 : 0;
    a.scratch = scratch;
    a.wt = wt;
    a.pairf = pairf;
    a.qin_x = qin_x, a.qin_d = dir ? qin_d : -1;
    a.M = M;
    a.rays = rays;
    a.ray_stride = ray_stride;
    a.view = dir ? 1 : 0;
    a.z = z;
    a.S = S;
    a.out = out;
    if (cx) {  // images in list order: the samples the list dropped keep exact zeros
        a.cidx = cx->idx;
        a.cstats = cx->stats;
        NH_LAUNCH(k_point_grad_zero, nh_ceil_div(M * 2, 256), 256, 0, stream, out, M * 2);
        rc = nh_launch_status("point_grad_zero");
        if (rc) return rc;
    }
    // persistent workgroups: as many per CU as the images leave room for
    int per_cu = NH_PG_LDS_BUDGET / y.lds_bytes;
    per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);
    int64_t grid = nh_ceil_div(M, NH_PG_ROWS);
    if (grid > (int64_t)nh_compute_units() * per_cu) grid = (int64_t)nh_compute_units() * per_cu;
    if (y.ext) {
        rc = nh_lds_limit(k_point_grad<NH_PG_TX_EXT, NH_PG_TD_EXT>, y.lds_bytes);
        if (rc) return rc;
        NH_LAUNCH_NAMED("k_point_grad", (k_point_grad<NH_PG_TX_EXT, NH_PG_TD_EXT>), grid, 64 * NH_PG_WAVES, y.lds_bytes, stream, a);
    } else {
        rc = nh_lds_limit(k_point_grad<NH_PG_TX, NH_PG_TD>, y.lds_bytes);
        if (rc) return rc;
        NH_LAUNCH_NAMED("k_point_grad", (k_point_grad<NH_PG_TX, NH_PG_TD>), grid, 64 * NH_PG_WAVES, y.lds_bytes, stream, a);
    }
    return nh_launch_status("point_grad");
}

// nh_ray_grad's sum over a ray's samples (render.hip), of the [M][8] buffer
static int nh_ray_grad_sum(const float* rays, int stride, int64_t n, const float* z, int S, int view, const float* pg, const float* g_norm,
                    float* g_rays, int accumulate, nerfhip_stream_t stream) {
    if (n == 0) return NERFHIP_OK;
    NH_REQUIRE(rays && z && pg && g_rays && S > 0 && stride >= (view ? 11 : 8), "ray_grad_sum: bad arguments");
    RaySumArgs a;
    memset(&a, 0, sizeof(a));
    a.rays = rays;
    a.stride = stride;
    a.z = z;
    a.S = S;
    a.view = view;
    a.pg = pg;
    a.g_norm = g_norm;
    a.g_rays = g_rays;
    a.accumulate = accumulate;
    NH_LAUNCH(k_ray_grad_sum, n, 64, 0, stream, a);
    return nh_launch_status("ray_grad_sum");
}
