// occ/occ_train.hip -- the density grid that keeps an occupancy grid alive while the nets change (include/nerfhip.h "occupancy grid in
// training"): nerfhip_occ_density_update (probes as nerfhip_occ_update's -- the shared part lives in occupancy.hip --,
// then dens = max(dens * decay, relu(raw[3])) per cell) and nerfhip_occ_density_bits (bit = dens > min(tau, mean(dens))).
// No atomics: every cell, every word and every partial sum has one writer, and the mean is summed in a fixed order.
#include "../nh_mlp.h"
#include "../nh_occ.h"

namespace {

int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// one thread per four consecutive cells (its only writer): dens = fmaxf(dens * decay, s), s = raw[3] > 0 ? raw[3] : 0 (a NaN raw[3]
// fails the comparison: s = 0).  raw: the probe forward's rows of the range, dens: the range's first cell (both 16-byte aligned)
NH_KERNEL void k_occ_density(const float* __restrict__ raw, int64_t nquads, float decay, float* __restrict__ dens) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nquads) return;
    const float4* const rows = (const float4*)raw + (size_t)q * 4;
    const float r0 = rows[0].w, r1 = rows[1].w, r2 = rows[2].w, r3 = rows[3].w;
    float4 d = ((const float4*)dens)[q];
    d.x = fmaxf(d.x * decay, r0 > 0.0f ? r0 : 0.0f);
    d.y = fmaxf(d.y * decay, r1 > 0.0f ? r1 : 0.0f);
    d.z = fmaxf(d.z * decay, r2 > 0.0f ? r2 : 0.0f);
    d.w = fmaxf(d.w * decay, r3 > 0.0f ? r3 : 0.0f);
    ((float4*)dens)[q] = d;
}

constexpr int NH_DENS_THREADS = 256, NH_DENS_PER_THREAD = 16, NH_DENS_CELLS = NH_DENS_THREADS * NH_DENS_PER_THREAD;

// the sum of the block's 256 per-thread values, in thread order, by thread 0 (a fixed order whatever the schedule)
NH_DEVICE double block_sum_in_order(double v, double* lds) {
    lds[threadIdx.x] = v;
    nh_block_sync();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int t = 0; t < NH_DENS_THREADS; ++t) s += lds[t];
    return s;  // (thread 0's alone is the sum)
}

// stage 1: one fp64 partial per workgroup of 4096 cells; a thread sums its 16 consecutive cells in index order
NH_KERNEL void k_occ_density_partial(const float* __restrict__ dens, int64_t ncells, double* __restrict__ partial) {
    NH_SHARED double lds[NH_DENS_THREADS];
    const int64_t base = (int64_t)blockIdx.x * NH_DENS_CELLS + (int64_t)threadIdx.x * NH_DENS_PER_THREAD;
    double v = 0.0;
    for (int e = 0; e < NH_DENS_PER_THREAD; e += 4)
        if (base + e < ncells) {  // (ncells is a multiple of 32: a quad is whole or absent)
            const float4 d = *(const float4*)(dens + base + e);
            v += (double)d.x;
            v += (double)d.y;
            v += (double)d.z;
            v += (double)d.w;
        }
    const double s = block_sum_in_order(v, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// stage 2: ONE workgroup over the partials in index order (thread t: the t-th run of `per` partials), then thr = min(tau, mean)
NH_KERNEL void k_occ_density_thr(const double* __restrict__ partial, int nparts, int per, int64_t ncells, float tau, float* __restrict__ thr) {
    NH_SHARED double lds[NH_DENS_THREADS];
    double v = 0.0;
    for (int e = 0; e < per; ++e) {
        const int i = (int)threadIdx.x * per + e;
        if (i < nparts) v += partial[i];
    }
    const double s = block_sum_in_order(v, lds);
    if (threadIdx.x == 0) *thr = fminf(tau, (float)(s / (double)ncells));
}

// one thread per 32-cell word (its only writer): bit k = dens[32 w + k] > thr
NH_KERNEL void k_occ_density_bits(const float* __restrict__ dens, int64_t nwords, const float* __restrict__ thr_p, uint32_t* __restrict__ words) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwords) return;
    const float thr = *thr_p;
    const float4* const d = (const float4*)dens + (size_t)w * 8;
    uint32_t v = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float4 x = d[k];
        v |= (x.x > thr ? 1u : 0u) << (4 * k);
        v |= (x.y > thr ? 1u : 0u) << (4 * k + 1);
        v |= (x.z > thr ? 1u : 0u) << (4 * k + 2);
        v |= (x.w > thr ? 1u : 0u) << (4 * k + 3);
    }
    words[w] = v;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int nerfhip_occ_density_update(nerfhip_plan_t plan, const float* packed, const nerfhip_occ_grid* grid, float* dens, float decay,
                                          int pass, uint64_t seed, int64_t cell_first, int64_t cell_count, void* tmp, int64_t tmp_bytes,
                                          nerfhip_stream_t stream) {
    int rc = nh_occ_check_box(grid, "occ_density_update");
    if (rc) return rc;
    rc = nh_occ_probe_check("occ_density_update", plan, packed, grid, pass, cell_first, cell_count);
    if (rc) return rc;
    NH_REQUIRE(dens && aligned16(dens), "occ_density_update: dens is NULL or not 16-byte aligned");
    NH_REQUIRE(decay >= 0.0f && decay <= 1.0f, "occ_density_update: decay must lie in [0, 1] (got %g)", (double)decay);
    if (cell_count == 0) return NERFHIP_OK;
    float* raw = nullptr;
    rc = nh_occ_probe_run("occ_density_update", plan, packed, grid, pass, seed, cell_first, cell_count, tmp, tmp_bytes, stream, &raw);
    if (rc) return rc;
    const int64_t nquads = cell_count / 4;
    NH_LAUNCH(k_occ_density, nh_ceil_div(nquads, 256), 256, 0, stream, (const float*)raw, nquads, decay, dens + cell_first);
    return nh_launch_status("occ_density");
}

extern "C" int64_t nerfhip_occ_density_bits_tmp_bytes(const int* res) {
    if (!res || res[0] < 1 || res[1] < 1 || res[2] < 1) return -1;
    const int64_t ncells = (int64_t)res[0] * res[1] * res[2];
    return 256 + align256(nh_ceil_div(ncells, NH_DENS_CELLS) * 8);
}

extern "C" int nerfhip_occ_density_bits(const float* dens, const int* res, float tau, uint32_t* bits_out, void* tmp, int64_t tmp_bytes,
                                        nerfhip_stream_t stream) {
    const int rc = nh_occ_check_res(res, "occ_density_bits");
    if (rc) return rc;
    NH_REQUIRE(dens && aligned16(dens) && bits_out, "occ_density_bits: dens (16-byte aligned) / bits_out is NULL");
    NH_REQUIRE(tau == tau, "occ_density_bits: tau is NaN");
    const int64_t need = nerfhip_occ_density_bits_tmp_bytes(res);
    NH_REQUIRE(tmp && tmp_bytes >= need, "occ_density_bits: tmp too small (%lld < %lld)", (long long)tmp_bytes, (long long)need);
    const int64_t ncells = (int64_t)res[0] * res[1] * res[2];
    const int nparts = (int)nh_ceil_div(ncells, NH_DENS_CELLS);  // (at most 512^3 / 4096 = 32768)
    float* const thr = (float*)tmp;
    double* const partial = (double*)((char*)tmp + 256);
    NH_LAUNCH(k_occ_density_partial, nparts, NH_DENS_THREADS, 0, stream, dens, ncells, partial);
    int rc2 = nh_launch_status("occ_density_partial");
    if (rc2) return rc2;
    NH_LAUNCH(k_occ_density_thr, 1, NH_DENS_THREADS, 0, stream, (const double*)partial, nparts, (int)nh_ceil_div(nparts, NH_DENS_THREADS),
              ncells, tau, thr);
    rc2 = nh_launch_status("occ_density_thr");
    if (rc2) return rc2;
    const int64_t nwords = ncells / 32;
    NH_LAUNCH(k_occ_density_bits, nh_ceil_div(nwords, 256), 256, 0, stream, dens, nwords, (const float*)thr, bits_out);
    return nh_launch_status("occ_density_bits");
}
