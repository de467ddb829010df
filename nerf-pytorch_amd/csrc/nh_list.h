// nh_list.h -- the ordered sample list of NhCompact (nh_mlp.h), built for any row predicate: what compact.hip (rows whose cotangent is
// not all zero) and occ/occupancy.hip (samples whose point lies in an occupied cell) share.
//
// Two launches, no atomics: k_list_count (per 2048-sample block: the number of kept rows) and k_list_scatter (block offset = sum of the
// counts in front of it; ranks inside the block by a prefix sum over its threads).  The list is padded with sample 0 up to the next
// multiple of 128.
//
// A predicate is a trivially copyable device functor, passed by value in the kernel arguments:
//     int  operator()(int64_t m) const   1: sample m is kept.  Called once per sample by EACH of the two kernels: it must be pure.
//     void rejected(int64_t m) const     called once, by the scatter kernel, for every sample of the launch that is not kept
#pragma once
#include "nh_mlp.h"

constexpr int NH_LIST_THREADS = 256, NH_LIST_PER_THREAD = 8, NH_LIST_SAMPLES = NH_LIST_THREADS * NH_LIST_PER_THREAD;

NH_DEVICE int nh_list_wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += nh_shfl_xor_i(v, m);
    return v;
}

template <class Pred>
NH_KERNEL void k_list_count(Pred pred, int64_t M, int* __restrict__ counts) {
    NH_SHARED int wsum[NH_LIST_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * NH_LIST_SAMPLES + (int64_t)threadIdx.x * NH_LIST_PER_THREAD;
    int c = 0;
#pragma unroll
    for (int e = 0; e < NH_LIST_PER_THREAD; ++e)
        if (base + e < M) c += pred(base + e);
    c = nh_list_wave_sum(c);
    if (nh_lane() == 0) wsum[nh_wave_in_block()] = c;
    nh_block_sync();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < NH_LIST_THREADS / 64; ++w) t += wsum[w];
        counts[blockIdx.x] = t;
    }
}

template <class Pred>
NH_KERNEL void k_list_scatter(Pred pred, int64_t M, const int* __restrict__ counts, int nblocks, int* __restrict__ idx,
                              int* __restrict__ stats) {
    NH_SHARED int wsum[NH_LIST_THREADS / 64 + 1];
    const int lane = nh_lane(), wave = nh_wave_in_block();
    const int64_t base = (int64_t)blockIdx.x * NH_LIST_SAMPLES + (int64_t)threadIdx.x * NH_LIST_PER_THREAD;
    int flags = 0, c = 0;
#pragma unroll
    for (int e = 0; e < NH_LIST_PER_THREAD; ++e)
        if (base + e < M) {
            if (pred(base + e))
                flags |= 1 << e, ++c;
            else
                pred.rejected(base + e);
        }
    // inclusive prefix sum of c over the wave
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = nh_shfl_i(incl, lane - d < 0 ? 0 : lane - d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    // the samples in front of this block: wave 0 sums the counts of blocks 0 .. blockIdx.x - 1
    if (wave == 0) {
        int s = 0;
        for (int b = lane; b < (int)blockIdx.x; b += 64) s += counts[b];
        s = nh_list_wave_sum(s);
        if (lane == 0) wsum[NH_LIST_THREADS / 64] = s;
    }
    nh_block_sync();
    int off = wsum[NH_LIST_THREADS / 64];
    for (int w = 0; w < wave; ++w) off += wsum[w];
    off += incl - c;
#pragma unroll
    for (int e = 0; e < NH_LIST_PER_THREAD; ++e)
        if (flags & (1 << e)) idx[off++] = (int)(base + e);
    if ((int)blockIdx.x == nblocks - 1) {  // the last block knows the total: statistics and the padding slots
        int total = wsum[NH_LIST_THREADS / 64];
        for (int w = 0; w < NH_LIST_THREADS / 64; ++w) total += wsum[w];
        const int padded = (total + 127) & ~127;
        for (int q = total + (int)threadIdx.x; q < padded; q += NH_LIST_THREADS) idx[q] = 0;
        if (threadIdx.x == 0) {
            stats[NH_CSTAT_ACTIVE] = total;
            stats[NH_CSTAT_TOTAL] = (int)M;
        }
    }
}

// (k_count / k_scatter: the two launches' names in a profile report, "k_..."; an error message names them without the "k_")
template <class Pred>
static inline int nh_list_build(const Pred& pred, int64_t M, const NhCompact& c, const char* k_count, const char* k_scatter,
                                nerfhip_stream_t stream) {
    const int nblocks = (int)nh_ceil_div(M, NH_LIST_SAMPLES);
    NH_LAUNCH_NAMED(k_count, (k_list_count<Pred>), nblocks, NH_LIST_THREADS, 0, stream, pred, M, c.counts);
    int rc = nh_launch_status(k_count + 2);
    if (rc) return rc;
    NH_LAUNCH_NAMED(k_scatter, (k_list_scatter<Pred>), nblocks, NH_LIST_THREADS, 0, stream, pred, M, (const int*)c.counts, nblocks, c.idx,
                    c.stats);
    return nh_launch_status(k_scatter + 2);
}
