// compact.hip -- the sample list of a COMPACTED backward (nerfhip_plan_set_bwd_compaction).
//
// The reference differentiates every sample point densely (autograd of nerf/models.py:233-256 under train_nerf.py:259).  But
// sigma_a = relu(raw[..., 3] + noise) (nerf/volume_rendering_utils.py:38): wherever that ReLU is off -- and behind the sample at which a
// ray's transmittance reaches 0 -- the sample's weight is exactly 0, so its d(loss)/d(raw) is exactly zero in all four channels, and
// with it every d(pre-activation) row of that sample in every layer: a zero term of every weight-gradient sum.  The compacted backward
// drops those terms instead of multiplying them: this file lists the samples whose cotangent row is not all zero (ascending sample
// index: a fixed order), the data-gradient kernels walk that list (mlp16.hip / mlp_f16w.hip: gather d(raw) and the ReLU masks by
// index, write the d(pre-activation) images compacted) and the weight-gradient kernels multiply the compacted images with the
// activation rows gathered through the same list (wgrad.hip / wgrad_f16.hip).  Same sums, zero terms dropped.
//
// Two launches, no atomics: the count / scatter kernels of nh_list.h with the predicate "the row is not all zero" (occ/occupancy.hip builds
// its list with the same two kernels and another predicate).  The list is padded with sample 0 up to the next multiple of 128 (the
// data-gradient kernels then write whole zero rows for the padding slots, and 0 * finite = 0).
#include "nh_list.h"

namespace {

constexpr int CB_SAMPLES = NH_LIST_SAMPLES;

// the row predicate of the compacted backward's list (nh_list.h): d(raw output) row m is not all zero
struct RowNonzero {
    const float* g_out;
    NH_MEMBER int operator()(int64_t m) const {
        const float4 v = *(const float4*)(g_out + (size_t)m * 4);
        return (v.x != 0.0f || v.y != 0.0f || v.z != 0.0f || v.w != 0.0f) ? 1 : 0;  // (a NaN row counts: it propagates as in the dense path)
    }
    NH_MEMBER void rejected(int64_t) const {}
};

}  // namespace

int64_t nh_compact_ints(int64_t M) {
    // statistics | per-block counts | the list: one slot per sample, whole 128-sample groups, + one 1-KiB copy piece of slack
    return NH_CSTAT_WORDS + ((nh_ceil_div(M, CB_SAMPLES) + 15) & ~(int64_t)15) + nh_ceil_div(M, 128) * 128 + 256;
}

NhCompact nh_compact_view(int* area, int64_t M) {
    NhCompact c;
    c.stats = area;
    c.counts = area + NH_CSTAT_WORDS;
    c.idx = c.counts + ((nh_ceil_div(M, CB_SAMPLES) + 15) & ~(int64_t)15);
    c.stash_in_list_order = false;
    return c;
}

int nh_compact_build(const float* g_out, int64_t M, const NhCompact& c, nerfhip_stream_t stream) {
    NH_REQUIRE(g_out && c.idx && M > 0 && M < ((int64_t)1 << 31), "compact: bad arguments");
    return nh_list_build(RowNonzero{g_out}, M, c, "k_compact_count", "k_compact_scatter", stream);
}
