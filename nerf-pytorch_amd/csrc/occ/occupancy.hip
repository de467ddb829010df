// occ/occupancy.hip -- the occupancy grid of the inference render (include/nerfhip.h "occupancy grid").
//
// One bit per cell of a box around the scene.  A pass of nerfhip_render_fwd_occ (fused.hip) lists the samples whose point falls into an
// occupied cell -- the count / scatter kernels of nh_list.h, which compact.hip uses with another predicate: ascending sample index, no
// atomics -- and writes the empty row (0, 0, 0, NERFHIP_OCC_EMPTY_RAW) for every other sample in the scatter launch; the MLP then runs
// over the list alone (the LIST instantiations of the forward kernels).  The grid itself is built by nerfhip_occ_update (one probe per
// cell through the plan's ordinary fused-input forward, S = 1) and nerfhip_occ_dilate.  The probe-and-forward part is shared with the
// density grid of training (occ_train.hip): nh_occ_probe_check / nh_occ_probe_run.
#include "../nh_list.h"
#include "../nh_occ.h"

namespace {

int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// the row predicate of the culled render's list (nh_list.h): the cell of sample m's point is occupied; a rejected sample gets the
// empty row
struct OccPred {
    NhOccGrid g;
    const float* rays;
    int ray_stride;
    const float* z;
    int S;
    float* raw;
    NH_MEMBER int operator()(int64_t m) const {
        const int mi = (int)m;  // (the host checks M < 2^31)
        const float* const rr = rays + (size_t)(mi / S) * (size_t)ray_stride;
        float px, py, pz;
        nh_occ_point(rr, z[mi], &px, &py, &pz);
        return nh_occ_test(g, px, py, pz);
    }
    NH_MEMBER void rejected(int64_t m) const {
        float4 e;
        e.x = 0.0f;
        e.y = 0.0f;
        e.z = 0.0f;
        e.w = NERFHIP_OCC_EMPTY_RAW;
        *(float4*)(raw + (size_t)m * 4) = e;
    }
};

NH_KERNEL void k_occ_mark(OccPred p, int64_t M, uint8_t* __restrict__ flags) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m < M) flags[m] = (uint8_t)p(m);
}

struct ProbeArgs {
    float lo[3], cell[3];
    int res[3];
    int pass;
    uint64_t seed;
    int64_t ncells, cell_first, cell_count;
    float* rows;  // [cell_count, 11]
    float* z;     // [cell_count]
};

// one thread per cell: its probe as a packed ray row (origin = the probe, direction 0, near = far = 0, viewdir (0, 0, 1)) and depth 0
NH_KERNEL void k_occ_probe(ProbeArgs a) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.cell_count) return;
    const int64_t b = a.cell_first + t;
    int i[3];
    i[0] = (int)(b % a.res[0]);
    i[1] = (int)((b / a.res[0]) % a.res[1]);
    i[2] = (int)(b / ((int64_t)a.res[0] * a.res[1]));
    float* const row = a.rows + (size_t)t * 11;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const float u = a.pass == 0 ? 0.5f
                                    : nh_rand_uniform(a.seed, (uint32_t)NERFHIP_OCC_RNG_STREAM,
                                                      3ull * ((uint64_t)a.pass * (uint64_t)a.ncells + (uint64_t)b) + (uint64_t)ax);
        row[ax] = a.lo[ax] + ((float)i[ax] + u) * a.cell[ax];
    }
    row[3] = row[4] = row[5] = 0.0f;
    row[6] = row[7] = 0.0f;
    row[8] = row[9] = 0.0f;
    row[10] = 1.0f;
    a.z[t] = 0.0f;
}

// one thread per 32-cell word (its only writer): bit k |= raw[3] of cell 32 w + k's probe > tau
NH_KERNEL void k_occ_or(const float* __restrict__ raw, int64_t nwords, float tau, uint32_t* __restrict__ words) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwords) return;
    uint32_t v = 0u;
    for (int k = 0; k < 32; ++k) v |= (raw[((size_t)w * 32 + (size_t)k) * 4 + 3] > tau ? 1u : 0u) << k;
    words[w] |= v;
}

struct DilateArgs {
    const uint32_t* in;
    uint32_t* out;
    int res[3];
    int64_t nwords;
};
NH_DEVICE unsigned occ_bit(const uint32_t* bits, int64_t b) { return (bits[b >> 5] >> (unsigned)(b & 31)) & 1u; }

// one thread per 32-cell word of the output: a cell is set if it or a face neighbour INSIDE the box is set
NH_KERNEL void k_occ_dilate(DilateArgs a) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= a.nwords) return;
    const int rx = a.res[0], ry = a.res[1], rz = a.res[2];
    const int64_t sy = rx, sz = (int64_t)rx * ry;
    uint32_t v = a.in[w];
    for (int k = 0; k < 32; ++k) {
        if ((v >> k) & 1u) continue;
        const int64_t b = w * 32 + k;
        const int ix = (int)(b % rx), iy = (int)((b / rx) % ry), iz = (int)(b / sz);
        unsigned s = 0u;
        if (ix > 0) s |= occ_bit(a.in, b - 1);
        if (ix + 1 < rx) s |= occ_bit(a.in, b + 1);
        if (iy > 0) s |= occ_bit(a.in, b - sy);
        if (iy + 1 < ry) s |= occ_bit(a.in, b + sy);
        if (iz > 0) s |= occ_bit(a.in, b - sz);
        if (iz + 1 < rz) s |= occ_bit(a.in, b + sz);
        v |= s << k;
    }
    a.out[w] = v;
}

int check_res(const int* res, const char* what) {
    NH_REQUIRE(res, "%s: res is NULL", what);
    for (int a = 0; a < 3; ++a)
        NH_REQUIRE(res[a] >= 1 && res[a] <= NERFHIP_OCC_MAX_RES, "%s: grid resolution %d x %d x %d: each axis must be 1 .. %d", what, res[0],
                   res[1], res[2], NERFHIP_OCC_MAX_RES);
    NH_REQUIRE(((int64_t)res[0] * res[1] * res[2]) % 32 == 0, "%s: grid resolution %d x %d x %d: the cell count must be a multiple of 32",
               what, res[0], res[1], res[2]);
    return NERFHIP_OK;
}

NhOccGrid device_grid(const nerfhip_occ_grid* g) {
    NhOccGrid d;
    d.bits = g->bits;
    for (int a = 0; a < 3; ++a) {
        d.lo[a] = g->lo[a];
        d.inv[a] = (float)g->res[a] / (g->hi[a] - g->lo[a]);
        d.res[a] = g->res[a];
    }
    d.outside = g->outside ? 1 : 0;
    return d;
}

}  // namespace

int nh_occ_check_res(const int* res, const char* what) { return check_res(res, what); }

int nh_occ_check(const nerfhip_occ_grid* g, const char* what) {
    NH_REQUIRE(g, "%s: the occupancy grid is NULL", what);
    NH_REQUIRE(g->bits, "%s: the occupancy grid has no bits", what);
    return nh_occ_check_box(g, what);
}

int nh_occ_check_box(const nerfhip_occ_grid* g, const char* what) {
    NH_REQUIRE(g, "%s: the occupancy grid is NULL", what);
    const int rc = check_res(g->res, what);
    if (rc) return rc;
    for (int a = 0; a < 3; ++a)
        NH_REQUIRE(g->hi[a] > g->lo[a], "%s: the occupancy grid's box needs hi > lo on every axis (axis %d: lo %g, hi %g)", what, a,
                   (double)g->lo[a], (double)g->hi[a]);
    return NERFHIP_OK;
}

int nh_occ_list(const nerfhip_occ_grid* g, const float* rays, int ray_stride, const float* z, int S, int64_t M, float* raw,
                const NhCompact& list, nerfhip_stream_t stream) {
    NH_REQUIRE(rays && z && raw && list.idx && list.counts && list.stats && S > 0 && M > 0 && M < ((int64_t)1 << 31),
               "occ_list: bad arguments");
    const OccPred p = {device_grid(g), rays, ray_stride, z, S, raw};
    return nh_list_build(p, M, list, "k_occ_count", "k_occ_scatter", stream);
}

extern "C" int nerfhip_occ_mark(const float* rays, int ray_stride, int64_t n, const float* z, int S, const nerfhip_occ_grid* grid,
                                uint8_t* flags_u8, nerfhip_stream_t stream) {
    int rc = nh_occ_check(grid, "occ_mark");
    if (rc) return rc;
    NH_REQUIRE(n >= 0 && S > 0 && ray_stride >= 6, "occ_mark: bad arguments");
    if (n == 0) return NERFHIP_OK;
    const int64_t M = n * S;
    NH_REQUIRE(rays && z && flags_u8, "occ_mark: bad arguments");
    NH_REQUIRE(M < ((int64_t)1 << 31), "occ_mark: at most 2^31 - 1 sample points per call (got %lld)", (long long)M);
    const OccPred p = {device_grid(grid), rays, ray_stride, z, S, nullptr};
    NH_LAUNCH(k_occ_mark, nh_ceil_div(M, 256), 256, 0, stream, p, M, flags_u8);
    return nh_launch_status("occ_mark");
}

extern "C" int64_t nerfhip_occ_update_tmp_bytes(int64_t cell_count) {
    if (cell_count < 0) return -1;
    return align256(cell_count * 44) + align256(cell_count * 4) + align256(cell_count * 16);
}

// The probe-and-forward part of nerfhip_occ_update, shared with nerfhip_occ_density_update (occ_train.hip).  nh_occ_probe_check: the
// plan, the pass and the cell range (the grid's box is the caller's to check); nh_occ_probe_run: tmp, then one probe per cell of the
// range and the plan's inference forward over them -- *raw: the output rows inside tmp (the layout of include/nerfhip.h)
int nh_occ_probe_check(const char* what, nerfhip_plan_t plan, const float* packed, const nerfhip_occ_grid* grid, int pass,
                       int64_t cell_first, int64_t cell_count) {
    NH_REQUIRE(plan && packed, "%s: plan / packed is NULL", what);
    const int64_t ncells = (int64_t)grid->res[0] * grid->res[1] * grid->res[2];
    NH_REQUIRE(pass >= 0 && pass < 4096, "%s: pass must be 0 .. 4095 (got %d)", what, pass);
    NH_REQUIRE(cell_first >= 0 && cell_count >= 0 && cell_first % 32 == 0 && cell_count % 32 == 0 && cell_first + cell_count <= ncells,
               "%s: cells [%lld, %lld + %lld) must be multiples of 32 inside the grid's %lld cells", what, (long long)cell_first,
               (long long)cell_first, (long long)cell_count, (long long)ncells);
    return NERFHIP_OK;
}

int nh_occ_probe_run(const char* what, nerfhip_plan_t plan, const float* packed, const nerfhip_occ_grid* grid, int pass, uint64_t seed,
                     int64_t cell_first, int64_t cell_count, void* tmp, int64_t tmp_bytes, nerfhip_stream_t stream, float** raw_out) {
    const int64_t need = nerfhip_occ_update_tmp_bytes(cell_count);
    NH_REQUIRE(tmp && tmp_bytes >= need, "%s: tmp too small (%lld < %lld)", what, (long long)tmp_bytes, (long long)need);
    ProbeArgs a;
    memset(&a, 0, sizeof(a));
    for (int ax = 0; ax < 3; ++ax) {
        a.lo[ax] = grid->lo[ax];
        a.cell[ax] = (grid->hi[ax] - grid->lo[ax]) / (float)grid->res[ax];
        a.res[ax] = grid->res[ax];
    }
    a.pass = pass;
    a.seed = seed;
    a.ncells = (int64_t)grid->res[0] * grid->res[1] * grid->res[2];
    a.cell_first = cell_first;
    a.cell_count = cell_count;
    a.rows = (float*)tmp;
    a.z = (float*)((char*)tmp + align256(cell_count * 44));
    float* const raw = (float*)((char*)a.z + align256(cell_count * 4));
    NH_LAUNCH(k_occ_probe, nh_ceil_div(cell_count, 256), 256, 0, stream, a);
    int rc = nh_launch_status("occ_probe");
    if (rc) return rc;
    NhMlpInput in;
    memset(&in, 0, sizeof(in));
    in.mode = 1;
    in.rays = a.rows;
    in.ray_stride = 11;
    in.z = a.z;
    in.S = 1;
    *raw_out = raw;
    return nh_mlp_forward(plan, packed, in, cell_count, raw, nullptr, stream);
}

extern "C" int nerfhip_occ_update(nerfhip_plan_t plan, const float* packed, const nerfhip_occ_grid* grid, float tau, int pass,
                                  uint64_t seed, int64_t cell_first, int64_t cell_count, void* tmp, int64_t tmp_bytes,
                                  nerfhip_stream_t stream) {
    int rc = nh_occ_check(grid, "occ_update");
    if (rc) return rc;
    rc = nh_occ_probe_check("occ_update", plan, packed, grid, pass, cell_first, cell_count);
    if (rc) return rc;
    NH_REQUIRE(tau == tau, "occ_update: tau is NaN");
    if (cell_count == 0) return NERFHIP_OK;
    float* raw = nullptr;
    rc = nh_occ_probe_run("occ_update", plan, packed, grid, pass, seed, cell_first, cell_count, tmp, tmp_bytes, stream, &raw);
    if (rc) return rc;
    const int64_t nwords = cell_count / 32;
    NH_LAUNCH(k_occ_or, nh_ceil_div(nwords, 256), 256, 0, stream, (const float*)raw, nwords, tau,
              const_cast<uint32_t*>(grid->bits) + cell_first / 32);
    return nh_launch_status("occ_or");
}

extern "C" int nerfhip_occ_dilate(const uint32_t* bits_in, uint32_t* bits_out, const int* res, nerfhip_stream_t stream) {
    const int rc = check_res(res, "occ_dilate");
    if (rc) return rc;
    NH_REQUIRE(bits_in && bits_out && bits_in != bits_out, "occ_dilate: bits_in and bits_out must be two different buffers");
    DilateArgs a;
    a.in = bits_in;
    a.out = bits_out;
    for (int ax = 0; ax < 3; ++ax) a.res[ax] = res[ax];
    a.nwords = (int64_t)res[0] * res[1] * res[2] / 32;
    NH_LAUNCH(k_occ_dilate, nh_ceil_div(a.nwords, 256), 256, 0, stream, a);
    return nh_launch_status("occ_dilate");
}
