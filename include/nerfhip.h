/* nerfhip.h -- C ABI of libnerfhip.so: the MI355X (gfx950) NeRF render + training hot path.
 *
 * This is the drop-in boundary underneath the Python API of krrish94/nerf-pytorch.  The reference has no
 * FFI of its own for this path (it is pure PyTorch); every entry point below names the reference
 * function it replaces (file:line relative to the reference tree).  The binding a maintainer adds on the
 * reference side is a ctypes stub -- see INTEGRATION.md.
 *
 * Conventions (all entry points):
 *   - plain C types only; every pointer marked "dev" is a device pointer (hipMalloc'ed / a torch CUDA
 *     tensor's data_ptr()), fp32 row-major contiguous unless a stride argument says otherwise;
 *   - returns 0 on success, a negative NERFHIP_ERR_* code otherwise; nerfhip_last_error() then returns a
 *     thread-local message.  Nothing throws across the ABI;
 *   - the library never allocates or frees caller-visible memory, never creates streams, never
 *     synchronises the device: work is enqueued on the `stream` argument (a hipStream_t passed as void*;
 *     NULL = the legacy default stream) and the caller owns all buffers for the duration of that work;
 *   - `plan` handles are host-only objects (weight packing tables, kernel schedules).
 *
 * Random draws: wherever the reference calls torch.rand / torch.randn the caller may pass the draws in
 * (parity mode: identical results for identical draws) or pass NULL and a (seed, ray_offset) pair, in
 * which case a counter-based Philox4x32-10 generator is evaluated in-kernel (production mode).  Stream
 * ids: 0 = stratified t_rand, 1 = coarse sigma noise, 2 = inverse-CDF u, 3 = fine sigma noise, 4 = background colour.
 * nerfhip_rng_fill() writes exactly the numbers the kernels would draw.
 */
#ifndef NERFHIP_H_
#define NERFHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* nerfhip_stream_t;

#define NERFHIP_OK 0
#define NERFHIP_ERR_ARG (-1)
#define NERFHIP_ERR_UNSUPPORTED (-2)
#define NERFHIP_ERR_LAUNCH (-3)
#define NERFHIP_ERR_WORKSPACE (-4)

#define NERFHIP_RNG_UNIFORM 0
#define NERFHIP_RNG_NORMAL 1

/* ---- library --------------------------------------------------------------------------------------------------- */
int nerfhip_version(void);
const char* nerfhip_last_error(void);
/* 0 for the product library.  (The CPU wave-emulator build used by the test-suite returns 1.) */
int nerfhip_is_emulated(void);

/* Writes n draws of the in-kernel generator: element e of `stream_id` under `seed`, e = first .. first+n-1. */
int nerfhip_rng_fill(int kind, uint64_t seed, uint32_t stream_id, uint64_t first, int64_t n, float* out_dev,
                     nerfhip_stream_t stream);

/* Per-kernel timing: while enabled, every kernel launch is bracketed by HIP events recorded on the launch stream.
 * nerfhip_profile_report waits for them and writes "kernel_name launches total_ms\n" lines into buf, then clears. */
int nerfhip_profile_enable(int on);
int nerfhip_profile_report(char* buf, int64_t cap);
/* pre-creates the event pairs of `launches` launches (reused after every report), so that none is created while timing */
int nerfhip_profile_reserve(int64_t launches);
/* Shader clock under load: while profiling is enabled the three MLP kernels stamp every workgroup with the shader-clock
 * counter (s_memtime) and the constant 100 MHz counter (s_memrealtime).  out[3k + 0/1/2] = shader cycles / 100 MHz ticks /
 * workgroups summed over the workgroups of kernel k (0 = k_mlp_fwd16, 1 = k_mlp_dgrad16, 2 = k_wgrad):
 * clock = 0.1 GHz * out[3k] / out[3k + 1].  Waits for the device; clears the counters.  out: host uint64[9]. */
int nerfhip_profile_clocks(uint64_t* out);

/* ---- K1: rays -------------------------------------------------------------------------------------------------- */
/* get_ray_bundle (nerf/nerf_helpers.py:67-110) incl. meshgrid_xy (:28-40).  c2w: dev, rows >= 3, row stride
 * c2w_ld floats (columns 0..2 rotation, column 3 translation).  pixels: dev int64 linear ids (row*width+col) of
 * the n rays wanted, or NULL for the whole image (then n must be height*width; output is (H,W,3) row-major).
 * ray_origins / ray_directions: dev [n,3].  Directions are NOT normalised (reference behaviour). */
int nerfhip_ray_bundle(int height, int width, float focal, const float* c2w, int c2w_ld, const int64_t* pixels,
                       int64_t n, float* ray_origins, float* ray_directions, nerfhip_stream_t stream);

/* ndc_rays (nerf/nerf_helpers.py:170-197).  cw = -1/(W/(2*focal)), ch = -1/(H/(2*focal)), two_near = 2*near,
 * neg_two_near = -2*near are evaluated by the caller exactly as the reference's Python scalar arithmetic does. */
int nerfhip_ndc_rays(float near, float cw, float ch, float two_near, float neg_two_near, const float* rays_o,
                     const float* rays_d, int64_t n, float* out_o, float* out_d, nerfhip_stream_t stream);
/* Its vector-Jacobian product (what autograd computes through nerf/nerf_helpers.py:170-197 when the rays require grad --
 * pose optimisation on LLFF scenes): g_rays_o/d [n,3] = J^T (g_out_o, g_out_d) at (rays_o, rays_d). */
int nerfhip_ndc_rays_bwd(float near, float cw, float ch, float two_near, float neg_two_near, const float* rays_o,
                         const float* rays_d, const float* g_out_o, const float* g_out_d, int64_t n, float* g_rays_o,
                         float* g_rays_d, nerfhip_stream_t stream);

/* viewdirs + ray packing of run_one_iter_of_nerf (nerf/train_utils.py:143-168):
 * rays[n, 8|11] = [o(3) d(3) near far (d/||d||)(3)].  viewdir_src (dev [n,3]) is the PRE-ndc direction the
 * reference normalises; pass NULL for use_viewdirs = false (row width 8). */
int nerfhip_pack_rays(const float* rays_o, const float* rays_d, const float* viewdir_src, float near, float far,
                      int64_t n, float* rays_out, nerfhip_stream_t stream);

/* ---- K3: positional encoding ----------------------------------------------------------------------------------- */
/* positional_encoding (nerf/nerf_helpers.py:113-157).  x: dev [m,d]; freqs: dev [num_freqs] frequency bands as the
 * reference builds them; out: dev [m, d*(include_input + 2*num_freqs)] laid out
 * [x | sin(f0 x) | cos(f0 x) | sin(f1 x) | ...]. */
int nerfhip_positional_encoding(const float* x, int64_t m, int d, const float* freqs, int num_freqs, int include_input,
                                float* out, nerfhip_stream_t stream);

/* ---- K2: stratified depth samples ------------------------------------------------------------------------------ */
/* predict_and_render_radiance lines nerf/train_utils.py:38-65.  rays: dev rows of ray_stride floats with near/far in
 * columns 6/7; t_vals: dev [nc] = torch.linspace(0,1,nc); t_rand: dev [n,nc] uniform draws or NULL (in-kernel
 * stream 0).  z_out: dev [n,nc]. */
int nerfhip_stratified_z(const float* rays, int ray_stride, int64_t n, const float* t_vals, int nc, int lindisp,
                         int perturb, const float* t_rand, uint64_t seed, uint64_t ray_offset, float* z_out,
                         nerfhip_stream_t stream);

/* ---- K5: sigma/alpha compositing ------------------------------------------------------------------------------- */
/* cumprod_exclusive (nerf/nerf_helpers.py:43-64) over the last dimension of x[rows, cols]. */
int nerfhip_cumprod_exclusive(const float* x, int64_t rows, int cols, float* out, nerfhip_stream_t stream);

/* Its backward (autograd of nerf/nerf_helpers.py:43-64, as tiny_nerf.py:100-101 needs it): y = the forward result,
 * g_y = cotangent of y, g_x (out) = cotangent of x; all dev [rows, cols].  Division-free: exact for rows with zeros. */
int nerfhip_cumprod_exclusive_bwd(const float* x, const float* y, const float* g_y, int64_t rows, int cols, float* g_x,
                                  nerfhip_stream_t stream);

/* volume_render_radiance_field (nerf/volume_rendering_utils.py:6-53).  raw: dev [n,s,4]; z: dev [n,s];
 * rd: dev rows of rd_stride floats whose first 3 entries are the ray direction; noise: dev [n,s] N(0,1) draws or
 * NULL (in-kernel stream `rng_stream` when noise_std > 0).  Outputs (any may be NULL): rgb [n,3], disp [n],
 * acc [n], weights [n,s], depth [n]. */
int nerfhip_volume_render_fwd(const float* raw, const float* z, const float* rd, int rd_stride, int64_t n, int s,
                              float noise_std, const float* noise, uint64_t seed, uint32_t rng_stream,
                              uint64_t ray_offset, int white_background, float* rgb, float* disp, float* acc,
                              float* weights, float* depth, nerfhip_stream_t stream);

/* Closed-form backward of the above (what autograd computes for nerf/volume_rendering_utils.py:26-50).
 * g_rgb [n,3], g_depth [n], g_acc [n], g_weights [n,s] are the output cotangents (each may be NULL = 0; the
 * disparity cotangent is folded into g_depth/g_acc by the caller).  g_raw: dev [n,s,4]. */
int nerfhip_volume_render_bwd(const float* raw, const float* z, const float* rd, int rd_stride, int64_t n, int s,
                              float noise_std, const float* noise, uint64_t seed, uint32_t rng_stream,
                              uint64_t ray_offset, int white_background, const float* g_rgb, const float* g_depth,
                              const float* g_acc, const float* g_weights, float* g_raw, nerfhip_stream_t stream);

/* ---- K6: inverse-CDF importance sampling ----------------------------------------------------------------------- */
/* sample_pdf_2 (nerf/nerf_helpers.py:260-302) including the torchsearchsorted call (:288, side="right").
 * bins: dev [n,nbins]; weights: dev [n,nbins-1]; u: dev [n,nf] uniform draws, or NULL with det=1 (then u_det: dev
 * [nf] = torch.linspace(0,1,nf)) or NULL with det=0 (in-kernel stream 2).  samples: dev [n,nf];
 * inds (optional): dev int64 [n,nf] searchsorted result; cdf (optional): dev [n,nbins]. */
int nerfhip_sample_pdf(const float* bins, const float* weights, int64_t n, int nbins, const float* u, int det,
                       const float* u_det, int nf, uint64_t seed, uint64_t ray_offset, float* samples, int64_t* inds,
                       float* cdf, nerfhip_stream_t stream);

/* The hierarchical step of predict_and_render_radiance (nerf/train_utils.py:96-105): z_vals_mid, sample_pdf_2 on
 * weights[...,1:-1], detach, sort(cat(z_coarse, z_samples)).  z_coarse, weights: dev [n,nc]; z_samples (optional):
 * dev [n,nf]; z_fine: dev [n,nc+nf] ascending. */
int nerfhip_hierarchical_z(const float* z_coarse, const float* weights, int64_t n, int nc, const float* u, int det,
                           const float* u_det, int nf, uint64_t seed, uint64_t ray_offset, float* z_samples,
                           float* z_fine, nerfhip_stream_t stream);

/* ---- K4/K8: the MLP (models.FlexibleNeRFModel, nerf/models.py:185-256) ----------------------------------------- */
typedef struct nerfhip_model_cfg {
    int num_layers;         /* models.py:188 */
    int hidden_size;        /* models.py:189; 2..512 (kernel widths 64 / 128 / 256 / 512; other sizes ride zero-padded on the next width) */
    int skip_connect_every; /* models.py:190; cat(h, xyz) before layers_xyz[i] iff i % skip == 0 and i > 0 */
    int num_encoding_fn_xyz; /* 0..16 (every config .yml of the reference: <= 10) */
    int num_encoding_fn_dir; /* 0..10 (every config .yml of the reference: <= 4) */
    int include_input_xyz;
    int include_input_dir;
    int log_sampling_xyz;
    int log_sampling_dir;
    int use_viewdirs;
} nerfhip_model_cfg;

typedef struct nerfhip_plan* nerfhip_plan_t;

/* Host-only.  Returns NULL (and sets the error string) for an unsupported geometry. */
nerfhip_plan_t nerfhip_plan_create(const nerfhip_model_cfg* cfg);
/* Arithmetic of the plan's GEMMs.  FP32 (= nerfhip_plan_create): exact fp32 products on v_mfma_f32_16x16x4_f32 / 32x32x2 -- the
 * reference's own arithmetic, the path the headline benchmark runs; never replaced implicitly.
 *
 * F16X3 family (round 4): every GEMM as THREE fp16 MFMAs on operands split into two IEEE fp16 pieces, hi = f16(v), lo = f16(v - hi),
 * both round-to-nearest: x.w ~ xh.wh + xh.wl + xl.wh with fp32 accumulation.  A piece carries 11 significant bits and the rounding
 * error of hi is at most half an ulp, so hi + lo reproduces v to 2^-24 relative -- fp32's own rounding -- wherever the low piece is
 * a normal or subnormal fp16 number (the gfx950 matrix pipe multiplies fp16 subnormals exactly; measured: scripts/probe/
 * f16_mfma_probe.hip); the dropped xl.wl term is 2^-24 relative as well.  So a product block carries ~3 x 2^-24: fp32-grade
 * arithmetic, and the GPU parity suite holds these plans to the SAME bounds as the fp32 kernels (tests/tolerances.py).  What fp16's
 * 5-bit exponent costs is handled inside the library, all in exact powers of two: the packed weight pieces (and
 * biases) carry 2^8 -- so |w| must stay below 255.9; larger weights are saturated by nerfhip_pack_weights_plan, not turned into Inf --;
 * every SAMPLE carries the exponent of its current activations / d(pre-activation), chosen by the epilogue that produced them so that
 * its largest value lands in [2^13, 2^14) -- no activation range is out of reach, no cotangent too small --; the stash and every
 * output are plain fp32 values; the weight-gradient kernel splits a region at the power of two its producers recorded for it (one
 * word per region behind the stash / scratch, no host synchronisation) and divides it out exactly in its reduction.  Forward and
 * data gradient run with two waves per SIMD on v_mfma_f32_16x16x32_f16 (csrc/mlp_f16w.hip), the weight gradient on
 * v_mfma_f32_32x32x16_f16 (csrc/wgrad_f16.hip).
 *   F16X3            INFERENCE-ONLY plan: its own packed image (nerfhip_plan_packed_floats / nerfhip_plan_pack_index /
 *                    nerfhip_pack_weights_plan), serves nerfhip_mlp_fwd without a stash and the render entry points with
 *                    training = 0; every training / backward entry point refuses it.
 *   F16X3_FWD        training-capable: the forward passes on fp16 pieces (writes the same fp32 stash and ReLU masks), the backward
 *                    kernels the exact fp32 ones; the packed image holds the fp32 image and the fp16-piece image.
 *   F16X3_FWD_DGRAD  ... and the data-gradient chain on fp16 pieces; the weight-gradient GEMMs stay fp32.
 *   F16X3_TRAIN      ... and the large weight-gradient GEMMs (hidden x hidden blocks: ~94 % of those FLOPs) on the fp16 MFMAs, with
 *                    the thin blocks that share a region with one of them -- a skip layer's xyz columns, fc_alpha, the direction
 *                    columns -- riding along in the same launch; layer1's block and fc_rgb | fc_out stay on the fp32 kernel.
 * Supported for kernel widths 64, 128 and 256 (hidden_size <= 256; 64-wide nets: new in round 5 -- config/fern.yml's declared 4 x 64 --,
 * their weight-gradient GEMMs all stay on the fp32 kernel: _TRAIN is _FWD_DGRAD there), num_encoding_fn_xyz <= 10,
 * num_encoding_fn_dir <= 4.  Opt-in, labelled.
 * Values 1 .. 4 named round 3's bf16-piece plans (~2^-16 per product: they did not hold the parity bounds); removed in round 5,
 * nerfhip_plan_create_ex refuses them with a message, the numbers stay reserved. */
#define NERFHIP_PRECISION_FP32 0
#define NERFHIP_PRECISION_F16X3 5
#define NERFHIP_PRECISION_F16X3_FWD 6
#define NERFHIP_PRECISION_F16X3_FWD_DGRAD 7
#define NERFHIP_PRECISION_F16X3_TRAIN 8
nerfhip_plan_t nerfhip_plan_create_ex(const nerfhip_model_cfg* cfg, int precision);
int nerfhip_plan_precision(nerfhip_plan_t plan);
void nerfhip_plan_destroy(nerfhip_plan_t plan);
/* Number of fp32 parameters of the model = length of the flat parameter/gradient vector, laid out as the
 * concatenation of the reference state_dict tensors in registration order (layer1.weight, layer1.bias,
 * layers_xyz.{i}.weight/.bias, layers_dir.0.weight/.bias, fc_alpha.*, fc_rgb.*, fc_feat.* | fc_out.*). */
int64_t nerfhip_plan_num_params(nerfhip_plan_t plan);
int nerfhip_plan_dim_xyz(nerfhip_plan_t plan);
int nerfhip_plan_dim_dir(nerfhip_plan_t plan);
/* Number of tensors and, for tensor i, its name, offset into the flat vector and 2-D shape (cols = 0 for a bias). */
int nerfhip_plan_num_tensors(nerfhip_plan_t plan);
int nerfhip_plan_tensor_info(nerfhip_plan_t plan, int i, const char** name, int64_t* offset, int* rows, int* cols);
/* Human-readable kernel schedule of the plan (host-only): kernel width, and one line per weight-gradient job -- tiles, wave
 * grid, per-wave patch, split-K cost, and the thin weight block riding on it as side tiles, if any. */
int nerfhip_plan_describe(nerfhip_plan_t plan, char* buf, int64_t cap);
/* MFMA-packed weight image: number of floats, and the gather table (host int32[packed_floats]: source index into
 * the flat parameter vector, or -1 for zero padding). */
int64_t nerfhip_plan_packed_floats(nerfhip_plan_t plan);
int nerfhip_plan_pack_index(nerfhip_plan_t plan, int32_t* host_table);
/* packed[i] = table[i] >= 0 ? params[table[i]] : 0   (run once per optimiser step). */
int nerfhip_pack_weights(const float* params, const int32_t* table, int64_t n, float* packed, nerfhip_stream_t stream);
/* The same for any plan: fp32 plans gather as above; F16X3* plans write, per table entry, the bias word (times 2^8) or the two fp16
 * pieces hi = f16(2^8 w), lo = f16(2^8 w - hi) of the weight into the high / low blocks of the image.  table: dev
 * int32[packed_floats] (nerfhip_plan_pack_index), packed: dev, packed_floats 32-bit words. */
int nerfhip_pack_weights_plan(nerfhip_plan_t plan, const float* params, const int32_t* table, float* packed,
                              nerfhip_stream_t stream);
/* Bytes of activation stash a training forward over m sample points needs (0-filled is not required). */
int64_t nerfhip_plan_stash_bytes(nerfhip_plan_t plan, int64_t m);
/* Bytes of scratch nerfhip_mlp_bwd needs for m sample points. */
int64_t nerfhip_plan_bwd_scratch_bytes(nerfhip_plan_t plan, int64_t m);
/* Compacted backward (round 6; off by default).  sigma_a = relu(raw[..., 3] + noise) (nerf/volume_rendering_utils.py:38): wherever
 * that ReLU is off, and behind the sample at which a ray's transmittance reaches 0, a sample's weight is exactly 0, so its
 * d(loss)/d(raw) is exactly zero in all four channels -- and with it every d(pre-activation) row of that sample in every layer, a zero
 * term of every weight-gradient sum the reference's autograd (train_nerf.py:259) computes densely.  With the option on,
 * nerfhip_mlp_bwd (and the render backward entry points, which end in it) first lists the samples whose g_out row is not all zero
 * (ascending sample index; two small launches, no atomics, no host synchronisation), the data-gradient kernels walk that list and
 * the weight-gradient kernels sum over it: the same sums in a fixed order with their zero terms dropped -- equal to the dense
 * gradient up to the rounding of a different split of the sample range over the workgroups.  The forward and the stash are
 * unchanged.  A launch whose regions exceed 4 GiB (m >= 2^22 sample points) runs dense regardless.
 *   on = 0  dense (default);
 *   on = 1  compacted: the training forward writes the whole stash as always, the weight-gradient kernels gather the listed samples'
 *           rows out of it;
 *   on = 2  compacted AND recomputed, inside the fused render entry points (nerfhip_render_fwd / _bwd and their _parts forms): the
 *           training forward of this plan writes NO stash (it is the inference instantiation of the same kernel: bit-identical
 *           outputs), and the backward, once it has the list, re-runs the forward for the listed samples only, which leaves their
 *           activation rows and ReLU masks in list order -- the weight-gradient kernels then read contiguous blocks.  Pays where most
 *           rows are dropped and the stash-writing forward is much slower than the plain one (the fp16-piece plans: DESIGN.md).
 *           nerfhip_mlp_fwd / nerfhip_mlp_bwd, whose caller owns the stash between the two calls, treat 2 as 1.
 *   on = 3  fused (plans with an LDS-resident image only: fp32, hidden_size <= 64, view directions, at most 4 layers none of which is a
 *           skip layer, num_encoding_fn_xyz <= 10, num_encoding_fn_dir <= 4 -- config/fern.yml, config/llff.yml; other plans:
 *           NERFHIP_ERR_ARG), inside the fused render entry points: the training forward writes no stash, and ONE persistent kernel per
 *           net keeps all its weights in LDS, recomputes the forward of 128 sample points at a time, runs the data-gradient chain and
 *           sums the weight gradients in registers -- no stash, no d(pre-activation) images, no separate weight-gradient kernel; a
 *           fixed-order reduction of one partial per workgroup follows (no atomics: bit-reproducible).  Every sample is differentiated.
 *   on = 4  fused over the list: the same kernel walks the samples whose d(raw) row is not all zero (the list of mode 1).
 *   on = 5  fused over a register-image stash (same plans as 3): the training forward -- the persistent LDS-resident kernel -- also
 *           stores the registers the backward's chain works on (both encodings, every layer's activations: 64 L + 192 floats per
 *           sample point, whole-KiB stores, inside the plan's stash region of the render workspace), and the fused kernel reads them
 *           back (each array re-loaded for the next 64 samples right behind its last use) instead of recomputing the forward.  Same
 *           arithmetic on the same values in the same order as 3: the gradient is bit-identical; a third fewer multiplies in the
 *           backward for 2 x 1.8 KB of HBM traffic per sample point.  Every sample is differentiated.
 *           A render backward that must leave the d(pre-activation) images (nerfhip_render_bwd_rays with g_rays) runs 3 / 4 / 5 as 2;
 *           nerfhip_mlp_fwd / nerfhip_mlp_bwd treat them as 1. */
int nerfhip_plan_set_bwd_compaction(nerfhip_plan_t plan, int on);
int nerfhip_plan_bwd_compaction(nerfhip_plan_t plan);
/* Byte offset, inside a backward scratch for m sample points, of int32[2] = {samples the last compacted backward kept, samples of
 * that launch} (written on the launch stream; meaningful after a compacted nerfhip_mlp_bwd only).  Inside a render workspace the
 * scratch of a net is the region "bwd_scratch_coarse" / "bwd_scratch_fine" (nerfhip_render_workspace_region), m = n_rays * samples. */
int64_t nerfhip_plan_bwd_stats_offset(nerfhip_plan_t plan, int64_t m);
/* Frequency bands (host float[16] each) exactly as the reference builds them are supplied by the caller. */
int nerfhip_plan_set_freqs(nerfhip_plan_t plan, const float* freqs_xyz, const float* freqs_dir);

/* FlexibleNeRFModel.forward (nerf/models.py:233-256) on already-encoded rows x: dev [m, dim_xyz+dim_dir] ->
 * out: dev [m,4] = cat(rgb_raw, sigma_raw).  stash: NULL (inference) or dev buffer of
 * nerfhip_plan_stash_bytes(plan, m) for a later nerfhip_mlp_bwd. */
int nerfhip_mlp_fwd(nerfhip_plan_t plan, const float* packed, const float* x, int64_t m, float* out, void* stash,
                    nerfhip_stream_t stream);
/* Backward w.r.t. all parameters (what autograd computes for models.py:233-256): g_out: dev [m,4]; g_params: dev
 * flat gradient vector (overwritten); scratch: dev, nerfhip_plan_bwd_scratch_bytes. */
int nerfhip_mlp_bwd(nerfhip_plan_t plan, const float* packed, const float* g_out, int64_t m, const void* stash,
                    void* scratch, int64_t scratch_bytes, float* g_params, nerfhip_stream_t stream);
/* Gradient w.r.t. the encoded input x of the same forward (autograd gives it for models.py:233-256 when x requires
 * grad; the render path never does): call after nerfhip_mlp_bwd with the same m and scratch (it reads the
 * d(pre-activation) images left there).  params: dev flat parameter vector (reference layout, not the packed image);
 * g_x: dev [m, dim_xyz+dim_dir] (overwritten). */
int nerfhip_mlp_bwd_input(nerfhip_plan_t plan, const float* params, int64_t m, const void* scratch, float* g_x,
                          nerfhip_stream_t stream);

/* ---- fused render (predict_and_render_radiance, nerf/train_utils.py:28-127, + run_network :8-25) --------------- */
typedef struct nerfhip_render_cfg {
    int num_coarse;
    int num_fine; /* 0 = coarse only */
    int perturb;
    int lindisp;
    int white_background;
    float noise_std; /* radiance_field_noise_std */
    int ray_stride;  /* 8 or 11 floats per ray row */
} nerfhip_render_cfg;

/* Caller-supplied random draws (each may be NULL -> in-kernel generator). */
typedef struct nerfhip_render_rand {
    const float* t_rand;       /* [n, num_coarse]            stream 0 */
    const float* noise_coarse; /* [n, num_coarse]            stream 1 */
    const float* u;            /* [n, num_fine]              stream 2 */
    const float* noise_fine;   /* [n, num_coarse + num_fine] stream 3 */
} nerfhip_render_rand;

/* Outputs; any pointer may be NULL.  *_fine are ignored when num_fine == 0. */
typedef struct nerfhip_render_out {
    float* rgb_coarse;   /* [n,3] */
    float* disp_coarse;  /* [n]   */
    float* acc_coarse;   /* [n]   */
    float* depth_coarse; /* [n]   (not returned by the reference) */
    float* rgb_fine;
    float* disp_fine;
    float* acc_fine;
    float* depth_fine;
} nerfhip_render_out;

/* training: 0 = inference (no activation stash); 1 = training with one set of backward buffers per net (required when
 * the two nets' backward chains run on different streams, nerfhip_render_bwd_parts); 2 = training with ONE set of
 * backward buffers shared by the two nets (smaller: by the coarse net's d(pre-activation) scratch; valid for
 * nerfhip_render_bwd and for parts calls that pass NERFHIP_PART_SHARED_BWD). */
int64_t nerfhip_render_workspace_bytes(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine,
                                       const nerfhip_render_cfg* cfg, int64_t n_rays, int training);

/* Where a forward leaves its per-sample intermediates inside the workspace (byte offset and size), for inspection:
 * name = "z_coarse" [n,nc] (nerf/train_utils.py:58-65), "raw_coarse" [n,nc,4] (run_network's output, :70-77),
 * "weights_coarse" [n,nc] (:86), "z_fine" [n,nc+nf] (:103-105), "raw_fine" [n,nc+nf,4] (:108-115).  The reference
 * function returns none of them; the parity tests read the sample depths to count inverse-CDF index flips.
 * Training layouts also name "bwd_scratch_coarse" / "bwd_scratch_fine": the scratch each net's backward runs in, and
 * "bwd_g_raw_coarse" [n,nc,4] / "bwd_g_raw_fine" [n,nc+nf,4]: d(loss)/d(raw) as the net's compositing backward left it (training = 2:
 * the two share one buffer, which holds the rows of the net whose backward ran last). */
int nerfhip_render_workspace_region(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine, const nerfhip_render_cfg* cfg,
                                    int64_t n_rays, int training, const char* name, int64_t* offset, int64_t* bytes);

/* rays: dev [n, ray_stride]; t_vals: dev [num_coarse] linspace(0,1); u_det: dev [num_fine] linspace(0,1) (used
 * when perturb == 0); workspace: dev, nerfhip_render_workspace_bytes (keeps everything render_bwd needs when
 * training != 0). */
int nerfhip_render_fwd(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine, const nerfhip_render_cfg* cfg,
                       const float* rays, int64_t n_rays, const float* packed_coarse, const float* packed_fine,
                       const float* t_vals, const float* u_det, const nerfhip_render_rand* rnd, uint64_t seed,
                       uint64_t ray_offset, const nerfhip_render_out* out, void* workspace, int64_t workspace_bytes,
                       int training, nerfhip_stream_t stream);

/* Backward of the fused render w.r.t. both nets' parameters.  g_rgb_coarse / g_rgb_fine: dev [n,3] cotangents of
 * the two colour maps (the only outputs the reference's loss touches, train_nerf.py:244-258).  g_params_*: dev
 * flat gradient vectors (overwritten).  The workspace must be the one a training nerfhip_render_fwd filled (sized
 * with training = 1 or 2), with the same rays / packed weights / random arguments. */
int nerfhip_render_bwd(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine, const nerfhip_render_cfg* cfg,
                       const float* rays, int64_t n_rays, const float* packed_coarse, const float* packed_fine,
                       const nerfhip_render_rand* rnd, uint64_t seed, uint64_t ray_offset, const float* g_rgb_coarse,
                       const float* g_rgb_fine, void* workspace, int64_t workspace_bytes, float* g_params_coarse,
                       float* g_params_fine, nerfhip_stream_t stream);

/* The same two calls cut at the coarse / fine seam (`parts`: NERFHIP_PART_COARSE, NERFHIP_PART_FINE or both).  The
 * reference runs coarse forward -> fine forward -> one backward sequentially (nerf/train_utils.py:68-117,
 * train_nerf.py:244-259); the coarse net's backward only needs the coarse colour map, so a caller may enqueue it on a
 * second stream while the fine forward still runs, and launch the fine net's gradient all-reduce while the coarse
 * backward is in flight (TrainEngine does both).  The fine part reads what the coarse part left in the workspace
 * (depths, weights); each net's backward uses its own scratch region of the workspace.  Cotangents of the depth and
 * accumulation maps are optional (NULL = 0): losses that only touch the colour maps pass g_rgb_* alone. */
#define NERFHIP_PART_COARSE 1
#define NERFHIP_PART_FINE 2
/* nerfhip_render_bwd_parts only: the caller runs the two nets' backward chains one after the other on one stream, so
 * they may share one set of backward buffers (workspace sized with training = 2 or 1). */
#define NERFHIP_PART_SHARED_BWD 4
typedef struct nerfhip_render_cotangents {
    const float* g_rgb_coarse;   /* [n,3] */
    const float* g_acc_coarse;   /* [n]   */
    const float* g_depth_coarse; /* [n]   */
    const float* g_rgb_fine;
    const float* g_acc_fine;
    const float* g_depth_fine;
} nerfhip_render_cotangents;
int nerfhip_render_fwd_parts(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine, const nerfhip_render_cfg* cfg,
                             const float* rays, int64_t n_rays, const float* packed_coarse, const float* packed_fine,
                             const float* t_vals, const float* u_det, const nerfhip_render_rand* rnd, uint64_t seed,
                             uint64_t ray_offset, const nerfhip_render_out* out, void* workspace,
                             int64_t workspace_bytes, int training, int parts, nerfhip_stream_t stream);
int nerfhip_render_bwd_parts(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine, const nerfhip_render_cfg* cfg,
                             const float* rays, int64_t n_rays, const float* packed_coarse, const float* packed_fine,
                             const nerfhip_render_rand* rnd, uint64_t seed, uint64_t ray_offset,
                             const nerfhip_render_cotangents* g, void* workspace, int64_t workspace_bytes,
                             float* g_params_coarse, float* g_params_fine, int parts, nerfhip_stream_t stream);

/* nerfhip_render_bwd_parts that ALSO returns d(loss)/d(rays): under autograd the reference differentiates
 * pts = ro + rd * z (nerf/train_utils.py:67,107) and dists * ||rd|| (nerf/volume_rendering_utils.py:24) w.r.t. the ray
 * batch (pose optimisation).  params_*: dev flat parameter vectors (reference layout -- the packed images do not hold
 * the encoding columns in a usable order); tmp: dev scratch of nerfhip_render_bwd_rays_tmp_bytes; g_rays: dev
 * [n, ray_stride], overwritten: columns 0..2 d/d(origin), 3..5 d/d(direction), 8..10 d/d(viewdirs), the rest 0 (the
 * depths are constants of the ray: near / far carry no gradient, as for every loss the reference's scripts build).
 * g_rays == NULL (then params_* / tmp may be NULL) is exactly nerfhip_render_bwd_parts. */
int64_t nerfhip_render_bwd_rays_tmp_bytes(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine, const nerfhip_render_cfg* cfg,
                                          int64_t n_rays);
int nerfhip_render_bwd_rays(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine, const nerfhip_render_cfg* cfg,
                            const float* rays, int64_t n_rays, const float* packed_coarse, const float* packed_fine,
                            const nerfhip_render_rand* rnd, uint64_t seed, uint64_t ray_offset,
                            const nerfhip_render_cotangents* g, void* workspace, int64_t workspace_bytes,
                            float* g_params_coarse, float* g_params_fine, int parts, const float* params_coarse,
                            const float* params_fine, void* tmp, int64_t tmp_bytes, float* g_rays, nerfhip_stream_t stream);

/* The two backward entry points above with a cotangent of the RAY WEIGHTS w_i = alpha_i T_i of each pass as well (losses on the
 * distribution of weights along a ray: nerfhip_spread_loss below): g_weights_coarse dev [n, num_coarse], g_weights_fine dev
 * [n, num_coarse + num_fine], each NULL = 0.  They reach the compositing backward as nerfhip_volume_render_bwd's g_weights; a pass
 * runs if any of its four cotangents is given.  The first six members are nerfhip_render_cotangents; with both weight cotangents NULL
 * each call is, bit for bit, the entry point it extends. */
typedef struct nerfhip_render_cotangents_w {
    const float* g_rgb_coarse;
    const float* g_acc_coarse;
    const float* g_depth_coarse;
    const float* g_rgb_fine;
    const float* g_acc_fine;
    const float* g_depth_fine;
    const float* g_weights_coarse; /* [n, num_coarse]            */
    const float* g_weights_fine;   /* [n, num_coarse + num_fine] */
} nerfhip_render_cotangents_w;
int nerfhip_render_bwd_parts_w(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine, const nerfhip_render_cfg* cfg,
                               const float* rays, int64_t n_rays, const float* packed_coarse, const float* packed_fine,
                               const nerfhip_render_rand* rnd, uint64_t seed, uint64_t ray_offset,
                               const nerfhip_render_cotangents_w* g, void* workspace, int64_t workspace_bytes,
                               float* g_params_coarse, float* g_params_fine, int parts, nerfhip_stream_t stream);
int nerfhip_render_bwd_rays_w(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine, const nerfhip_render_cfg* cfg,
                              const float* rays, int64_t n_rays, const float* packed_coarse, const float* packed_fine,
                              const nerfhip_render_rand* rnd, uint64_t seed, uint64_t ray_offset,
                              const nerfhip_render_cotangents_w* g, void* workspace, int64_t workspace_bytes,
                              float* g_params_coarse, float* g_params_fine, int parts, const float* params_coarse,
                              const float* params_fine, void* tmp, int64_t tmp_bytes, float* g_rays, nerfhip_stream_t stream);

/* ---- ray-weight spread loss (mip-NeRF 360's L_dist, Barron et al. 2022, eq. 15) ------------------------------------------------
 * ("Distortion" names the lens in this library; this regulariser measures the SPREAD of a ray's weights.)  For one ray of a pass with
 * s samples, depths z_0 <= ... <= z_{s-1}, and near, far = columns 6, 7 of its packed row:
 *     inv   = far > near ? 1 / (far - near) : 0
 *     s_i   = (z_i - near) inv
 *     e_i   = s_{i+1} for i < s - 1,   e_{s-1} = max(s_{s-1}, 1)          (the last sample owns [z_{s-1}, far])
 *     m_i   = (s_i + e_i) / 2,         delta_i = e_i - s_i                 (formed in fp64 from the fp32 depths)
 *     w_i   = alpha_i T_i exactly as the compositing forms it (nerfhip_volume_render_fwd's weights, bit for bit: the same noise
 *             draws -- noise_std, noise, seed, rng_stream, ray_offset -- and fp64 transmittance scan)
 *     L     = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i
 *     dL/dw_i = 2 [m_i (W_<i - W_>i) - (WM_<i - WM_>i)] + (2/3) w_i delta_i,
 *             W_<i = sum_{j<i} w_j, WM_<i = sum_{j<i} w_j m_j, likewise _>i   (valid because m ascends; ties are harmless)
 * The depths are constants (the reference detaches the fine samples; the coarse ones do not depend on parameters): the gradient
 * reaches the nets through w alone.  A ray with inv = 0 has L = 0 and a zero gradient; NaN propagates.  O(s) per ray: prefix and
 * suffix sums in fp64, a fixed order of summation (no atomics), each output rounded to fp32 once.
 * raw dev [n,s,4], z dev [n,s], rays dev [n, ray_stride >= 8]; loss (optional) dev [n]: the unscaled L of each ray; g_weights
 * (optional) dev [n,s] = scale_ray dL/dw_i, scale_ray = scale * (g_loss ? g_loss[ray] : 1), g_loss dev [n] or NULL -- the cotangent
 * nerfhip_volume_render_bwd and the _w entry points above take.  At least one output; 1 <= s <= 8192; n == 0 launches nothing. */
int nerfhip_spread_loss(const float* raw, const float* z, const float* rays, int ray_stride, int64_t n, int s, float noise_std,
                        const float* noise, uint64_t seed, uint32_t rng_stream, uint64_t ray_offset, float scale,
                        const float* g_loss, float* loss, float* g_weights, nerfhip_stream_t stream);

/* ---- depth priors (DS-NeRF, Deng et al. 2022): supervise the ray weights from sparse per-ray depths ------------------------------
 * One pass of one ray has s samples at depths z_0 <= ... <= z_{s-1} (the ray parameter t: for this library's pin-hole rays, whose
 * camera-frame direction has third component -1, the camera-space z-depth of a structure-from-motion point; for NDC rays the units
 * are the caller's), far = column 7 of its packed row, and the weights w_i = alpha_i T_i exactly as the compositing forms them (as
 * for nerfhip_spread_loss: the same noise draws and fp64 transmittance scan).  Its prior row is (D, c, sigma): depth, confidence
 * weight, standard deviation.  If !(c > 0) -- c = NaN included -- the ray has NO PRIOR: both losses are exactly 0, its gradient row
 * exactly 0, D and sigma are not interpreted (NaN or garbage there is harmless), and raw is not read for it.  Otherwise, with
 * eps = 1e-5:
 *     d^   = sum_i w_i z_i
 *     E    = c (d^ - D)^2                                                           the "expected-depth" term
 *     k_i  = exp(-(z_i - D)^2 / (2 sigma^2)),  delta_i = z_{i+1} - z_i,  delta_{s-1} = max(far - z_{s-1}, 0)
 *     Tm   = c sum_i -log(w_i + eps) k_i delta_i                                    the "termination" term (DS-NeRF eq. 10, its code's eps)
 *     dE/dw_i = 2 c (d^ - D) z_i               dTm/dw_i = -c k_i delta_i / (w_i + eps)
 * The depths are constants, as for the spread loss: the gradient reaches the nets (and the rays) through w alone.  NaN in raw
 * propagates on a ray with c > 0.  A row with c > 0 and sigma <= 0 is outside the contract (no access leaves the buffers for it).
 * raw dev [n,s,4], z dev [n,s], rays dev [n, ray_stride >= 8].  The prior row of ray r is prior + (inds ? inds[r] : r) * prior_stride
 * (prior dev, prior_stride >= 3 floats; inds dev int64 [n] or NULL); an index outside [0, prior_rows) is a row without a prior, and
 * nothing is read for it.  loss (optional) dev [n,2]: (E, Tm) of each ray, unscaled.  g_weights (optional) dev [n,s]:
 *     g_weights[r,i] = scale (w_expected g_loss[r,0] dE/dw_i + w_termination g_loss[r,1] dTm/dw_i)
 * formed in fp64 and rounded to fp32 once; g_loss dev [n,2] or NULL (= 1): the cotangents of the two losses.  A term whose weight is
 * exactly 0 contributes nothing (not 0 * inf).  accumulate != 0: the value is ADDED to what g_weights[r,i] holds (one fp32 add), and a
 * ray without a prior leaves its row untouched -- the term stacks on the cotangent nerfhip_spread_loss wrote; accumulate == 0: every
 * row is written, zeros for a ray without a prior.  At least one output, and a single-output call gives the combined call's bits;
 * 1 <= s <= 8192; n == 0 launches nothing.  O(s) per ray, fp64 sums in a fixed order (no atomics). */
int nerfhip_depth_prior_loss(const float* raw, const float* z, const float* rays, int ray_stride, int64_t n, int s, float noise_std,
                             const float* noise, uint64_t seed, uint32_t rng_stream, uint64_t ray_offset, const float* prior,
                             int64_t prior_stride, const int64_t* inds, int64_t prior_rows, float w_expected, float w_termination,
                             float scale, const float* g_loss, float* loss, float* g_weights, int accumulate,
                             nerfhip_stream_t stream);

/* ---- interlevel proposal loss (mip-NeRF 360's L_prop, Barron et al. 2022, eq. 13): train the coarse net from the fine weights ----
 * One ray has a coarse pass and a fine pass:
 * - The coarse pass has Sc samples at depths z^_0 <= ... <= z^_{Sc-1} with weights w^_j.
 * - The fine pass has Sf samples at depths z_0 <= ... <= z_{Sf-1} with weights w_i.
 * - Both sets of weights are formed exactly as the compositing forms them. That means nerfhip_volume_render_fwd's weights bit for
 *   bit: the same noise draws (streams 1 and 3) and the same fp64 transmittance scan, as in spread.hip.
 * - far is column 7 of the packed row.
 * Edges follow the spread loss's convention. Sample k owns [z_k, z_{k+1}], and the last sample owns [z_last, max(far, z_last)]:
 *     e^_0..e^_Sc :  e^_j = z^_j (j < Sc),  e^_Sc = max(far, z^_{Sc-1})        e_0..e_Sf likewise from z
 *     lo_i = min( #{k in 1..Sc   : e^_k <= e_i     },  Sc-1 )              (searchsorted right on e^[1:])
 *     hi_i = max( #{k in 0..Sc-1 : e^_k <  e_{i+1} } - 1,  lo_i )          (searchsorted left on e^[:-1])
 *     B_i  = sum_{j=lo_i..hi_i} w^_j                                       (the bound: coarse intervals overlapping fine interval i)
 *     L    = sum_i max(0, w_i - B_i)^2 / (w_i + eps),   eps = 2^-23        (multinerf's eps)
 *     dL/dw^_j = sum_{i : lo_i <= j <= hi_i}  -2 max(0, w_i - B_i) / (w_i + eps)
 *     dL/dw_i == 0                                                         (stop-gradient on the fine weights)
 * - The comparisons are on the fp32 depths, which is exact.
 * - Every fine interval overlaps at least one coarse interval. This covers zero-width intervals, the deterministic case
 *   z_last == far, and fine samples outside the coarse range.
 * - Exactly touching intervals do not overlap.
 * - lo and hi are non-decreasing in i. Hence the set of i that reaches a given j is a contiguous range.
 * - Depths are constants, as for the sibling losses. NaN in either raw propagates.
 * raw_coarse dev [n,Sc,4], z_coarse dev [n,Sc], raw_fine dev [n,Sf,4], z_fine dev [n,Sf], rays dev [n, ray_stride >= 8];
 * noise_coarse dev [n,Sc] / noise_fine dev [n,Sf] or NULL (in-kernel draws of streams 1 / 3 keyed by seed and ray_offset), read
 * when noise_std > 0.  loss (optional) dev [n]: the unscaled L of each ray.  g_weights_coarse (optional) dev [n,Sc] =
 * scale * (g_loss ? g_loss[r] : 1) * dL/dw^_j, g_loss dev [n] or NULL: the coarse pass's cotangent that nerfhip_volume_render_bwd and
 * the _w entry points take.  accumulate != 0: the value is ADDED to what g_weights_coarse[r,j] holds (one fp32 add) -- the term
 * stacks behind the spread and depth terms; accumulate == 0: every entry is written.  At least one output, and a single-output call
 * gives the combined call's bits.  Sc >= 1, Sf >= 1, and THE CAP: Sc + Sf <= 4096 (the ray's prefix sums and index ranges live in
 * 20 / 12 bytes of LDS per coarse / fine sample, 80 KiB at most); anything above is refused, never launched.  n == 0 launches nothing.
 * O((Sc + Sf) log) per ray: fp64 prefix sums in a fixed order (no atomics; the coarse prefix in two doubles, so that B_i behind an
 * opaque sample keeps its own relative precision), bounded binary searches, each output rounded to fp32 once. */
int nerfhip_proposal_loss(const float* raw_coarse, const float* z_coarse, int s_coarse, const float* raw_fine, const float* z_fine,
                          int s_fine, const float* rays, int ray_stride, int64_t n, float noise_std, const float* noise_coarse,
                          const float* noise_fine, uint64_t seed, uint64_t ray_offset, float scale, const float* g_loss, float* loss,
                          float* g_weights_coarse, int accumulate, nerfhip_stream_t stream);

/* d(loss)/d(rays) ALONE, for frozen nets (camera localisation against a trained field): nerfhip_render_bwd_rays' contract -- parts,
 * NERFHIP_PART_SHARED_BWD, the first pass that runs overwrites g_rays and the second accumulates, params_* = the flat vectors the
 * packed images were made from (theta_eff under an encoding window) -- without g_params: no parameter gradient is computed or
 * stored (no weight-gradient launch, no reduction).  Per pass: compositing backward, the plan's list / recomputation and its
 * data-gradient chain (fused 64-wide modes run as mode 2), then the input-gradient GEMM and the positional encoding's backward in one
 * MFMA kernel and a per-ray sum (nh_raygrad.h).  tmp: dev scratch of nerfhip_render_grad_rays_tmp_bytes (16-byte aligned).  A sample's
 * contribution depends only on that sample, so plans in mode 0, 1 and 2 give the same bits.  n_rays == 0: nothing is launched. */
int64_t nerfhip_render_grad_rays_tmp_bytes(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine, const nerfhip_render_cfg* cfg,
                                           int64_t n_rays);
int nerfhip_render_grad_rays(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine, const nerfhip_render_cfg* cfg,
                             const float* rays, int64_t n_rays, const float* packed_coarse, const float* packed_fine,
                             const nerfhip_render_rand* rnd, uint64_t seed, uint64_t ray_offset,
                             const nerfhip_render_cotangents* g, void* workspace, int64_t workspace_bytes, int parts,
                             const float* params_coarse, const float* params_fine, void* tmp, int64_t tmp_bytes, float* g_rays,
                             nerfhip_stream_t stream);

/* ---- occupancy grid: the inference render skips empty space (Instant-NGP / NerfAcc / PlenOctrees style) ------------------------
 * One bit per cell of an axis-aligned box, built once from the trained density.  A sample whose point falls into an empty cell is
 * never sent through the MLP: its raw row becomes the EMPTY ROW (0, 0, 0, NERFHIP_OCC_EMPTY_RAW), whose sigma_a =
 * relu(raw[3] + noise) is exactly 0 -- a finite value on purpose: no 0 * inf can arise downstream.  (In training: further below.)
 *
 * Cell of point p: i_a = (int)floorf((p_a - lo_a) * inv_a), inv_a = res_a / (hi_a - lo_a) formed once on the host in fp32 (as
 * (float)res_a / (hi_a - lo_a)); bit index b = (i_z * res_y + i_y) * res_x + i_x lives in word b >> 5 at position b & 31.  The point
 * is the one the MLP kernels encode: p_a = ro_a + rd_a * z (an fp32 multiply, then an fp32 add) of the packed ray row -- for NDC rays
 * the NDC-space point.  A point outside the box counts as `outside` says; a sample with a NaN coordinate counts as occupied (it
 * propagates as in the dense path).  1 <= res_a <= 512, res_x * res_y * res_z a multiple of 32, hi_a > lo_a. */
#define NERFHIP_OCC_EMPTY_RAW (-1e30f)
#define NERFHIP_OCC_MAX_RES 512
typedef struct nerfhip_occ_grid {
    const uint32_t* bits; /* dev [res_x * res_y * res_z / 32] */
    float lo[3], hi[3];
    int res[3];
    int outside; /* a point outside the box: 0 = empty, 1 = occupied */
} nerfhip_occ_grid;

/* The per-sample predicate alone (tests, diagnostics): flags_u8 dev [n * S], 1 = the cell of sample (ray, s) is occupied.
 * rays: dev [n, ray_stride]; z: dev [n, S]. */
int nerfhip_occ_mark(const float* rays, int ray_stride, int64_t n, const float* z, int S, const nerfhip_occ_grid* grid,
                     uint8_t* flags_u8, nerfhip_stream_t stream);

/* One probe per cell of [cell_first, cell_first + cell_count) (both multiples of 32; cells in bit-index order) through the plan's
 * ordinary inference forward; bit b |= (raw[3] of cell b's probe > tau).  Bits are only ever set: the caller zeroes `grid->bits`
 * before the first pass (grid->bits is written, its const notwithstanding; every word has a single writer).  A NaN raw[3] sets
 * nothing.  pass 0 probes the cell centre lo + (i + 0.5) * cell, cell_a = (hi_a - lo_a) / res_a in fp32; pass k > 0 probes
 * lo + (i + u) * cell, u_a = draw (3 * (k * ncells + b) + a) of the uniform generator (nerfhip_rng_fill, NERFHIP_RNG_UNIFORM) under
 * `seed` with stream id NERFHIP_OCC_RNG_STREAM, ncells = res_x * res_y * res_z.
 * tmp (dev, 256-byte aligned, nerfhip_occ_update_tmp_bytes(cell_count)) holds, and keeps after the call:
 *   offset 0                              probe rows [cell_count, 11]: packed ray rows (probe point, direction 0 0 0, near 0, far 0,
 *                                         viewdir 0 0 1) -- with the depths below, the fused-input forward encodes exactly the probe
 *   offset r = align256(cell_count * 44)  depths [cell_count], all 0
 *   offset r + align256(cell_count * 4)   raw [cell_count, 4]: the forward's output rows */
#define NERFHIP_OCC_RNG_STREAM 16
int64_t nerfhip_occ_update_tmp_bytes(int64_t cell_count);
int nerfhip_occ_update(nerfhip_plan_t plan, const float* packed, const nerfhip_occ_grid* grid, float tau, int pass, uint64_t seed,
                       int64_t cell_first, int64_t cell_count, void* tmp, int64_t tmp_bytes, nerfhip_stream_t stream);

/* bits_out: a cell is set if it or one of its six face neighbours is set in bits_in; no wrap-around at the box faces.
 * bits_in != bits_out, both dev [res_x * res_y * res_z / 32]; res: host int[3]. */
int nerfhip_occ_dilate(const uint32_t* bits_in, uint32_t* bits_out, const int* res, nerfhip_stream_t stream);

/* nerfhip_render_fwd_parts for inference with empty-space skipping.  Per pass that runs: the samples whose cell is occupied are
 * listed (ascending; the two-launch count / scatter scheme of the compacted backward, no atomics) and every other sample's raw row
 * is set to the empty row; the MLP runs over the list alone and writes each result at its sample's own row (bit for bit the dense
 * kernel's row); the compositing is the unchanged nerfhip_volume_render_fwd.  grid_coarse / grid_fine: host structs (they may be the
 * same one), read during the call.  tmp: dev, 256-byte aligned, nerfhip_render_occ_tmp_bytes; after the call its first four int32 are
 * {kept_coarse, total_coarse, kept_fine, total_fine} (a pass that did not run leaves its pair untouched).  The sample list of the
 * LAST pass that ran stays behind them, for inspection: with Mmax = n_rays * (num_coarse + num_fine) and
 * C = 16 * ceil(ceil(Mmax / 2048) / 16), int32 words 16 .. 16 + C - 1 are per-block counts and the list -- `kept` sample indices,
 * ascending, padded with sample 0 up to the next multiple of 128 -- starts at word 16 + C.
 * Refused (NERFHIP_ERR_ARG, nothing launched): training != 0; a NULL grid of a pass that runs; res out of range or the cell count no
 * multiple of 32; hi <= lo; tmp too small; n_rays * samples >= 2^31; a 512-wide plan or one on the extended encoding registers. */
int64_t nerfhip_render_occ_tmp_bytes(const nerfhip_render_cfg* cfg, int64_t n_rays);
int nerfhip_render_fwd_occ(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine, const nerfhip_render_cfg* cfg,
                           const float* rays, int64_t n_rays, const float* packed_coarse, const float* packed_fine,
                           const float* t_vals, const float* u_det, const nerfhip_render_rand* rnd, uint64_t seed,
                           uint64_t ray_offset, const nerfhip_render_out* out, void* workspace, int64_t workspace_bytes,
                           int training, int parts, const nerfhip_occ_grid* grid_coarse, const nerfhip_occ_grid* grid_fine,
                           void* tmp, int64_t tmp_bytes, nerfhip_stream_t stream);

/* ---- occupancy grid in training: the culled training forward, and a density grid that follows the nets -------------------------
 * nerfhip_render_fwd_occ_train: nerfhip_render_fwd_occ as the forward of a TRAINING step.  Arguments as nerfhip_render_fwd_occ, with
 * training = 1 or 2 naming the workspace layout as in nerfhip_render_fwd_parts; tmp and its four count words as in the inference call.
 * It exists for plans whose training forward leaves nothing in the stash -- backward modes 2 (recompute), 3 (fused) and 4 (fused over
 * the list) of nerfhip_plan_set_bwd_compaction: that forward is the inference forward, so the listed forward gives each kept sample's
 * raw row bit for bit.  The backward entry points (nerfhip_render_bwd_parts, nerfhip_render_bwd) are used as they are: a culled
 * sample's row is the empty row, its weight is exactly 0 and its d(loss)/d(raw) row exactly zero, so the list of a compacted
 * backward (modes 2, 4) drops it by itself and the second forward runs over kept samples only -- the backward IS the gradient of the
 * culled render.  Mode 3 is correct as well (the culled samples contribute exact zeros) but walks every sample: it saves no backward
 * work.  Refused (NERFHIP_ERR_ARG, nothing launched): everything nerfhip_render_fwd_occ refuses except `training`; training not 1
 * or 2; a pass that runs whose plan is in mode 0, 1 or 5, is inference-only (NERFHIP_PRECISION_F16X3), or has more sample points
 * than the recomputing flow takes (ceil(M / 128) * 128 * 1024 >= 2^32). */
int nerfhip_render_fwd_occ_train(nerfhip_plan_t plan_coarse, nerfhip_plan_t plan_fine, const nerfhip_render_cfg* cfg,
                                 const float* rays, int64_t n_rays, const float* packed_coarse, const float* packed_fine,
                                 const float* t_vals, const float* u_det, const nerfhip_render_rand* rnd, uint64_t seed,
                                 uint64_t ray_offset, const nerfhip_render_out* out, void* workspace, int64_t workspace_bytes,
                                 int training, int parts, const nerfhip_occ_grid* grid_coarse, const nerfhip_occ_grid* grid_fine,
                                 void* tmp, int64_t tmp_bytes, nerfhip_stream_t stream);

/* The density grid (Instant-NGP's update rule): dens, dev fp32 [ncells], 16-byte aligned, one value per cell in bit-index order.
 * nerfhip_occ_density_update: probes and draws are EXACTLY those of nerfhip_occ_update -- same `pass` / counter rule, same tmp
 * (nerfhip_occ_update_tmp_bytes(cell_count)) with the same layout kept after the call --, then for every cell b of the range
 *     dens[b] = fmaxf(dens[b] * decay, s),   s = raw[3] > 0 ? raw[3] : 0   (a NaN raw[3]: s = 0, so dens[b] * decay stays)
 * with one writer per cell (a thread takes four consecutive cells: 16-byte loads and stores).  grid: the box and the resolution are
 * read; grid->bits is neither read nor written (it may be NULL).  decay in [0, 1].
 * nerfhip_occ_density_bits: bit b of bits_out (dev [ncells / 32], every word written by its single writer) = dens[b] > thr,
 * thr = min(tau, mean(dens)) -- a grid that is still nearly empty of density does not cull everything.  The mean is a two-stage sum
 * in a fixed order, in fp64: one partial per workgroup of 4096 cells, then one workgroup over the partials in index order; rounded to
 * fp32 once.  tmp (dev, 256-byte aligned, nerfhip_occ_density_bits_tmp_bytes(res)) keeps after the call: offset 0: thr (one float);
 * offset 256: the partials (doubles).  res: host int[3].
 * Refused (NERFHIP_ERR_ARG, nothing launched): a resolution out of range or a cell count no multiple of 32; hi <= lo; a cell range
 * that is not 32-aligned or leaves the grid; pass outside 0 .. 4095; decay outside [0, 1] or NaN; a NaN tau; a NULL or misaligned
 * pointer; tmp too small. */
int nerfhip_occ_density_update(nerfhip_plan_t plan, const float* packed, const nerfhip_occ_grid* grid, float* dens, float decay,
                               int pass, uint64_t seed, int64_t cell_first, int64_t cell_count, void* tmp, int64_t tmp_bytes,
                               nerfhip_stream_t stream);
int64_t nerfhip_occ_density_bits_tmp_bytes(const int* res);
int nerfhip_occ_density_bits(const float* dens, const int* res, float tau, uint32_t* bits_out, void* tmp, int64_t tmp_bytes,
                             nerfhip_stream_t stream);

/* ---- loss + optimiser (train_nerf.py:244-270) ------------------------------------------------------------------ */
/* mse_loss(rgb_coarse, target) + mse_loss(rgb_fine, target) and its cotangents; loss_out: dev float[3] =
 * {coarse_mse, fine_mse, sum}.  target rows have target_stride floats (RGB or RGBA; only [:3] is used). */
int nerfhip_mse_loss_fwd_bwd(const float* rgb_coarse, const float* rgb_fine, const float* target, int target_stride,
                             int64_t n, float grad_scale, float* g_rgb_coarse, float* g_rgb_fine, float* loss_out,
                             nerfhip_stream_t stream);
/* The loss of ONE compositing pass against RGBA targets (one call per net), with its cotangents g_rgb and g_acc for the fused backward
 * (nerfhip_render_cotangents: g_rgb_* / g_acc_*).  rgb: dev [n,3]; acc: dev [n]; target: dev rows of target_stride >= 4 floats
 * (C_r, C_g, C_b, a), alpha straight (un-premultiplied); a is clamped to [0, 1] on read, a NaN propagates.  loss_out: dev float[3] =
 * {photometric, alpha, entropy}, unscaled means.  g_rgb: dev [n,3], g_acc: dev [n]; either may be NULL.
 * Background b_r of ray r: row r of bg (dev [n,3]) if bg != NULL; else, if bg_random, three uniform draws of Philox stream 4, element
 * 3 (ray_offset + r) + c under `seed` -- what nerfhip_rng_fill(NERFHIP_RNG_UNIFORM, seed, 4, 3 ray_offset, 3 n) writes; else the
 * constant (bg_r, bg_g, bg_b).
 * mode 0 (matte): t_c = a C_c + (1 - a) b_c and p_c = rgb_c + (1 - acc) b_c, both in fp64 from the fp32 inputs; d_c = (float)(p_c - t_c);
 *   photometric = sum d_c^2 / (3 n); g_rgb_c = d_c k with k = 2 / (3 n) * grad_scale formed as nerfhip_mse_loss_fwd_bwd forms it;
 *   alpha = sum (acc - a)^2 / n.
 * mode 1 (weight): a is a per-pixel loss weight (a mask of transient objects or sky: 0 = ignore).  d_c = rgb_c - C_c in fp32;
 *   photometric = sum a d_c^2 / (3 n) (the divisor is 3 n, not the sum of the weights: the ranks of a data-parallel step agree on the
 *   scale); g_rgb_c = (d_c k) a; the background is not read; alpha = 0 and lam_alpha must be 0 (alpha is no opacity here).
 * Both modes: entropy = mean of H(x) = -(x log x + (1 - x) log(1 - x)), x = min(max(acc, 1e-6), 1 - 1e-6); dH/dacc = log((1 - x) / x)
 *   inside the clamp and exactly 0 where the clamp acted.
 * g_acc[r] = -sum_c g_rgb_c b_c (matte only) + (2 lam_alpha / n) grad_scale (acc - a) + (lam_entropy / n) grad_scale dH/dacc, formed in
 *   fp64 and rounded once; a term whose weight is exactly 0 contributes nothing (not 0 * inf).
 * One workgroup, fp64 sums in a fixed order, no atomics; the photometric sum walks nerfhip_mse_loss_fwd_bwd's elements in its order, so
 * that in weight mode with a == 1 everywhere loss_out[0] and g_rgb are that entry point's bits.
 * Refused (NERFHIP_ERR_ARG, nothing launched): n <= 0; target_stride < 4; a NULL rgb, acc, target or loss_out; mode not 0 or 1; a
 * negative or non-finite lam_alpha or lam_entropy; lam_alpha != 0 in weight mode. */
int nerfhip_matte_loss_fwd_bwd(const float* rgb, const float* acc, const float* target, int target_stride, int64_t n,
                               int mode, const float* bg, int bg_random, float bg_r, float bg_g, float bg_b,
                               uint64_t seed, uint64_t ray_offset, float lam_alpha, float lam_entropy, float grad_scale,
                               float* g_rgb, float* g_acc, float* loss_out, nerfhip_stream_t stream);
/* The photometric loss of ONE compositing pass under a robust kind, with an optional trim of the call's largest per-ray residuals
 * (one call per net), and its cotangent g_rgb for the fused backward.  rgb: dev [n,3]; target: dev rows of target_stride >= 3 floats.
 * d = rgb_c - t_c, formed in fp32 as nerfhip_mse_loss_fwd_bwd forms it.  rho is formed in fp64 from the fp32 d.  h = psi / 2 is rounded
 * to fp32 once.
 *   kind 0, l2:          rho = d^2;                                                    h = d;                          param ignored
 *   kind 1, l1:          rho = |d|;                                                    h = 0.5 sign(d) (0 at 0);       param ignored
 *   kind 2, huber:       rho = d^2 if |d| <= delta, else delta (2 |d| - delta);        h = d, else delta sign(d);      param = delta > 0
 *   kind 3, charbonnier: rho = sqrt(d^2 + eps^2) - eps;                                h = 0.5 d / sqrt(d^2 + eps^2);  param = eps > 0
 *   kind 4, relative:    rho = d^2 / (p + eps)^2, p = rgb_c held constant (RawNeRF);   h = d / (p + eps)^2;            param = eps > 0
 * The Huber form continues l2 beyond delta, so that delta -> inf recovers the plain loss and a learning rate carries over.
 * Cotangent and loss: k = 2 / (3 n) * grad_scale, formed as nerfhip_mse_loss_fwd_bwd forms it; g_rgb_c = (h k) m_r;
 *   loss = sum_r m_r sum_c rho / (3 n).  The divisor stays 3 n whatever is trimmed (as the matte loss's weight mode: the ranks of a
 *   data-parallel step agree on the scale).
 * Trimming (keep < 1): e_r = (float) sum_c rho(d_c) is the per-ray residual, non-negative.  kk = min(n, max(1, ceil((double)keep * n))).
 *   tau is the kk-th smallest e_r of the call.  m_r = !(e_r > tau): ties at tau are all kept.  A NaN residual is never trimmed (it
 *   sorts behind +inf): its ray stays, and the loss becomes NaN, so divergence remains visible.  tau and the mask are constants of the
 *   step: no gradient flows through them; a trimmed ray's g_rgb row is +0.  keep == 1 runs no selection, reports tau = +inf and
 *   kept = 1, and needs no tmp.
 * loss_out: dev float[3] = {loss, kept fraction = (float)(sum_r m_r / n), tau}.  g_rgb: dev [n,3]; resid_out: dev [n] floats (e_r);
 * mask_out: dev [n] bytes (m_r); each of the three may be NULL.  tmp: dev, nerfhip_robust_loss_tmp_bytes(n) bytes, aligned to 4.
 * One workgroup, fp64 sums in a fixed order, integer counts, no atomics: the results do not depend on scheduling.  Kind 0 with
 * keep == 1 gives nerfhip_mse_loss_fwd_bwd(rgb, NULL, ...)'s loss_out[0] and g_rgb bit for bit (the same element-to-thread
 * assignment, wave sums, block sums and final division), and so does kind 2 with a delta beyond every |d|.
 * Refused (NERFHIP_ERR_ARG, nothing launched): n <= 0 or n >= 2^31; target_stride < 3; a NULL rgb, target or loss_out; a kind outside
 * 0..4; a non-positive or non-finite param where the kind reads it; keep outside (0, 1] or NaN; keep < 1 with tmp NULL, misaligned or
 * smaller than nerfhip_robust_loss_tmp_bytes(n). */
int64_t nerfhip_robust_loss_tmp_bytes(int64_t n);
int nerfhip_robust_loss_fwd_bwd(const float* rgb, const float* target, int target_stride, int64_t n,
                                int kind, float param, float keep, float grad_scale,
                                float* g_rgb, float* resid_out, unsigned char* mask_out, float* loss_out,
                                void* tmp, int64_t tmp_bytes, nerfhip_stream_t stream);
/* torch.optim.Adam single-tensor step (no amsgrad, no weight decay) on a flat vector; step counts from 1. */
int nerfhip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                      float beta1, float beta2, float eps, int64_t step, float grad_scale, nerfhip_stream_t stream);

/* ---- next to the path: training-ray selection and the 8-bit output stage -------- */
/* Distinct sample positions: out[i] = P(first + i), P = a keyed pseudo-random permutation of [0, population)
 * (6-round Feistel network, cycle-walking; round keys = Philox4x32-10(seed, step)).  Replaces
 * np.random.choice(population, n, replace=False) of train_nerf.py:185-189 and :219-221: distinct, uniformly
 * spread, reproducible, O(1) per index; ranks of a data-parallel job take disjoint [first, first+n) ranges of the
 * same permutation.  population <= 2^32, first + n <= population. */
int nerfhip_select_indices(uint64_t seed, uint64_t step, int64_t population, int64_t first, int64_t n, int64_t* out,
                           nerfhip_stream_t stream);

typedef struct nerfhip_select_cfg {
    int32_t height, width; /* select index k addresses pixel (row k % height, col k / height): the reference goes
                              through coords = stack(meshgrid_xy(arange(H), arange(W)), -1).reshape(-1, 2)
                              (train_nerf.py:214-225) */
    float focal;
    float near, far;       /* options.dataset.near / far (train_utils.py:164-165) */
    int32_t use_viewdirs;  /* rows of 11 floats (else 8) */
    int32_t ndc;           /* options.dataset.no_ndc is False: ndc_rays(H, W, focal, 1.0, ...) (train_utils.py:156-160) */
    float ndc_near, ndc_cw, ndc_ch, ndc_two_near, ndc_neg_two_near; /* as for nerfhip_ndc_rays */
    int32_t channels;      /* floats per target pixel (3 or 4); the loss reads [:3] */
    uint64_t seed, step;   /* permutation key, used when select_inds == NULL */
    int64_t first;         /* first permutation position of this rank */
} nerfhip_select_cfg;

/* Image branch of the training loop (train_nerf.py:210-227) fused with run_one_iter_of_nerf's ray packing
 * (train_utils.py:143-168): for n selected pixels generate ONLY their rays from the pose (c2w: dev, row-major,
 * row stride c2w_ld >= 4), write packed rows rays[n, 8|11] and gather target[n, channels] from image[H, W, channels]
 * (image/target may be NULL).  select_inds: dev int64 [n] flat select indices as the reference draws them, or NULL
 * to draw them here (nerfhip_select_indices with population H*W); inds_out (optional) receives the indices used. */
int nerfhip_select_rays(const nerfhip_select_cfg* cfg, const float* c2w, int c2w_ld, const float* image,
                        const int64_t* select_inds, int64_t n, float* rays, float* target, int64_t* inds_out,
                        nerfhip_stream_t stream);
/* Cached branch (train_nerf.py:175-194): rows of a stored ray bundle (ray_origins / ray_directions: dev
 * [population, 3]) and of targets[population, channels]. */
int nerfhip_select_cached_rays(const nerfhip_select_cfg* cfg, const float* ray_origins, const float* ray_directions,
                               const float* targets, int64_t population, const int64_t* select_inds, int64_t n,
                               float* rays, float* target, int64_t* inds_out, nerfhip_stream_t stream);

/* ---- pose gradient (pose refinement: NeRF--, BARF, noisy COLMAP poses) --------------------------------------------------
 * The reference's get_ray_bundle is torch arithmetic on tform_cam2world, so autograd carries d(loss)/d(rays) back to a pose
 * that requires grad.  These are the vector-Jacobian products of nerfhip_ray_bundle and nerfhip_select_rays w.r.t. c2w:
 * g_c2w: dev float[3, 4] (row-major, overwritten) = d(loss)/d(c2w[:3, :4]) summed over the n rays (the rows of c2w below the
 * third carry no gradient).  The sum is a fixed-order reduction without atomics (per-workgroup partials in tmp, then one
 * workgroup sums them): its order depends on n only, so the result is bit-reproducible from run to run and machine to
 * machine.  tmp: dev scratch of nerfhip_pose_grad_tmp_bytes(n) bytes (-1 for n < 0).  Two launches on `stream`. */
int64_t nerfhip_pose_grad_tmp_bytes(int64_t n);
/* VJP of nerfhip_ray_bundle: pixels as there (NULL = all height*width pixels in row order, then n must be height*width);
 * g_ray_origins / g_ray_directions: dev [n,3] cotangents of its two outputs (either may be NULL = zero, not both unless
 * n == 0). */
int nerfhip_ray_bundle_bwd(int height, int width, float focal, const int64_t* pixels, int64_t n, const float* g_ray_origins,
                           const float* g_ray_directions, void* tmp, int64_t tmp_bytes, float* g_c2w, nerfhip_stream_t stream);
/* VJP of nerfhip_select_rays (image branch: pin-hole rays -> optional ndc_rays -> [o d near far viewdirs] rows).  cfg / c2w /
 * c2w_ld: those of the forward; inds: dev int64 [n], the inds_out of the forward (the select indices it used); g_rays: dev
 * rows [n, g_rays_stride >= 8|11] of d(loss)/d(rays); g_rays_2: a second set of rows of the same layout that is added to the
 * first one row by row before anything else (the coarse and the fine net's parts of the ray gradient), or NULL.  Columns
 * 6 / 7 (near / far) carry no gradient; 8..10 go through the normalisation of the pre-NDC direction. */
int nerfhip_select_rays_bwd(const nerfhip_select_cfg* cfg, const float* c2w, int c2w_ld, const int64_t* inds, int64_t n,
                            const float* g_rays, const float* g_rays_2, int g_rays_stride, void* tmp, int64_t tmp_bytes,
                            float* g_c2w, nerfhip_stream_t stream);

/* ---- one batch over a stack of views (batching across the image set; refining all cameras of a capture at once) --------
 * The image branch of nerfhip_select_rays over the population num_views * H * W: global index g addresses view
 * v = g / (H * W) and the reference's flat select index k = g % (H * W) of that view (row k % height, col k / height, as
 * above).  poses: dev, the pose of view v starts at poses + v * pose_view_stride floats, row-major with row stride
 * pose_ld >= 4 (a contiguous [V, 4, 4] or [V, 3, 4] table, or a strided slice of a larger one; pose_view_stride >=
 * 2 * pose_ld + 4 when num_views > 1); images: dev [V, H, W, channels] or NULL.  Height, width, focal, near / far, NDC and
 * viewdirs come from cfg and are shared by all views (intrinsics that live on the device, fx != fy or an off-centre principal
 * point: the `intr` forms below).  select_inds: dev int64 [n] global indices in [0, V * H * W), or NULL:
 * positions cfg->first .. + n - 1 of the keyed permutation of [0, V * H * W) (ranks take disjoint slices, as above).
 * Row i equals, bit for bit, the row nerfhip_select_rays writes for (poses[v], images[v], select_inds = {k}); with
 * num_views == 1 the whole call equals nerfhip_select_rays.  Limits: 1 <= num_views <= NERFHIP_MAX_VIEWS,
 * num_views * H * W <= 2^32.  One launch. */
#define NERFHIP_MAX_VIEWS 65536
int nerfhip_select_rays_views(const nerfhip_select_cfg* cfg, int num_views, const float* poses, int64_t pose_view_stride,
                              int pose_ld, const float* images, const int64_t* select_inds, int64_t n, float* rays,
                              float* target, int64_t* inds_out, nerfhip_stream_t stream);
/* Its VJP w.r.t. the poses.  inds: dev int64 [n], the inds_out of the forward; g_rays / g_rays_2 / g_rays_stride: as for
 * nerfhip_select_rays_bwd; g_poses: dev float [V][3][4], written completely (a view without a ray in the batch, and n == 0:
 * exact zeros).  g_poses[v] is bit-identical to what nerfhip_select_rays_bwd returns for pose v when handed only the rays
 * of view v in ascending batch position: the rays are grouped by view with integer work only (a stable counting sort) and
 * each view is summed along the single-view tree with n = n_v.  No floating-point atomics; the result depends on the rays'
 * view assignment and values only.  tmp: dev scratch of nerfhip_pose_grad_views_tmp_bytes(n, num_views) bytes (0 for
 * n == 0; -1 for n < 0, n >= 2^31 or num_views outside 1 .. NERFHIP_MAX_VIEWS).  Three launches on `stream` (one for
 * n == 0), their grids functions of (n, num_views) only. */
int64_t nerfhip_pose_grad_views_tmp_bytes(int64_t n, int num_views);
int nerfhip_select_rays_views_bwd(const nerfhip_select_cfg* cfg, int num_views, const float* poses, int64_t pose_view_stride,
                                  int pose_ld, const int64_t* inds, int64_t n, const float* g_rays, const float* g_rays_2,
                                  int g_rays_stride, void* tmp, int64_t tmp_bytes, float* g_poses, nerfhip_stream_t stream);

/* ---- learned intrinsics: fx, fy, cx, cy on the device, with their gradient (NeRF--, a COLMAP focal that is a few per cent off) -----
 * intr: dev float[4] = (fx, fy, cx, cy) in pixels, shared by all views of a call.  Pixel (row, col) has the camera direction
 *     dc = ((col - cx) / fx, -(row - cy) / fy, -1),
 * the arithmetic of the scalar forms operation for operation: intr = (focal, focal, (float)(W * 0.5), (float)(H * 0.5)) gives their
 * bits.  NDC: the five constants stay those of cfg, fixed on the host, and do NOT follow intr -- ndc_rays is a fixed projective change
 * of coordinates of the space the nets live in, any (cw, ch) is a valid one, and moving it during training would move the scene
 * under the nets.  So intr enters through the pin-hole direction only and d(loss)/d(intr) is defined through that path only; a caller
 * who wants the NDC box to follow a learned focal rebuilds cfg on the host at a time of their choosing.  cfg->focal is not read.
 *
 * nerfhip_select_rays_views reading intr in place of cfg->focal (num_views == 1: the single-view form).  One launch, the same kernel. */
int nerfhip_select_rays_views_intr(const nerfhip_select_cfg* cfg, const float* intr, int num_views, const float* poses,
                                   int64_t pose_view_stride, int pose_ld, const float* images, const int64_t* select_inds, int64_t n,
                                   float* rays, float* target, int64_t* inds_out, nerfhip_stream_t stream);
/* Its VJP w.r.t. the poses and the intrinsics.  g_poses: dev float [V][3][4], g_intr: dev float [4]; either may be NULL, not both;
 * each one given is written completely (n == 0: exact zeros).  g_poses: nerfhip_select_rays_views_bwd's three launches with dc taken
 * from intr.  g_intr: with g_d the cotangent of the pre-NDC direction (after the NDC backward, the viewdir normalisation's backward
 * and the g_rays + g_rays_2 add) and g_dc[k] = sum_c g_d[c] c2w[c][k], ray i adds
 *     g_fx += -g_dc[0] dc[0] / fx,   g_fy += -g_dc[1] dc[1] / fy,   g_cx += -g_dc[0] / fx,   g_cy += g_dc[1] / fy,
 * summed over all n rays, whatever their view, along the single-view tree of nerfhip_select_rays_bwd in batch order (G(n) partials
 * of four sums, then one workgroup; each ray reads the pose of its own view inds[i] / (H W)): two more launches, no grouping, no
 * atomics, a result that depends on n and the batch order only and is bit-reproducible.  An index outside [0, V H W) is dropped by
 * both outputs.  Either output has the same bits whether the other one is asked or not.  tmp: dev scratch of
 * nerfhip_intr_grad_views_tmp_bytes(n, num_views) bytes (-1 where nerfhip_pose_grad_views_tmp_bytes is). */
int64_t nerfhip_intr_grad_views_tmp_bytes(int64_t n, int num_views);
int nerfhip_select_rays_views_intr_bwd(const nerfhip_select_cfg* cfg, const float* intr, int num_views, const float* poses,
                                       int64_t pose_view_stride, int pose_ld, const int64_t* inds, int64_t n, const float* g_rays,
                                       const float* g_rays_2, int g_rays_stride, void* tmp, int64_t tmp_bytes, float* g_poses,
                                       float* g_intr, nerfhip_stream_t stream);
/* nerfhip_ray_bundle from intr (evaluation under learned intrinsics).  Forward only.  One launch, the same kernel. */
int nerfhip_ray_bundle_intr(int height, int width, const float* intr, const float* c2w, int c2w_ld, const int64_t* pixels, int64_t n,
                            float* ray_origins, float* ray_directions, nerfhip_stream_t stream);
/* The parametrisation Adam steps (q: dev float[4], base: dev float[4] = fx0 fy0 cx0 cy0, intr: dev float[4]):
 *     fx = fx0 exp(q0),   fy = fy0 exp(q1) -- fy0 exp(q0) when tie_focal --,   cx = cx0 + q2,   cy = cy0 + q3.
 * The log-focal keeps the focal positive and makes Adam's step scale-free.  fp64 between the fp32 inputs and outputs; q = 0 gives
 * base bit for bit.  One thread, one launch. */
int nerfhip_intrinsics_fwd(const float* q, const float* base, int tie_focal, float* intr, nerfhip_stream_t stream);
/* Its pull-back: g_q0 = g_fx fx (+ g_fy fy when tied), g_q1 = g_fy fy (0 when tied), g_q2 = g_cx, g_q3 = g_cy.  mask: dev, one byte
 * per entry of q, or NULL = every entry learned: an entry whose byte is 0 gets an exact zero (with Adam it never moves).  g_q: dev
 * float[4], written completely.  The step is nerfhip_adam_step on the four floats.  One launch. */
int nerfhip_intrinsics_bwd(const float* q, const float* base, int tie_focal, const float* g_intr, const unsigned char* mask,
                           float* g_q, nerfhip_stream_t stream);

/* ---- lens distortion: k1, k2, p1, p2 on the device, with their gradient (COLMAP's OPENCV model; Self-Calibrating NeRF) --------------
 * dist: dev float[4] = (k1, k2, p1, p2), shared by all views of a call.  RADIAL is p1 = p2 = 0, SIMPLE_RADIAL additionally k2 = 0.
 * With (x, y) the UNDISTORTED normalised image point (y down), (xd, yd) = ((col - cx) / fx, (row - cy) / fy) the observed pixel,
 * r2 = x^2 + y^2 and rad = 1 + k1 r2 + k2 r2^2:
 *     xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2),
 *     yd = y rad + p1 (r2 + 2 y^2) + 2 p2 x y,                                   (xd, yd) = F(x, y; dist).
 * A ray needs the inverse: F(x, y) = (xd, yd) is solved by Newton's iteration from (xd, yd) with the analytic 2 x 2 Jacobian J
 * (symmetric for this model), NERFHIP_UNDISTORT_ITERS steps on every ray in fp32 -- no data-dependent exit, a ray's bits depend on
 * its inputs only.  The camera direction is dc = (x, -y, -1); everything downstream is what the pin-hole forms do (rotation, NDC with
 * cfg's fixed constants, packing, view directions).  dist = (0, 0, 0, 0) gives the rows of the form without dist bit for bit (J is
 * exactly I, every residual exactly zero).
 * Domain: the model is defined where det J >= 1/2 along the Newton path (moderate distortion over the image: e.g.
 * (-0.25, 0.08, 5e-3, -4e-3) up to the normalised radius 1).  Outside it the outputs are unspecified; nothing checks for it.
 * Gradient: by the implicit-function theorem at the solution, never through the iterations.  With g_dc = R^T g_d (g_d: the cotangent
 * of the pre-NDC direction, as for g_intr above), g_xy = (g_dc[0], -g_dc[1]) and lambda = J^-T g_xy, ray i adds
 *     g_k1 -= r2 (lambda . (x, y)),     g_k2 -= r2^2 (lambda . (x, y)),
 *     g_p1 -= lambda0 2 x y + lambda1 (r2 + 2 y^2),     g_p2 -= lambda0 (r2 + 2 x^2) + lambda1 2 x y,
 *     g_fx -= lambda0 xd / fx,   g_cx -= lambda0 / fx,   g_fy -= lambda1 yd / fy,   g_cy -= lambda1 / fy;
 * the pose VJP is the pin-hole one on the undistorted dc. */
#define NERFHIP_UNDISTORT_ITERS 8
/* nerfhip_select_rays_views_intr with the extra pointer dist (not NULL).  intr == NULL: the scalar camera of cfg (focal, focal, W / 2,
 * H / 2).  One launch, the same kernel. */
int nerfhip_select_rays_views_dist(const nerfhip_select_cfg* cfg, const float* intr, const float* dist, int num_views,
                                   const float* poses, int64_t pose_view_stride, int pose_ld, const float* images,
                                   const int64_t* select_inds, int64_t n, float* rays, float* target, int64_t* inds_out,
                                   nerfhip_stream_t stream);
/* Its VJP w.r.t. the poses, the intrinsics and the distortion coefficients.  g_poses: dev float [V][3][4], g_intr: dev float [4],
 * g_dist: dev float [4]; each may be NULL, not all three; each one given is written completely (n == 0: exact zeros) and has the same
 * bits whether or not the others are asked.  g_poses, g_intr: as for nerfhip_select_rays_views_intr_bwd, on the undistorted dc.
 * g_dist: ONE sum over all n rays in batch order along the single-view tree, exactly as g_intr is (G(n) partials of four sums, then
 * one workgroup; two more launches; no atomics, no grouping; bit-reproducible); an index outside [0, V H W) is dropped.
 * dist_mask: dev, one byte per coefficient, or NULL = all learned: an entry whose byte is 0 gets an exact zero (with Adam it never
 * moves); the coefficients are stepped directly by nerfhip_adam_step.  dist = 0 gives the g_poses and g_intr of
 * nerfhip_select_rays_views_intr_bwd bit for bit.  tmp: dev scratch of nerfhip_dist_grad_views_tmp_bytes(n, num_views) bytes (-1 where
 * nerfhip_pose_grad_views_tmp_bytes is). */
int64_t nerfhip_dist_grad_views_tmp_bytes(int64_t n, int num_views);
int nerfhip_select_rays_views_dist_bwd(const nerfhip_select_cfg* cfg, const float* intr, const float* dist, int num_views,
                                       const float* poses, int64_t pose_view_stride, int pose_ld, const int64_t* inds, int64_t n,
                                       const float* g_rays, const float* g_rays_2, int g_rays_stride, void* tmp, int64_t tmp_bytes,
                                       float* g_poses, float* g_intr, float* g_dist, const unsigned char* dist_mask,
                                       nerfhip_stream_t stream);
/* nerfhip_ray_bundle under dist (evaluation under a learned lens).  intr == NULL: the camera of (height, width, focal); else focal is
 * not read.  Forward only.  One launch, the same kernel. */
int nerfhip_ray_bundle_dist(int height, int width, float focal, const float* intr, const float* dist, const float* c2w, int c2w_ld,
                            const int64_t* pixels, int64_t n, float* ray_origins, float* ray_directions, nerfhip_stream_t stream);

/* ---- per-view exposure: a colour gain and offset per view behind the render, with their gradient (NeRF-W / URF style) ----------------
 * expo: dev float [V][6], row v = (s_r, s_g, s_b, b_r, b_g, b_b): per-channel log-gain and offset of view v.  Ray i belongs to view
 * inds[i] / hw (inds: the GLOBAL indices the views selection returns, hw = height * width); its corrected prediction in channel c is
 *     p' = e p + b,   e = exp(s[v][c]),   b = b[v][c],
 * alike for the coarse and the fine rgb, and the loss is nerfhip_mse_loss_fwd_bwd's on p'.  A zero table is the identity; an index
 * outside [0, V hw) belongs to no view: identity in the loss, dropped from the table gradient.
 * Arithmetic (fp32, one rounding per operation, unless said): e = (float)exp((double)s) -- one fp64 exp --; q = e p; d = (q + b) - t;
 * k = 2 / (3 n) * grad_scale; the loss sums (double)d (double)d as the plain loss does; g_rgb = (d k) e; per ray and net the table
 * gradient adds (d k) q to g_s[v][c] and d k to g_b[v][c], the coarse term first.
 * Limits: 1 <= num_views <= NERFHIP_MAX_VIEWS, hw >= 1, num_views * hw <= 2^32, n < 2^31, target_stride >= 3; expo must not be NULL. */
/* nerfhip_mse_loss_fwd_bwd under the table: one launch, the same workgroup, order of summation and fp64 sums; rgb_fine and
 * either g_rgb_* may be NULL; n > 0.  expo == 0 gives nerfhip_mse_loss_fwd_bwd's loss words and cotangents. */
int nerfhip_mse_loss_views_fwd_bwd(const float* rgb_coarse, const float* rgb_fine, const float* target, int target_stride, int64_t n,
                                   float grad_scale, const int64_t* inds, int64_t hw, const float* expo, int num_views,
                                   float* g_rgb_coarse, float* g_rgb_fine, float* loss_out, nerfhip_stream_t stream);
/* d(loss_coarse + loss_fine)/d(expo) -> g_expo: dev float [V][6], written completely (n == 0, or a view without a ray: exact zeros).
 * Row v is ONE sum over view v's rays in ascending batch position along the single-view tree of the pose VJP with n = n_v: three
 * launches whose grids depend on (n, V) only (the grouping of nerfhip_select_rays_views_bwd, floor(n / 256) + V workgroups of six
 * partial sums, V workgroups that add them), no atomics, bit-reproducible; the result depends on the rays' view assignment and values
 * only.  mask: dev, V * 6 bytes, or NULL = all learned: an entry whose byte is 0 gets an exact zero (with Adam it never moves).
 * tmp: dev scratch of nerfhip_exposure_grad_tmp_bytes(n, num_views) = 4 (6 (floor(n / 256) + V) + 2 V + n) bytes (-1 for n < 0,
 * n >= 2^31 or num_views outside 1 .. NERFHIP_MAX_VIEWS). */
int64_t nerfhip_exposure_grad_tmp_bytes(int64_t n, int num_views);
int nerfhip_exposure_bwd(const float* rgb_coarse, const float* rgb_fine, const float* target, int target_stride, int64_t n,
                         float grad_scale, const int64_t* inds, int64_t hw, const float* expo, int num_views, const unsigned char* mask,
                         void* tmp, int64_t tmp_bytes, float* g_expo, nerfhip_stream_t stream);

/* ---- camera table: one se(3) twist per view composed onto a base pose (the parametrisation pose refinement steps) --------
 * poses[v] = base[v] * Exp(xi[v]): a camera-frame perturbation.  xi: dev float [V][6] = [w (3), v (3)]; Exp is the full SE(3)
 * exponential: R = I + A W + B W^2, t = (I + B W + C W^2) v with W = hat(w), th = |w|, A = sin th / th, B = (1 - cos th) / th^2,
 * C = (th - sin th) / th^3 (evaluated without cancellation; th = 0 included).  base: dev, the base pose of view v is 3 rows of
 * base_ld >= 4 floats at base + v * base_view_stride (the strided-table convention of nerfhip_select_rays_views;
 * base_view_stride >= 2 * base_ld + 4 when num_views > 1).  poses: dev float [V][3][4], contiguous -- directly a pose table of
 * nerfhip_select_rays_views (pose_ld 4, pose_view_stride 12).  A view whose six twist entries are all zero gets its base bit for
 * bit.  Limits: 1 <= num_views <= NERFHIP_MAX_VIEWS.  One launch. */
int nerfhip_pose_table_fwd(const float* xi, const float* base, int64_t base_view_stride, int base_ld, int num_views,
                           float* poses, nerfhip_stream_t stream);
/* Its VJP w.r.t. the twists (closed form; base carries no gradient).  g_poses: dev float [V][3][4] = d(loss)/d(poses), e.g. what
 * nerfhip_select_rays_views_bwd wrote; active: dev, one byte per view, or NULL = every view active: an inactive view (byte 0) gets
 * exact zeros and its g_poses row is not read (freezing an anchor view fixes the gauge); g_xi: dev float [V][6], written
 * completely.  The twists are stepped with nerfhip_adam_step on the flat [V * 6] vector.  One launch. */
int nerfhip_pose_table_bwd(const float* xi, const float* base, int64_t base_view_stride, int base_ld, int num_views,
                           const float* g_poses, const unsigned char* active, float* g_xi, nerfhip_stream_t stream);

/* ---- coarse-to-fine window over the encoding's frequency bands (BARF; joint pose-and-field training from poor poses) --------
 * Every encoding column enters the net through a linear layer, and W (w (.) gamma(x)) = (W diag(w)) gamma(x): the net on a windowed
 * encoding is the unwindowed net run on theta_eff = theta (.) m, m = 1 except on the weight columns that multiply a windowed band.
 * So the forward packs its image from theta_eff, the input / ray gradient reads theta_eff where it reads the flat vector
 * (nerfhip_mlp_bwd_input, nerfhip_render_bwd_rays), and d(loss)/d(theta) = m (.) d(loss)/d(theta_eff); no other kernel changes.
 * Band k of an encoding owns the six columns sin(3), cos(3) of frequency k (nerf/nerf_helpers.py:130-157); the include_input
 * columns are never windowed.  The caller evaluates w_k(alpha) = (1 - cos(pi clamp(alpha - k, 0, 1))) / 2 on the host in fp64 and
 * rounds once to fp32: the kernels take the weights by value and do one IEEE multiply per windowed entry. */
typedef struct nerfhip_window {
    float xyz[16]; /* band weights of the xyz encoding (entries beyond num_encoding_fn_xyz are not read) */
    float dir[10]; /* ... of the direction encoding */
} nerfhip_window;
/* Host-only.  host_table: uint8[nerfhip_plan_num_params]: one code per entry of the flat parameter vector -- 0 = not windowed,
 * 1 + k = multiplies xyz band k, 17 + k = direction band k.  Windowed: the encoding columns of layer1.weight, the trailing dim_xyz
 * columns of every skip layer's layers_xyz.{i}.weight (cat(h, xyz): hidden first), the trailing dim_dir columns of
 * layers_dir.0.weight (cat(feat, view)). */
int nerfhip_plan_window_index(nerfhip_plan_t plan, uint8_t* host_table);
/* out[i] = codes[i] ? params[i] * weight(codes[i]) : params[i], weight(1 + k) = w->xyz[k], weight(17 + k) = w->dir[k] (a code above
 * 26 is read as 0).  params, out: dev float[n], distinct buffers; codes: dev uint8[n].  One launch. */
int nerfhip_window_params(const float* params, const uint8_t* codes, int64_t n, const nerfhip_window* w, float* out,
                          nerfhip_stream_t stream);
/* The same multiply in place on a flat gradient: an entry of a closed band (weight 0) becomes an exact zero. */
int nerfhip_window_grads(float* g_params, const uint8_t* codes, int64_t n, const nerfhip_window* w, nerfhip_stream_t stream);

/* cast_to_image (eval_nerf.py:23-29): ToPILImage of a float image = mul(255) then byte conversion (truncation).
 * rgb: dev [pixels, in_channels >= 3] (first three used); out: dev uint8 [pixels, 3] (H, W, 3 byte order). */
int nerfhip_cast_to_image(const float* rgb, int in_channels, int64_t pixels, uint8_t* out, nerfhip_stream_t stream);
/* cast_to_disparity_image (eval_nerf.py:32-35): min-max normalise, clamp(0,1)*255, truncate.  NaN pixels make
 * min()/max() NaN in the reference, which zeroes the whole image -- reproduced.  scratch3: dev float[3]. */
int nerfhip_cast_to_disparity_image(const float* disparity, int64_t pixels, float* scratch3, uint8_t* out,
                                    nerfhip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NERFHIP_H_ */
