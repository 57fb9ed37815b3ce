/* loner_amd.h — C ABI of the MI355X-native LONER implicit-map optimisation path.
 *
 * Every entry point replaces one piece of the reference's sigma-field step
 * (esulimma/LONER @ 2024_08_07; file:line relative to /root/reference):
 *
 *   lnr_hashgrid_fwd/_bwd(_rays)  tinycudann HashGrid encode used by
 *                                 tcnn.NetworkWithInputEncoding  src/models/nerf_tcnn.py:35-38,68/71
 *                                 and tcnn.Encoding              src/models/nerf_tcnn.py:40,64
 *   lnr_sigma_mlp_fwd/_bwd        tcnn FullyFusedMLP (32->64 ReLU->1, no bias)
 *                                 src/models/nerf_tcnn.py:35-38, cfg/nerf_config/default_nerf_hash.yaml:26-31
 *   lnr_sample_ogm / _uniform     OccGridRaySampler / UniformRaySampler + sample_pdf
 *                                 src/models/ray_sampling.py:18-92, src/models/rendering_tcnn.py:19-68
 *   lnr_composite                 raw2outputs / raw2outputs_adjusted src/models/rendering_tcnn.py:70-295
 *   lnr_composite_loss_bwd        compute_loss (LiDAR branch) + autograd through raw2outputs
 *                                 src/mapping/optimizer.py:701-859, src/models/losses.py:29-51
 *   lnr_field_train               fused sigma MLP fwd + composite + loss + composite bwd + MLP bwd
 *                                 (the body of one optimiser step, src/mapping/optimizer.py:436-450)
 *   lnr_loss_finalize             scalar loss / mean depth-eps from per-ray partials (optimizer.py:767,838-844)
 *   lnr_adam_step                 torch.optim.Adam step on the flat params  src/mapping/optimizer.py:255-265,460
 *   lnr_hashgrid_bwd_rays_jac_adam  the table's backward with that Adam step fused in (optimizer.py:450,460)
 *   lnr_ogm_update                Optimizer._step_occupancy_grid  src/mapping/optimizer.py:897-908
 *   lnr_rgb_render                colour head (SH4 + 2^19 HashGrid + FullyFusedMLP) + colour map
 *                                 src/models/nerf_tcnn.py:80-95, src/models/rendering_tcnn.py:283-289
 *   lnr_rgb_train / lnr_build_camera_rays  colour-head training (camera phase)
 *                                 src/mapping/optimizer.py:541-688,861-894, src/common/ray_utils.py:175-212
 *   lnr_motion_compensate / lnr_sky_rays  per-keyframe scan preprocessing
 *                                 src/common/sensors.py:169-231, examples/fdt_optimize_implicit_map_utils.py:38-77
 *   lnr_build_lidar_rays          per-step ray selection (RANDOM / MASK / sky) + KeyFrame.build_lidar_rays
 *                                 src/mapping/optimizer.py:363-424, src/mapping/keyframe.py:75-105,
 *                                 src/common/ray_utils.py:31-60,269-322
 *   lnr_cloud_cell_keys / lnr_voxel_heads / lnr_voxel_reduce / lnr_nn_search / lnr_dist_stats
 *                                 Open3D's voxel_down_sample and compute_point_cloud_distance, and the metric sums
 *                                 analysis/evaluate_lidar_map.py:16-81, analysis/renderer_lidar.py:292-349
 *   lnr_mesh_face_areas / lnr_mesh_sample_points / lnr_mesh_vertex_normals
 *                                 Open3D's sample_points_uniformly and compute_vertex_normals
 *                                 analysis/compute_metrics/maps/mesh_to_pcd.py:21-27, analysis/meshing.py:122
 *
 * Conventions:
 *   - all data pointers are DEVICE pointers owned by the caller (PyTorch); no allocation, no host
 *     synchronisation inside any call; every call only enqueues work on `stream` (a hipStream_t,
 *     NULL = default stream) and is safe to capture in a hipGraph;
 *   - return 0 (LNR_OK) or a negative error code; lnr_last_error() returns a thread-local message;
 *   - stateless and re-entrant.
 *
 * Layouts:
 *   rays     (R, 13) fp32  [o(3) d(3) viewdir(3) 0 0 near far]   src/common/ray_utils.py:314-317
 *   z        (R, S)  fp32  sorted sample depths (normalised units)
 *   table    (n_entries, 2) fp16 forward shadow; fp32 master/grad/m/v in the optimiser
 *   enc      "level-major": element (sample n, level l) at enc[l * enc_stride + n], one half2
 *            (uint32) per element; enc_stride >= N.  The tcnn-compatible AoS layout (N, 2L) is
 *            produced by lnr_enc_to_aos.
 *   d_enc    same indexing, one float2 per element
 *   mlp      sigma MLP weights, row-major [out][in] per layer: W0 (64,32) then W1 (16,64); fp16
 */
#ifndef LONER_AMD_H
#define LONER_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LNR_OK 0
#define LNR_ERR_ARG (-1)
#define LNR_ERR_HIP (-2)

#define LNR_MAX_LEVELS 32

const char* lnr_last_error(void);
int lnr_version(void);

/* ---------------------------------------------------------------- per-step scalars (graph replay) */
/* The scalars that change from one optimiser step to the next, in DEVICE memory, so that a step
 * captured once in a hipGraph replays with the current step's values (no kernel argument changes).
 * Every entry point that takes `dev_step` (or a struct holding it) reads these fields from it when it
 * is not NULL, in place of the corresponding host argument:
 *   key             the draw key (lnr_step_key(seed, global_step)): lnr_sample_ogm / _uniform, the
 *                   ray build (lnr_ray_window.dev_step), the sigma noise (lnr_loss_params.dev_step)
 *   los_lambda      lnr_loss_params.los_lambda (optimizer.py:712-716, decayed on global_step + 1)
 *   los_eps         lnr_loss_params.los_eps (optimizer.py:781-785)
 *   adam_step_size  lr / (1 - beta1^t), adam_bc2_sqrt = sqrt(1 - beta2^t): lnr_adam_step(_ranges)
 *                   (lnr_adam_coefficients forms both exactly as those calls do from step and lr) */
typedef struct lnr_step_scalars {
  uint32_t key;
  float los_lambda;
  float los_eps;
  float adam_step_size;
  float adam_bc2_sqrt;
  uint32_t pad[3];
} lnr_step_scalars;
/* dev[0..n) = values[0..n) (n <= 4 HOST structs, carried as the kernel's argument), enqueued on `stream`:
 * the launch before a captured step's replay sets that step's scalars (and the next step's, for its
 * prefetched ray build and sampling) in stream order. */
int lnr_step_scalars_set(const lnr_step_scalars* values, int32_t n, lnr_step_scalars* dev, void* stream);
/* Host: the fp32 Adam coefficients lnr_adam_step forms for 1-based step t and learning rate lr. */
int lnr_adam_coefficients(int32_t step, double lr, double beta1, double beta2, float* step_size, float* bc2_sqrt);

/* ---------------------------------------------------------------- hash grid */
typedef struct lnr_grid_desc {
  uint32_t n_levels;          /* tcnn "n_levels" */
  uint32_t n_features;        /* tcnn "n_features_per_level"; must be 2 */
  uint32_t log2_hashmap_size; /* tcnn "log2_hashmap_size" */
  uint32_t base_resolution;   /* tcnn "base_resolution" */
  float per_level_scale;      /* tcnn "per_level_scale" (default 2.0) */
  uint32_t n_entries;         /* sum of level sizes */
  float scale[LNR_MAX_LEVELS];
  uint32_t resolution[LNR_MAX_LEVELS];
  uint32_t size[LNR_MAX_LEVELS];
  uint32_t offset[LNR_MAX_LEVELS + 1];
} lnr_grid_desc;

/* Fill `d` exactly as tcnn v1.7's GridEncodingTemplated constructor lays the levels out. */
int lnr_grid_desc_init(lnr_grid_desc* d, uint32_t n_levels, uint32_t n_features, uint32_t log2_hashmap_size,
                       uint32_t base_resolution, float per_level_scale);

/* pos01 (N,3) fp32 in [0,1]^3 -> enc (level-major half2).  tcnn Encoding forward.
 * bwd_ws (optional, may be NULL): the backward workspace of the SAME positions; when given, the
 * forward also records the backward's per-block record histogram, so a following backward can be
 * called with LNR_BWD_COUNTS_READY and skips its counting pass. */
int lnr_hashgrid_fwd(const lnr_grid_desc* d, const float* pos01, int64_t n, const uint16_t* table,
                     uint32_t* enc, int64_t enc_stride, void* bwd_ws, int64_t bwd_ws_bytes, void* stream);
/* Positions generated from rays and samples: pos01 = (o + d*z + 1) / 2 (nerf_tcnn.py:63). */
int lnr_hashgrid_fwd_rays(const lnr_grid_desc* d, const float* rays, const float* z, int64_t n_rays,
                          int32_t n_samples, const uint16_t* table, uint32_t* enc, int64_t enc_stride,
                          void* bwd_ws, int64_t bwd_ws_bytes, void* stream);
/* Early ray termination, the encode of one phase: samples [lo, hi) (multiples of 64; n_samples % 64 == 0) of
 * the rays ray_list[0 .. *ray_count) (DEVICE; ray_list NULL: every ray), as lnr_hashgrid_fwd_rays encodes them;
 * the other samples' encodings are left unwritten.  bwd_ws (the first phase only, lo == 0, every ray): the
 * backward's record histogram of EVERY sample, as lnr_hashgrid_fwd_rays records it, for a full backward with
 * LNR_BWD_COUNTS_READY (the live backward counts its own).  Without bwd_ws only the listed rays' phase samples
 * are encoded, by a grid that leaves at once past the list's end.  expect_rays: the caller's estimate of
 * *ray_count (0: none); a small one selects a grid for a sparse phase (one level per workgroup, walking the
 * listed rows).  Every grid encodes exactly the listed rays' samples, whatever the count.  See
 * lnr_field_sigma_phase. */
int lnr_hashgrid_fwd_rays_phase(const lnr_grid_desc* d, const float* rays, const float* z, int64_t n_rays,
                                int32_t n_samples, const uint16_t* table, uint32_t* enc, int64_t enc_stride,
                                void* bwd_ws, int64_t bwd_ws_bytes, const uint32_t* ray_list,
                                const uint32_t* ray_count, int64_t expect_rays, int32_t lo, int32_t hi,
                                void* stream);
/* Forward of samples whose compositing weight can be zero (the colour head: rgb = sum w_i c_i + ...,
 * rendering_tcnn.py:286): samples with live[n] == 0 (exactly) issue no gathers, every other sample is
 * encoded exactly as lnr_hashgrid_fwd_rays does.  A dead sample gets a zero encoding when its aligned
 * 16-sample tile (n / 16) holds a live sample; the encodings of a tile with no live sample are left
 * unwritten (lnr_rgb_render and lnr_rgb_train skip such tiles).  live = the (R,S) weights of the sigma
 * pass.  No backward histogram. */
int lnr_hashgrid_fwd_rays_live(const lnr_grid_desc* d, const float* rays, const float* z, int64_t n_rays,
                               int32_t n_samples, const uint16_t* table, const float* live, uint32_t* enc,
                               int64_t enc_stride, void* stream);
/* lnr_hashgrid_fwd_rays_live that also records the backward's histogram in `bwd_ws` (as
 * lnr_hashgrid_fwd_rays does), counting a sample with live[n] == 0 at the coherent levels only (its
 * zero gradient merges into the runs there) and not at the others: the records of
 * lnr_hashgrid_bwd_rays_live, which can then be called with LNR_BWD_COUNTS_READY (no counting pass). */
int lnr_hashgrid_fwd_rays_live_ws(const lnr_grid_desc* d, const float* rays, const float* z, int64_t n_rays,
                                  int32_t n_samples, const uint16_t* table, const float* live, uint32_t* enc,
                                  int64_t enc_stride, void* bwd_ws, int64_t bwd_ws_bytes, void* stream);
/* Backward: d_table (n_entries,2) fp32 = scatter of corner weights * d_enc, as an atomic-free
 * binned scatter of 8-byte records (fp16 values at a per-level power-of-two scale from max |d_enc|)
 * with int64 fixed-point accumulation at a unit that depends on N alone.  d_table is OVERWRITTEN (every entry, zero where
 * no sample touches it, all zero for N = 0) and the result is bitwise reproducible; `workspace` holds
 * at least lnr_hashgrid_bwd_workspace_bytes(d, N) bytes.
 * Input gradient (tcnn's backward w.r.t. the positions, src/models/nerf_tcnn.py:63,68-71 when pos
 * requires grad, e.g. joint pose + map optimisation, src/mapping/optimizer.py:256-262): when d_pos is
 * not NULL, d_pos (N,3) fp32 = dL/dpos01 (OVERWRITTEN): per sample, the sum over (level, feature) of
 * d_enc * d enc / d pos01, the trilinear blend's derivative from the fp16 `table` (the forward's
 * operand, 4-byte aligned): tcnn v1.7 kernel_grid's dy_dx + kernel_grid_backward_input.  The _rays
 * forms give it per sample w.r.t. pos01 = (o + d z + 1) / 2.  Deterministic (one fixed-order sum per
 * sample).  d_table may be NULL (no table gradient: workspace unused), d_pos may be NULL (table unused),
 * not both.  The input gradient is its own launch, so a call without d_pos costs nothing extra. */
#define LNR_BWD_COUNTS_READY 1
#define LNR_BWD_NO_ACCUM 2      /* stop after the scatter: lnr_hashgrid_bwd_accum then finishes level ranges */
#define LNR_BWD_LEVEL_MAX_READY 4 /* the caller stored max |d_enc| per level at lnr_hashgrid_bwd_level_max():
                                     no pass over d_enc for it.  The maxima may be rank-local under data
                                     parallelism: they only pick each level's power-of-two record scale,
                                     fp16 rounding is scale-invariant, and the fixed-point unit sits far
                                     below what reaches Adam */
#define LNR_BWD_PREPARE_ONLY 16   /* stop before the scatter: the live records' histogram (or, with
                                     LNR_BWD_COUNTS_READY, the forward's) scanned into bucket offsets; needs
                                     LNR_BWD_LIVE or LNR_BWD_COUNTS_READY (reads d_sigma, not J) */
#define LNR_BWD_PREPARED 32       /* a LNR_BWD_PREPARE_ONLY call with the same arguments ran: scatter + accumulate */
#define LNR_BWD_LIVE 8            /* lnr_hashgrid_bwd_rays_jac(_adam): the live backward.  A sample with
                                     d_sigma[n] == 0 (relu(sigma + noise) = 0 or transmittance 0,
                                     rendering_tcnn.py:252-266) adds exactly 0 to every entry, so only samples with
                                     d_sigma != 0 emit records (coherent levels: only runs holding one), after its
                                     own histogram pass over those samples (a forward histogram is not needed and,
                                     with LNR_BWD_COUNTS_READY, not read).  The fixed-point unit depends on N alone,
                                     so d_table is BITWISE the full backward's.  Pays when most samples are dead (a
                                     trained field: ~89 % at C2); ignored where the level-looped scatter does not
                                     apply (small batches, other grids). */
int64_t lnr_hashgrid_bwd_workspace_bytes(const lnr_grid_desc* d, int64_t n);
/* Device address of the n_levels per-level max |d_enc| floats inside `workspace` (the same for
 * every n: the workspace's first bytes). */
float* lnr_hashgrid_bwd_level_max(const lnr_grid_desc* d, int64_t n, void* workspace);
/* Device address of the last backward's bucket segment starts inside `workspace` (n_buckets + 1 uint64,
 * buckets = the levels' 4096-entry table chunks in level order; the last is the number of records the
 * scatter placed): for tests and tools that measure the record volume (e.g. of the live backward). */
const uint64_t* lnr_hashgrid_bwd_seg_start(const lnr_grid_desc* d, int64_t n, void* workspace);
int lnr_hashgrid_bwd(const lnr_grid_desc* d, const float* pos01, int64_t n, const float* d_enc,
                     int64_t enc_stride, float* d_table, const uint16_t* table, float* d_pos, void* workspace,
                     int64_t workspace_bytes, int32_t flags, void* stream);
int lnr_hashgrid_bwd_rays(const lnr_grid_desc* d, const float* rays, const float* z, int64_t n_rays,
                          int32_t n_samples, const float* d_enc, int64_t enc_stride, float* d_table,
                          const uint16_t* table, float* d_pos, void* workspace, int64_t workspace_bytes,
                          int32_t flags, void* stream);
/* The table gradient of samples with a live mask (the colour grid: live = the compositing weights, d_enc
 * of a weight-0 sample is 0): at the levels that are not coherent, samples with live[n] == 0 emit no records
 * (the others emit theirs, zero or not).  Bitwise the same d_table as lnr_hashgrid_bwd_rays (records of zero
 * add nothing and the fixed-point unit does not follow the record counts).  With LNR_BWD_COUNTS_READY the histogram must come from
 * lnr_hashgrid_fwd_rays_live_ws with the same mask. */
int lnr_hashgrid_bwd_rays_live(const lnr_grid_desc* d, const float* rays, const float* z, int64_t n_rays,
                               int32_t n_samples, const float* d_enc, int64_t enc_stride, const float* live,
                               float* d_table, void* workspace, int64_t workspace_bytes, int32_t flags,
                               void* stream);
/* The same, from lnr_field_train's compact encoding gradient: d_enc = d_sigma[n] * J[l][n] with J
 * level-major fp16 pairs (one uint32 per level and sample, level stride jac_stride). */
int lnr_hashgrid_bwd_rays_jac(const lnr_grid_desc* d, const float* rays, const float* z, int64_t n_rays,
                              int32_t n_samples, const uint32_t* d_jac, const float* d_sigma, int64_t jac_stride,
                              float* d_table, const uint16_t* table, float* d_pos, void* workspace,
                              int64_t workspace_bytes, int32_t flags, void* stream);
/* The same with Adam fused in: where the backward finishes a table entry's gradient it applies
 * torch.optim.Adam's update to that parameter (the arithmetic of lnr_adam_step, so the parameters,
 * moments and fp16 shadow come out bitwise equal) instead of storing the gradient, for the
 * 2 * n_entries table parameters at the head of `param`, `shadow`, `m`, `v`.  The step's Adam on the
 * parameters after the table (the MLP) stays a lnr_adam_step.  N = 0 is Adam with a zero gradient.
 * LNR_BWD_NO_ACCUM is refused (a gradient exchanged between ranks must reach memory first). */
typedef struct lnr_adam_epilogue {
  float* param;
  uint16_t* shadow;
  float* m;
  float* v;
  int32_t step;  /* 1-based, as lnr_adam_step */
  double lr, beta1, beta2, eps;
  const lnr_step_scalars* dev_step; /* non-NULL: step size and bias correction from device memory */
} lnr_adam_epilogue;
int lnr_hashgrid_bwd_rays_jac_adam(const lnr_grid_desc* d, const float* rays, const float* z, int64_t n_rays,
                                   int32_t n_samples, const uint32_t* d_jac, const float* d_sigma, int64_t jac_stride,
                                   const lnr_adam_epilogue* adam, void* workspace, int64_t workspace_bytes,
                                   int32_t flags, void* stream);
/* With flags & LNR_BWD_NO_ACCUM the three calls above stop after the scatter; this finishes the
 * levels [level_begin, level_end) (n = samples of that call, same workspace): their slice of
 * d_table is final on return, so a data-parallel caller can all-reduce it while the next range
 * accumulates. */
int lnr_hashgrid_bwd_accum(const lnr_grid_desc* d, int64_t n, void* workspace, int64_t workspace_bytes,
                           uint32_t level_begin, uint32_t level_end, float* d_table, void* stream);
/* The same after a live backward (flags: the backward's LNR_BWD_LIVE): picks the accumulation for its smaller
 * record counts (the unit work list); the result is the same either way. */
int lnr_hashgrid_bwd_accum_flags(const lnr_grid_desc* d, int64_t n, void* workspace, int64_t workspace_bytes,
                                 uint32_t level_begin, uint32_t level_end, float* d_table, int32_t flags, void* stream);
/* Same result with one fp32 atomic pair per corner (coarse levels merged in-wave); d_table
 * accumulates.  Kept as an independent implementation for cross-checking and A/B timing. */
int lnr_hashgrid_bwd_atomic(const lnr_grid_desc* d, const float* pos01, int64_t n, const float* d_enc,
                            int64_t enc_stride, float* d_table, void* stream);
int lnr_hashgrid_bwd_rays_atomic(const lnr_grid_desc* d, const float* rays, const float* z, int64_t n_rays,
                                 int32_t n_samples, const float* d_enc, int64_t enc_stride, float* d_table,
                                 void* stream);
/* level-major half2 -> tcnn AoS (N, 2L) fp16, and AoS fp16/fp32 grads -> level-major float2. */
int lnr_enc_to_aos(const uint32_t* enc, int64_t enc_stride, int64_t n, uint32_t n_levels, uint16_t* out, void* stream);
int lnr_aos_grad_to_enc(const uint16_t* g_aos_f16, const float* g_aos_f32, int64_t n, uint32_t n_levels,
                        float* d_enc, int64_t enc_stride, void* stream);

/* tcnn "SphericalHarmonics" encoding (colour head, nerf_tcnn.py:43,86): dir01 (N,3) fp32 in [0,1]^3
 * -> out (N, degree^2) fp16 row-major.  degree 1..4 (LONER uses 4). */
int lnr_sh_encode(const float* dir01, int64_t n, int32_t degree, uint16_t* out, void* stream);

/* ---------------------------------------------------------------- sigma MLP */
#define LNR_SIGMA_W0 (64 * 32)
#define LNR_SIGMA_W1 (16 * 64)
#define LNR_SIGMA_MLP_PARAMS (LNR_SIGMA_W0 + LNR_SIGMA_W1)

/* sigma (N) fp16 = MLP(enc).  Non-finite outputs are clamped to +-65504 (nerf_tcnn.py:74-78). */
int lnr_sigma_mlp_fwd(const uint16_t* w, const uint32_t* enc, int64_t enc_stride, int64_t n, uint16_t* sigma,
                      void* stream);
/* Number of fp32 words of workspace lnr_sigma_mlp_bwd / lnr_field_train need for dW slabs. */
int64_t lnr_dw_workspace_words(int64_t n_rows);
/* d_sigma (N) fp32 -> d_enc (level-major float2, overwritten) and d_w (3072 fp32, ACCUMULATED). */
int lnr_sigma_mlp_bwd(const uint16_t* w, const uint32_t* enc, int64_t enc_stride, int64_t n, const float* d_sigma,
                      float* d_enc, float* d_w, float* workspace, void* stream);

/* ---------------------------------------------------------------- sampling */
/* Random draws: when u_* is NULL, draws come from the counter-based generator keyed by `key`
 * (see lnr_step_key) and the GLOBAL ray index ray_offset + r, so a sharded batch draws exactly
 * what the unsharded batch draws.  Otherwise u_jitter is (R, S/2) and u_pdf is (R, S/2). */
uint32_t lnr_step_key(uint32_t seed, uint32_t step);
int lnr_sample_ogm(const float* rays, int64_t n_rays, int32_t n_samples, const float* occ, int32_t occ_res,
                   float perturb, const float* u_jitter, const float* u_pdf, uint32_t key, int64_t ray_offset,
                   float* z, const lnr_step_scalars* dev_step, void* stream);
int lnr_sample_uniform(const float* rays, int64_t n_rays, int32_t n_samples, float perturb, const float* u_jitter,
                       uint32_t key, int64_t ray_offset, float* z, const lnr_step_scalars* dev_step, void* stream);

/* ---------------------------------------------------------------- compositing + loss */
#define LNR_RENDER_DEFAULT 0
#define LNR_RENDER_ADJUSTED 1

#define LNR_LOSS_L1_JS 0
#define LNR_LOSS_L2_JS 1
#define LNR_LOSS_L1_LOS 2
#define LNR_LOSS_L2_LOS 3

typedef struct lnr_loss_params {
  int32_t kind;            /* LNR_LOSS_* (optimizer.py:757-791) */
  float scale;             /* world-cube scale factor (metres per normalised unit) */
  float los_lambda;        /* already decayed for this global step (optimizer.py:712-716) */
  float depthloss_lambda;  /* loss.depthloss_lambda */
  float min_depth_eps;     /* loss.min_depth_eps */
  float min_js, max_js, js_alpha; /* loss.JS_loss */
  float los_eps;           /* L*_LOS only: decayed depth_eps for this iteration (optimizer.py:781-785) */
  float far_ref;           /* far bound of GLOBAL ray 0: optimizer.py:724 compares every ray with it */
  float inv_n_opaque;      /* 1 / (global opaque-ray count) */
  float inv_rs;            /* 1 / (global rays * samples) */
  const float* dev_n_opaque; /* optional DEVICE scalar: global opaque count (e.g. after an all-reduce);
                                when non-NULL it overrides inv_n_opaque (= 1/max(count,1)) */
  const float* dev_far_ref;  /* optional DEVICE scalar overriding far_ref (rays built on the device:
                                lnr_build_lidar_rays writes it) */
  uint32_t* dev_status;      /* optional DEVICE word: LNR_STATUS_* bits are OR-ed in (no host sync; the
                                caller reads it when it chooses, e.g. once per window) */
  float* dev_loss_out;       /* optional DEVICE [8]: lnr_field_train also writes lnr_loss_finalize's output
                                here, in its last launch (one launch less per step) */
  int32_t flags;             /* LNR_LP_* */
  const lnr_step_scalars* dev_step; /* optional DEVICE: key (the noise), los_lambda and los_eps from here */
  float* dev_d_ray;          /* optional DEVICE (R,2), lnr_field_train: [dL/d|d|, dL/dfar] per ray, the loss's
                                dependence on the ray itself when the poses are optimised (optimizer.py:258-262;
                                rendering_tcnn.py:248,274-278; the samples z are detached, ray_sampling.py:75-90).
                                With the hash grid's input gradient (lnr_hashgrid_bwd_rays_jac's d_pos) it gives
                                dL/d{origin, direction, far} of every ray (joint pose + map) */
  uint32_t* dev_term_hist;   /* optional DEVICE LNR_TERM_HIST_SLOTS x (n_samples / 64 + 1) counters, slot-major,
                                lnr_field_train with n_samples a multiple of 64: ray r adds 1 to bin c / 64 of slot
                                r mod LNR_TERM_HIST_SLOTS, c = the number of its samples after which its
                                transmittance product is still >= LNR_ERT_T_MIN (c = n_samples: it never terminates).
                                The caller sums the slots (they only spread the atomics) and differences two reads:
                                the library never clears them.  The rays alive after sample k (a multiple of 64)
                                are the bins >= k / 64, which is what picks the phases of
                                lnr_hashgrid_fwd_rays_phase / lnr_field_sigma_phase */
} lnr_loss_params;
#define LNR_TERM_HIST_SLOTS 256
#define LNR_ERT_T_MIN 1e-50      /* early ray termination: a ray whose transmittance product fell below this has
                                    float transmittance exactly 0 at every later sample (csrc/field.hip) */
#define LNR_LP_DW_OVERWRITE 1  /* lnr_field_train STORES d_w (the MLP gradient) instead of adding to it */
#define LNR_LP_SIGMA_READY 2   /* lnr_field_train: sigma is already in its workspace (lnr_field_sigma_phase), the
                                  MLP forward is not run again (n_samples in {64, 128, 256, 512}) */
#define LNR_LP_FORWARD_ONLY 4  /* lnr_field_train (n_samples in {64, 128, 256, 512}, d_enc_jac): the sigma forward and
                                  the compositing + loss + its backward only (dL/dsigma in the workspace); a second
                                  call with the same arguments and LNR_LP_BACKWARD_ONLY runs the MLP backward and the
                                  reductions.  Between the two, work that needs dL/dsigma but not J (the live
                                  backward's LNR_BWD_PREPARE_ONLY) can run on another stream */
#define LNR_LP_BACKWARD_ONLY 8

/* Status bits (replace the reference's per-step host checks):
 *   LNR_STATUS_NAN_LOSS     loss is NaN: optimizer.py:854 asserts "NaN Loss Encountered"
 *   LNR_STATUS_INF_LOSS     loss is +-inf
 *   LNR_STATUS_SIGMA_CLIPPED a sigma was non-finite and clipped by nan_to_num (nerf_tcnn.py:74-78 warns) */
#define LNR_STATUS_NAN_LOSS 1u
#define LNR_STATUS_INF_LOSS 2u
#define LNR_STATUS_SIGMA_CLIPPED 4u
#define LNR_STATUS_NONFINITE_OUTPUT 8u  /* lnr_status_scan found nan/inf (rendering_tcnn.py:419-424 DEBUG scan) */
/* ORs `bit` into the device word `status` when any of values[0..n) is nan or inf (no host sync). */
int lnr_status_scan(const float* values, int64_t n, uint32_t bit, uint32_t* status, void* stream);

/* Per-ray partial sums written by the loss kernels: [depth_sq_err, los_sum, opacity_abs_err, eps, opaque] */
#define LNR_RAY_STATS 5

/* Forward compositing from given sigma (R,S) fp32 (fp16-valued) and noise (R,S) (NULL + noise_std>0 ->
 * generated; noise_std==0 -> none).  Outputs may be NULL except depth. */
int lnr_composite(const float* rays, const float* z, const float* sigma, int64_t n_rays, int32_t n_samples,
                  int32_t strategy, float noise_std, const float* noise, uint32_t key, int64_t ray_offset,
                  float* weights, float* depth, float* opacity, float* variance, void* stream);
/* Training loss + gradient from given sigma: d_sigma (R,S) fp32, ray_stats (R, LNR_RAY_STATS). */
int lnr_composite_loss_bwd(const float* rays, const float* z, const float* sigma, const float* depth_gt,
                           int64_t n_rays, int32_t n_samples, float noise_std, const float* noise, uint32_t key,
                           int64_t ray_offset, const lnr_loss_params* lp, float* weights, float* depth,
                           float* opacity, float* d_sigma, float* ray_stats, void* stream);
/* Autograd backward of lnr_composite (the tcnn-compatible render_rays path, where the loss is the
 * caller's torch code): d_sigma (R,S) fp32 from upstream gradients of weights (R,S), depth, opacity
 * and variance (R); any of them may be NULL (= zero).  Same noise arguments as the forward, so the
 * noise is regenerated bit-identically instead of being stored.  d_ray (optional, (R,2)): the
 * render's gradient w.r.t. the ray itself, [dL/d|d| (deltas are scaled by the direction's norm,
 * rendering_tcnn.py:248), dL/dfar (the default depth's far term, :274-278; 0 for the adjusted
 * strategy)] - what autograd returns when the rays require grad (poses under optimisation). */
int lnr_composite_bwd(const float* rays, const float* z, const float* sigma, int64_t n_rays, int32_t n_samples,
                      int32_t strategy, float noise_std, const float* noise, uint32_t key, int64_t ray_offset,
                      const float* g_weights, const float* g_depth, const float* g_opacity, const float* g_variance,
                      float* d_sigma, float* d_ray, void* stream);
/* Workspace (fp32 words) lnr_field_train needs: the dW slabs, then an (n_rays, n_samples) d_sigma
 * buffer between its ray phase and its tile-parallel MLP backward. */
int64_t lnr_field_train_workspace_words(int64_t n_rays, int32_t n_samples);
/* Fused: sigma MLP forward from enc, compositing, loss, compositing backward, MLP backward.
 * Writes d_enc (level-major float2), accumulates d_w (3072 fp32), per-ray stats; optional outputs NULL.
 * d_enc_level_max (optional, 16 floats): OVERWRITTEN with max |d_enc| per level, the hash-grid
 * backward's record scales (pass lnr_hashgrid_bwd_level_max(...) and LNR_BWD_LEVEL_MAX_READY).
 * d_enc_jac (optional; n_samples 64, 128, 256 or 512): written INSTEAD of d_enc (which may be NULL):
 * J = d sigma / d enc as level-major fp16 pairs, one uint32 per (level, sample), so that
 * d_enc = d_sigma * J with d_sigma the (n_rays, n_samples) fp32 dL/dsigma this call leaves at
 * workspace + lnr_dw_workspace_words(n_rays); lnr_hashgrid_bwd_rays_jac takes both (half the bytes).
 * J is written only for the 32-sample tile pairs holding a sample with d_sigma != 0: elsewhere d_enc is 0
 * whatever J is, and the J entries keep stale values (every consumer of the pair forms d_sigma * J as 0 where
 * d_sigma == 0).  The MLP gradient is bitwise the one with every pair computed (a dead pair adds exact zeros).
 * workspace: lnr_field_train_workspace_words(n_rays, n_samples) fp32 words. */
int lnr_field_train(const uint16_t* w, const uint32_t* enc, int64_t enc_stride, const float* rays, const float* z,
                    const float* depth_gt, int64_t n_rays, int32_t n_samples, float noise_std, const float* noise,
                    uint32_t key, int64_t ray_offset, const lnr_loss_params* lp, float* d_enc, float* d_w,
                    float* workspace, float* ray_stats, float* depth, float* opacity, float* weights,
                    float* d_enc_level_max, uint32_t* d_enc_jac, void* stream);
/* Early ray termination (the training step on a trained field): the sigma MLP forward of samples [lo, hi) of
 * the rays list_in[0 .. *count_in) (DEVICE; ignored when lo == 0: every ray) (multiples of 64) into
 * lnr_field_train's workspace, where lnr_field_train with LNR_LP_SIGMA_READY reads it.  When hi < n_samples it
 * then takes each listed ray's transmittance[r] (fp64; 1 before lo == 0) times the
 * product over the phase of s = 1 - alpha + 1e-10 (the compositing's own arithmetic: noise, deltas as
 * lnr_field_train draws them; key, noise_std, noise, ray_offset, lp->dev_step as there), and lists the rays whose
 * product stays >= LNR_ERT_T_MIN in list_out[0 .. *count_out) in list order (through `scratch`, at least
 * n_rays 32-bit words); the others get sigma 0 at their samples [hi, n_samples).  A ray whose product fell below
 * 1e-50 has every later
 * sample's float transmittance 0 in the compositing, whose own double products associate differently but agree
 * to ~1e-13 relative (the margin to float's 1.4e-45 is 1e5), so its later samples' sigma and encodings do not
 * reach any output: the phases lnr_hashgrid_fwd_rays_phase -> lnr_field_sigma_phase, phase by phase (the lists
 * alternating between two buffers), then lnr_field_train with LNR_LP_SIGMA_READY, give the step's results without
 * evaluating them.  That equivalence is empirical, not a theorem: the step is bitwise the one without termination
 * on every field tested (tests/test_gpu_live.py), under the bound csrc/field.hip states for the later samples'
 * alpha (factors below 1e-50 / T in the suffix sums of the samples before them).
 * lp: optional (dev_status: LNR_STATUS_SIGMA_CLIPPED for the evaluated samples; dev_step: the key). */
int lnr_field_sigma_phase(const uint16_t* w, const uint32_t* enc, int64_t enc_stride, const float* rays,
                          const float* z, int64_t n_rays, int32_t n_samples, int32_t lo, int32_t hi, float noise_std,
                          const float* noise, uint32_t key, int64_t ray_offset, const lnr_loss_params* lp,
                          float* workspace, const uint32_t* list_in, const uint32_t* count_in, uint32_t* list_out,
                          uint32_t* count_out, double* transmittance, void* scratch, void* stream);
/* Early ray termination, the march: what the phases lnr_hashgrid_fwd_rays_phase -> lnr_field_sigma_phase give
 * at the bounds lo, lo + 64, ..., n_samples (lo a multiple of 64, 0 < lo < n_samples), in one launch and bitwise
 * (tests/test_gpu_ert_march.py): for every ray of list_in[0 .. *count_in) (DEVICE: the rays alive at lo, as the
 * phase ending at lo listed them) one workgroup encodes the ray's next 64 samples at all 16 levels into enc (the
 * level-major array of lnr_hashgrid_fwd_rays, table = the fp16 table), evaluates their sigma into
 * lnr_field_train's workspace, multiplies transmittance[r] by the unit's product of s = 1 - alpha + 1e-10 (the
 * arithmetic and order of lnr_field_sigma_phase), and goes on to the next 64 while the product stays >=
 * LNR_ERT_T_MIN; a ray that falls below gets sigma 0 at its remaining samples, whose encodings are left unwritten.
 * The last 64 samples update nothing, as the last phase.  No list is written: transmittance[r] >= LNR_ERT_T_MIN
 * tells which rays were still alive after sample n_samples - 64.  The sigma grid only (16 levels of 2 features).
 * noise_std, noise, key, ray_offset, lp as lnr_field_sigma_phase. */
int lnr_field_ert_march(const lnr_grid_desc* d, const uint16_t* table, uint32_t* enc, int64_t enc_stride,
                        const uint16_t* w, const float* rays, const float* z, int64_t n_rays, int32_t n_samples,
                        int32_t lo, float noise_std, const float* noise, uint32_t key, int64_t ray_offset,
                        const lnr_loss_params* lp, float* workspace, const uint32_t* list_in,
                        const uint32_t* count_in, double* transmittance, void* stream);
/* Joint pose + map (optimizer.py:235-262): the per-keyframe gradient of the pose tensors [t, axis-angle] (K, 6)
 * from a step's per-sample dL/dpos01 d_pos (n_rays * n_samples, 3) (lnr_hashgrid_bwd_rays_jac) and per-ray
 * [dL/d|d|, dL/dfar] d_ray (n_rays, 2) (lnr_loss_params.dev_d_ray), for rays built as
 * LidarRayDirections.build_lidar_rays builds them (o = (t + shift) / scale, d = R v / |R v|, far = min(r_max /
 * scale, get_far_val(o, d)); ray_utils.py:31-60,269-322): ray r is window slot slots[r] (slots NULL: slot0 + r),
 * of keyframe slot_kf[slot], and carries slot_pose[slot] (1: a LiDAR ray of an optimised pose, 0: a sky ray --
 * built from the detached pose, keyframe.py:98 -- or an anchored keyframe).  grad (K, 6) is OVERWRITTEN (a
 * fixed-order, deterministic sum); ray_ws: n_rays * 12 floats.  far_range = r_max / scale. */
int lnr_pose_grad(const float* rays, const float* z, const float* d_pos, const float* d_ray, int64_t n_rays,
                  int32_t n_samples, const int64_t* slots, int64_t slot0, const int32_t* slot_kf, const float* slot_pose,
                  const float* pose6, int32_t n_kf, float scale, float far_range, float* ray_ws, float* grad,
                  void* stream);
/* The poses' Adam step (torch.optim.Adam, the pose group of optimizer.py:262: betas, eps, lr = lrate_pose x the
 * ExponentialLR factor; step = this Adam's step count, from 1) on pose6 with moments m, v (K, 6), for keyframes
 * with optimise[k] != 0 (NULL: all), then rows (K, 12) = [R | t] of every pose (the RayWindow's pose layout; may
 * be NULL).  grad NULL: only the rows are written (m, v, step unused).  The hyper-parameters are doubles, as
 * lnr_adam_step's: 1 - beta is formed in double before its rounding to fp32. */
int lnr_pose_adam(float* pose6, float* m, float* v, const float* grad, const uint8_t* optimise, int32_t n_kf,
                  int64_t step, double lr, double beta1, double beta2, double eps, float* rows, void* stream);
/* Forward-only render from enc (inference path, C3 shape): sigma MLP + compositing.  With weights
 * (R,S) given, the sigma MLP runs tile-parallel first and stages sigma in weights, which the
 * compositing then overwrites with the weights (weights must not alias the other buffers); without,
 * one fused kernel per ray.  Same results either way. */
int lnr_field_render(const uint16_t* w, const uint32_t* enc, int64_t enc_stride, const float* rays, const float* z,
                     int64_t n_rays, int32_t n_samples, int32_t strategy, float noise_std, const float* noise,
                     uint32_t key, int64_t ray_offset, float* depth, float* opacity, float* variance,
                     float* weights, void* stream);
/* Colour head forward + colour map (DecoupledNeRF colour branch nerf_tcnn.py:80-95, raw2outputs
 * rendering_tcnn.py:283-289): w_rgb = tcnn flat fp16 params of the 48 -> 64 x n_hidden_layers -> 3
 * FullyFusedMLP (1..4 hidden layers), enc_rgb = level-major colour hash-grid encodings (16 levels x 2),
 * weights (R,S) = the sigma pass's compositing weights (lnr_field_render).  Directions = rays[:, 6:9]
 * (SH degree 4 of (viewdir + 1) / 2).  rgb (R,3) = sum_i w_i sigmoid(c_i) + 1 - sum_i w_i. */
int lnr_rgb_render(const uint16_t* w_rgb, int32_t n_hidden_layers, const uint32_t* enc_rgb, int64_t enc_stride,
                   const float* rays, const float* weights, int64_t n_rays, int32_t n_samples, float* rgb,
                   void* stream);
/* out[0] = loss, out[1] = mean eps, out[2..4] = depth/los/opacity terms, out[5] = opaque count,
 * from (R, LNR_RAY_STATS). */
int lnr_loss_finalize(const float* ray_stats, int64_t n_rays, const lnr_loss_params* lp, float* out, void* stream);

/* out[0] = number of opaque rays: depth_gt > 0 && !(depth_gt > far_ref) (optimizer.py:724-727).
 * dev_far_ref: optional DEVICE scalar overriding far_ref. */
int lnr_count_opaque(const float* depth_gt, int64_t n_rays, float far_ref, const float* dev_far_ref, float* out,
                     void* stream);

/* ---------------------------------------------------------------- ray selection + building */
#define LNR_SELECT_RANDOM 0 /* torch.randint over each scan (optimizer.py:365-366) */
#define LNR_SELECT_MASK 1   /* int(0.75 n) trunk points (0.5 < z_sensor < 8 m) + the rest from the other points,
                               each without replacement (optimizer.py:367-379) */
#define LNR_SELECT_ALL 2    /* every point of every scan, in order (LidarRayDirections.fetch_chunk_rays) */
#define LNR_SELECT_GIVEN 3  /* caller-supplied scan-local indices, one per slot (parity tests) */

/* The active keyframe window, resident on the device for the whole window.  All pointers are
 * DEVICE pointers; counts are validated by the caller (loner_amd.rays.RayWindow). */
typedef struct lnr_ray_window {
  int32_t n_kf;
  float scale;                /* WorldCube.scale_factor */
  float shift[3];             /* WorldCube.shift */
  float r_min, r_max;         /* ray_range (metres) */
  const float* poses;         /* [K][12]: the 3x4 [R | t] rows of each keyframe's lidar pose (world) */
  const float* dirs;          /* [P][3] sensor-frame ray directions (LidarScan.ray_directions, transposed) */
  const float* dists;         /* [P] ranges (metres) */
  const int32_t* scan_off;    /* [K+1] point offsets of each keyframe's scan in dirs / dists */
  const int32_t* order;       /* MASK: [P] per keyframe, scan-local indices of its trunk points, then the rest */
  const int32_t* n_trunk;     /* MASK: [K] trunk points per keyframe */
  const float* sky_dirs;      /* [Q][3] sky directions (LidarScan.sky_rays), or NULL without sky rays */
  const int32_t* sky_off;     /* [K+1] offsets into sky_dirs, or NULL */
  const int32_t* ray_off;     /* [K+1] output slots of each keyframe: its LiDAR rays, then its sky rays */
  const int32_t* n_sel;       /* [K] LiDAR slots per keyframe (slots beyond them are sky rays) */
  const int32_t* n_sel_trunk; /* MASK: [K] LiDAR slots drawn from the trunk points */
  const lnr_step_scalars* dev_step; /* optional DEVICE: the draw key from here instead of `key` */
} lnr_ray_window;

/* Build output slots [slot0, slot0 + n_slots) of the window's ray batch: rays (n_slots, 13), depth
 * (n_slots) normalised, valid (n_slots) = far > near + 1 m / scale (the reference drops invalid rays;
 * NULL allowed), point_index (n_slots) scan-local point of each slot (NULL allowed), far_ref (1) =
 * far bound of the first valid slot of the WHOLE batch (NULL allowed).  Draws keyed by
 * (key, keyframe, slot-in-keyframe): a sharded build reproduces the unsharded one slot for slot. */
int lnr_build_lidar_rays(const lnr_ray_window* window, int32_t select, const int32_t* given, uint32_t key,
                         int64_t slot0, int64_t n_slots, float* rays, float* depth, uint8_t* valid,
                         int32_t* point_index, float* far_ref, void* stream);

/* Camera rays (KeyFrame.build_camera_rays, src/mapping/keyframe.py:108-127 ->
 * CameraRayDirections.build_rays, src/common/ray_utils.py:175-212): for pixel p = j * width + i,
 * rays[k] = [o, d, -d, i, j, r_min / scale, get_far_val(o, d)] with d = normalise(R dirs[p]),
 * o = (t + shift) / scale; intensities[k] = image[p] (channels floats, optional).  dirs = the
 * (height * width, 3) undistorted camera-frame directions (get_ray_directions, ray_utils.py:62-124,
 * computed once per calibration by the host). */
typedef struct lnr_camera_desc {
  int32_t width, height, channels;
  float scale;        /* WorldCube.scale_factor */
  float shift[3];     /* WorldCube.shift */
  float r_min;        /* ray_range[0] (metres) */
  float pose[12];     /* camera pose in the world, 3x4 [R | t] rows */
} lnr_camera_desc;
int lnr_build_camera_rays(const lnr_camera_desc* cam, const float* dirs, const float* image, const int64_t* pixels,
                          int64_t n, float* rays, float* intensities, void* stream);
/* A whole camera window in one launch: frames = DEVICE array of n_frames {camera, image}; frame f
 * fills slots [f n_per_frame, (f + 1) n_per_frame) from pixels[f stride + first + j] (a window's
 * per-frame pixel schedules, optimizer.py:626-644).  intensities may be NULL. */
typedef struct lnr_camera_frame {
  lnr_camera_desc cam;
  const float* image;   /* (height * width, channels) fp32, DEVICE */
} lnr_camera_frame;
int lnr_build_camera_rays_window(const lnr_camera_frame* frames, int32_t n_frames, const float* dirs,
                                 const int64_t* pixels, int64_t stride, int64_t first, int64_t n_per_frame,
                                 float* rays, float* intensities, void* stream);

/* Colour-head training, camera phase (Optimizer._do_iterate_optimizer_camera + compute_loss_camera,
 * src/mapping/optimizer.py:541-688,861-894): sigma frozen and detached (weights = the sigma pass's
 * compositing weights, lnr_field_render); rgb as lnr_rgb_render; loss = l1(rgb, intensities) as a
 * mean over the 3 * (global) rays: inv_count = 1 / (3 n_rays_global).  Writes rgb (R,3), loss[0]
 * (optional; local rays only), d_enc (level-major float2, the colour-grid backward's input, as
 * lnr_field_train's) and d_w (OVERWRITTEN: the colour MLP's weight gradient, tcnn flat layout,
 * lnr_rgb_mlp_params floats).  Deterministic (fixed-order slab reduction).  d_enc_level_max
 * (optional, 16 floats): OVERWRITTEN with max |d_enc| per level, as lnr_field_train's (pass
 * lnr_hashgrid_bwd_level_max(...) and LNR_BWD_LEVEL_MAX_READY to the colour grid's backward). */
int64_t lnr_rgb_mlp_params(int32_t n_hidden_layers);
int64_t lnr_rgb_train_workspace_bytes(int32_t n_hidden_layers, int64_t n_rays);
int lnr_rgb_train(const uint16_t* w_rgb, int32_t n_hidden_layers, const uint32_t* enc_rgb, int64_t enc_stride,
                  const float* rays, const float* weights, const float* intensities, int64_t n_rays,
                  int32_t n_samples, float inv_count, float* rgb, float* loss, float* d_enc, float* d_w,
                  void* workspace, int64_t workspace_bytes, float* d_enc_level_max, void* stream);

/* ---------------------------------------------------------------- optimiser */
/* torch.optim.Adam (no weight decay); step is 1-based.  shadow (fp16) may be NULL.  dev_step (optional):
 * the step size and bias correction from there (step and lr are then ignored). */
int lnr_adam_step(float* param, uint16_t* shadow, const float* grad, float* m, float* v, int64_t n, int32_t step,
                  double lr, double beta1, double beta2, double eps, const lnr_step_scalars* dev_step, void* stream);
/* The same step over up to LNR_ADAM_MAX_RANGES independent ranges in one launch (the sharded
 * optimiser's per-level-range chunks, loner_amd.step.StepEngine(zero=...)). */
#define LNR_ADAM_MAX_RANGES 8
typedef struct lnr_adam_range {
  float* param;
  uint16_t* shadow; /* may be NULL */
  const float* grad;
  float* m;
  float* v;
  int64_t n;
} lnr_adam_range;
int lnr_adam_step_ranges(const lnr_adam_range* ranges, int32_t n_ranges, int32_t step, double lr, double beta1,
                         double beta2, double eps, const lnr_step_scalars* dev_step, void* stream);
/* OGM update: occ (res^3) -= lr * grid_sample^T(logits_grad(z*scale - depth_gt*scale)).  grad_ws is
 * workspace of ws_words fp32 (lnr_ogm_workspace_words(occ_res) for full speed; at least 3 res^3):
 * the splat accumulates in int64 fixed point in replicas of the grid that spread same-voxel
 * atomics (bitwise reproducible), and grad_ws[0, res^3) receives the fp32 gradient. */
int64_t lnr_ogm_workspace_words(int32_t occ_res);
int lnr_ogm_update(const float* rays, const float* z, const float* depth_gt, int64_t n_rays, int32_t n_samples,
                   float scale, float lr, float* occ, float* grad_ws, int64_t ws_words, int32_t occ_res, void* stream);

/* Split form for data-parallel runs: grad_ws[0:res^3] = grid_sample^T(logits_grad) (the call zeroes the
 * workspace), then occ -= lr * grad_ws[0:res^3] after the caller has all-reduced that slice. */
int lnr_ogm_grad(const float* rays, const float* z, const float* depth_gt, int64_t n_rays, int32_t n_samples,
                 float scale, float* grad_ws, int64_t ws_words, int32_t occ_res, void* stream);
int lnr_sgd_step(float* param, const float* grad, int64_t n, float lr, void* stream);

/* OccupancyGridModel.interpolate (src/models/model_tcnn.py:126-134) as an operator of its own, for the
 * module-level drop-in (Optimizer._step_occupancy_grid, src/mapping/optimizer.py:897-908, calls it and
 * backpropagates through it).  Replaces torch.nn.functional.grid_sample on a (1, 1, res, res, res) grid
 * with (n, 3) points in [-1, 1]: trilinear, align_corners=False, zeros padding.
 *   lnr_grid_sample3d      out[i] = grid_sample(grid, pts[i])
 *   lnr_grid_sample3d_bwd  dgrid = sum_i dout[i] d out[i] / d grid (overwritten; the points get no
 *                          gradient: the reference's points are detached).  Deterministic: int64
 *                          fixed point with a unit from max |dout| and n (about 2^-42 of max |dout|
 *                          per point at n = 10^6); ws: lnr_grid_sample3d_bwd_workspace_words(res)
 *                          fp32 words, 8-byte aligned (2 + 2 res^3 at least). */
int lnr_grid_sample3d(const float* grid, int32_t res, const float* pts, int64_t n, float* out, void* stream);
int64_t lnr_grid_sample3d_bwd_workspace_words(int32_t res);
int lnr_grid_sample3d_bwd(const float* pts, const float* dout, int64_t n, int32_t res, float* dgrid, float* ws,
                          int64_t ws_words, void* stream);

/* ---------------------------------------------------------------- per-keyframe scan preprocessing */
/* LidarScan.motion_compensate (src/common/sensors.py:169-231).  Host-computed per scan: the start pose
 * rotation (row-major) and translation, end - start translation, axis/angle of R_start^T R_end
 * (identity = angle < 1e-9), timestamps t0/t1 of the two poses, and the first 3 rows of
 * inv(T_world_to_target).  dirs (P,3) / dists (P) are rewritten in place. */
typedef struct lnr_motion_comp {
  float start_rot[9];
  float start_t[3];
  float delta_t[3];
  float axis[3];
  float angle;
  float t0, t1;
  float target_inv[12];
  int32_t identity;
} lnr_motion_comp;
int lnr_motion_compensate(const lnr_motion_comp* mc, const float* timestamps, float* dirs, float* dists,
                          int64_t n_points, void* stream);

/* compute_sky_rays (examples/fdt_optimize_implicit_map_utils.py:38-77): sky directions (rotated by
 * rot, the lidar pose rotation, row-major) of one scan's dirs (P,3), written as (count, 3) into out
 * (capacity cap directions, lnr_sky_rays_capacity() is enough); count (1 int32, device) = number. */
typedef struct lnr_sky_params {
  float rot[9];
  int32_t top_rows;     /* TOP_ROWS = 3 */
  float horizon_deg;    /* HORIZON_OFFSET = 10 */
} lnr_sky_params;
int64_t lnr_sky_rays_capacity(void);
int lnr_sky_rays(const float* dirs, int64_t n_points, const lnr_sky_params* params, float* out, int64_t cap,
                 int32_t* count, void* stream);

/* ---------------------------------------------------------------- mesh extraction (analysis/mesher.py) */
/* The weight volume of mesher.py:139-180: every sample of weights (R,S) with weight > 0 whose ray has
 * depth[r] < depth_max (and variance[r] < var_max when var_max > 0; variance may be NULL otherwise) and whose point
 * o + d z (fp32) lies in [b[0], b[n - 1]] on every axis raises volume[cell] to its weight, cell = x_buck * nz +
 * y_buck * nx * nz + z_buck (the reference's formula, kept literally: its (ny, nx, nz) layout), *_buck =
 * torch.bucketize(point, b, right=False) = the first i with b[i] >= point.  bx[nx], by[ny], bz[nz]: DEVICE float64
 * boundaries, non-decreasing.  volume (nx * ny * nz floats, non-negative) is ACCUMULATED with the true maximum (an
 * integer atomic max on the weight's bits: independent of order and chunking); cells >= nx * ny * nz are dropped. */
int lnr_volume_splat_max(const float* rays, const float* z, const float* weights, const float* depth,
                         const float* variance, int64_t n_rays, int32_t n_samples, const double* bx, int32_t nx,
                         const double* by, int32_t ny, const double* bz, int32_t nz, float depth_max, float var_max,
                         float* volume, void* stream);
/* Indexed marching cubes of volume (nx, ny, nz) fp32, C order, at `level` (a corner is inside iff value > level).
 * Each crossed grid edge belongs to the voxel at its lower end; voxel v = (ix ny + iy) nz + iz owns up to three
 * vertices (its edges along x, y, z, in that order) and the triangles of the cell whose lower corner it is.
 *   _count  vert_count[v], tri_count[v] (nx ny nz int32 each)
 *   _emit   vert_offset / tri_offset = the EXCLUSIVE scans of those counts (int64; the scan is the caller's),
 *           n_verts / n_faces their totals: verts (n_verts, 3) = lower corner index x spacing, plus
 *           (level - f_a) / (f_b - f_a) x spacing along the edge's axis (fp32, in this order); faces (n_faces, 3)
 *           int32 vertex ids, in cell order then table order, wound so that normals point from inside to outside.
 * The case table resolves a face with inside corners on one diagonal by cutting off each inside corner, from the
 * face's own corners alone: adjacent cells agree and the mesh is closed wherever the surface avoids the border. */
int lnr_marching_cubes_count(const float* volume, int32_t nx, int32_t ny, int32_t nz, float level,
                             int32_t* vert_count, int32_t* tri_count, void* stream);
int lnr_marching_cubes_emit(const float* volume, int32_t nx, int32_t ny, int32_t nz, float level, float sx, float sy,
                            float sz, const int64_t* vert_offset, const int64_t* tri_offset, int64_t n_verts,
                            int64_t n_faces, float* verts, int32_t* faces, void* stream);

/* ---------------------------------------------------------------- frame-to-frame tracking (src/tracking/tracker.py) */
/* Normals of a cloud, Open3D's estimate_normals() with KDTreeSearchParamKNN(k): for each point of pts (n, 3) its exact k
 * nearest neighbours in the same cloud (itself included), ordered by (squared fp32 distance, index); the covariance
 * about their mean and the unit eigenvector of its smallest eigenvalue in fp64, turned towards the origin
 * (normal . point <= 0); (0, 0, 1) when the covariance is all zero.  3 <= k <= 64, k <= n <= 2^18; the work is O(n^2). */
int lnr_cloud_normals(const float* pts, int64_t n, int32_t k, float* normals, void* stream);

/* Point-to-plane ICP (Open3D's registration_icp with TransformationEstimationPointToPlane) as a schedule of kernels
 * around a device-resident state.  T (row-major 4x4) maps source points into the target's frame. */
#define LNR_ICP_MAX_POINTS (1 << 24)
typedef struct lnr_icp_state {
  double T[16];
  double fitness;     /* kept pairs / n_src of the last evaluation */
  double rmse;        /* sqrt(sum d^2 / kept pairs) of the last evaluation, 0 without pairs */
  double sum_d2;
  double sums[27];    /* the last evaluation's J^T J (upper triangle, row-major, 21) and J^T r (6) */
  int64_t n_corr;
  int32_t iterations; /* updates applied in this stage */
  int32_t converged;
} lnr_icp_state;
int64_t lnr_icp_workspace_bytes(int64_t n_src);  /* 0 for an n_src outside [1, LNR_ICP_MAX_POINTS] */
/* state <- {T0 (16 HOST doubles, copied before the call returns), everything else 0}. */
int lnr_icp_init(lnr_icp_state* state, const double* T0, void* stream);
/* One stage from the state's T: max_iterations + 1 rounds of two kernels, all enqueued by this call.
 *   correspond  p = T s in fp64; the nearest target point q of p rounded to fp32, by (squared fp32 distance, index);
 *               the pair is kept iff d^2 < threshold^2 (fp32).  Kept pairs add J^T J, J^T r (J = [p x n, n],
 *               r = (p - q) . n, n = q's normal; fp64), 1 to the count and |p - q|^2 to sum d^2, as one row of
 *               partial sums per block in the workspace.  corr_idx (n_src int32, -1 = none) and corr_d2 (n_src fp32,
 *               0 = none) are written when not NULL.
 *   update      the rows added in a fixed order; fitness and rmse; from the second round on, converged iff
 *               |fitness - previous| < rel_fitness and |rmse - previous| < rel_rmse; otherwise, while fewer than
 *               max_iterations updates were applied, T <- M(x) T with J^T J x = -J^T r (6x6 Cholesky, fp64) and
 *               M = Rz(x2) Ry(x1) Rx(x0) | x3..5.  Fewer than 6 pairs or a failed solve leave T as it is.
 * Rounds after convergence do nothing.  The first round clears `converged` and `iterations` and keeps T, so stages
 * chain without a host decision; the results repeat bit for bit.  workspace: lnr_icp_workspace_bytes(n_src) bytes,
 * 8-byte aligned. */
int lnr_icp_stage(const float* src, int64_t n_src, const float* tgt, const float* tgt_normals, int64_t n_tgt,
                  float threshold, int32_t max_iterations, double rel_fitness, double rel_rmse, lnr_icp_state* state,
                  void* workspace, int64_t ws_bytes, int32_t* corr_idx, float* corr_d2, void* stream);

/* ---------------------------------------------------------------- map evaluation (analysis/evaluate_lidar_map.py) */
/* Voxel filter, nearest-neighbour distances and their statistics: what the reference's map evaluation hands to Open3D
 * (voxel_down_sample, compute_point_cloud_distance).  Sorting and prefix sums between the calls are the caller's
 * (a STABLE sort of the keys; loner_amd/map_eval.py).  No float atomics; every result repeats bit for bit. */
#define LNR_CLOUD_MAX_POINTS (1 << 27)
#define LNR_CLOUD_CELL_BITS 21              /* cell indices per axis: [0, 2^21) */
#define LNR_CLOUD_BAD_KEY INT64_MAX         /* the key of a point without a cell: the largest one */
#define LNR_CLOUD_NONFINITE 1u              /* status: a coordinate was nan or inf */
#define LNR_CLOUD_GRID_RANGE 2u             /* status: a cell index fell outside [0, 2^21) */
#define LNR_CLOUD_VOXEL_CHUNK 64            /* points per partial sum of the voxel filter */
#define LNR_NN_MAX_RINGS 4                  /* rings a query expands before it joins the exhaustive scan */
/* keys[i] = ix << 42 | iy << 21 | iz of pts (n, 3), i_a = floor((double(p_a) - origin[a]) / cell) with an IEEE fp64
 * subtraction and division.  origin: 3 DEVICE doubles.  A non-finite coordinate ORs LNR_CLOUD_NONFINITE into *status
 * (1 device uint32, never cleared here), an index outside [0, 2^21) (a non-finite origin included) LNR_CLOUD_GRID_RANGE;
 * such a point gets LNR_CLOUD_BAD_KEY.  No entry point below uses a key as an index: keys are only compared.
 * 1 <= n <= LNR_CLOUD_MAX_POINTS, 1e-12 <= cell < inf. */
int lnr_cloud_cell_keys(const float* pts, int64_t n, const double* origin, double cell, int64_t* keys,
                        uint32_t* status, void* stream);
/* heads[i] = 1 where sorted_keys[i] starts a run of equal keys (i = 0, or a key unlike its predecessor's), else 0.
 * The inclusive scan of heads numbers the occupied voxels in ascending key order from 1. */
int lnr_voxel_heads(const int64_t* sorted_keys, int64_t n, int32_t* heads, void* stream);
/* 0 for sizes outside 1 <= n_vox <= n <= LNR_CLOUD_MAX_POINTS. */
int64_t lnr_voxel_workspace_bytes(int64_t n, int64_t n_vox);
/* Open3D's voxel_down_sample from the sorted order: perm[i] (int64) is the point at sorted position i, head_scan[i]
 * (int64) the inclusive scan of lnr_voxel_heads, n_vox its last entry.  means (n_vox, 3) fp32: the mean of each
 * voxel's points, summed in fp64 and rounded once; counts (n_vox int32) when not NULL; both in ascending key order
 * (Open3D's own order is that of an unordered map).  A voxel's points are cut, in sorted order, into chunks of
 * LNR_CLOUD_VOXEL_CHUNK; one thread sums a chunk front to back and the voxel's chunk sums are added in chunk order:
 * the order of every sum depends on the data alone, and a stable sort makes it the points' input order.  Entries of
 * perm outside [0, n) and of head_scan outside [1, n_vox] are skipped, never followed.  workspace:
 * lnr_voxel_workspace_bytes(n, n_vox) bytes, 8-byte aligned. */
int lnr_voxel_reduce(const float* pts, const int64_t* perm, const int64_t* head_scan, int64_t n, int64_t n_vox,
                     void* workspace, int64_t ws_bytes, float* means, int32_t* counts, void* stream);
/* Open3D's compute_point_cloud_distance: for each point of src (n_src, 3) the target point with the smallest
 * (d2, index), d2 = dx dx + dy dy + dz dz in fp32 with every operation rounded (no contraction), so ties go to the
 * lower index.  The target comes as a uniform grid: tgt_sorted (n_tgt, 3) in ascending key order, tgt_keys their
 * lnr_cloud_cell_keys for (origin, cell), tgt_perm (int32) each one's index in the caller's order; dims: 3 DEVICE
 * int32, the grid's cells per axis (every target cell index < dims[a] <= 2^21).  Outputs: idx (int32, the caller's
 * index), d2 (fp32, the search key), dist (fp64: sqrt of the fp64 squared distance to the winner, recomputed).
 * A query expands Chebyshev rings of cells around its own (signed: it may lie outside the box; rings are cut to the
 * box, empty ones skipped) and stops after ring r >= 1 once d2 <= (r cell)^2 (1 - 2^-20), or when the box is
 * covered; after LNR_NN_MAX_RINGS rings, or at a ring of more than 81 columns, it joins a list in the workspace (an
 * integer counter; the list's order is arbitrary and no result depends on it) and is answered by an exhaustive scan
 * of the target with the same key.  Either way the result is the exact minimum of the key over all targets,
 * whatever `cell` is.  A non-finite query ORs LNR_CLOUD_NONFINITE into *status and gets idx -1, d2 = dist = inf.
 * 1 <= n_src, n_tgt <= LNR_CLOUD_MAX_POINTS, cell as above.  workspace: lnr_nn_workspace_bytes(n_src) bytes (0 for
 * an n_src outside the limits), 8-byte aligned. */
int64_t lnr_nn_workspace_bytes(int64_t n_src);
int lnr_nn_search(const float* src, int64_t n_src, const float* tgt_sorted, const int64_t* tgt_keys,
                  const int32_t* tgt_perm, int64_t n_tgt, const double* origin, double cell, const int32_t* dims,
                  void* workspace, int64_t ws_bytes, int32_t* idx, float* d2, double* dist, uint32_t* status,
                  void* stream);
/* out[0] = sum of dist[0 .. n), out[1] = the number of entries > threshold (as a double), fp64: one row of partial
 * sums per 4096 entries in the workspace, the rows added in a fixed order.  0 for n outside [1, LNR_CLOUD_MAX_POINTS]. */
int64_t lnr_dist_stats_workspace_bytes(int64_t n);
int lnr_dist_stats(const double* dist, int64_t n, double threshold, void* workspace, int64_t ws_bytes, double* out,
                   void* stream);

/* ---------------------------------------------------------------- ground-truth LiDAR map (examples/fusion_portable/create_lidar_map.py) */
/* A return at its own pose, k nearest neighbours on the grid of lnr_nn_search, and the two sums of Open3D's
 * remove_statistical_outlier.  status: 1 device uint32, ORed into and never cleared here.  No float atomics; every
 * result repeats bit for bit. */
#define LNR_KNN_MAX_K 64                    /* neighbours per query: one per lane of a wave */
/* out[p] (n, 3) fp32 = fp32(R pts[p] + x), the pose (R, x) of the trajectory at t[p] (fp64, absolute seconds), all in
 * fp64 and rounded once.  The trajectory: traj_t (n_poses, strictly increasing), traj_xyz (n_poses, 3), traj_rot
 * (n_poses, 9, row-major), rel_rotvec (n_poses - 1, 3) = the rotation vector of R_i^-1 R_i+1; DEVICE float64, prepared
 * on the host (loner_amd/lidar_map.py).  Interval i = searchsorted(traj_t, t, 'left') - 1, a t equal to traj_t[0] in
 * interval 0 (scipy's Slerp and interp1d); alpha = (t - t_i) / (t_i+1 - t_i); R = R_i exp(alpha rel_rotvec_i)
 * (Rodrigues, the series 1 - th^2 / 6 and 1 / 2 - th^2 / 24 below 1e-4 rad); x = x_i + alpha (x_i+1 - x_i).
 * valid[p] (uint8) = 0 and out[p] = 0 when |pts[p]| (fp64) is not > min_range, when t[p] lies outside
 * [traj_t[0], traj_t[n_poses - 1]] (never extrapolated), or when an input or the result is nan or inf, which also
 * ORs LNR_CLOUD_NONFINITE into *status.  1 <= n <= LNR_CLOUD_MAX_POINTS, 2 <= n_poses. */
int lnr_trajectory_transform(const float* pts, const double* t, int64_t n, const double* traj_t,
                             const double* traj_xyz, const double* traj_rot, const double* rel_rotvec,
                             int64_t n_poses, double min_range, float* out, uint8_t* valid, uint32_t* status,
                             void* stream);
/* The exact k nearest targets of each point of src (n_src, 3) by the key of lnr_nn_search, (d2, index) with d2 in fp32
 * and every operation rounded; the target is described as there (tgt_sorted, tgt_keys, tgt_perm, origin, cell, dims).
 * idx (n_src, k) int32 in the caller's indices and d2 (n_src, k) fp32, both ascending by the key; mean_dist (n_src)
 * fp64 when not NULL: the fp64 distances to the k winners (recomputed from the coordinates), added in list order,
 * divided by k.  A query that is a target finds itself at distance 0.  One wave per query expands Chebyshev rings and
 * stops after ring r >= 1 once it holds k keys and the k-th d2 <= (r cell)^2 (1 - 2^-20), or when the box is covered;
 * after LNR_NN_MAX_RINGS rings, or at a ring of more than 81 columns, it joins a list in the workspace (an integer
 * counter; no result depends on the list's order) and is answered by an exhaustive scan with the same key: the result
 * is the exact k smallest keys over all targets, whatever `cell` is.  A non-finite query ORs LNR_CLOUD_NONFINITE into
 * *status and its row is idx -1, d2 = mean_dist = inf; so are the entries a query cannot fill because fewer than k
 * targets are finite.  1 <= k <= min(LNR_KNN_MAX_K, n_tgt); sizes and cell as for lnr_nn_search.  workspace:
 * lnr_knn_workspace_bytes(n_src) bytes (0 for an n_src outside the limits), 8-byte aligned. */
int64_t lnr_knn_workspace_bytes(int64_t n_src);
int lnr_knn_search(const float* src, int64_t n_src, const float* tgt_sorted, const int64_t* tgt_keys,
                   const int32_t* tgt_perm, int64_t n_tgt, const double* origin, double cell, const int32_t* dims,
                   int32_t k, void* workspace, int64_t ws_bytes, int32_t* idx, float* d2, double* mean_dist,
                   uint32_t* status, void* stream);
/* Over the entries v[i] > 0 of v (n fp64): out[0] = their sum, out[1] = their number (as a double), out[2] = the sum
 * of (v[i] - c)^2, c = *centre_dev when centre_dev (1 DEVICE double) is not NULL, else `centre`.  One row of partial
 * sums per 4096 entries in the workspace, the rows added in a fixed order.  The workspace query returns 0 for n
 * outside [1, LNR_CLOUD_MAX_POINTS]. */
int64_t lnr_dist_moments_workspace_bytes(int64_t n);
int lnr_dist_moments(const double* v, int64_t n, double centre, const double* centre_dev, void* workspace,
                     int64_t ws_bytes, double* out, void* stream);

/* ---------------------------------------------------------------- registration on the cell grid (full-size clouds) */
/* lnr_cloud_normals and lnr_icp_stage for clouds their exhaustive searches cannot take: the neighbours come from the
 * grid of lnr_nn_search.  Both searches order targets by the same (fp32 d2, index) key and both paths add the same
 * fp64 terms in the same order, so wherever both can run the results are the same bits. */
/* normals[i] (n, 3) fp32 of the query pts[i] (n, 3) from its neighbour list: the points tgt[idx[i * k + j]], j < k, in
 * the order given (idx (n, k) int32, lnr_knn_search's).  The same steps as lnr_cloud_normals after its search: fp64
 * mean and covariance, the eigenvector of the smallest eigenvalue, (0, 0, 1) for a zero covariance, turned so that
 * normal . pts[i] <= 0; with the list lnr_cloud_normals finds, the same bits.  A row with an index outside
 * [0, n_tgt) follows none of its indices and gets the fallback (0, 0, 1), turned the same way.  3 <= k <= 64,
 * 1 <= n, n_tgt <= LNR_CLOUD_MAX_POINTS. */
int lnr_normals_from_knn(const float* pts, int64_t n, const float* tgt, int64_t n_tgt, const int32_t* idx, int32_t k,
                         float* normals, void* stream);
/* Host only: the rings of `cell` a correspondence search with `threshold` has to walk, the smallest R >= 1 with
 * (R cell)^2 (1 - 2^-20) >= thr2, thr2 = (float)((double)threshold * threshold) as lnr_icp_stage forms it: a target
 * outside rings 0 .. R has a key strictly above that bound (lnr_nn_search's stopping rule) and cannot be a kept pair.
 * 0 when R would exceed LNR_NN_MAX_RINGS, or for a threshold that is not positive and finite (its fp32 square
 * included) or a cell outside [1e-12, inf). */
int32_t lnr_icp_grid_rings(float threshold, double cell);
int64_t lnr_icp_grid_workspace_bytes(int64_t n_src);  /* 0 for an n_src outside [1, LNR_ICP_MAX_POINTS] */
/* lnr_icp_stage with the target as a grid (tgt_sorted, tgt_keys, tgt_perm, origin, cell, dims as for lnr_nn_search;
 * tgt_normals (n_tgt, 3) in the caller's order, which corr_idx also reports).  The contract is lnr_icp_stage's:
 * max_iterations + 1 rounds enqueued by this call, rounds after convergence do nothing, the first round clears
 * `converged` and `iterations` and keeps T, so grid and exhaustive stages chain on one state; partial rows of 16
 * consecutive source points, each added in index order, and the same update: the state after every round, corr_idx
 * and corr_d2 are lnr_icp_stage's bit for bit.  A query walks the rings of its cell as in lnr_nn_search but never
 * beyond R = lnr_icp_grid_rings(threshold, cell), and there is no exhaustive pass: a query without a target in rings
 * 0 .. R has no pair, as d2 < thr2 would have decided.  The call is refused before any launch when R is 0.  A source
 * point whose p = T s is not finite has no pair and ORs LNR_CLOUD_NONFINITE into *status (1 device uint32, never
 * cleared here); a target with LNR_CLOUD_BAD_KEY sorts last and is never visited.  workspace:
 * lnr_icp_grid_workspace_bytes(n_src) bytes, 8-byte aligned. */
int lnr_icp_stage_grid(const float* src, int64_t n_src, const float* tgt_sorted, const int64_t* tgt_keys,
                       const int32_t* tgt_perm, int64_t n_tgt, const double* origin, double cell, const int32_t* dims,
                       const float* tgt_normals, float threshold, int32_t max_iterations, double rel_fitness,
                       double rel_rmse, lnr_icp_state* state, void* workspace, int64_t ws_bytes, int32_t* corr_idx,
                       float* corr_d2, uint32_t* status, void* stream);

/* ---------------------------------------------------------------- mesh sampling(analysis/compute_metrics/maps/mesh_to_pcd.py) */
/* A triangle mesh as a cloud (Open3D's sample_points_uniformly) and its vertex normals (compute_vertex_normals,
 * analysis/meshing.py:122).  verts (n_verts, 3) fp32, faces (n_faces, 3) int32; 1 <= n_verts < 2^31,
 * 1 <= n_faces <= LNR_CLOUD_MAX_POINTS.  status: 1 device uint32, ORed into and never cleared here.  A face with an
 * index outside [0, n_verts) ORs LNR_MESH_BAD_INDEX and counts as a face of area 0; its indices are never followed.
 * All geometry is fp64 from the fp32 vertices, every operation rounded once, in the order written here, so a float64
 * restatement gives the same bits (loner_amd/mesh_cloud.py).  Scans and sorts between the calls are the caller's.
 * No float atomics; every result repeats bit for bit. */
#define LNR_MESH_BAD_INDEX 1u               /* status: a face index fell outside [0, n_verts) */
#define LNR_MESH_NO_FACE 2u                 /* status: a point index at or above bounds[n_faces - 1] */
/* c = e1 x e2 with e1 = v1 - v0, e2 = v2 - v0: c = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x);
 * |c| = sqrt((cx cx + cy cy) + cz cz); area[f] = 0.5 |c| (fp64; Open3D's GetTriangleArea); normal (n_faces, 3) fp32,
 * when not NULL: c / |c| rounded to fp32, (0, 0, 1) when |c| = 0. */
int lnr_mesh_face_areas(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, double* area,
                        float* normal, uint32_t* status, void* stream);
/* The points with global indices i in [first, first + count), to points[i - first] (count, 3) fp32 and, when not NULL,
 * their faces to face_of[i - first] (int32).  bounds (n_faces int64, non-decreasing): face t owns the points
 * [bounds[t - 1], bounds[t]), so point i lies on the first face with bounds[t] > i and a face of zero area
 * (bounds[t] = bounds[t - 1]) gets none.  Open3D's allocation is bounds[t] = floor(cum[t] / cum[n_faces - 1] N + 0.5),
 * cum the inclusive fp64 scan of the areas: stratified over the area's cdf, not multinomial.  An i >= bounds[n_faces - 1]
 * ORs LNR_MESH_NO_FACE and a point whose face has a bad index LNR_MESH_BAD_INDEX; both get a zero point and face -1.
 * The draws are r1 = U(key, stream 7, i, 0) and r2 = U(key, stream 7, i, 1) of the counter generator (24 bits, [0, 1))
 * widened to fp64; s = sqrt(r1), a = 1 - s, b = s (1 - r2), c = s r2; p = (a v0 + b v1) + c v2 per component, rounded
 * to fp32 once.  A point depends on (key, i) alone: chunks [first, first + count) concatenate to the whole run.
 * 0 <= first, 0 <= count (0: nothing is done), first + count <= LNR_CLOUD_MAX_POINTS: i fits the generator's 32-bit
 * counter and the result fits the voxel filter. */
int lnr_mesh_sample_points(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                           const int64_t* bounds, int64_t first, int64_t count, uint32_t key, float* points,
                           int32_t* face_of, uint32_t* status, void* stream);
/* normals (n_verts, 3) fp32: the sum of the cross products c (above: unnormalised, so area-weighted) of a vertex's
 * incident faces divided by its norm sqrt((x x + y y) + z z), rounded to fp32; (0, 0, 1) for a zero sum.  The caller
 * inverts the faces: corner_perm (3 n_faces int64) is the STABLE argsort of faces.reshape(-1), row_start (n_verts + 1
 * int64) the exclusive scan of the vertices' corner counts.  One thread per vertex adds the c of face
 * corner_perm[j] / 3 for j in [row_start[v], row_start[v + 1]), in that order: the order of every sum depends on the
 * data alone.  Entries of corner_perm outside [0, 3 n_faces), rows outside it and faces with a bad index (which OR
 * LNR_MESH_BAD_INDEX) are skipped, never followed.  A vertex runs as long as its row: marching-cubes meshes have
 * valence 4 to about 12 and no list is split, so one vertex shared by a large part of the faces serialises them. */
int lnr_mesh_vertex_normals(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                            const int64_t* corner_perm, const int64_t* row_start, float* normals, uint32_t* status,
                            void* stream);

/* ---------------------------------------------------------------- utilities */
/* dst[i] = lo + (hi-lo) * U(splitmix64(((uint64)seed << 32) + start + i)) */
int lnr_fill_uniform(float* dst, int64_t n, uint32_t seed, float lo, float hi, int64_t start, void* stream);
int lnr_f32_to_f16(const float* src, uint16_t* dst, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LONER_AMD_H */
