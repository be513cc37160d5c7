/*
 * ngp_hip.h — C ABI of libngp_hip.so, the MI355X (gfx950) instant-NGP hot path.
 *
 * This is the drop-in boundary for the reference's native extension surface:
 *   - `vren` (pybind11 module, /root/reference/models/csrc/binding.cpp:323-342,
 *     prototypes in models/csrc/include/utils.h:10-170), and
 *   - the tiny-cuda-nn objects the reference's field uses
 *     (models/networks.py:40-163: Grid/Hash encoding, SphericalHarmonics,
 *     CutlassMLP), plus the optimizer step the trainer runs (train.py:244).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous row-major data unless a
 *     parameter is explicitly documented as host memory;
 *   - the caller owns every buffer (allocated on the stream it passes in);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - return 0 on success, a negative NGP_E* code on failure; never throws,
 *     never allocates, never synchronises the device, no hidden global state
 *     (safe to capture into a hipGraph);
 *   - all floating point is fp32, indices are int32/int64 as the reference's;
 *   - empty batches (n == 0) are valid and return NGP_OK before any pointer is looked at;
 *   - the library reads no environment variable.
 *
 * Each entry point cites the reference interface it replaces.
 */
#ifndef NGP_HIP_H
#define NGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGP_OK 0
#define NGP_EINVAL (-22)   /* bad argument (null pointer, unsupported size) */
#define NGP_ELAUNCH (-5)   /* hipLaunch reported an error */

#define NGP_MAX_LEVELS 32

/* Activation codes shared by the MLP entry points. */
enum ngp_activation {
    NGP_ACT_NONE = 0,
    NGP_ACT_RELU = 1,
    NGP_ACT_SIGMOID = 2,
    NGP_ACT_SOFTPLUS = 3, /* torch.nn.Softplus(beta=1, threshold=20), models/networks.py:56,59 */
    NGP_ACT_EXP = 4
};

/* library / build identification: returns a static string "ngp_hip <ver> gfx950". */
const char* ngp_version(void);

/* hex digest of the sources (csrc + this header + compiler flags) the library was built from; the Python
 * binding refuses a library whose digest differs from the header it derives its prototypes from. */
const char* ngp_build_id(void);

/* ------------------------------------------------------------------------
 * R1  ray / AABB and ray / sphere intersection
 * replaces vren.ray_aabb_intersect  (binding.cpp:4-16,  intersection.cu:25-100)
 *          vren.ray_sphere_intersect (binding.cpp:19-31, intersection.cu:124-197)
 * outputs: hit_cnt (n_rays) i32 = number of voxels hit (not capped),
 *          hits_t (n_rays,max_hits,2) f32, hits_idx (n_rays,max_hits) i64,
 *          both sorted ascending by t1 with unused slots (-1) first, exactly as
 *          the reference's torch::sort + gather leaves them.
 * ---------------------------------------------------------------------- */
int ngp_ray_aabb_intersect(const float* rays_o, const float* rays_d,
                           const float* centers, const float* half_sizes,
                           int n_rays, int n_voxels, int max_hits,
                           int32_t* hit_cnt, float* hits_t, int64_t* hits_idx,
                           void* stream);

int ngp_ray_sphere_intersect(const float* rays_o, const float* rays_d,
                             const float* centers, const float* radii,
                             int n_rays, int n_spheres, int max_hits,
                             int32_t* hit_cnt, float* hits_t, int64_t* hits_idx,
                             void* stream);

/* render() pre-amble (models/rendering.py:30): t1 in [0,near) -> near, in place on
 * hits_t (n_rays, max_hits, 2) slot 0. */
int ngp_clamp_near(float* hits_t, int n_rays, int max_hits, float near_distance, void* stream);

/* ------------------------------------------------------------------------
 * O1  occupancy-grid helpers
 * replaces vren.morton3D / morton3D_invert / packbits
 *          (binding.cpp:74-101, raymarching.cu:35-161)
 * ---------------------------------------------------------------------- */
int ngp_morton3D(const int32_t* coords, int n, int32_t* indices, void* stream);
int ngp_morton3D_invert(const int32_t* indices, int n, int32_t* coords, void* stream);
/* threshold_dev (device scalar) overrides `threshold` when non-NULL: lets the caller keep
 * min(mean_density, density_threshold) (networks.py:405-407) on the device, with no .item() sync. */
int ngp_packbits(const float* density_grid, int n_bytes, float threshold, const float* threshold_dev,
                 uint8_t* density_bitfield, void* stream);

/* NGP.update_density_grid's point generation + EMA, fused (models/networks.py:388-403):
 * xyzs_w[i] = (coords[i]/(G-1)*2-1)*(s-s/G) + (noise[i]*2-1)*s/G  (noise in [0,1))   */
int ngp_grid_cell_points(const int32_t* coords, const float* noise, int n, int grid_size,
                         float s, float* xyzs_w, void* stream);
/* The sampled branch of NGP.update_density_grid, fused (networks.py:308-333 + 388-398): for ONE cascade, m uniformly
 * random cells + m cells drawn uniformly from the occupied ones (density_grid_c > density_threshold; none
 * occupied: the m uniform ones only), in Morton bucket order, with their jittered world points
 * x_w = (coord/(G-1)*2-1)*(s-s/G) + U(-1,1)*s/G.  Randomness is a counter-based hash of (seed, sample, draw): the
 * same on every rank, independent of launch order.  workspace: ngp_grid_sample_workspace(G, m) int32 elements
 * (host-only query).  outputs: indices (2m) i32 Morton cell indices, xyzs_w (2m,3) f32.
 * grid_size must be a power of two in 2..1024 (Morton keys of a G^3 grid span 3*ceil(log2 G) bits; only then is
 * every key a cell index < G^3): anything else is NGP_EINVAL from both entries, before any launch.
 * Order of the rows: by the top min(bits, 21) bits of the bits = 3*log2(G)-bit key, i.e. indices[i] >>
 * max(0, bits - 21) is non-decreasing (G <= 128: fully sorted); rows with equal sort keys come in any order.
 * The workspace is scratch: its contents need not be cleared or kept between calls, whatever they are. */
int64_t ngp_grid_sample_workspace(int grid_size, int m);
int ngp_grid_sample_cells(const float* density_grid_c, int grid_size, float density_threshold, int m,
                          int64_t seed, float s, int32_t* workspace, int32_t* indices, float* xyzs_w,
                          void* stream);
/* density_grid_tmp[c, indices] = sigmas (networks.py:398); several samples in one cell: the largest wins */
int ngp_density_grid_scatter_max(float* density_grid_tmp_c, const int32_t* indices, const float* sigmas, int n,
                                 void* stream);
/* EMA as ngp_density_grid_ema, plus threshold_out[0] = min(mean of the positive cells, density_threshold) and
 * threshold_out[1] = that mean (networks.py:405-407), kept on the device for ngp_packbits; partials: 1024 floats */
int ngp_density_grid_ema_threshold(float* density_grid, const float* density_grid_tmp, int n, float decay,
                                   float density_threshold, float* partials, float* threshold_out, void* stream);
/* grid = grid<0 ? grid : max(grid*decay, tmp)  (networks.py:400-403), n = K*G^3 */
int ngp_density_grid_ema(float* density_grid, const float* density_grid_tmp, int n,
                         float decay, void* stream);

/* ------------------------------------------------------------------------
 * R3  training ray marcher
 * replaces vren.raymarching_train (binding.cpp:104-131, raymarching.cu:166-332)
 *
 * Three launches: DDA count pass (one lane per ray, sample t's parked in
 * `t_scratch`), single-workgroup exclusive scan (writes rays_a and counter),
 * wave-per-ray expansion (coalesced xyzs/dirs/deltas/ts writes).
 * rays_a rows are in ray order with start indices monotone (a legal instance of
 * the reference's atomic order, raymarching.cu:237-241).
 *
 * t_scratch: (n_rays*max_samples) f32 workspace; ray_counts: (n_rays) i32 workspace.
 * xyzs/dirs: capacity `sample_capacity` rows (the reference allocates
 * n_rays*max_samples); rows >= counter[0] are left untouched unless zero_tail!=0,
 * in which case they are zero-filled like the reference's torch::zeros.
 * counter: (2) i32 -> {total samples, n_rays}.
 * grid_size must be a power of two in 1..1024 (the bitfield is indexed by the Morton code of the cell), else
 * NGP_EINVAL; the same holds for ngp_raymarching_test.
 * ---------------------------------------------------------------------- */
int ngp_raymarching_train(const float* rays_o, const float* rays_d, const float* hits_t /* (n_rays,2) */,
                          const uint8_t* density_bitfield, int cascades, float scale,
                          float exp_step_factor, const float* noise, int grid_size,
                          int max_samples, int n_rays,
                          float* t_scratch, int32_t* ray_counts,
                          int64_t* rays_a, float* xyzs, float* dirs, float* deltas, float* ts,
                          int32_t* counter, int64_t sample_capacity, int zero_tail,
                          void* stream);

/* ------------------------------------------------------------------------
 * T1  test-time marcher / compositor
 * replaces vren.raymarching_test (binding.cpp:134-163, raymarching.cu:335-454)
 *          vren.composite_test_fw (binding.cpp:262-320, volumerendering.cu:314-423)
 * hits_t (n_rays_total,2) is updated in place; outputs are (n_alive,N_samples,.)
 * and must be zero-initialised by the caller (reference: torch::zeros).
 * ---------------------------------------------------------------------- */
int ngp_raymarching_test(const float* rays_o, const float* rays_d, float* hits_t,
                         const int64_t* alive_indices, const uint8_t* density_bitfield,
                         int cascades, float scale, float exp_step_factor, int grid_size,
                         int max_samples, int n_samples, int n_alive,
                         float* xyzs, float* dirs, float* deltas, float* ts,
                         int32_t* n_eff_samples, void* stream);

int ngp_composite_test_fw(const float* sigmas, const float* rgbs, const float* normals,
                          const float* normals_raw, const float* sems, const float* deltas,
                          const float* ts, const float* hits_t, int64_t* alive_indices,
                          float T_threshold, int classes, const int32_t* n_eff_samples,
                          int n_alive, int n_samples,
                          float* opacity, float* depth, float* rgb, float* normal,
                          float* normal_raw, float* sem, void* stream);

/* ------------------------------------------------------------------------
 * V1/V2  training compositor
 * replaces vren.composite_alpha_fw (binding.cpp:166-180, volumerendering.cu:5-63)
 *          vren.composite_train_fw (binding.cpp:183-208, volumerendering.cu:65-164)
 *          vren.composite_train_bw (binding.cpp:211-259, volumerendering.cu:167-311)
 * One 32-lane half-wave per rays_a row, segmented transmittance scan, early stop
 * at T <= T_threshold.  Every per-sample output row of the ray is written (zeros
 * past the stop), so callers need not pre-zero per-sample outputs; per-ray
 * outputs are written for every rays_a row.  In ngp_composite_train_bw the outputs
 * dL_dnormals_pred / dL_dsems may be NULL (together with their upstream gradients)
 * when the loss does not use the composited normal / semantic maps, and any of
 * the upstream gradients dL_dopacity / dL_ddepth / dL_drgb / dL_dws may be NULL,
 * which reads as all zeros.
 * ---------------------------------------------------------------------- */
int ngp_composite_alpha_fw(const float* sigmas, const float* deltas, const int64_t* rays_a,
                           float T_threshold, int n_rays, float* alphas, float* ws, void* stream);

int ngp_composite_train_fw(const float* sigmas, const float* rgbs, const float* normals_pred,
                           const float* sems, const float* deltas, const float* ts,
                           const int64_t* rays_a, float T_threshold, int classes, int n_rays,
                           int64_t* total_samples, float* opacity, float* depth, float* rgb,
                           float* normal_pred, float* sem, float* ws, void* stream);

int ngp_composite_train_bw(const float* dL_dopacity, const float* dL_ddepth, const float* dL_drgb,
                           const float* dL_dnormal_pred, const float* dL_dsem, const float* dL_dws,
                           const float* sigmas, const float* rgbs, const float* normals_pred,
                           const float* ws, const float* deltas, const float* ts,
                           const int64_t* rays_a, const float* opacity, const float* depth,
                           const float* rgb, const float* normal_pred,
                           float T_threshold, int classes, int n_rays,
                           float* dL_dsigmas, float* dL_drgbs, float* dL_dnormals_pred,
                           float* dL_dsems, void* stream);

/* ------------------------------------------------------------------------
 * V3  Ref-NeRF normal regularisers
 * replaces vren.composite_refloss_fw/bw (binding.cpp, ref_loss.cu:4-175)
 * ---------------------------------------------------------------------- */
int ngp_composite_refloss_fw(const float* sigmas, const float* normals_diff, const float* normals_ori,
                             const float* deltas, const float* ts, const int64_t* rays_a,
                             float T_threshold, int n_rays, float* loss_o, float* loss_p,
                             void* stream);

int ngp_composite_refloss_bw(const float* dL_dloss_o, const float* dL_dloss_p,
                             const float* sigmas, const float* normals_diff, const float* normals_ori,
                             const float* deltas, const float* ts, const int64_t* rays_a,
                             const float* loss_o, const float* loss_p, float T_threshold, int n_rays,
                             float* dL_dsigmas, float* dL_dnormals_diff, float* dL_dnormals_ori,
                             void* stream);

/* ------------------------------------------------------------------------
 * D1  distortion loss
 * replaces vren.distortion_loss_fw/bw (binding.cpp, losses.cu:8-173)
 * ---------------------------------------------------------------------- */
int ngp_distortion_loss_fw(const float* ws, const float* deltas, const float* ts,
                           const int64_t* rays_a, int n_rays,
                           float* loss, float* ws_inclusive_scan, float* wts_inclusive_scan,
                           void* stream);

int ngp_distortion_loss_bw(const float* dL_dloss, const float* ws_inclusive_scan,
                           const float* wts_inclusive_scan, const float* ws, const float* deltas,
                           const float* ts, const int64_t* rays_a, int n_rays,
                           float* dL_dws, void* stream);

/* ------------------------------------------------------------------------
 * L1  loss glue, fused (each replaces a chain of torch elementwise ops in the reference)
 * ngp_nerf_loss      : NeRFLoss default terms reduced as train.py:307 does (sum of term means),
 *                      losses.py:96-105: terms[1] += mean (rgb-gt)^2, terms[2] += lambda_o mean(-o log o)
 *                      (o = opacity+1e-10), terms[3] += lambda_d mean(distortion) (per-ray distortion
 *                      loss of ngp_distortion_loss_fw, may be NULL), terms[0] += their sum; and the
 *                      gradients d_rgb = 2(rgb-gt)/(3n), d_opacity = lambda_o(-log o - 1)/n.
 * ngp_refloss_inputs : normals_diff = (n_raw-n_pred)^2, normals_ori = max(<n_raw, normalize(dir)>,0)^2
 *                      (rendering.py:243-245).
 * ngp_neg_normalize  : y = -F.normalize(x*scale3, eps=1e-6) on rows of 3 (networks.py:210,215), and
 *                      its backward.
 * ---------------------------------------------------------------------- */
int ngp_nerf_loss(const float* rgb, const float* target_rgb, const float* opacity,
                  const float* distortion, int n_rays, float lambda_opacity, float lambda_distortion,
                  float* terms /* (4), caller zeroes */, float* d_rgb, float* d_opacity, void* stream);
/* Default training recipe, everything between the field's raw outputs and the field's backward in ONE launch
 * (replaces, with the same arithmetic per ray: -F.normalize of d sigma/dx (scaled by scale3, device (3) or NULL) and of
 * the normal head, networks.py:198,215; softmax of the class logits, networks.py:219; composite_train_fw,
 * volumerendering.cu:65-164; the RefLoss inputs and forward, rendering.py:243-249 + ref_loss.cu; distortion_loss_fw/bw,
 * losses.cu; NeRFLoss's rgb / opacity / distortion terms reduced as sum(term.mean()), losses.py:96-105, train.py:307;
 * composite_train_bw, volumerendering.cu:167-311).  Outputs: the per-ray results of render() (total_samples int64,
 * opacity, depth, rgb, normal_pred, semantic, Ro = loss_o, Rp = loss_p (n_rays,3)), ws (N), vr_samples (1) int64 =
 * sum of total_samples, terms (4) = [loss, rgb, opacity, distortion], and the loss's gradients w.r.t. the field's
 * outputs dL_dsigmas (N), dL_drgbs (N,3).  terms and vr_samples are cleared here.  rays_a must cover every sample row;
 * classes <= 8; normal_head / sem_logits rows may be strided (ld_*). */
int ngp_render_loss_fused(const float* sigmas, const float* rgbs, const float* dsigma_dx, const float* scale3,
                          const float* normal_head, int64_t ld_normal, const float* sem_logits, int64_t ld_sem,
                          const float* dirs, const float* deltas, const float* ts, const int64_t* rays_a,
                          const float* target_rgb, const float* rgb_bg /* device (3) or NULL: rgb += bg (1 - opacity),
                          rendering.py:236-241 */, float T_threshold, int classes, int n_rays, float lambda_opacity,
                          float lambda_distortion, int64_t* total_samples, int64_t* vr_samples, float* opacity,
                          float* depth, float* rgb, float* normal_pred, float* sem, float* ws, float* loss_o,
                          float* loss_p, float* terms, float* dL_dsigmas, float* dL_drgbs, void* stream);
/* The same launch over a per-ray background (use_skybox, rendering.py:236-241 with rgb_bg = forward_skybox(rays_d)):
 * rgb_bg is (n_rays_total, 3), indexed by the ray index of the row like target_rgb, and must not be NULL.  One more output,
 * dL_drgb_bg (same shape): g_rgb (1 - opacity) with the ray's seed g_rgb = 2 (rgb - gt) / (3 R), written for every row of
 * rays_a, a ray without samples included (opacity 0, rgb = bg, dL_drgb_bg = g_rgb); rows of rays that rays_a does not
 * name are not touched.  Every other output is ngp_render_loss_fused's arithmetic: with every row of rgb_bg equal to one
 * colour the per-ray and per-sample outputs are that entry's bit for bit.  terms (4), classes <= 8. */
int ngp_render_loss_fused_sky(const float* sigmas, const float* rgbs, const float* dsigma_dx, const float* scale3,
                              const float* normal_head, int64_t ld_normal, const float* sem_logits, int64_t ld_sem,
                              const float* dirs, const float* deltas, const float* ts, const int64_t* rays_a,
                              const float* target_rgb, const float* rgb_bg, float T_threshold, int classes, int n_rays,
                              float lambda_opacity, float lambda_distortion, int64_t* total_samples, int64_t* vr_samples,
                              float* opacity, float* depth, float* rgb, float* normal_pred, float* sem, float* ws,
                              float* loss_o, float* loss_p, float* terms, float* dL_dsigmas, float* dL_drgbs,
                              float* dL_drgb_bg, void* stream);
/* The same launch for NeRFLoss(embed_msk=True) (losses.py:85-93, 142-151): mask (n_rays) is the transient mask m of
 * every ray.  Colour term mean((1 - m) e^2), its seed 2 (1 - m) e / (3 R) (the background's share of d_opacity uses it),
 * terms (5) = [loss, rgb, opacity, distortion, r_ms] with r_ms = size_delta mean(m^2) (the digit term has weight 0 in the
 * reference and is not formed), dL_dmask[r] = 2 size_delta m / R - sum_c e_rc^2 / (3 R).  Every rendered output,
 * `rgb` included, is that of ngp_render_loss_fused; with m = 0 and size_delta = 0 so is every other output, bit for bit.
 * vr_samples may sit at terms + 6 floats (one fill). */
int ngp_render_loss_fused_masked(const float* sigmas, const float* rgbs, const float* dsigma_dx, const float* scale3,
                                 const float* normal_head, int64_t ld_normal, const float* sem_logits, int64_t ld_sem,
                                 const float* dirs, const float* deltas, const float* ts, const int64_t* rays_a,
                                 const float* target_rgb, const float* rgb_bg, const float* mask, float size_delta,
                                 float T_threshold, int classes, int n_rays, float lambda_opacity, float lambda_distortion,
                                 int64_t* total_samples, int64_t* vr_samples, float* opacity, float* depth, float* rgb,
                                 float* normal_pred, float* sem, float* ws, float* loss_o, float* loss_p, float* terms,
                                 float* dL_dsigmas, float* dL_drgbs, float* dL_dmask, void* stream);
/* The same launch for NeRFLoss(semantic=True) (losses.py:120-123): labels (n_rays) int64, indexed by ray like target_rgb.
 * A label y is valid iff 0 <= y < classes; every other value (the reference's ignore_index 256, an 8-bit 255, negative
 * values, y >= classes) is ignored and never used as an index.  n_valid = number of valid labels among the n_rays rows.
 * terms (6) = [loss, rgb, opacity, distortion, CELoss, sky_depth]:
 *   CELoss    = lambda_sem sum_valid (logsumexp_c(S) - S_y) / n_valid, S = sem, the composited class probabilities
 *               (nn.CrossEntropyLoss(ignore_index=256) on them); 0, with zero gradients, when n_valid == 0 (torch: NaN);
 *   sky_depth = lambda_sky / n_rays sum_r [y_r == 4] exp(-depth_r), the literal 4 whatever `classes` is.
 * dL_dsem_logits (N, classes), dense: the CE term through S and the per-sample softmax with the weights held constant
 * (composite_train_bw drops dL_dsem from dL_dsigmas, volumerendering.cu:234-241, so the CE term does not enter
 * dL_dsigmas); zero behind a ray's stop.  The sky term enters dL_dsigmas through the depth.  sem_ws: device int32
 * (NGP_SEM_WS_INTS = 8, 8-byte aligned) workspace, filled by a count kernel launched here ahead of the tail on the same
 * stream (two launches, no host read, no allocation: capturable): [0] is n_valid afterwards, the rest holds the two
 * terms' sums in double (one rounding each instead of a float atomic per workgroup).  1 <= classes <= 16.  vr_samples may sit at terms + 6 floats (one fill).  With
 * lambda_sem = lambda_sky = 0 every output shared with ngp_render_loss_fused is that entry's. */
#define NGP_SEM_WS_INTS 8
int ngp_render_loss_fused_sem(const float* sigmas, const float* rgbs, const float* dsigma_dx, const float* scale3,
                              const float* normal_head, int64_t ld_normal, const float* sem_logits, int64_t ld_sem,
                              const float* dirs, const float* deltas, const float* ts, const int64_t* rays_a,
                              const float* target_rgb, const float* rgb_bg, const int64_t* labels, float lambda_sem,
                              float lambda_sky, float T_threshold, int classes, int n_rays, float lambda_opacity,
                              float lambda_distortion, int64_t* total_samples, int64_t* vr_samples, float* opacity,
                              float* depth, float* rgb, float* normal_pred, float* sem, float* ws, float* loss_o,
                              float* loss_p, float* terms, float* dL_dsigmas, float* dL_drgbs, int* sem_ws,
                              float* dL_dsem_logits, void* stream);
/* The same launch for NeRFLoss's normal_mono term (losses.py:111-118): normals_gt (n_rays, 3), indexed by ray like
 * target_rgb.  With N = normal_pred, N^ = N / max(|N|, 1e-12), g^ = g / max(|g|, 1e-12) (F.normalize's defaults):
 * terms (5) = [loss, rgb, opacity, distortion, normal_mono],
 *   normal_mono = lambda_nm / (3 n_rays) sum_r sum_c (|N^_c - g^_c| - 0.1 N^_c g^_c).
 * A target whose three components are exactly 0 marks a pixel without a normal: the ray adds nothing to the term and
 * its samples get a zero gradient; the divisor stays 3 n_rays.  With every target non-zero this is the module's term.
 * dL_dnormal_head (N, 3), dense: the term through N^, the composited sum and the per-sample -normalize(head, eps 1e-6)
 * with the weights held constant (composite_train_bw drops dL_dnormal_pred from dL_dsigmas, volumerendering.cu:234-241,
 * so dL_dsigmas and dL_drgbs are those of ngp_render_loss_fused); exactly zero behind a ray's stop and for a sample
 * without weight.  nrm_ws: device int32 (NGP_NRM_WS_INTS = 4, 8-byte aligned) workspace: the term's sum in double and the
 * count of finished workgroups (one rounding instead of a float atomic per workgroup).  vr_samples may sit at terms + 6
 * floats and nrm_ws at terms + 8 floats (one fill, one launch).  classes <= 8.  With lambda_nm = 0 every output shared
 * with ngp_render_loss_fused is that entry's. */
#define NGP_NRM_WS_INTS 4
int ngp_render_loss_fused_nrm(const float* sigmas, const float* rgbs, const float* dsigma_dx, const float* scale3,
                              const float* normal_head, int64_t ld_normal, const float* sem_logits, int64_t ld_sem,
                              const float* dirs, const float* deltas, const float* ts, const int64_t* rays_a,
                              const float* target_rgb, const float* rgb_bg, const float* normals_gt, float lambda_nm,
                              float T_threshold, int classes, int n_rays, float lambda_opacity, float lambda_distortion,
                              int64_t* total_samples, int64_t* vr_samples, float* opacity, float* depth, float* rgb,
                              float* normal_pred, float* sem, float* ws, float* loss_o, float* loss_p, float* terms,
                              float* dL_dsigmas, float* dL_drgbs, int* nrm_ws, float* dL_dnormal_head, void* stream);
/* The same launch for NeRFLoss's depth_mono term (losses.py:7-30, 125-131): depth_gt (n_rays), the raw monocular depth,
 * indexed by ray like target_rgb.  With z = depth_gt / 25 and D = depth, a ray is valid iff z > 0 (zero, negative and NaN
 * targets add nothing to the fit, the term or any gradient); (a, b) is the least-squares scale and shift of a D + b ~ z over
 * the batch's valid rays, D a constant of the fit, by Cramer's rule on the sums of D^2, D, 1, D z, z taken in double; a
 * singular system (det == 0 in double: no valid ray, one valid ray) gives a = b = 0.
 * terms (5) = [loss, rgb, opacity, distortion, depth_mono],
 *   depth_mono = lambda_dm / n_rays sum_valid exp(-D / scene_scale) (a D + b - z)^2       (the falloff is a constant too).
 * dL_dsigmas gains delta_s g_D (t_s T_s - (D - d_s)) with g_D = lambda_dm / n_rays [valid] exp(-D / scene_scale) 2 a
 * (a D + b - z) and d_s the inclusive prefix of w t; dL_drgbs is that of ngp_render_loss_fused.  A fit kernel runs ahead of
 * the tail on the same stream (no host read, no allocation: both launches can be captured).
 * dep_ws: device int32 (NGP_DEP_WS_INTS = 18, 8-byte aligned) workspace, cleared by the entry:
 *   [0:10] five doubles, the valid rays' sums of D^2, D, 1, D z, z; [10:12] one double, the sum of the rays' terms;
 *   [12] a, [13] b (float32) and [14] n_valid (int32), left there by the fit; [15], [16] finished workgroups of the fit and
 *   of the tail (one counter each); [17] unused.
 * vr_samples may sit at terms + 6 floats and dep_ws at terms + 8 floats (one fill).  classes <= 8, scene_scale > 0.
 * With lambda_dm = 0 every output shared with ngp_render_loss_fused is that entry's. */
#define NGP_DEP_WS_INTS 18
int ngp_render_loss_fused_dep(const float* sigmas, const float* rgbs, const float* dsigma_dx, const float* scale3,
                              const float* normal_head, int64_t ld_normal, const float* sem_logits, int64_t ld_sem,
                              const float* dirs, const float* deltas, const float* ts, const int64_t* rays_a,
                              const float* target_rgb, const float* rgb_bg, const float* depth_gt, float lambda_dm,
                              float scene_scale, float T_threshold, int classes, int n_rays, float lambda_opacity,
                              float lambda_distortion, int64_t* total_samples, int64_t* vr_samples, float* opacity,
                              float* depth, float* rgb, float* normal_pred, float* sem, float* ws, float* loss_o,
                              float* loss_p, float* terms, float* dL_dsigmas, float* dL_drgbs, int* dep_ws, void* stream);
/* The same launch with two or three of those optional terms at once (the reference's street-scene recipes set
 * render_semantic and normal_mono together and add depth_mono on top).  term_mask names them: NGP_TERM_SEM (labels,
 * lambda_sem, lambda_sky, dL_dsem_logits), NGP_TERM_NRM (normals_gt, lambda_nm, dL_dnormal_head), NGP_TERM_DEP (depth_gt,
 * lambda_dm, scene_scale); the arguments of a term that is not named are not looked at.  Each term's definition, validity
 * rule and deviation from torch is that of its single entry above and nothing else: ngp_render_loss_fused_sem (valid labels,
 * n_valid == 0, the literal sky class 4), ngp_render_loss_fused_nrm (a zero target row), ngp_render_loss_fused_dep (z > 0,
 * the fit, a singular system).
 * terms (8) = [loss, rgb, opacity, distortion, CELoss, sky_depth, normal_mono, depth_mono]; a term that is not named is
 * exactly 0.  dL_dsigmas carries the sky term's and the depth_mono term's depth seeds added into one.
 * multi_ws: device int32 (NGP_MULTI_WS_INTS = 30, 8-byte aligned) workspace, the three single workspaces back to back:
 *   [0:8] sem_ws ([NGP_MULTI_WS_LABELS_NVALID] = n_valid of the labels), [8:12] nrm_ws, [12:30] dep_ws
 *   ([NGP_MULTI_WS_FIT_A], [NGP_MULTI_WS_FIT_B] a, b as float32 and [NGP_MULTI_WS_FIT_NVALID] n_valid of the fit).
 * With one term named this launches that term's own kernel; with more, every term is still summed in double and rounded
 * once, behind one count of finished workgroups ([6] with NGP_TERM_SEM, else [10]).  The entry clears terms, vr_samples and
 * the workspace (vr_samples may sit at terms + 8 floats and multi_ws at terms + 10 floats: one fill), then launches the
 * label count (NGP_TERM_SEM), the depth fit (NGP_TERM_DEP) and the tail on the caller's stream: no host read, no allocation,
 * capturable.  1 <= classes <= 16 with NGP_TERM_SEM, classes <= 8 without; scene_scale > 0 with NGP_TERM_DEP.  Unknown bits
 * in term_mask are NGP_EINVAL, and so is a zero mask with rays to process (an empty batch is NGP_OK with it).  With every
 * optional lambda 0 every output shared with ngp_render_loss_fused is that entry's. */
#define NGP_TERM_SEM 1
#define NGP_TERM_NRM 2
#define NGP_TERM_DEP 4
#define NGP_MULTI_WS_INTS 30
#define NGP_MULTI_WS_LABELS_NVALID 0
#define NGP_MULTI_WS_FIT_A 24
#define NGP_MULTI_WS_FIT_B 25
#define NGP_MULTI_WS_FIT_NVALID 26
int ngp_render_loss_fused_multi(const float* sigmas, const float* rgbs, const float* dsigma_dx, const float* scale3,
                                const float* normal_head, int64_t ld_normal, const float* sem_logits, int64_t ld_sem,
                                const float* dirs, const float* deltas, const float* ts, const int64_t* rays_a,
                                const float* target_rgb, const float* rgb_bg, int term_mask, const int64_t* labels,
                                float lambda_sem, float lambda_sky, const float* normals_gt, float lambda_nm,
                                const float* depth_gt, float lambda_dm, float scene_scale, float T_threshold, int classes,
                                int n_rays, float lambda_opacity, float lambda_distortion, int64_t* total_samples,
                                int64_t* vr_samples, float* opacity, float* depth, float* rgb, float* normal_pred,
                                float* sem, float* ws, float* loss_o, float* loss_p, float* terms, float* dL_dsigmas,
                                float* dL_drgbs, int* multi_ws, float* dL_dsem_logits, float* dL_dnormal_head, void* stream);
int ngp_refloss_inputs(const float* normals_raw, const float* normals_pred, const float* dirs, int64_t n,
                       float* normals_diff, float* normals_ori, void* stream);
int ngp_neg_normalize(const float* x, int64_t ldx, const float* scale3 /* device (3) or NULL */, int64_t n,
                      float* y, void* stream);
int ngp_neg_normalize_bwd(const float* x, int64_t ldx, const float* dL_dy, int64_t n, float* dL_dx,
                          void* stream);
/* NeRFLoss(normal_ref=True)'s two terms behind ANY ngp_render_loss_fused* entry, which has left ws (0 behind a ray's
 * early stop), loss_o (Ro) and loss_p (Rp).  RefLoss composites with detached sigmas, so ws is a constant here and
 *     L = lambda_rp mean(Rp) + lambda_ro mean(Ro),   the means over 3 R and R values, R = n_rays (the rows of rays_a),
 * has per-sample gradients.  With n_raw = -normalize(dsigma_dx * scale3), n_pred = -normalize(normal_head) (eps 1e-6),
 * d = normalize(dirs), e = n_raw - n_pred, dot = max(<n_raw, d>, 0), G_p = lambda_rp ws / (3 R), G_o = lambda_ro ws / R:
 *     dL/dn_raw = 2 e G_p + 2 dot d G_o,   dL/dn_pred = -2 e G_p,
 * each taken through the backward of -normalize exactly as ngp_neg_normalize_bwd does it (a row of norm <= eps: -g 1e6);
 * scale3 (device (3) or NULL) is applied on the dsigma_dx side, so dL_dgrads (N,3) is w.r.t. dsigma_dx itself.
 * dL_dnormal_head (N,3) is written, or added to when add_to_normal_head != 0 (the tail's normal_mono gradient is there).
 * ref_terms (2) = [lambda_rp mean(Rp), lambda_ro mean(Ro)], the per-ray values summed in a fixed order (doubles).
 * 32 lanes per rays_a row; samples and rays that rays_a does not name are not touched.  Runs on the tail's stream,
 * behind the tail.  n_rays == 0 returns NGP_OK before any pointer is looked at; n_rays < 0, ld_normal_head < 3 or a NULL
 * pointer other than scale3 is NGP_EINVAL. */
int ngp_normal_ref_tail(const float* dsigma_dx, const float* scale3, const float* normal_head, int64_t ld_normal_head,
                        const float* dirs, const float* ws, const int64_t* rays_a, int n_rays, const float* loss_o,
                        const float* loss_p, float lambda_rp, float lambda_ro, int add_to_normal_head, float* dL_dgrads,
                        float* dL_dnormal_head, float* ref_terms, void* stream);

/* ------------------------------------------------------------------------
 * R4  torch_scatter.segment_csr(src, indptr) with sum reduction
 * (custom_functions.py:110-112).  src (n_rows, width), indptr (n_seg+1) i64.
 * ---------------------------------------------------------------------- */
int ngp_segment_csr_sum(const float* src, const int64_t* indptr, int n_seg, int width,
                        float* out, void* stream);

/* ------------------------------------------------------------------------
 * H1-H4  multiresolution hash grid (tcnn.Encoding otype Grid/HashGrid,
 * models/networks.py:40-52,67-76; semantics SURVEY.md Appendix B)
 * 3-D inputs in [0,1], linear interpolation, F in {1,2,4,8}.
 * ---------------------------------------------------------------------- */
typedef struct ngp_grid_desc {
    uint32_t n_levels;
    uint32_t n_features;            /* F */
    uint32_t offsets[NGP_MAX_LEVELS + 1]; /* in table rows (F floats each) */
    uint32_t resolution[NGP_MAX_LEVELS];
    float    scale[NGP_MAX_LEVELS];
} ngp_grid_desc;

/* Host-side helper: fills `desc` from the tcnn config keys; returns the number of
 * parameters (floats) of the table, or a negative error. */
int64_t ngp_grid_layout(int n_levels, int n_features, int log2_hashmap_size,
                        int base_resolution, double per_level_scale, ngp_grid_desc* desc);

/* y (n, L*F) = encode(x (n,3)); ldy / lddy = row stride in floats of y / dL_dy (>= L*F), so the
 * encoder can write into (and its backward read from) a column block of a wider matrix such as
 * rgb_net's [SH | grid features | appearance code] input (networks.py:229-231) with no concat. */
int ngp_grid_fwd(const ngp_grid_desc* desc /* host */, const float* table, const float* x,
                 int64_t n, float* y, int64_t ldy, void* stream);

/* dtable[(off+idx)*F+f] += w * dL_dy  (atomic fp32 scatter-add; caller zeroes dtable) */
int ngp_grid_bwd_param(const ngp_grid_desc* desc, const float* x, const float* dL_dy, int64_t lddy,
                       int64_t n, float* dtable, void* stream);
/* Same, with every sample's gradient row multiplied by row_scale[sample] (NULL = 1) as it is loaded:
 * dParam += w * row_scale[s] * dL_dy[s].  The density head has ONE output, so the gradient it sends into its
 * encoder is a per-sample multiple of d(sigma)/d(features) — which the forward pass already computed for the
 * analytic normals (networks.py:186-196): the backward needs no second data-gradient product. */
int ngp_grid_bwd_param_scaled(const ngp_grid_desc* desc, const float* x, const float* dL_dy, int64_t lddy,
                              const float* row_scale, int64_t n, float* dtable, void* stream);

/* dL_dx (n,3) = sum_l d enc_l / dx . dL_dy_l */
int ngp_grid_bwd_input(const ngp_grid_desc* desc, const float* table, const float* x,
                       const float* dL_dy, int64_t lddy, int64_t n, float* dL_dx, void* stream);

/* The training forward's density path in one launch, in place of the four launches
 *   ngp_grid_fwd -> ngp_mlp2_fwd_dact -> ngp_mlp_bwd_input -> ngp_grid_bwd_input
 * for the density head 128 -> 128 softplus -> 1 softplus:
 *   feat (n,128) = encode(x), a1 (n,128) = softplus(feat W1^T + b1), sig (n) = softplus(a1 . W2 + b2),
 *   dfeat (n,128) = d sig / d feat, grads (n,3) = d sig / dx.
 * feat, a1, sig and dfeat are bitwise what the four launches write; grads agree with theirs within 128 ulps of
 * the row's largest component (the same expression, contracted into FMAs differently by the compiler).
 * Takes F = 8 layouts of 16 levels that the tile kernels take (ngp_density_field_layout_ok, host-only: 1 or 0);
 * W1 (128,128) and W2 (1,128) row-major, b1 (128) / b2 (1) may be NULL; every output is contiguous, and W1, feat,
 * a1 and dfeat are 16-byte aligned.  Anything else returns NGP_EINVAL without a launch. */
int ngp_density_field_layout_ok(const ngp_grid_desc* desc);
int ngp_density_field_fwd(const ngp_grid_desc* desc, const float* table, const float* x, int64_t n,
                          const float* W1, const float* b1, const float* W2, const float* b2,
                          float* feat, float* a1, float* sig, float* dfeat, float* grads, void* stream);

/* double backward of ngp_grid_bwd_input: given dL_ddLdx (n,3) (gradient flowing into
 * dL_dx), accumulates dtable (atomic) and writes dL_ddLdy (n, L*F).  Either output
 * may be NULL. */
int ngp_grid_bwd_bwd_input(const ngp_grid_desc* desc, const float* table, const float* x,
                           const float* dL_dy, int64_t lddy, const float* dL_ddLdx, int64_t n,
                           float* dtable, float* dL_ddLdy, void* stream);

/* D2  second-order backward of the density head 128 -> 128 softplus -> 1 softplus: the element-wise pass of the route
 * loss(normals_raw) -> d(sigma)/dx -> density table and xyz_net (normal_ref), between products that other entries form.
 * With s1 = sigmoid(z1) = 1 - exp(-a1), s2 = sigmoid(z2) = 1 - exp(-sig), w2 = W2[0] and g = d_sig (NULL = 0), the
 * first order is  dfeat = m W1,  m = s2 (w2 * s1)  (what ngp_density_field_fwd leaves).  A gradient v on
 * grads = d(sigma)/dx becomes u = dL/d(dfeat) in ngp_grid_bwd_bwd_input, and r = u W1^T (n,128) in ngp_linear_fwd.
 * Per row this entry forms
 *     q = sum_h r_h w2_h s1_h,   e2 = q s2 (1 - s2) + g s2            (= dL/dz2, the first-order share included)
 *     m_h  = s2 w2_h s1_h                                              (dW1 += m^T u)
 *     e1_h = s1_h w2_h (e2 + r_h s2 (1 - s1_h))                        (= dL/dz1: dW1 += e1^T feat, db1 += sum e1,
 *                                                                        dL/dfeat = e1 W1)
 * writes m (n,128) and e1 (n,128) (e1 may be r itself) and ACCUMULATES (+=) dW2 (128) += sum_rows (e2 a1 + s2 r * s1),
 * db2 (1) += sum_rows e2.  1 - exp(-y) is evaluated as -expm1(-y) and 1 - s as exp(-y): both keep their digits at y = 1e-6
 * and at y = 30.  A persistent grid of at most NGP_DENSITY_BWD2_MAX_BLOCKS workgroups takes tiles of NGP_DENSITY_BWD2_ROWS
 * rows; a workgroup keeps its 129 sums in registers (doubles) across its tiles and stores them to `workspace`
 * (ngp_density_head_bwd2_workspace(n) floats, host-only query, 8-byte aligned; scratch: its contents need not be
 * cleared or kept, but two calls that may overlap need one each); a second launch adds them over the workgroups in a
 * fixed order: no atomics, the same bits on every run.
 * a1, r, m, e1 are contiguous and 16-byte aligned.  n == 0 returns NGP_OK before any pointer is looked at; n < 0, a NULL
 * pointer other than d_sig or a misaligned one is NGP_EINVAL, without a launch. */
#define NGP_DENSITY_BWD2_ROWS 8
#define NGP_DENSITY_BWD2_MAX_BLOCKS 1024
int64_t ngp_density_head_bwd2_workspace(int64_t n);
int ngp_density_head_bwd2(const float* a1, const float* sig, const float* r, const float* W2, const float* d_sig, int64_t n,
                          float* m, float* e1, float* dW2, float* db2, float* workspace, void* stream);

/* ------------------------------------------------------------------------
 * M1  transient mask field (models/implicit_mask.py): tcnn Grid/Hash encoding L = 8, F = 2 (desc must say so) of
 * uvi (n,3), then Linear(16,64) + ReLU + Linear(64,1) + Sigmoid with torch's nn.Linear layouts: W1 (64,16), b1 (64),
 * W2 (1,64), b2 (1).  One launch each way.
 * fwd: mask (n).  bwd: from dL_dmask (n) and the forward's mask (the table is gathered again, nothing else is saved)
 * it ACCUMULATES (+=, the caller zeroes) dtable (like ngp_grid_bwd_param: float atomics), dW1, db1, dW2, db2; the
 * weight sums are reduced inside a workgroup and added once per workgroup per element.
 * ---------------------------------------------------------------------- */
int ngp_mask_field_fwd(const ngp_grid_desc* desc, const float* table, const float* W1, const float* b1, const float* W2,
                       const float* b2, const float* uvi, int64_t n, float* mask, void* stream);
int ngp_mask_field_bwd(const ngp_grid_desc* desc, const float* table, const float* W1, const float* b1, const float* W2,
                       const float* uvi, const float* mask, const float* dL_dmask, int64_t n, float* dtable, float* dW1,
                       float* db1, float* dW2, float* db2, void* stream);

/* ------------------------------------------------------------------------
 * E1  per-image appearance codes (embed_a: train.py:104-108, 238-244, rendering.py:217-219): the broadcast of a ray's
 * row of the embedding table over the ray's samples, and the segmented sum of the gradient back.  One launch each
 * way, ray-parallel (one wave per row of rays_a).
 * weight (n_imgs, E) f32, 1 <= E <= 32; img_idxs (n_rays) i64: image of every ray; rays_a (n_rays, 3) i64: (ray
 * index, first sample, sample count) as the marcher emits them.
 * fwd: `out` points at the FIRST code column of a row-major matrix with row stride `ld` floats (column 144 of rgb_net's
 *   input): for every row r of rays_a and every sample s in [start, start + count)
 *     out[s][0:E] = weight[img_idxs[rays_a[r][0]]],  out[s][E:n_cols] = 1.0f  (tcnn's ones-padding), E <= n_cols <= 64.
 *   Sample rows that belong to no segment and the columns outside [0, n_cols) are not touched.
 * bwd: `dL_dcols` points at the first code column of the gradient matrix (row stride `ld`); d_weight (n_imgs, E) is
 *   ACCUMULATED into (+=, the caller zeroes): d_weight[i][c] += sum over the rays of image i, over their samples, of
 *   dL_dcols[s][c].  A ray's sum is formed inside its wave; consecutive rays of one image are merged before they go to
 *   memory as float atomics (sums depend on arrival order in the last bits).
 * A ray with count <= 0 contributes nothing.  A ray whose image index lies outside [0, n_imgs) (or whose ray index lies
 * outside [0, n_rays)) gets zeros in [0, E) forward and contributes nothing backward: such an index is never used as an
 * address.  n_rays == 0 returns NGP_OK before any pointer is looked at.
 * ---------------------------------------------------------------------- */
int ngp_embed_a_fwd(const float* weight, int64_t n_imgs, int E, const int64_t* img_idxs, const int64_t* rays_a,
                    int64_t n_rays, float* out, int64_t ld, int n_cols, void* stream);
int ngp_embed_a_bwd(const float* dL_dcols, int64_t ld, int E, const int64_t* img_idxs, const int64_t* rays_a,
                    int64_t n_rays, int64_t n_imgs, float* d_weight, void* stream);

/* ------------------------------------------------------------------------
 * T1  HDR-NeRF tone-mappers (use_exposure: models/networks_noCUDA.py:238-251, train.py:301-306): the three per-channel
 * tcnn networks 1 -> 64 (ReLU) -> 1 (Sigmoid) of NGP(rgb_act='None'), all channels in one launch each way.
 * params0..2: one channel's 2048 floats each in the tinycudann.Network layout, W1 (64,16) row-major, then W2 (16,64),
 * 16-byte aligned.  tcnn pads the one input to 16 columns with ones, so per channel c and sample s
 *     u = log_radiance[s][c] + ln(exposure),  z_j = W1[j][0] u + sum_{k=1..15} W1[j][k],  rgb[s][c] = sigmoid(sum_j W2[0][j] relu(z_j)).
 * log_radiance, rgb, dL_drgb, d_log_radiance (n,3).  exposure: NULL (unit exposure, ln = 0), or seconds with
 * exposure_stride 0 (one value for every sample) or 1 (one value per sample); the logarithm is taken here.
 * bwd: recomputes the hidden layer (nothing is saved but the inputs), writes d_log_radiance (NULL: not wanted) and
 *   ACCUMULATES (+=, the caller zeroes) the parameter gradients into dparams0..2 (the layout of params): rows 1..15 of W2
 *   are not touched, the 15 padding columns of a row of W1 all receive the same sum; the ReLU derivative is z_j > 0.
 *   There is no gradient for exposure.  A persistent grid keeps every workgroup's 576 sums in registers across its
 *   tiles and stores them as doubles to `workspace` (ngp_tonemap_bwd_workspace(n) floats, host-only query, at most
 *   2 * 576 * NGP_TONEMAP_BWD_MAX_BLOCKS, 8-byte aligned; scratch: its contents need not be cleared or kept, but two
 *   calls that may overlap need one each); a second launch adds them over the workgroups in a fixed order: no atomics,
 *   the same bits on every run.  Between its float32 inputs and outputs the backward works in double.
 * n == 0 returns NGP_OK before any pointer is looked at (nothing is launched, the sinks are left alone); n < 0 or a
 * stride other than 0 or 1 is NGP_EINVAL.
 * ---------------------------------------------------------------------- */
#define NGP_TONEMAP_BWD_MAX_BLOCKS 512
int ngp_tonemap_fwd(const float* params0, const float* params1, const float* params2, const float* log_radiance,
                    const float* exposure, int exposure_stride, int64_t n, float* rgb, void* stream);
int64_t ngp_tonemap_bwd_workspace(int64_t n);
int ngp_tonemap_bwd(const float* params0, const float* params1, const float* params2, const float* log_radiance,
                    const float* exposure, int exposure_stride, const float* dL_drgb, int64_t n, float* d_log_radiance,
                    float* dparams0, float* dparams1, float* dparams2, float* workspace, void* stream);

/* ------------------------------------------------------------------------
 * S1  skybox (use_skybox: models/networks.py:128-148, 284-291; train.py:160): the background colour of a ray from its
 * direction, SH degree 3 -> tcnn network 9 -> 32 (ReLU) -> 3 (Sigmoid), one launch each way.  Only the Sigmoid output
 * activation is supported.  params: the network's 1024 floats in the tinycudann.Network layout, W1 (32,16) row-major,
 * then W2 (16,32).  rays_d, rgb_bg, dL_drgb_bg (n_rays,3).  Per ray
 *     u = d / |d| (forward_skybox's normalisation, no epsilon),  x = (u + 1) / 2,
 *     y_0..8 = the degree-3 real SH basis of 2 x - 1 (ngp_sh_fwd's polynomial forms),
 *     z_j = sum_{k<9} W1[j][k] y_k + sum_{k=9..15} W1[j][k]   (tcnn pads the 9 inputs to 16 columns with ones),
 *     rgb_bg[c] = sigmoid(sum_j W2[c][j] relu(z_j)), c < 3     (rows 3..15 of W2 are unused).
 * bwd: recomputes the hidden layer (nothing is saved but the inputs) and ACCUMULATES (+=, the caller zeroes) the
 *   parameter gradients into dparams (the layout of params): columns 9..15 of a row of W1 all receive the same sum, rows
 *   3..15 of W2 are not touched; the ReLU derivative is z_j > 0.  There is no gradient for rays_d.  A persistent grid keeps
 *   every workgroup's 416 sums in registers across its tiles and stores them as doubles to `workspace`
 *   (ngp_skybox_bwd_workspace(n) floats, host-only query, at most 2 * 416 * NGP_SKYBOX_BWD_MAX_BLOCKS, 8-byte aligned;
 *   scratch: its contents need not be cleared or kept, but two calls that may overlap need one each); a second launch
 *   adds them over the workgroups in a fixed order: no atomics, the same bits on every run.  Between their float32
 *   inputs and outputs both directions work in double.
 * n_rays == 0 returns NGP_OK before any pointer is looked at (nothing is launched, dparams is left alone); n_rays < 0
 * is NGP_EINVAL.
 * ---------------------------------------------------------------------- */
#define NGP_SKYBOX_BWD_MAX_BLOCKS 256
int ngp_skybox_fwd(const float* params, const float* rays_d, int64_t n_rays, float* rgb_bg, void* stream);
int64_t ngp_skybox_bwd_workspace(int64_t n);
int ngp_skybox_bwd(const float* params, const float* rays_d, const float* dL_drgb_bg, int64_t n_rays, float* dparams,
                   float* workspace, void* stream);

/* ------------------------------------------------------------------------
 * P1  camera pose refinement (optimize_ext: train.py:143-149, 225-230; datasets/ray_utils.py:50-104): the rays of a
 * batch from per-image corrections, and the adjoint of that map reduced per image.  One launch each way.
 * poses (n_imgs, 3, 4) camera-to-world [Rp | t]; dR (n_imgs, 3) axis-angle, dT (n_imgs, 3); directions (n_pix, 3) camera
 * space; img_idxs, pix_idxs (n_rays) i64.
 * fwd (a lane per ray): with v = dR[img], theta = |v| + 1e-7, K = skew(v):
 *     Rd = (I + sin(theta)/theta K) + (1 - cos(theta))/theta^2 K^2,  R' = Rd Rp,
 *     rays_d[r][i] = (R'_i0 dir_0 + R'_i1 dir_1) + R'_i2 dir_2,  rays_o[r] = t + dT[img]
 *   in float32 without FMA contraction (1 - cos(theta) formed as 2 sin^2(theta / 2)).  At dR = dT = 0 the rays are bit for
 *   bit get_rays' fixed-order products.
 * bwd (a wave per chunk of consecutive rays_a rows): g_x (n, 3) and g_dir (n, 3) or NULL are the gradients of the loss
 *   w.r.t. the sample positions x_s = o + t_s d and the sample directions dir_s = d; ts (n); rays_a (n_rays, 3) i64 = (ray
 *   index, first sample, sample count).  Per row, g_o = sum_s g_x[s] and g_d = sum_s (g_x[s] ts[s] + g_dir[s])
 *   (RayMarcher.backward, custom_functions.py:104-114), then through R' = Rd(v) Rp to v.  g_dR, g_dT (n_imgs, 3) are
 *   ACCUMULATED into (+=, float atomics, consecutive rows of one image merged first; the caller zeroes); the term that
 *   goes through |v| is exactly 0 at v = 0, as torch's norm backward is.
 * An image, pixel, ray or sample index outside its range is never used as an address: forward such a ray is zero, backward
 * it (or the sample) contributes nothing.  Rows of images that no ray names are not touched.  n_rays == 0 (bwd: or
 * n == 0) returns NGP_OK before any pointer is looked at.
 * ---------------------------------------------------------------------- */
int ngp_pose_rays_fwd(const float* poses, const float* dR, const float* dT, const float* directions,
                      const int64_t* img_idxs, const int64_t* pix_idxs, int64_t n_imgs, int64_t n_pix, int64_t n_rays,
                      float* rays_o, float* rays_d, void* stream);
int ngp_pose_rays_bwd(const float* g_x, const float* g_dir, const float* ts, const int64_t* rays_a, const float* poses,
                      const float* dR, const float* directions, const int64_t* img_idxs, const int64_t* pix_idxs,
                      int64_t n_imgs, int64_t n_pix, int64_t n_rays, int64_t n, float* g_dR, float* g_dT, void* stream);

/* adjoint of ngp_sh_fwd_dirs at degree 4: dL_dd (n, 3) from dL_dy (n rows of 16, row stride lddy >= 16 floats) through
 * the basis, the [0,1] remap and F.normalize(eps = 1e-6) (under the clamp: g / eps) */
int ngp_sh_bwd_dirs(const float* d, const float* dL_dy, int64_t lddy, int64_t n, float* dL_dd, void* stream);

/* ------------------------------------------------------------------------
 * H5  spherical harmonics (tcnn.Encoding otype SphericalHarmonics, degree 1..4,
 * networks.py:78-85,128-135).  x (n,3) in [0,1] -> y (n, degree^2).
 * ---------------------------------------------------------------------- */
int ngp_sh_fwd(const float* x, int64_t n, int degree, float* y, int64_t ldy, void* stream);

/* same basis of a raw view direction d (n,3): y = SH((normalize(d, eps=1e-6) + 1) / 2), the three
 * steps of networks.py:198,222 (F.normalize, remap to [0,1], dir_encoder) in one launch */
int ngp_sh_fwd_dirs(const float* d, int64_t n, int degree, float* y, int64_t ldy, void* stream);
int ngp_sh_bwd_input(const float* x, const float* dL_dy, int64_t n, int degree,
                     float* dL_dx, void* stream);

/* ------------------------------------------------------------------------
 * M1-M4  small MLP layers on f32 MFMA (v_mfma_f32_32x32x2_f32)
 * replaces tcnn.Network(CutlassMLP) (networks.py:89-163) and the torch xyz_net
 * (networks.py:54-58).  Weights are (n_out, n_in) row-major (tcnn / nn.Linear).
 *
 * ngp_linear_fwd : y (n, n_out) = act(x (n, n_in) . W^T + b)      b may be NULL
 * ngp_linear_bwd_input : dx (n, n_in) = dz (n, n_out) . W
 * ngp_linear_bwd_weight: dW (n_out, n_in) += dz^T . x ; db (n_out) += sum dz
 *                        (atomic split-K over samples; caller zeroes dW/db)
 * ngp_act_bwd : dz = dy * act'(.) expressed through the layer OUTPUT y (post-activation):
 *               ReLU y>0, Sigmoid y(1-y), Exp y, Softplus 1-exp(-y) (= sigmoid of the input).
 * ngp_mlp_hidden_bwd : hidden-layer backward of a 2-layer MLP with a narrow output (n_out<=16,
 *               H in {32,64,128}): dz2 = dOut*act2'(out) (optional output), dz1 = (dz2.W2)*act1'(hidden);
 *               dOut == NULL means all ones (analytic d(sigma)/dx of the density head).
 * ldx/ldy/lddz/lddx/ldw are row strides in floats (>= the logical width); a W sub-block
 * (e.g. the columns of rgb_net's first layer that see the grid features) is addressed by
 * offsetting W and keeping ldw.
 * ---------------------------------------------------------------------- */
int ngp_linear_fwd(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* b,
                   int64_t n, int n_in, int n_out, int activation,
                   float* y, int64_t ldy, float* z_pre /* optional (n,n_out) pre-activation, may be NULL */,
                   void* stream);

/* Forward of a 2-layer MLP in one launch: hidden (n, H<=128) = act1(x W1^T + b1) is stored (the
 * backward needs it), out (n, n_out<=8) = act2(hidden W2^T + b2) is formed from the activated tile
 * in the MFMA kernel's epilogue — xyz_net (networks.py:54-59), rgb_net (89-100), norm_pred_header
 * (102-111), semantic_header (114-123, up to 8 classes).  b1 / b2 may be NULL (tcnn networks have no biases). */
int ngp_mlp2_fwd(const float* x, int64_t ldx, const float* W1, int64_t ldw1, const float* b1, int act1,
                 const float* W2, int64_t ldw2, const float* b2, int act2, int64_t n, int n_in, int H,
                 int n_out, float* hidden, int64_t ldh, float* out, int64_t ldo, void* stream);

/* the same, also writing dact_out (n, n_out, row stride ldo) = act2'(z2) expressed through the output — bitwise what
 * ngp_act_bwd(NULL, out, ...) would compute afterwards (the density head's d sigma / d x pass starts from it) */
int ngp_mlp2_fwd_dact(const float* x, int64_t ldx, const float* W1, int64_t ldw1, const float* b1, int act1,
                      const float* W2, int64_t ldw2, const float* b2, int act2, int64_t n, int n_in, int H,
                      int n_out, float* hidden, int64_t ldh, float* out, int64_t ldo, float* dact_out, void* stream);

int ngp_linear_bwd_input(const float* dz, int64_t lddz, const float* W, int64_t ldw,
                         int64_t n, int n_in, int n_out, float* dx, int64_t lddx,
                         int accumulate /* dx += instead of dx = */, void* stream);

int ngp_linear_bwd_weight(const float* dz, int64_t lddz, const float* x, int64_t ldx,
                          int64_t n, int n_in, int n_out, float* dW, int64_t ldw,
                          float* db /* may be NULL */, void* stream);

int ngp_act_bwd(const float* dy, const float* y, int64_t count, int activation,
                float* dz, void* stream);
/* the same over (n, cols <= 4) rows, which also accumulates sum_rows ||dz[row, :]||_2 into *row_norm_acc (what
 * ngp_row_norm_sum would compute from dz afterwards: the norm-bound sums of ngp_clip_decide without a launch of their own) */
int ngp_act_bwd_rows(const float* dy, const float* y_or_z, int64_t n, int cols, int activation, float* dz,
                     float* row_norm_acc, void* stream);

int ngp_mlp_hidden_bwd(const float* dOut, int64_t lddo, const float* out, int64_t ldo, int act2,
                       const float* W2, int64_t ldw2, const float* hidden, int64_t ldh, int act1,
                       int64_t n, int H, int n_out, float* dz2, int64_t lddz2,
                       float* dz1, int64_t lddz1,
                       float* dW2 /* NULL, or (n_out<=4, H): += dz2^T . hidden from the same pass */,
                       int64_t lddw2, float* db2 /* NULL or (n_out): += column sums of dz2 */, void* stream);

/* Backward of the FIRST layer of a 2-layer MLP  x -> hidden = act1(x W1^T + b1) -> out = act2(hidden W2^T + b2)
 * (n_out <= 4: xyz_net, rgb_net, norm_pred_header) with the hidden-layer gradient
 *     dz1 = act1'(hidden) * (dz2 . W2),   dz2 (n, n_out) = dL/dout * act2'(out)  [ngp_act_bwd]
 * formed inside the MFMA product while its operand tile is staged, so that dz1 is never written to or
 * read from HBM (it is n x 128 floats, and the plain route ngp_mlp_hidden_bwd -> ngp_linear_bwd_*
 * moves it three times):
 *   ngp_mlp_bwd_input : dx (n, n_in) (+)= dz1 . W1[:, :n_in]
 *   ngp_mlp_bwd_weight: dW1 (H, n_in) += dz1^T . x,  db1 (H) += column sums of dz1 (db1 may be NULL);
 *                       optionally also the SECOND layer's dW2 / db2, whose operands (dz2, hidden) this
 *                       product streams anyway */
int ngp_mlp_bwd_input(const float* dz2, int64_t lddz2, const float* W2, int64_t ldw2, const float* hidden,
                      int64_t ldh, int act1, const float* W1, int64_t ldw1, int64_t n, int n_in, int H,
                      int n_out, float* dx, int64_t lddx, int accumulate, void* stream);
int ngp_mlp_bwd_weight(const float* dz2, int64_t lddz2, const float* W2, int64_t ldw2, const float* hidden,
                       int64_t ldh, int act1, const float* x, int64_t ldx, int64_t n, int n_in, int H,
                       int n_out, float* dW1, int64_t ldw, float* db1,
                       float* dW2 /* NULL, or (n_out, H): += dz2^T . hidden from the same pass */,
                       int64_t lddw2, float* db2 /* NULL or (n_out): += column sums of dz2 */, void* stream);

/* ------------------------------------------------------------------------
 * fused Adam step (torch.optim.Adam(eps=1e-8) semantics, train.py:244) over one
 * flat fp32 tensor; optionally scales the gradient first (grad clipping /
 * 1/world_size) and zeroes it afterwards.
 * step is the 1-based step count.
 * ---------------------------------------------------------------------- */
int ngp_adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay,
                  int64_t step, const float* grad_scale /* device scalar or NULL */,
                  int zero_grad, void* stream);

/* the same with the launch width named: a grid-stride sweep on `workgroups` workgroups of 256 threads (0: the default, 2 per
 * CU = 512 on MI355X).  The result does not depend on it; what does is how the sweep shares the CUs with kernels on other
 * streams — one workgroup per CU leaves room for 8-wave MLP workgroups beside it, two finish the sweep sooner; which is
 * faster per step depends on the loop around it, so the trainer measures. */
int ngp_adam_step_width(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                        float lr, float beta1, float beta2, float eps, float weight_decay,
                        int64_t step, const float* grad_scale /* device scalar or NULL */,
                        int zero_grad, int workgroups, void* stream);

/* sum of squares of a flat tensor accumulated into *out (device scalar; caller zeroes) */
int ngp_sumsq(const float* x, int64_t n, float* out, void* stream);

/* torch.nn.utils.clip_grad_norm_ coefficient (train.py: gradient_clip_val=50) on device:
 * norm = sqrt(*sumsq)*extra_scale; *coef = extra_scale * min(1, max_norm/(norm+1e-6)).
 * extra_scale carries 1/world_size for summed (not yet averaged) data-parallel gradients. */
int ngp_clip_coef(const float* sumsq, float max_norm, float extra_scale, float* coef, void* stream);

/* Gradient clipping settled from an upper bound of the norm, without reading the 0.8 GB table gradients.
 * A 2-layer MLP (hidden activation with |act'| <= 1: ReLU, Softplus) sends dfeat[s] = (act'(h) * (dz2[s] . W2)) . W1
 * into its encoder, so ||dfeat[s]||_2 <= ||dz2[s]||_2 ||W2||_F ||W1||_F, and the encoder's scatter adds, per sample,
 * a vector whose norm is at most ||dfeat[s]||_2 (trilinear weights: sum of squares <= 1).  Hence
 *   ||table gradient||_2 <= ||W1||_F ||W2||_F * sum_s ||dz2[s]||_2 .
 * ngp_row_norm_sum accumulates sum_s ||x[s, 0:cols]||_2 into *out (caller zeroes);
 * ngp_clip_decide takes those sums for two tables (row_norm_sums[0], [1]), the two weight blocks of each MLP and the
 * EXACT sum of squares of every other gradient, forms bound = sqrt(B0^2 + B1^2 + *sumsq_rest) * extra_scale and, when
 * bound * 1.001 + 1e-6 < max_norm, writes *coef = extra_scale (the exact coefficient: nothing is clipped) and
 * *need_exact = 0; otherwise *need_exact = 1 and the caller's ngp_sumsq_if / ngp_clip_coef_if launches (no-ops when the
 * flag is 0) compute the exact norm and coefficient.  NaN / inf anywhere takes the exact route. */
int ngp_row_norm_sum(const float* x, int64_t ldx, int64_t n, int cols, float* out, void* stream);
int ngp_clip_decide(const float* row_norm_sums, const float* w1_a, int64_t n1_a, const float* w2_a, int64_t n2_a,
                    const float* w1_b, int64_t n1_b, const float* w2_b, int64_t n2_b, const float* sumsq_rest,
                    float max_norm, float extra_scale, float* coef, int32_t* need_exact, void* stream);
/* ngp_clip_decide with the exact part summed by the same launch: *sumsq (in: what has been summed already, usually 0)
 * += sum of squares of rest[0:n_rest] (the MLP gradients, ~40 k entries), then the decision as above with it. */
int ngp_clip_decide_rest(const float* row_norm_sums, const float* w1_a, int64_t n1_a, const float* w2_a, int64_t n2_a,
                         const float* w1_b, int64_t n1_b, const float* w2_b, int64_t n2_b, const float* rest,
                         int64_t n_rest, float* sumsq, float max_norm, float extra_scale, float* coef,
                         int32_t* need_exact, void* stream);
int ngp_sumsq_if(const float* x, int64_t n, float* out, const int32_t* flag, void* stream);
int ngp_clip_coef_if(const float* sumsq, float max_norm, float extra_scale, float* coef, const int32_t* flag,
                     void* stream);

/* ------------------------------------------------------------------------
 * M1  marching cubes on a dense lattice (mesh export; replaces the reference's extract_mesh.py:
 *     skimage.measure.marching_cubes, which has no native counterpart there)
 * volume (nx, ny, nz) f32, C order (z fastest, meshgrid indexing='ij').  A corner is inside iff v > level (NaN and
 * v == level are outside).  Every lattice point owns its edges toward +x, +y, +z; each owned edge whose ends classify
 * differently carries exactly one vertex, numbered point-major then x < y < z edge (welded, no atomics: the output is
 * the same from run to run), at origin + (idx + t*e_axis) * spacing with t = (level-v0)/(v1-v0) clamped by
 * fmaxf/fminf to [0,1] (NaN -> 0: on its edge even for non-finite inputs).  Triangles are cell-major, in table order
 * within a cell, wound so that (v1-v0) x (v2-v0) points from inside to outside (toward lower density).  The case
 * table resolves every ambiguous face by one face-local rule (inside corners are separated): surfaces that do not
 * touch the volume boundary are closed, consistently oriented 2-manifolds.
 * Two calls: ngp_mc_count leaves totals[0] = V, totals[1] = F on the device (-1: more than INT32_MAX, and the emit
 * then writes nothing) and, in workspace (ngp_mc_workspace(nx, ny, nz) int32 elements, host-only query), what
 * ngp_mc_emit needs; the caller reads the totals back to size verts (V, 3) f32 and faces (F, 3) i32.  origin3 and
 * spacing3 are HOST arrays of 3 floats.  A lattice with a dimension < 2 is empty (NGP_OK before any pointer is
 * looked at, nothing written); a negative dimension or nx*ny*nz >= 2^31 is NGP_EINVAL.
 * ngp_mc_tables (host-only) copies out the case table the kernels use: tri_table (256, 16) edge triples, -1
 * terminated; tri_count (256) triangles per case; edge_corner (12, 2) the corners each edge joins (low end first).
 * Corner c of a cell sits at offset (c & 1, c >> 1 & 1, c >> 2 & 1); bit c of the case index is corner c inside.
 * ---------------------------------------------------------------------- */
int64_t ngp_mc_workspace(int nx, int ny, int nz);
int ngp_mc_tables(int8_t* tri_table, int8_t* tri_count, int8_t* edge_corner);
int ngp_mc_count(const float* volume, int nx, int ny, int nz, float level, int32_t* workspace, int32_t* totals,
                 void* stream);
int ngp_mc_emit(const float* volume, int nx, int ny, int nz, float level, const float* origin3 /* host */,
                const float* spacing3 /* host */, const int32_t* workspace, float* verts, int32_t* faces,
                void* stream);

/* ------------------------------------------------------------------------
 * M2  connected components and compaction of a triangle mesh (mesh cleaning: keep the large pieces, drop floaters;
 *     the reference's family keeps the largest cluster on the CPU)
 * faces (n_faces, 3) int32 over n_verts vertices; every index must lie in [0, n_verts) (the caller checks it).  Two
 * faces are connected when they share a vertex.
 * Labels: ngp_mesh_labels_init writes labels[v] = v; each ngp_mesh_labels_round (two launches: hook the faces'
 * corner labels to their minimum with atomicMin, then pointer jumping) only lowers labels, and writes changed[0] = 1
 * when it lowered one (the caller zeroes the word).  The caller repeats rounds until one leaves the word at 0; then
 * labels[v] is the smallest vertex index of v's component (a vertex in no face keeps its own), whatever the thread
 * order.  No launch waits on another workgroup's stores.
 * ngp_mesh_face_counts: face_counts[r] = faces of the component whose label is r (0 elsewhere); zeroes it itself.
 * Compaction, two calls: ngp_mesh_compact_count flags the kept faces (keep[labels[corner]] != 0, keep a (n_verts)
 * uint8 array indexed by label) and the kept vertices (those some kept face uses), and leaves totals[0] = kept
 * vertices, totals[1] = kept faces on the device with what the emits need in workspace
 * (ngp_mesh_clean_workspace(n_verts, n_faces) int32 elements, host-only query; NGP_EINVAL for a negative size or
 * n_faces > INT32_MAX / 3).  ngp_mesh_compact_rows copies the kept rows of any per-vertex array (row_bytes bytes per
 * vertex: positions, normals, colours) in their original order; ngp_mesh_compact_faces writes the kept faces in their
 * original order with their corners renumbered.  Empty inputs return NGP_OK before any pointer is looked at.
 * ---------------------------------------------------------------------- */
int64_t ngp_mesh_clean_workspace(int n_verts, int n_faces);
int ngp_mesh_labels_init(int32_t* labels, int n_verts, void* stream);
int ngp_mesh_labels_round(const int32_t* faces, int n_faces, int n_verts, int32_t* labels, int32_t* changed,
                          void* stream);
int ngp_mesh_face_counts(const int32_t* faces, int n_faces, int n_verts, const int32_t* labels, int32_t* face_counts,
                         void* stream);
int ngp_mesh_compact_count(const int32_t* faces, int n_faces, int n_verts, const int32_t* labels,
                           const int32_t* face_counts, const uint8_t* keep, int32_t* workspace, int32_t* totals,
                           void* stream);
int ngp_mesh_compact_rows(const void* src, int row_bytes, int n_verts, int n_faces, const int32_t* workspace,
                          void* dst, void* stream);
int ngp_mesh_compact_faces(const int32_t* faces, int n_faces, int n_verts, const int32_t* workspace,
                           int32_t* faces_out, void* stream);

/* ------------------------------------------------------------------------
 * M3  mesh simplification: uniform vertex clustering (Rossignac-Borrel) with one quadric solve per cell (Lindstrom)
 * verts (n_verts, 3) f32, faces (n_faces, 3) int32 with every index in [0, n_verts) (the caller checks it);
 * n_verts, n_faces <= 2^28.  The cell key of a vertex is floorf((v_a - origin3[a]) * inv_cell) per axis in f32
 * without contraction (inv_cell = 1.f / cell, formed by the caller); vertices with equal keys form a cluster, and
 * clusters are numbered in ascending order of their smallest member.  A face with two corners in one cluster is
 * degenerate; of the faces with the same unordered cluster triple only the one with the smallest index is kept.
 * ngp_mesh_simplify_count (the count-only path: nothing is summed or emitted) leaves on the device totals[0] =
 * clusters, totals[1] = kept faces, totals[2] = degenerate faces, totals[3] = error bits (1: a non-finite coordinate
 * or a key outside [0, 2^21); 2: a hash table had no room; the other totals mean nothing then), and in workspace
 * (ngp_mesh_simplify_workspace(n_verts, n_faces) int32 elements, 8-byte aligned; host-only query, NGP_EINVAL for a
 * size that is negative or above 2^28) what the calls below need.  Its tables are open-addressing, at least twice
 * the element count, filled with integer atomicCAS / atomicMin; every probe loop is bounded by the capacity, and no
 * launch reads what another workgroup stored in that launch except through an atomic's return value.
 * ngp_mesh_simplify_groups writes vert_cluster (n_verts) and corner_cluster (3 n_faces, index 3 * face + corner).
 * The caller sorts each once, stably, into sorted_* (the cluster numbers, ascending) and order_* (the vertex, or
 * 3 * face + corner, of each entry), int32.  ngp_mesh_simplify_place then writes one vertex per cluster
 * (n_clusters = totals[0]): all sums in double over the f32 inputs in that order, no floating-point atomics (the same
 * bytes from run to run).  m = the members' mean.  quadric == 0: x = m.  Otherwise every corner of every input face
 * adds n n^T to A and (n . p0) n to b of its cluster, n = (p1 - p0) x (p2 - p0); t = trace A; t zero or not finite:
 * x = m; else lambda = regularization * t / 3 and (A + lambda I) x = b + lambda m by Cholesky, x clamped per axis to
 * [origin + key * cell, origin + (key + 1) * cell] in double; rounded to f32.  normals / colors (n_verts, 3) f32 /
 * uint8 or NULL: normals_out = the members' mean, normalised ((0,0,0) where it vanishes), colors_out = floor(mean +
 * 0.5) in integers.  ngp_mesh_simplify_faces writes the kept faces (totals[1], 3) as cluster numbers in their
 * original order and winding and adds to used[c] (n_clusters, zeroed by the caller) the kept corners at cluster c:
 * with labels[c] = c and keep[c] = 1 that is the face_counts ngp_mesh_compact_* (M2) takes to drop unused clusters.
 * origin3 is a HOST array of 3 floats.  n_verts == 0 returns NGP_OK before any pointer is looked at (n_faces == 0
 * too where only faces are written); every pointer is checked (NGP_EINVAL) before any launch.
 * ---------------------------------------------------------------------- */
int64_t ngp_mesh_simplify_workspace(int n_verts, int n_faces);
int ngp_mesh_simplify_count(const float* verts, int n_verts, const int32_t* faces, int n_faces,
                            const float* origin3 /* host */, float inv_cell, int32_t* workspace, int32_t* totals,
                            void* stream);
int ngp_mesh_simplify_groups(const int32_t* faces, int n_faces, int n_verts, const int32_t* workspace,
                             int32_t* vert_cluster, int32_t* corner_cluster, void* stream);
int ngp_mesh_simplify_place(const float* verts, int n_verts, const int32_t* faces, int n_faces,
                            const float* origin3 /* host */, float cell, float inv_cell, double regularization,
                            int quadric, int n_clusters, const int32_t* sorted_v, const int32_t* order_v,
                            const int32_t* sorted_c, const int32_t* order_c, const float* normals,
                            const uint8_t* colors, float* verts_out, float* normals_out, uint8_t* colors_out,
                            void* stream);
int ngp_mesh_simplify_faces(const int32_t* faces, int n_faces, int n_verts, const int32_t* workspace,
                            int32_t* faces_out, int32_t* used, void* stream);

/* ------------------------------------------------------------------------
 * M4  mesh evaluation: area-weighted surface samples and the exact distance from points to a triangle mesh
 *     (accuracy / completeness / Chamfer / F-score of an export, mesh.py mesh_distance, tools/eval_mesh.py)
 * verts (n_verts, 3) f32, faces (n_faces, 3) int32 with every index in [0, n_verts) (the caller checks it).  All f32
 * arithmetic below is uncontracted, in the order written.
 * ngp_mesh_sample_surface: sample i of n (n <= 2^30) depends on (seed, i) alone - one thread per sample, no state,
 * the same bytes from run to run and for any launch shape.  With fmix32 the 32-bit finaliser of MurmurHash3 (h ^= h >>
 * 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16) and integers mod 2^32: u_k = fmix32(seed +
 * 0x9E3779B9 * (3 i + k + 1)), k = 0, 1, 2.  cdf (n_faces) f64 is the inclusive running sum of the face areas and
 * total = cdf[n_faces - 1], both from the caller (total zero, negative or not finite: NGP_EINVAL).  t = ((u_0 + 0.5) *
 * 2^-32) * total in double; the face is the first f with cdf[f] > t (binary search), clamped to the first f with
 * cdf[f] >= total (the last face with an area): a face that adds nothing to cdf is never drawn.  r1 = (u_1 >> 8) *
 * 2^-24, r2 = (u_2 >> 8) * 2^-24 in f32; if r1 + r2 > 1 (f32) then r1 = 1 - r1, r2 = 1 - r2; per axis
 * p = (v0 + r1 * (v1 - v0)) + r2 * (v2 - v0).  Writes points (n, 3) f32 and face (n) int32.
 * The grid: dims3[a] cells of edge 1 / inv_cell per axis from origin3 (both HOST arrays; dims3[a] in [1, 1024],
 * dims3[0] * dims3[1] * dims3[2] <= 2^24), cell (x, y, z) at index (x * dims3[1] + y) * dims3[2] + z.  The cell
 * coordinate of a position is floorf((p_a - origin3[a]) * inv_cell) per axis, as in M3.  A face is referenced from
 * every cell of the box [min, max] of its corners' cell coordinates (clamped to the grid; a corner outside the grid
 * raises error bit 2 - the caller's grid must cover the mesh), except that a face whose f32 cross product
 * (v1 - v0) x (v2 - v0) = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x) is exactly (0,0,0) is
 * referenced nowhere, and a face with a non-finite corner raises error bit 1 and is referenced nowhere.
 * ngp_mesh_grid_count adds each face's references to cell_count (cells, int32, zeroed by the caller; integer
 * atomicAdd) and leaves totals[0] = references, totals[1] = error bits (2 int64 on the device; it zeroes them first).
 * The caller forms cell_offset (cells + 1, int32): 0, then the inclusive running sum of cell_count (references <=
 * 2^28).  ngp_mesh_grid_fill writes face f at cell_faces[cell_offset[cell] + (what an integer atomicAdd on
 * cell_cursor[cell] returned)] (cell_cursor: cells int32, zeroed by the caller): the order inside a cell is arbitrary.
 * Within a launch threads learn about each other only through the return values of atomics; the tables are read in
 * later launches only.
 * ngp_mesh_closest: one thread per point; d2[i] = the smallest squared distance from points[i] to a face with a
 * non-zero cross product, face[i] = that face; among equal d2 the smallest face index; candidates are compared with <,
 * so a NaN or infinite d2 never wins; if the winner's d2 > max_dist * max_dist (one f32 product) or nothing won,
 * d2[i] = max_dist * max_dist and face[i] = -1 (n_faces == 0: every point).  The squared distance to a triangle
 * (a, b, c), with dot(x, y) = (x.x * y.x + x.y * y.y) + x.z * y.z and the first region that applies (Ericson, Real-Time
 * Collision Detection 5.1.5):
 *   ab = b - a, ac = c - a, ap = p - a, d1 = dot(ab, ap), d2 = dot(ac, ap);   d1 <= 0 and d2 <= 0: q = a
 *   bp = p - b, d3 = dot(ab, bp), d4 = dot(ac, bp);                           d3 >= 0 and d4 <= d3: q = b
 *   vc = d1 * d4 - d3 * d2;       vc <= 0 and d1 >= 0 and d3 <= 0: q = a + ab * (d1 / (d1 - d3))
 *   cp = p - c, d5 = dot(ab, cp), d6 = dot(ac, cp);                           d6 >= 0 and d5 <= d6: q = c
 *   vb = d5 * d2 - d1 * d6;       vb <= 0 and d2 >= 0 and d6 <= 0: q = a + ac * (d2 / (d2 - d6))
 *   va = d3 * d6 - d5 * d4;       va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
 *                                 q = b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))
 *   else den = 1 / ((va + vb) + vc), q = (a + ab * (vb * den)) + ac * (vc * den)
 *   e = p - q, result dot(e, e); every division is IEEE.
 * The search walks the cells of growing Chebyshev distance r from the point's own (unclamped) cell coordinate and stops
 * after a whole ring when no face it has not seen can win or tie (a lower bound that allows for the rounding of the
 * cell coordinates and of the distance itself: csrc/ring_walk.h), after ceil(max_dist * inv_cell) + 1 rings (plus
 * that allowance), or when the grid is exhausted: every loop is bounded before it starts, none waits on another thread,
 * and the result does not depend on the grid or on the order inside a cell.  No floating-point atomics: the same bytes
 * from run to run.
 * n == 0 returns NGP_OK before any pointer is looked at (ngp_mesh_grid_*: n_faces == 0); every pointer and size is
 * checked (NGP_EINVAL) before any launch; max_dist must be >= 0 (infinity is allowed).
 * ---------------------------------------------------------------------- */
int ngp_mesh_sample_surface(const float* verts, int n_verts, const int32_t* faces, int n_faces, const double* cdf,
                            double total, int64_t n, uint32_t seed, float* points, int32_t* face, void* stream);
int ngp_mesh_grid_count(const float* verts, int n_verts, const int32_t* faces, int n_faces,
                        const float* origin3 /* host */, float inv_cell, const int32_t* dims3 /* host */,
                        int32_t* cell_count, int64_t* totals, void* stream);
int ngp_mesh_grid_fill(const float* verts, int n_verts, const int32_t* faces, int n_faces,
                       const float* origin3 /* host */, float inv_cell, const int32_t* dims3 /* host */,
                       const int32_t* cell_offset, int32_t* cell_cursor, int32_t* cell_faces, void* stream);
int ngp_mesh_closest(const float* points, int64_t n, const float* verts, int n_verts, const int32_t* faces,
                     int n_faces, const float* origin3 /* host */, float inv_cell, const int32_t* dims3 /* host */,
                     const int32_t* cell_offset, const int32_t* cell_faces, float max_dist, float* d2, int32_t* face,
                     void* stream);

/* ------------------------------------------------------------------------
 * M5  point clouds: the nearest point of a cloud with the sums of a registration step, and voxel means
 *     (scores an export against a laser-scan reference: cloud.py nearest_points / icp / voxel_downsample / tnt_score,
 *     tools/eval_mesh.py --ref_points)
 * All f32 and f64 arithmetic below is uncontracted, in the order written.
 * The grid is M4's: dims3[a] cells of edge 1 / inv_cell per axis from origin3 (both HOST arrays; dims3[a] in
 * [1, 1024], at most 2^24 cells), cell (x, y, z) at index (x * dims3[1] + y) * dims3[2] + z, the cell coordinate of a
 * position floorf((p_a - origin3[a]) * inv_cell) per axis.  The caller sorts the cloud by cell index (stable) and
 * passes cloud4 (n_cloud, 4) f32, 16-byte aligned: row k = (x, y, z, the bit pattern of the int32 original index) of
 * the k-th point in that order, every coordinate finite and inside the grid, and cell_offset (cells + 1, int32): the
 * rows of cell c are [cell_offset[c], cell_offset[c + 1]) (offsets outside [0, n_cloud] are clamped, never followed).
 * ngp_cloud_nearest: one thread per query (queries (n, 3) f32, n <= 2^31 - 1; the caller sorts them by cell for speed,
 * the result does not depend on it).  xform12: a HOST array of 12 floats, row-major 3 x 4 (R | t), or NULL; with it the
 * query is p'_a = ((R_a0 * x + R_a1 * y) + R_a2 * z) + t_a in f32, without it p' = (x, y, z).  For a point q of the
 * cloud d2 = (dx * dx + dy * dy) + dz * dz in f32 with d = p' - q; candidates are compared with <, so a NaN or infinite
 * d2 never wins; among equal d2 the smallest original index wins; if the winner's d2 > max_dist * max_dist (one f32
 * product) or nothing won (n_cloud == 0: every query; then no grid argument is looked at), d2[i] = max_dist * max_dist
 * and index[i] = -1, else d2[i] and index[i] = the winner's d2 and original index.  d2 and index may each be NULL.
 * The search is M4's walk over the rings of cells around the query's unclamped cell coordinate with its stop rule and
 * ring cap (csrc/ring_walk.h; cloud_kernels.hip says why the bound holds for points): every loop is bounded before it
 * starts - a query with a NaN coordinate walks the grid's cells once, matches nothing and gets index -1 - and no
 * thread waits on another.
 * partials (workgroups x 18 doubles, workgroups = ceil(n / 256); may be NULL; needs centre3, a HOST array of 3 finite
 * floats): row w holds, over the queries 256 w .. 256 w + 255 with index >= 0, and with p~ = (double)p' -
 * (double)centre3, q~ = (double)q - (double)centre3 (q the winner):
 *   [0] the count, [1..3] sum p~, [4..6] sum q~, [7 + 3 a + b] sum p~_a * q~_b, [16] sum (p~_x^2 + p~_y^2) + p~_z^2,
 *   [17] sum (double)d2.
 * Each entry is wave_sum<double> (xor butterfly 32 -> 1) over the terms of a wave, zero for a query that did not
 * match, then the 4 waves added in order.  A workgroup writes its own row and nothing else.
 * ngp_cloud_sum_partials: sums18[e] = the sum of column e of partials (rows x 18): accumulator g of 14 adds the rows
 * g, g + 14, g + 28, ... in rising order from 0.0, then the 14 are added in order g = 0 .. 13.  One workgroup, no
 * atomics: the same 18 * 8 bytes on every run.  rows == 0 writes 18 zeros.
 * ngp_cloud_voxel_mean: points (n, 3) f32 sorted by voxel (the caller's stable sort, so the original order inside a
 * voxel) and offsets (n_voxels + 1, int64, DEVICE): voxel v owns the rows [offsets[v], offsets[v + 1]) (clamped to
 * [0, n]).  One thread per voxel adds its rows in order in double from 0.0 per axis, divides by the count (IEEE, double)
 * and rounds once to f32 into points_out (n_voxels, 3).  normals (n, 3) f32 -> normals_out likewise (the mean, not
 * renormalised); colors (n, 3) uint8 -> colors_out = (uint8)floor(sum / count + 0.5) in double (half away from zero).
 * normals and colors may be NULL (then their outputs are not looked at); an empty run writes zeros.
 * No entry allocates or synchronises.  ngp_cloud_nearest and ngp_cloud_voxel_mean: n == 0 returns NGP_OK before any
 * pointer is looked at (n_voxels == 0 likewise); every pointer and size is checked (NGP_EINVAL) before any launch
 * (n < 0, n_voxels > n, max_dist not >= 0 - infinity is allowed -, partials without centre3, a grid M4 would refuse).
 * ---------------------------------------------------------------------- */
int ngp_cloud_nearest(const float* queries, int64_t n, const float* cloud4, int n_cloud,
                      const float* origin3 /* host */, float inv_cell, const int32_t* dims3 /* host */,
                      const int32_t* cell_offset, float max_dist, const float* xform12 /* host */,
                      const float* centre3 /* host */, float* d2, int32_t* index, double* partials, void* stream);
int ngp_cloud_sum_partials(const double* partials, int64_t rows, double* sums18, void* stream);
int ngp_cloud_voxel_mean(const float* points, const float* normals, const uint8_t* colors, int64_t n,
                         const int64_t* offsets, int64_t n_voxels, float* points_out, float* normals_out,
                         uint8_t* colors_out, void* stream);

/* ------------------------------------------------------------------------
 * I1  SSIM of rendered images (replaces torchmetrics' StructuralSimilarityIndexMeasure(data_range=1) of the
 *     reference's validation step, train.py:93,353-386; no conv2d / MIOpen on the way)
 * pred, gt: `count` images of H*W rows of 3 floats, row-major, channel-last (what render() returns and the loaders
 * keep in `rays`).  out (count) f32: the mean SSIM of each image over its (H-10) x (W-10) fully inside window
 * positions and 3 channels.  Window 11x11 separable Gaussian, sigma 1.5, taps exp(-x^2/(2 sigma^2)), x = -5..5,
 * normalised to sum 1 (double on the host, rounded once to float); per window mu_x, mu_y, var_x = E[x^2] - mu_x^2,
 * var_y, cov_xy; C1 = 0.01^2, C2 = 0.03^2; ssim = (2 mu_x mu_y + C1)(2 cov_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(var_x +
 * var_y + C2)).  Moments are accumulated in float about a per-tile pivot (the tile's centre pixel: no
 * cancellation in the variances where a 26x26 tile is flat; a window on another flat level of a tile that straddles an
 * edge is evaluated as well as in plain float32, no better), per-workgroup sums
 * go to `partial` (ngp_ssim_workspace(count, H, W) doubles, host-only query) and a second launch adds them in a fixed
 * order in double: no atomics, the same bits from run to run and for an image alone or inside a batch.
 * count == 0 returns NGP_OK before anything else is looked at; H or W < 11, H*W > INT32_MAX/3, count > 65535 or a
 * NULL pointer is NGP_EINVAL.
 * ---------------------------------------------------------------------- */
int64_t ngp_ssim_workspace(int count, int H, int W);
int ngp_ssim(const float* pred, const float* gt, int count, int H, int W, double* partial, float* out, void* stream);

/* ------------------------------------------------------------------------
 * I2  8-bit frames from the per-ray outputs of the test-time renderer, one launch per frame (replaces the numpy /
 *     cv2 conversions of the reference's render.py:17-31,150-185 and utils.py:84-95 done on the host in float)
 * With u8(v) = (uint8)(clip(v, 0, 1) * 255) (truncation), all in float32 in the order written, true division:
 *   rgb_u8 (n,3)        = u8(rgb (n,3))                                            render.py:158-159
 *   opacity_u8 (n)      = u8(opacity (n))
 *   depth_u8 (n,3)      = lut[u8(depth (n) / depth_scale)]                         render.py:17-23,168
 *   normal_u8, normal_raw_u8 (n,3): n' = n + 1e-6, c_j = (n'_0 R_0j + n'_1 R_1j) + n'_2 R_2j, u8((c_j + 1) / 2)
 *                         with R (3,3) row-major DEVICE floats, the frame's camera-to-world rotation
 *                         (convert_normal: world -> camera)                        utils.py:92-95, render.py:176-185
 *   semantic_u8 (n,3)   = lut[u8(level * (float)semantic (n) int64)], level = 1.0f / (classes - 1)   render.py:25-31
 * lut (256,3) uint8 is the colour table (the package ships Turbo).  Every output pointer is optional (NULL = not
 * wanted); an output that is asked for needs its inputs (and classes >= 2 for semantic_u8), else NGP_EINVAL.
 * n == 0 returns NGP_OK before any pointer is looked at.
 * ---------------------------------------------------------------------- */
int ngp_frame_pack(int64_t n, const float* rgb, const float* opacity, const float* depth, float depth_scale,
                   const float* normal_pred, const float* normal_raw, const float* R, const int64_t* semantic,
                   int classes, const uint8_t* lut, uint8_t* rgb_u8, uint8_t* opacity_u8, uint8_t* depth_u8,
                   uint8_t* normal_u8, uint8_t* normal_raw_u8, uint8_t* semantic_u8, void* stream);

/* ------------------------------------------------------------------------
 * I3  8-bit antialiased bicubic resize, one launch per call: what PIL.Image.resize((out_w, out_h), BICUBIC) returns
 *     for `L` and `RGB` images, byte for byte (brings the supersampled frames of --anti_aliasing_factor back to the
 *     image size, render.py:150-156 of the reference, without copying the large frame to the host)
 * src: `count` images of (in_h, in_w, channels) bytes, row-major, channel-last; dst the same at (out_h, out_w);
 * channels 1 or 3.  The taps are computed by the caller in float64 per axis (n_in -> n_out samples; an axis with
 * n_in == n_out has no pass and takes NULL taps): scale = n_in / n_out, fs = max(scale, 1), support = 2 fs,
 * ksize = ceil(support) * 2 + 1; for output xx: center = (xx + 0.5) scale, xmin = max((int)(center - support + 0.5),
 * 0), xmax = min((int)(center + support + 0.5), n_in) - xmin, k[x] = f((x + xmin - center + 0.5) / fs) for x < xmax
 * with f the Keys cubic (a = -0.5), normalised by their sum taken in order; kk[x] = (int)(k[x] 2^22 +- 0.5) (toward
 * zero), unused slots 0.  k* (n_out, ksize) int32 and b* (n_out, 2) int32 = (xmin, xmax) are DEVICE arrays.
 * Rows first into an 8-bit intermediate (kept in LDS), then columns; each byte is
 * clip((2^21 + sum_x src[xmin + x] kk[x]) >> 22, 0, 255) in int32.  Integers only and no atomics: the same bits from
 * run to run and for an image alone or inside a batch.
 * count == 0 returns NGP_OK before anything else is looked at, count < 0 is NGP_EINVAL; then NGP_EINVAL for channels
 * other than 1 or 3, a non-positive size, count > 65535, n_in > 8 n_out on an axis, a ksize that is not the one above
 * on an axis that changes, or a NULL pointer that is needed.  Both axes unchanged is a copy.
 * ---------------------------------------------------------------------- */
int ngp_resize_bicubic_u8(const uint8_t* src, int count, int in_h, int in_w, int channels, uint8_t* dst, int out_h,
                          int out_w, const int32_t* kx, const int32_t* bx, int ksize_x, const int32_t* ky,
                          const int32_t* by, int ksize_y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NGP_HIP_H */
