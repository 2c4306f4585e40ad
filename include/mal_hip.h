/*
 * mal_hip.h -- C ABI of libmal_hip.so: the MI355X (gfx950) kernels for MAL's photometric
 * reprojection + motion-aware loss hot path.
 *
 * The reference (YuejiangDong/MAL) has no FFI for this path: it sits behind plain Python
 * imports of manydepth/layers.py, manydepth/loss_utils.py and three Trainer methods
 * (manydepth/trainer.py:29-30,44).  These entry points are what a
 * ctypes binding in those modules calls instead of the chain of ATen ops; each one cites
 * the reference lines it replaces.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless the name says otherwise
 *     (u8 = uint8_t, f64 = double); images are NCHW; 4x4 matrices are row-major [B][16].
 *   - every function returns 0 (MAL_OK) or a negative MAL_E* code; nothing throws, nothing
 *     allocates, nothing synchronises: work is enqueued on `stream` (a hipStream_t passed
 *     as void*; NULL = the default stream) and scratch memory comes from the caller's
 *     workspace (`mal_workspace_bytes`).
 *   - `convention`: 0 = ManyDepth / DynamicDepth (grid = (u/(W-1)-0.5)*2 sampled with
 *     align_corners=True, manydepth/layers.py:192-194 + trainer.py:1122-1125);
 *     1 = DualRefine (grid = 2*(u+0.5)/W-1 sampled with align_corners=False,
 *     dualrefine/layers.py:224-225 + dualrefine/trainer.py:444-447).
 *   - F = number of source frames (2: frame ids -1, +1); arrays "[F]" are host arrays of F
 *     device pointers, copied by value at launch (F <= MAL_MAX_FRAMES).
 */
#ifndef MAL_HIP_H
#define MAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAL_VERSION 100 /* 0.1.0 */
#define MAL_MAX_FRAMES 2
#define MAL_MAX_CAND 4 /* warped -1,+1 and the temporal-hint "syn" -1,+1 (loss_utils.py:79-90) */
#define MAL_MAX_INSTANCES 64 /* matched instance masks per sample of the temporal-hint producer */
#define MAL_MATCH_MAX 128    /* instances per side of the temporal-hint producer's matcher (mal_match) */
#define MAL_INSTANCES_MAX_QK 16384 /* mal_instances: queries x classes (Q*K) per image; Q=200, K=80 is 16000 */
#define MAL_INSTANCES_MAX_K1 1025  /* mal_instances: logits per query (K+1) */
#define MAL_INSTANCES_MAX_N 65535  /* mal_instances: images per call */
#define MAL_MSDA_MAX_L 8    /* mal_msda_*: feature levels */
#define MAL_MSDA_MAX_P 8    /* mal_msda_*: sampling points per head and level */
#define MAL_MSDA_MAX_LP 32  /* mal_msda_*: L*P, the samples of one (query, head) */
#define MAL_MSDA_MAX_D 64   /* mal_msda_*: channels per head */

enum {
  MAL_OK = 0,
  MAL_EINVAL = -1,    /* bad argument (null pointer, non-positive size, F/n_cand out of range) */
  MAL_ESHAPE = -2,    /* image smaller than 2x2 (reflection pad needs >= 2) or too large for int32 indexing; mal_msda_*: a
                         size outside the bounds stated there */
  MAL_EWORKSPACE = -3,/* workspace too small: call mal_workspace_bytes */
  MAL_ELAUNCH = -4,   /* hipLaunchKernel / hipGetLastError failed */
  MAL_ENODEVICE = -5, /* no HIP device */
  MAL_ESTALE = -6     /* a later call of a one-call step (_fwd after _warp, _bwd) found options that change the task
                         decomposition (march_rows, march_rows_fwd, pack_rows, march_halo1, device_cus) set differently
                         from the step's first call */
};

/* flags for mal_pass_fused / mal_photo_* */
enum {
  MAL_F_AUTOMASK = 1,   /* mask = argmin([min_c r_c, ident + 1e-5*noise]) == 0  (loss_utils.py:105-110) */
  MAL_F_GRAD = 2,       /* also produce the (unnormalised) gradient maps */
  MAL_F_POSE_GRAD = 4,  /* ... and d/dT (teacher pass; the student pass detaches T, trainer.py:1107-1109) */
  MAL_F_NO_SSIM = 8,    /* --no_ssim: r = mean_c |t - p| (trainer.py:1217-1218) */
  MAL_F_AVG = 16,       /* --avg_reprojection (dualrefine/trainer.py:579-583): mean over candidates */
  MAL_F_EPILOGUE = 32,  /* student epilogue: consistency + distillation terms (loss_utils.py:193-254) */
  MAL_F_DUAL_DISTIL = 64,/* --dual_distil (loss_utils.py:232-234): the idx==0 target keeps its graph */
  MAL_F_SRC_PACKED = 128,/* mal_pass_fused: src[f] are texel copies made by mal_pack_texels */
  MAL_F_TGT_PACKED = 256,/* ... and so is target */
  MAL_F_ZERO_IMG = 512, /* mal_photo_holes_*: --zero_img (dynamicdepth/trainer.py:961-965): candidate and target zeroed at the
                           candidate's holes before r is taken; the target keeps the zeros */
  MAL_F_SELECT = 1024   /* mal_photo_holes_*: --selec_reproj (dynamicdepth/trainer.py:1058-1064): where one candidate is a
                           hole the other one supplies rp; where both are, rp = 0 */
};

/* choice bytes of mal_photo_holes_fwd beside the candidate indices 0 and 1 */
#define MAL_HOLE_CHOICE_NONE 254 /* both candidates are holes under MAL_F_SELECT: rp = 0, no gradient */
#define MAL_HOLE_CHOICE_AVG 255  /* MAL_F_AVG: rp is the mean, every candidate receives 1/n_cand */

int mal_version(void);
const char* mal_strerror(int code);
/* 0 if a gfx950-class HIP device is present, else MAL_ENODEVICE. Never called by the loaders. */
int mal_device_check(void);

/* Scratch bytes the fused / warp-backward / photo entry points need for a (B,H,W) batch. */
size_t mal_workspace_bytes(int B, int H, int W);

/* ---- a1: manydepth/layers.py:14-23 ------------------------------------------------ */
int mal_disp_to_depth(const float* disp, size_t n, float min_depth, float max_depth,
                      float* scaled_out /*nullable*/, float* depth_out /*nullable*/, void* stream);
/* g_disp = g_scaled*(1/min-1/max) - g_depth*depth^2*(1/min-1/max) */
int mal_disp_to_depth_bwd(const float* disp, const float* g_scaled /*nullable*/, const float* g_depth /*nullable*/,
                          size_t n, float min_depth, float max_depth, float* g_disp, void* stream);

/* ---- a2: BackprojectDepth.forward, manydepth/layers.py:163-168 ---------------------- */
int mal_backproject(const float* depth /*B,1,H,W*/, const float* inv_K /*B,16*/, int B, int H, int W,
                    float* points /*B,4,HW*/, void* stream);
int mal_backproject_bwd(const float* g_points /*B,4,HW*/, const float* inv_K, int B, int H, int W,
                        float* g_depth /*B,1,H,W*/, void* stream);

/* ---- a3: Project3D.forward, manydepth/layers.py:184-199; dualrefine/layers.py:216-226 -- */
int mal_project3d(const float* points /*B,4,HW*/, const float* K, const float* T, int B, int H, int W,
                  float eps, int convention, float* grid /*B,H,W,2*/, float* z_out /*nullable B,1,H,W*/,
                  void* stream);
/* g_points (B,4,HW) and g_T (B,16, = K^T [g_P;0]); g_z nullable. ws: mal_workspace_bytes. */
int mal_project3d_bwd(const float* points, const float* K, const float* T, const float* g_grid,
                      const float* g_z /*nullable*/, int B, int H, int W, float eps, int convention,
                      float* g_points /*nullable*/, float* g_T /*nullable B,16*/, void* ws, size_t ws_bytes,
                      void* stream);

/* ---- a4: F.grid_sample(bilinear, border), trainer.py:1122-1125; dualrefine/trainer.py:444-447 */
int mal_grid_sample(const float* src /*B,C,H,W*/, const float* grid /*B,Ho,Wo,2*/, int B, int C, int H, int W,
                    int Ho, int Wo, int align_corners, float* out /*B,C,Ho,Wo*/, void* stream);
/* gradient wrt the grid only (the reference's sources carry no gradient) */
int mal_grid_sample_bwd(const float* src, const float* grid, const float* g_out, int B, int C, int H, int W,
                        int Ho, int Wo, int align_corners, float* g_grid /*B,Ho,Wo,2*/, void* stream);

/* ---- a7: SSIM.forward, manydepth/layers.py:243-257 ----------------------------------- */
int mal_ssim(const float* x, const float* y, int B, int C, int H, int W, float* out /*B,C,H,W*/, void* stream);
int mal_ssim_bwd(const float* x, const float* y, const float* g_out, int B, int C, int H, int W,
                 float* g_x /*nullable*/, float* g_y /*nullable*/, void* stream);

/* ---- a8: compute_reprojection_loss, manydepth/loss_utils.py:46-55 -------------------- */
int mal_reprojection_loss(const float* pred, const float* target, int B, int C, int H, int W, int no_ssim,
                          float* out /*B,1,H,W*/, void* stream);
int mal_reprojection_loss_bwd(const float* pred, const float* target, const float* g_out /*B,1,H,W*/,
                              int B, int C, int H, int W, int no_ssim,
                              float* g_pred /*nullable*/, float* g_target /*nullable*/, void* stream);

/* ---- a12: get_smooth_loss on mean-normalised disparity, layers.py:210-223 + loss_utils.py:119-121
 * normalise != 0: disp is divided by (mean_HW disp + 1e-7) per sample first.
 * loss_out[0] (f64, device) = mean_x-term + mean_y-term.  With g_disp != NULL also writes
 * d loss / d disp (exact, including the mean-normalisation coupling).                      */
int mal_smooth_loss(const float* disp /*B,1,H,W*/, const float* img /*B,C,H,W*/, int B, int C, int H, int W,
                    int normalise, double* loss_out, float* g_disp /*nullable*/, void* ws, size_t ws_bytes,
                    void* stream);

/* ---- a5 (materialising): Trainer.generate_images_pred, manydepth/trainer.py:1093-1125 --
 * depth = 1/(1/max + (1/min-1/max)*disp); for f<F: grid_f = Project3D(Backproject(depth), K, T_f);
 * warped_f = grid_sample(src_f, grid_f).  Any of the outputs may be NULL.                  */
/* `convention` of mal_warp_fwd/bwd may be OR'ed with MAL_WARP_TEXELS: src[f] are then the texel copies made by
 * mal_pack_texels (one gather per bilinear tap instead of three); results are bit-identical. */
#define MAL_WARP_TEXELS 256
int mal_warp_fwd(const float* disp /*B,1,H,W, full resolution*/, const float* K, const float* inv_K,
                 const float* const* T /*[F] B,16*/, const float* const* src /*[F] B,3,H,W*/,
                 int B, int H, int W, int F, float min_depth, float max_depth, float eps, int convention,
                 float* depth_out, float* const* grid_out /*[F] B,H,W,2*/, float* const* warped_out /*[F] B,3,H,W*/,
                 void* stream);
/* Backward of the above.  g_warped[f] / g_grid[f] / g_depth may each be NULL (absent).
 * g_disp (B,1,H,W) is overwritten; g_T[f] (B,16) nullable.                                */
int mal_warp_bwd(const float* disp, const float* K, const float* inv_K, const float* const* T,
                 const float* const* src, const float* const* g_warped, const float* const* g_grid,
                 const float* g_depth, int B, int H, int W, int F, float min_depth, float max_depth, float eps,
                 int convention, float* g_disp, float* const* g_T, void* ws, size_t ws_bytes, void* stream);

/* ---- a8-a10 on materialised candidates: the per-pixel min / automask reduction --------
 * cand[c] (B,3,H,W), c < n_cand <= MAL_MAX_CAND.  r_c = compute_reprojection_loss(cand_c, target);
 * rp = min_c r_c (first minimum wins, as torch.min on CPU) or the mean with MAL_F_AVG;
 * weight w = automask * ext_mask (each optional; ext_mask (B,1,H,W)).
 * ident: (B,1,H,W) min over the identity losses (mal_photo_fwd on the raw sources with
 *        flags=0 produces it); noise: (B,1,H,W) N(0,1) draws (CPU generator upstream).
 * Outputs: min_reproj (B,1,H,W, nullable), argmin_u8 (B,1,H,W, nullable),
 *          weight_out (B,1,H,W nullable), sums[0]=sum(rp*w), sums[1]=sum(w)  (f64, device).   */
int mal_photo_fwd(const float* target, const float* const* cand, int n_cand, const float* ident /*nullable*/,
                  const float* noise /*nullable*/, const float* ext_mask /*nullable*/, int B, int H, int W,
                  int flags, float* min_reproj, uint8_t* argmin_u8, float* weight_out, double* sums,
                  void* ws, size_t ws_bytes, void* stream);
/* d(sum(rp*w))/d cand_c -> g_cand[c] (B,3,H,W), scaled by *scale (device f32 scalar, nullable = 1)
 * divided by (sums[1] + 1e-7) when sums != NULL.  weight / argmin come from mal_photo_fwd.  */
int mal_photo_bwd(const float* target, const float* const* cand, int n_cand, const uint8_t* argmin_u8,
                  const float* weight, const float* scale, const double* sums, int B, int H, int W, int flags,
                  float* const* g_cand, void* stream);

/* ---- DynamicDepth's hole-aware reprojection loss on materialised candidates (mal_holes.hip) --------
 * dynamicdepth/trainer.py:958-975 (compute_reprojection_loss under --zero_img) and :1058-1064 (--selec_reproj), both on by
 * default upstream.  cand[c] (B,3,H,W), c < n_cand <= 2; target (B,3,H,W) as it stands in memory.
 *   hole test    h_c = ((P_c[0] + P_c[1]) + P_c[2]) < 0.1f per pixel (pred.sum(1) < 0.1 in ATen's order)
 *   ZERO_IMG     U_c = h_0 | .. | h_c;  r_c = r(P_c * !h_c, target * !U_c) with the r of mal_photo_fwd: the zeroed pixels lie
 *                inside the 3x3 windows of their neighbours.  Without the flag r_c = r(P_c, target).
 *   reduction    rp = min_c r_c (first minimum wins) or the mean with MAL_F_AVG
 *   SELECT       n_cand == 2: where h_0, rp = r_1; where h_1, rp = r_0 (this one overrides); where both, rp = 0
 *   weight, sums as mal_photo_fwd (MAL_F_AUTOMASK against ident + 1e-5 * noise, ext_mask; sums[0..1], f64, device)
 * Outputs: holes (n_cand,B,H,W) bytes 0/1 (required with either hole flag), min_reproj, choice (B,1,H,W bytes: the
 * candidate that feeds rp, MAL_HOLE_CHOICE_AVG or MAL_HOLE_CHOICE_NONE), weight_out; each map nullable.
 * The call does NOT write the target: mal_holes_commit, launched behind it on the same stream, applies
 * target <- target * !U_{n_cand-1}, upstream's in-place `target[mask] = 0` (so the next call -- the identity pair, the next
 * scale, the student -- meets the zeros).  No allocation, read-back or synchronisation: both calls can be captured.
 * ws: mal_workspace_bytes(B,H,W).  MAL_EINVAL: a null required pointer, B < 1, H or W < 2, n_cand outside 1..2,
 * MAL_F_SELECT with n_cand != 2, a flag other than AUTOMASK, NO_SSIM, AVG, ZERO_IMG, SELECT.
 * One workgroup per 32x8 tile stages the zeroed pair with its halo in LDS; mal_photo_holes_plan reports the tile, the
 * halos (forward, backward), the workgroups and the LDS bytes of both launches -- pure host code, same checks. */
int mal_photo_holes_plan(int B, int H, int W, int* tile_w, int* tile_h, int* halo_fwd, int* halo_bwd, int* blocks,
                         size_t* lds_fwd, size_t* lds_bwd);
int mal_photo_holes_fwd(const float* target, const float* const* cand, int n_cand, const float* ident /*nullable*/,
                        const float* noise /*nullable*/, const float* ext_mask /*nullable*/, int B, int H, int W,
                        int flags, uint8_t* holes, float* min_reproj, uint8_t* choice, float* weight_out, double* sums,
                        void* ws, size_t ws_bytes, void* stream);
int mal_holes_commit(float* target, const uint8_t* holes, int n_cand, int B, int H, int W, void* stream);
/* The weight of a call whose identity term did not exist yet when its rp was taken: upstream evaluates the identity pair
 * AFTER the warped pair, on the target the warped pair zeroed (trainer.py:1025-1047), so the automask of the warped pair
 * is formed behind both.  weight_out = [min_reproj <= ident + 1e-5 * noise] * ext_mask (each nullable, noise only with
 * ident), sums[0] = sum(min_reproj * w), sums[1] = sum(w), as the forward forms them.  Pointwise; ws as above. */
int mal_holes_weight(const float* min_reproj, const float* ident /*nullable*/, const float* noise /*nullable*/,
                     const float* ext_mask /*nullable*/, int B, int H, int W, float* weight_out, double* sums, void* ws,
                     size_t ws_bytes, void* stream);
/* d(sum(rp*w))/d cand_c -> g_cand[c] (B,3,H,W, nullable), scaled as mal_photo_bwd.  target is the target AS THE FORWARD
 * READ IT (a copy taken before mal_holes_commit and before any later call zeroed it further); holes, choice, weight come
 * from the forward.  Under MAL_F_ZERO_IMG exactly zero at the h_c pixels of candidate c (the masked copy was written over),
 * hence in both candidates where both are holes; a pixel whose choice is MAL_HOLE_CHOICE_NONE hands on no gradient. */
int mal_photo_holes_bwd(const float* target, const float* const* cand, int n_cand, const uint8_t* holes,
                        const uint8_t* choice, const float* weight, const float* scale, const double* sums, int B, int H,
                        int W, int flags, float* const* g_cand, void* stream);

/* ---- the fused pass: a2-a4 + a7-a10 (+ the a11 epilogue) in ONE launch ------------------
 * Replaces generate_images_pred + compute_mono_losses / compute_main_losses /
 * generate_images_pred_ensemble when the warped images need not be materialised
 * (manydepth/trainer.py:573-612, loss_utils.py:57-254).
 *
 * Inputs: disp (full res), K, inv_K, T[F], src[F], target; ident/noise (automask), ext_mask
 * (the student's consistency_mask*(1-augmentation_mask), expanded to B,1,H,W).
 * Epilogue inputs (MAL_F_EPILOGUE): mono_depth, mono_reproj, ens_reproj (nullable -> 2-way argmin).
 * Outputs:
 *   min_reproj (B,1,H,W, nullable)         per-pixel min_c r_c
 *   sums (f64[8], device): [0] sum(rp*w) [1] sum(w) [2] sum|d_multi-d_mono|*(1-w) [3] sum|distil-d_multi|*w
 *   with MAL_F_GRAD:
 *     g_reproj (B,1,H,W): d sum(rp*w) / d disp            (caller scales by g/(sums[1]+1e-7))
 *     g_cons, g_distil (B,1,H,W, MAL_F_EPILOGUE): d sums[2] / d disp, d sums[3] / d disp
 *     g_T[f] (B,16, MAL_F_POSE_GRAD): d sum(rp*w) / d T_f
 *   consistency_target (B,1,H,W nullable): 1/(mono*cmask + multi*(1-cmask)), loss_utils.py:212-215
 *   depth_out (B,1,H,W nullable)                                                               */
int mal_pass_fused(const float* disp, const float* disp2 /*nullable: disparity = (disp+disp2)/2, trainer.py:598*/,
                   const float* K, const float* inv_K, const float* const* T,
                   const float* const* src, const float* target, const float* ident, const float* noise,
                   const float* ext_mask, const float* sample_scale /*nullable (B): w *= scale[b], e.g.
                   1-augmentation_mask, loss_utils.py:194*/, const float* mono_depth, const float* mono_reproj,
                   const float* ens_reproj, int B, int H, int W, int F, float min_depth, float max_depth,
                   float eps, int convention, int flags, float* min_reproj, double* sums, float* g_reproj,
                   float* g_cons, float* g_distil, float* const* g_T, float* consistency_target,
                   float* depth_out, void* ws, size_t ws_bytes, void* stream);

/* ---- a11 epilogue on materialised depth (non-fused path): loss_utils.py:193-254 ---------
 * w = ext_mask. sums[2], sums[3] as above; g_multi_cons / g_multi_distil are d/d multi_depth
 * (unnormalised sums); g_mono_distil (nullable) is d sums[3] / d mono_depth for --dual_distil. */
int mal_distil_epilogue(const float* multi_depth, const float* mono_depth, const float* multi_reproj,
                        const float* mono_reproj, const float* ens_reproj /*nullable*/, const float* ext_mask,
                        int B, int H, int W, int flags, double* sums /*f64[8]*/, float* g_multi_cons,
                        float* g_multi_distil, float* g_mono_distil, float* consistency_target,
                        void* ws, size_t ws_bytes, void* stream);
/* ... with --learn_ens (loss_utils.py:240-241; trainer.py:596-600): the ensemble depth is ens_depth = disp_to_depth of the
 * learnt head's output instead of (mono + multi) / 2; g_ens_depth (nullable) = d sums[3] / d ens_depth (unnormalised),
 * non-zero where the ensemble wins the three-way min; ens_reproj is required. */
int mal_distil_epilogue_learned(const float* multi_depth, const float* mono_depth, const float* ens_depth,
                                const float* multi_reproj, const float* mono_reproj, const float* ens_reproj,
                                const float* ext_mask, int B, int H, int W, double* sums /*f64[8]*/, float* g_multi_cons,
                                float* g_multi_distil, float* g_ens_depth, float* consistency_target,
                                void* ws, size_t ws_bytes, void* stream);

/* (B,3,H,W) -> (B,H,W,n) texels, n = mal_texel_floats() (3: r,g,b 12 bytes apart): each bilinear tap of the fused
 * pass becomes one per-lane gather instead of three 4-byte ones.  Sources change per batch, not per pass: pack once.
 * dst holds B*H*W*n floats. */
int mal_texel_floats(void);
int mal_pack_texels(const float* src, int B, int H, int W, float* dst, void* stream);

/* ---- a13: Trainer.compute_matching_mask, manydepth/trainer.py:1066-1076 ----------------
 * out = consistency_mask * [ (1/lowest_cost - mono)/mono < 1 ] * [ (mono - 1/lowest_cost)*lowest_cost < 1 ] */
int mal_matching_mask(const float* lowest_cost /*B,H,W*/, const float* mono_depth /*B,1,H,W*/,
                      const float* consistency_mask /*nullable B,H,W*/, size_t n, float* out, void* stream);

/* ---- gradient assembly: out[i] = sum_k coef_k * maps[k][i], coef_k = (scale_k ? *scale_k : 1) *
 * mult_k / (denom_k ? (*denom_k + denom_eps_k) : 1); all scalars are read on the device so the
 * autograd backward needs no host sync.  n_terms <= 6.                                        */
int mal_axpy_maps(int n_terms, const float* const* maps, const float* const* scale, const double* const* denom,
                  const float* mult, const float* denom_eps, size_t n, float* out, int accumulate, void* stream);

/* f64 device scalar -> f32 device scalars: out[k] = num[k] / (den ? den[k] + eps : 1) */
int mal_finish_scalars(const double* num, const double* den /*nullable*/, float eps, float mult, int n,
                       float* out, void* stream);

/* sum of a float array into a f64 device scalar (the student's sum(m), known before the pass) */
int mal_sum_f64(const float* x, size_t n, double* out, void* ws, size_t ws_bytes, void* stream);

/* ---- a16: transformation_from_parameters, manydepth/layers.py:26-100 -----------------------
 * axisangle[f], translation[f]: (B,3) (the reference's (B,1,3)); invert[f] (host ints): frame ids
 * < 0 are inverted (networks/repdepth.py:159-160).  T[f]: (B,16).  One launch for all f, b. */
int mal_pose_fwd(const float* const* axisangle, const float* const* translation, const int* invert,
                 int B, int F, float* const* T, void* stream);
int mal_pose_bwd(const float* const* axisangle, const float* const* translation, const int* invert,
                 const float* const* g_T, int B, int F, float* const* g_axisangle /*[F] nullable each*/,
                 float* const* g_translation /*[F] nullable each*/, void* stream);

/* ---- the whole loss half of process_batch (manydepth/trainer.py:573-642 with --distil) as one call.
 * Forward enqueues ~18 kernels (pose composition, texel packing, identity term, teacher / ensemble /
 * student passes with the matching mask and the consistency*(1-augmentation) mask formed in the
 * kernel, both smoothness terms, reductions); backward enqueues 2 (gradient assembly, pose backward).
 * losses[16] (device f32): 0 reproj_t 1 smooth_t 2 loss_t(=0+1e-3*1) 3 reproj_s 4 consistency 5 smooth_s
 *   6 distil 7 loss_main(=3+4+1e-3*5) 8 total = w_main*(7+2) + w_distil*6   (what backward differentiates)
 *   9 reproj_s+reproj_t ("reproj_loss/0") 10 (7+6)+2 ("loss" without --loss_blc) 11 7+2 (loss_list[0])
 * Without --loss_blc pass w_main = w_distil = 1; with it w_main = bs*w0, w_distil = bs*w1
 * (loss_utils.py:303-318).  All maps the step needs between kernels live in `ws`
 * (mal_step_workspace_bytes); the same ws must be handed to _bwd. */
enum {
  MAL_STEP_NO_ENS = 1,   /* --no_ens: 2-way distillation argmin, no ensemble pass */
  MAL_STEP_AUG_MASK = 2, /* `augmentation_keep` holds augmentation_mask itself; 1 - mask is formed on the device */
  MAL_STEP_TEMPORAL = 8, /* --temporal (loss_utils.py:84-88): r(syn_f, target) of the two synthesised images joins the
                            teacher's per-pixel min.  Three calls around the producer (dyn_utils.image_synthesis):
                              mal_loss_step_warp  first sweep + the teacher's warped images -> warp_m1 / warp_p1
                              [syn_f = producer(warp_f)]
                              mal_loss_step_fwd   syn_m1 / syn_p1 in; losses out; g_syn_* out = d sum(rp*w) / d syn_f
                                                  (UNNORMALISED: the 1/(sum w + 1e-7) and loss weights are applied in _bwd)
                              [g_warp_f = producer^T(g_syn_f), linear]
                              mal_loss_step_bwd   g_warp_* in (same scale); runs the teacher's gradient sweep with the
                                                  four-way decisions of _fwd and adds what arrives through syn */
  MAL_STEP_NOISE_PHILOX = 4, /* the automask tie-break noise (loss_utils.py:105-106: + 1e-5 * randn) is drawn inside the
                               step's first kernel: N(0,1) by Box-Muller from Philox4x32-10 keyed by noise_seed, counter =
                               (pixel, step); `noise` must be NULL.  No host RNG, no device RNG launch on the step. */
  MAL_STEP_TEXEL_INPUTS = 64, /* color0 / color_m1 / color_p1 are (B,H,W,3) texel images -- a (B,3,H,W) tensor in torch.channels_last
                                memory format is exactly that --: the step gathers from them directly and skips the re-layout of
                                its first sweep (53 MB of stores per step at B=12 192x640); results are bit-identical */
  MAL_STEP_DUAL_DISTIL = 32, /* --dual_distil (loss_utils.py:231-234; only with MAL_STEP_NO_ENS, as upstream: the flag is read on the
                               two-way branch only): where the teacher wins the distillation argmin its depth is NOT detached --
                               g_disp_teacher also receives w_distil/N * sign(mono - multi) * (1 - consistency weight) * d mono / d disp */
  MAL_STEP_SYN_SPARSE = 16, /* with MAL_STEP_TEMPORAL and syn_region: syn_* hold the synthesised images ONLY at pixels whose
                               region byte has bit 0 set (a producer that writes its regions into otherwise untouched
                               buffers); elsewhere they are by definition the warped images mal_loss_step_warp wrote
                               (warp_*, still set), which the sweep reads there.  warp2_* may then be NULL: the pass in
                               front of the producer writes the warped images once instead of twice. */
  MAL_STEP_GSYN_SPARSE = 8192, /* with MAL_STEP_SYN_SPARSE: the caller vouches that NOTHING reads g_syn_* densely -- the producer's
                               backward turns those very buffers into g_warp_* in place (g_warp_* == g_syn_* in _bwd, MAL_EINVAL
                               otherwise), reading the g_syn_region_* snapshots and writing region pixels only.  mal_loss_step_fwd
                               then leaves the pixels of g_syn_* whose tile (60 columns x "syn_rows" rows) keeps more than two
                               pixels away from the region UNWRITTEN -- their gradient is zero, and the teacher's gradient sweep
                               of _bwd skips them by the workspace's tile map instead of reading zeros back.  Without the flag
                               g_syn_* is dense (the zero-fill); the A/B switch is the flag itself. */
  MAL_STEP_MAIN_TEMPORAL = 128, /* --main_temporal (manydepth/trainer.py:1164, loss_utils.py:152-155): the STUDENT's pass takes the
                               hint as well -- its own warped images go through the producer and r(syn_f, target) joins the
                               student's per-pixel min (weight: consistency x matching x (1 - augmentation), unchanged).  With
                               or without MAL_STEP_TEMPORAL; the same three calls, the exchange through the *_s_* members:
                                 mal_loss_step_warp  also writes warp_s_m1 / warp_s_p1 (student's disparity, the teacher's poses);
                                                     mal_loss_step_student_ready before the student's producer reads them
                                 mal_loss_step_fwd   syn_s_* in, g_syn_s_* out (unnormalised, as g_syn_*)
                                 mal_loss_step_bwd   g_warp_s_* in: the student's gradient sweep takes the four-way decisions
                                                     of _fwd and adds what arrives through syn */
  MAL_STEP_SYN_S_SPARSE = 256, /* MAL_STEP_SYN_SPARSE for the student's pair (syn_s_* / syn_s_region / warp_s_*) */
  MAL_STEP_NO_MOTION_MASK = 1024, /* mal_loss_multiscale_* only: --disable_motion_masking (manydepth/trainer.py:1321-1323): the student's
                                  weight leaves the consistency mask out (no matching mask is formed either: consistency_mask_out
                                  is not written) */
  MAL_STEP_NO_AUG = 2048,      /* mal_loss_multiscale_* only: --no_matching_augmentation (:1324-1326): ... and (1 - augmentation_mask) */
  MAL_STEP_ENSEMBLE = 4096,    /* mal_loss_multiscale_* only: --ensemble on the non-distillation route (manydepth/trainer.py:1346-1351):
                                  + mean(|(depth_teacher.detach() + depth_student)/2 - depth_student| * mask) per scale for the student;
                                  losses[44 + s] */
  MAL_STEP_NO_SSIM = 512       /* mal_loss_multiscale_* only: --no_ssim, r = mean_c |target - pred| (manydepth/trainer.py:1217-1218 --
                                  upstream reads the flag on this, the non-distillation, route only); not with MAL_STEP_TEMPORAL */
};
typedef struct mal_step_args {
  int B, H, W;
  float min_depth, max_depth;
  int flags;
  float w_main, w_distil;
  const float *color0, *color_m1, *color_p1;      /* (B,3,H,W) */
  const float *K, *inv_K;                         /* (B,16) */
  const float *disp_teacher, *disp_student;       /* (B,1,H,W), full resolution */
  const float *axisangle_m1, *translation_m1, *axisangle_p1, *translation_p1; /* (B,3) */
  const float *consistency_mask;                  /* (B,H,W), before the matching mask */
  const float *augmentation_keep;                 /* (B): 1 - augmentation_mask (or the mask, MAL_STEP_AUG_MASK) */
  const float *lowest_cost;                       /* (B,H,W) */
  const float *noise;                             /* (B,1,H,W) N(0,1), nullable */
  float *losses;                                  /* 16 */
  float *loss_total;                              /* nullable: receives losses[8], the differentiable total */
  float *mono_reproj, *ens_reproj, *multi_reproj; /* (B,1,H,W) nullable outputs */
  float *consistency_mask_out;                    /* (B,H,W) nullable: mask * matching mask */
  const float *g_total;                           /* backward: device scalar d(final)/d(total), nullable = 1 */
  float *g_disp_teacher, *g_disp_student;         /* backward outputs, nullable */
  float *g_axisangle_m1, *g_translation_m1, *g_axisangle_p1, *g_translation_p1;
  void *ws; size_t ws_bytes; void *stream;
  /* Parity instrumentation (tests; NULL in production): the per-pixel DECISIONS the teacher / student pass took,
   * MAL_DEC_PLANES uint32 planes of B*H*W each -- what a CPU checker has to be told to reproduce the discontinuous
   * choices of loss_utils.py:103-113,178-199,237-254 instead of re-deciding near-ties.  Requesting them selects
   * instrumented instantiations of the same kernels (identical arithmetic); H, W < 4096.                       */
  uint32_t *dec_teacher, *dec_student;
  /* MAL_STEP_NOISE_PHILOX: key; step number = *noise_counter when noise_counter != NULL (a device word the step's
   * last kernel advances by one, so a replayed HIP graph draws fresh noise every replay), else noise_step;
   * noise_out: (B,1,H,W) nullable, receives the N(0,1) values that were used (tests). */
  uint64_t noise_seed, noise_step; uint64_t* noise_counter; float* noise_out;
  /* MAL_STEP_TEMPORAL, all (B,3,H,W) planar */
  float *warp_m1, *warp_p1;               /* out of mal_loss_step_warp: outputs[("color", f, 0)] of the teacher */
  const float *syn_m1, *syn_p1;           /* in of _fwd: outputs[("syn", f, 0)] */
  float *g_syn_m1, *g_syn_p1;             /* out of _fwd */
  const float *g_warp_m1, *g_warp_p1;     /* in of _bwd */
  int warp_sample_stride;                 /* floats between two samples of warp_m1 / warp_p1; 0 = 3*H*W.  6*H*W with
                                             warp_p1 = warp_m1 + 3*H*W lays the two images of a sample side by side --
                                             the (2,3,H,W) pair the instance segmenter is fed (dyn_utils.py:139-140) */
  float *warp2_m1, *warp2_p1;             /* nullable, contiguous (B,3,H,W): a second copy of the warped images, written by
                                             mal_loss_step_warp -- the buffers the producer makes syn_f in (it then only
                                             overwrites the pixels its instances touch, mal_dyn_item.prefilled)           */
  const uint8_t *syn_region;              /* nullable, (B,H,W) bytes, bit 0 = the producer touched this pixel (elsewhere
                                             syn_f == warp_f): mal_loss_step_fwd then evaluates the synthesised candidates
                                             only where their 3x3 window can differ -- an exact tie goes to the warped
                                             candidate anyway, torch.min takes the first minimum                          */
  float *g_syn_region_m1, *g_syn_region_p1; /* nullable (with syn_region), (B,3,H,W): g_syn_* once more, written only at
                                             touched pixels -- what a producer's in-place backward gathers from
                                             (mal_dyn_item.region_only) */
  /* --learn_ens (loss_utils.py:240-241, trainer.py:596-600), nullable: the learnt ensemble head's disparity (B,1,H,W).
   * The ensemble pass then warps with it instead of (disp_teacher + disp_student) / 2, its depth is the distillation
   * target where the ensemble wins the three-way min, and g_ens_disp (backward output, nullable) receives
   * d total / d ens_disp.  Not with MAL_STEP_NO_ENS. */
  const float *ens_disp; float *g_ens_disp;
  /* MAL_STEP_MAIN_TEMPORAL: the members above once more for the student's pass (same shapes; warp_s_* use warp_sample_stride) */
  float *warp_s_m1, *warp_s_p1;
  const float *syn_s_m1, *syn_s_p1;
  float *g_syn_s_m1, *g_syn_s_p1;
  const float *g_warp_s_m1, *g_warp_s_p1;
  const uint8_t *syn_s_region;
  float *g_syn_s_region_m1, *g_syn_s_region_p1;
} mal_step_args;
int mal_loss_step_warp(const mal_step_args* args);
/* A MAL_STEP_TEMPORAL step whose producer failed between mal_loss_step_warp and mal_loss_step_fwd: joins the ensemble
 * pass that _warp forked onto the library's side stream back into args->stream (no-op when nothing is pending), so the
 * next step cannot overwrite buffers that pass still reads and a stream capture does not end with unjoined work. */
int mal_loss_step_abort(const mal_step_args* args);
/* Option "tail_overlap" (mal_set_option; --temporal steps): call between the step's forward and the producer's backward.
 * *stream receives the stream the producer's backward is to be enqueued on: the library's side stream -- made to wait for
 * the fused sweep, the producer of d loss / d syn -- when the option applies, args->stream otherwise.  mal_loss_step_bwd
 * then runs the teacher's gradient sweep behind it on that stream (beside the epilogue and the reduction of the forward, which
 * args->stream may still be running) and joins it back in front of the assembly.  _cancel: the caller enqueued nothing there
 * after all (its producer is not one whose backward can be redirected); the side stream is joined back at once. */
int mal_loss_step_tail_begin(const mal_step_args* args, void** stream);
int mal_loss_step_tail_cancel(const mal_step_args* args);
/* --distil with --scales 0..sclm (sclm 1..3) and the temporal hint: generate_images_pred (manydepth/trainer.py:1088-1165) warps
 * the full-resolution sources once more per scale s > 0 with ("disp", s) upsampled (bilinear, align_corners=False) and calls
 * the producer on each; the losses read scale 0 only, and has_ins is the LAST call's answer.  mal_loss_step_warp_scales
 * enqueues those warps -- ONE forward-only launch for every hinted pass (teacher: MAL_STEP_TEMPORAL, student:
 * MAL_STEP_MAIN_TEMPORAL) and scale -- on args->stream; call it right after mal_loss_step_warp on the same args / ws (it reads
 * the camera block and texels of that call's first sweep), before the producers.  The producers' answers then go into
 * scale 0's exchange (has_ins of the last call decides whether syn_* join the min); nothing of scales > 0 reaches
 * mal_loss_step_fwd / _bwd, and their disparities receive no gradient.  MAL_EINVAL: sclm outside 1..3, no hinted pass, a NULL
 * disparity or warp of a hinted pass, one of a warp2 pair NULL; MAL_ESHAPE: H or W not divisible by 2**sclm -- all before any
 * device work. */
enum { MAL_MS_MAX_SCALES = 4 };  /* scales 0..3 (mal_step_scales_args, mal_ms_args) */
typedef struct mal_step_scales_args {
  int sclm;                                           /* 1..3; index [s] = scale s, [0] unused */
  const float *disp_teacher[MAL_MS_MAX_SCALES], *disp_student[MAL_MS_MAX_SCALES]; /* (B,1,H>>s,W>>s) */
  float *warp_m1[MAL_MS_MAX_SCALES], *warp_p1[MAL_MS_MAX_SCALES];       /* out: ("color", f, s) of the teacher, (B,3,H,W)
                                                                            planar, args->warp_sample_stride apart */
  float *warp_s_m1[MAL_MS_MAX_SCALES], *warp_s_p1[MAL_MS_MAX_SCALES];   /* ... of the student */
  float *warp2_m1[MAL_MS_MAX_SCALES], *warp2_p1[MAL_MS_MAX_SCALES];     /* nullable: contiguous (B,3,H,W) second copies */
  float *warp2_s_m1[MAL_MS_MAX_SCALES], *warp2_s_p1[MAL_MS_MAX_SCALES];
} mal_step_scales_args;
int mal_loss_step_warp_scales(const mal_step_args* args, const mal_step_scales_args* scales);
/* MAL_STEP_MAIN_TEMPORAL: call after mal_loss_step_warp (and after the teacher's producer, with MAL_STEP_TEMPORAL) and BEFORE the
 * student's producer reads warp_s_*: with both hints the student's forward pass runs on the library's side stream beside the
 * teacher's producer chain, and args->stream waits for it here (a no-op when the pass ran on args->stream itself). */
int mal_loss_step_student_ready(const mal_step_args* args);
/* Measurement hook (bench.py's `roofline` block): enqueues `launches` (1..4096) back-to-back launches of the teacher's
 * pass -- the fused warp + SSIM + L1 + min + automask forward+backward sweep, manydepth/loss_utils.py:57-113 with
 * trainer.py:1078-1125 -- exactly as mal_loss_step_fwd enqueues it for a step WITHOUT MAL_STEP_TEMPORAL (same parameter
 * block, instantiation and task decomposition) and nothing else.  `args->ws` must hold a finished mal_loss_step_fwd of
 * the same arguments; the launches rewrite what its teacher pass left with the same values.  Captured into a graph and
 * replayed, two events outside the graph time the kernel alone. */
int mal_loss_step_teacher_replay(const mal_step_args* args, int launches);
/* the same noise map on its own (tests; bit-identical to what the step draws for that seed / step) */
int mal_tiebreak_noise(uint64_t seed, uint64_t step, int B, int H, int W, float* out, void* stream);
enum {
  MAL_DEC_WIN = 0,     /* bits 0-1: winning candidate of the per-pixel min (0/1 = warped frame -1/+1, 2/3 = syn -1/+1);
                          bit 2: automask bit `min_c r_c <= identity + 1e-5*noise` (1 when the pass has no automask) */
  MAL_DEC_DISTIL = 1,  /* student: index of the distillation argmin (0 teacher, 1 ensemble, 2 student) */
  MAL_DEC_SMOOTH_X = 2,/* 1 + sign(d[y,x] - d[y,x+1]) of the smoothness term (layers.py:210-223), x < W-1 */
  MAL_DEC_SMOOTH_Y = 3,/* 1 + sign(d[y,x] - d[y+1,x]), y < H-1 */
  MAL_DEC_TAP0 = 4,    /* frame -1: x0 | y0 << 12 (floor of the clipped sampling position) | bit 24: x on/over the
                          border (grid gradient cut), bit 25: same for y */
  MAL_DEC_TAP1 = 5,    /* frame +1 */
  MAL_DEC_L1 = 6,      /* 1 + sign(pred - target) of the winning candidate's L1 term, channels r | g << 2 | b << 4 */
  MAL_DEC_PLANES = 7
};
size_t mal_step_workspace_bytes(int B, int H, int W);
int mal_loss_step_fwd(const mal_step_args* args);
int mal_loss_step_bwd(const mal_step_args* args);

/* ---- the loss half of process_batch WITHOUT --distil and with sclm > 0 (BASELINE.json configs[1] runs the four-scale
 * decoder): manydepth/trainer.py:573-612 calling compute_losses (:1248-1475) for the teacher and for the student over
 * scales 0..sclm, after generate_images_pred (:1078-1170) upsampled each scale's disparity to full resolution
 * (bilinear, align_corners=False) and warped the full-resolution sources with it.  Per scale s:
 *   teacher  reproj_s = sum(min_f r * automask) / (sum automask + 1e-7), identity term from the raw sources + 1e-5 noise_s
 *   student  mask m = consistency_mask (x matching mask, :592-593, when lowest_cost is given) x (1 - augmentation_mask);
 *            reproj_s over m;  consistency_s = mean |depth_student_s - depth_teacher_s| (1 - m)
 *   both     + 1e-3 * smooth(disp_s / mean disp_s, color_s) / 2**s        (disp_s, color_s at the scale's own size)
 * total = (sum_s loss_teacher_s + sum_s loss_student_s) / (sclm + 1).  One host call forward (first sweep, upsampling,
 * 2 marching launches + 2 smoothness sweeps per scale, one reduction), one backward (adjoint upsampling, gathered in a
 * fixed order: no atomics).  --v1_multiscale, --ensemble are not covered (MAL_EINVAL is not how they fail: the Python
 * mirror routes them through the operator-level API); --no_ssim: MAL_STEP_NO_SSIM; the temporal hint: MAL_STEP_TEMPORAL. */
typedef struct mal_ms_args {
  int B, H, W, sclm;                              /* scale s is (H >> s, W >> s); H, W divisible by 2**sclm */
  float min_depth, max_depth;
  int flags;                                      /* MAL_STEP_AUG_MASK, _NOISE_PHILOX, _TEMPORAL, _NO_SSIM, _NO_MOTION_MASK, _NO_AUG;
                                                     --disable_automasking: pass no noise (upstream compares against the identity
                                                     term even then, manydepth/trainer.py:1296-1311: only the noise goes) */
  const float *color0, *color_m1, *color_p1;      /* (B,3,H,W) */
  const float *color0_s[MAL_MS_MAX_SCALES];       /* inputs[("color",0,s)]: (B,3,H>>s,W>>s); [0] NULL = color0 */
  const float *K, *inv_K;                         /* (B,16) */
  const float *disp_teacher[MAL_MS_MAX_SCALES], *disp_student[MAL_MS_MAX_SCALES]; /* (B,1,H>>s,W>>s) */
  const float *axisangle_m1, *translation_m1, *axisangle_p1, *translation_p1;     /* (B,3) */
  const float *consistency_mask;                  /* (B,H,W) */
  const float *augmentation_keep;                 /* (B) */
  const float *lowest_cost;                       /* (B,H,W) nullable: no matching mask */
  const float *noise[MAL_MS_MAX_SCALES];          /* (B,1,H,W) each, all NULL with MAL_STEP_NOISE_PHILOX */
  uint64_t noise_seed, noise_step; uint64_t* noise_counter;
  float *losses;                                  /* 48: [net][scale][reproj, consistency, smooth, loss] (net 0 teacher),
                                                     [32] teacher total, [33] student total, [34] their sum,
                                                     [36+s] reproj student+teacher, [40+s] loss student+teacher,
                                                     [44+s] the student's ensemble term (MAL_STEP_ENSEMBLE, else 0) */
  float *loss_total;                              /* nullable: receives losses[34] */
  float *consistency_mask_out;                    /* (B,H,W) nullable */
  const float *g_total;                           /* backward: device scalar, nullable = 1 */
  float *g_disp_teacher[MAL_MS_MAX_SCALES], *g_disp_student[MAL_MS_MAX_SCALES];   /* backward outputs, nullable */
  float *g_axisangle_m1, *g_translation_m1, *g_axisangle_p1, *g_translation_p1;
  void *ws; size_t ws_bytes; void *stream;
  /* MAL_STEP_TEMPORAL in `flags` (--temporal on this path, trainer.py:1161-1162 + 1279-1283): generate_images_pred calls the
   * producer once PER SCALE on that scale's full-resolution warp of the teacher, and compute_losses adds r(syn_f^s, target)
   * to scale s's per-pixel min when the LAST call reported instances (has_ins is overwritten per scale, :1162).  Three calls
   * around the producers, as mal_loss_step_*: mal_loss_multiscale_warp (everything that does not wait for them: first
   * sweep, upsampling, the teacher's forward pass per scale -> warp_*[s], the student's passes, smoothness),
   * [syn^s = producer(warp^s)], mal_loss_multiscale_fwd (syn_*[s] in; losses, g_syn_*[s] out, unnormalised),
   * [g_warp^s = producer^T(g_syn^s)], mal_loss_multiscale_bwd (g_warp_*[s] in).  Members per scale s <= sclm, all (B,3,H,W)
   * planar, with the meaning of their mal_step_args namesakes; bit s of syn_sparse = MAL_STEP_SYN_SPARSE for scale s. */
  float *warp_m1[MAL_MS_MAX_SCALES], *warp_p1[MAL_MS_MAX_SCALES];
  const float *syn_m1[MAL_MS_MAX_SCALES], *syn_p1[MAL_MS_MAX_SCALES];
  float *g_syn_m1[MAL_MS_MAX_SCALES], *g_syn_p1[MAL_MS_MAX_SCALES];
  const float *g_warp_m1[MAL_MS_MAX_SCALES], *g_warp_p1[MAL_MS_MAX_SCALES];
  const uint8_t *syn_region[MAL_MS_MAX_SCALES];
  float *g_syn_region_m1[MAL_MS_MAX_SCALES], *g_syn_region_p1[MAL_MS_MAX_SCALES];
  int warp_sample_stride, syn_sparse;
  /* parity instrumentation (tests), per scale: the per-pixel decisions of that scale's gradient passes, as mal_step_args.
   * dec_teacher / dec_student (int32 (MAL_DEC_PLANES,B,H,W) each; MAL_DEC_WIN, _TAP0/1, _L1 are written -- the smoothness signs of
   * this path are those of the raw disparity differences at the scale's own size, which a checker forms from the inputs
   * exactly).  NULL (the default): the specialised, uninstrumented kernels run; results are bit-identical either way. */
  uint32_t *dec_teacher[MAL_MS_MAX_SCALES], *dec_student[MAL_MS_MAX_SCALES];
} mal_ms_args;
size_t mal_ms_workspace_bytes(int B, int H, int W, int sclm);
int mal_loss_multiscale_warp(const mal_ms_args* args); /* MAL_STEP_TEMPORAL only */
/* a MAL_STEP_TEMPORAL step whose producer failed between _warp and _fwd: joins the library's side stream (the students' passes
 * run there beside the producers) back into args->stream; a no-op when nothing is pending */
int mal_loss_multiscale_abort(const mal_ms_args* args);
int mal_loss_multiscale_fwd(const mal_ms_args* args);
int mal_loss_multiscale_bwd(const mal_ms_args* args);
/* ---- DualRefine's loss loops over the deq iterations of scale 0 in one call per direction ------------------------------
 * dualrefine/trainer.py:395-451 (generate_images_pred, Project3D convention B + align_corners=False) and :530-633
 * (compute_losses, the per-deq-iteration branch).  Per iteration it = 0..n_iters-1:
 *   reproj_it = sum(min_f r(warp_f) * mask) / (sum mask + 1e-7),  mask = automask(identity term + 1e-5 noise_it)
 *               [x consistency_mask for it > 0, :593-597]
 *   consistency_it = mean |depth_it - depth_0| (1 - mask)  for it > 0 (no gradient to depth_0, :606-618)
 *   loss_it = reproj_it + consistency_it + smooth_weight * smooth(disp_it / mean disp_it, color)
 * and upstream's running loss is added to the total once per iteration (:624-631): total = sum_it (n_iters - it) loss_it.
 * T_m1[it] / T_p1[it] are the 4x4 poses the trainer selects for that iteration (:420-435: the refined pose for frame -1
 * and it > 0, ...); which of them are detached is the caller's business: a NULL g_T_* output is a detached pose.
 * losses: [4*it + {0 reproj, 1 consistency, 2 smooth, 3 running loss after it}], [4*MAL_DR_MAX_ITERS] total,
 * [4*MAL_DR_MAX_ITERS + 1] the final running loss (what every "loss/0_it" entry reads upstream).
 * One call = the iterations of ONE scale (`scale`, below); --avg_reprojection / --no_ssim: MAL_DR_AVG / MAL_DR_NO_SSIM.
 * MAL_DR_POSE_UPDATE (scale 0 only): the same call also evaluates the pose-update losses (:457-480 pose_update_generate_images_pred,
 * :699-767 compute_pose_update_losses) in ONE more marching pass whose two candidates are warped with two different
 * disparities: frame -1 with pu_disp_m1 (the last iteration's disparity -- or iteration 0's, detached, with --Tstar_D0_pair)
 * under the refined pose pu_T_m1 = ("cam_T_cam", 0, -1, 1); frame +1 as ("color", 1, 0, 0) was: pu_disp_p1 = iteration 0's
 * disparity under pu_T_p1 = ("cam_T_cam", 0, 1).  min (or mean) over the two, automask against the identity term + 1e-5 pu_noise,
 * no consistency mask, no smoothness: losses[4*MAL_DR_MAX_ITERS + 2] = sum(rp mask) / (sum mask + 1e-7).  It is NOT part of
 * losses[4*MAL_DR_MAX_ITERS] / loss_total (upstream adds it after the division by len(scales), :337-343): the caller adds it,
 * and hands its cotangent in g_pu_total. */
enum { MAL_DR_MAX_ITERS = 4 };
enum { MAL_DR_AVG = 8,      /* --avg_reprojection (dualrefine/trainer.py:569-583): the MEAN over the two frames of r and of the
                               identity term instead of their min; both frames take half of every gradient */
       MAL_DR_NO_SSIM = 16, /* --no_ssim (:493-494): r = mean_c |target - pred| */
       MAL_DR_NO_AUTOMASK = 1, MAL_DR_NO_MOTION_MASK = 2,
       MAL_DR_NOISE_PHILOX = 4, /* the tie-break noise of every iteration is drawn in the step's first launch (Philox4x32-10
                                  keyed by noise_seed, step number = step * MAL_DR_MAX_ITERS + it: mal_tiebreak_noise with
                                  that step number reproduces iteration it's map); every noise[it] must be NULL.  The
                                  pose-update pass's map: key noise_seed ^ MAL_DR_POSE_NOISE_KEY, step number step * MAL_DR_MAX_ITERS */
       MAL_DR_POSE_UPDATE = 32 /* the pose-update losses ride on this call (see above) */ };
#define MAL_DR_POSE_NOISE_KEY 0x706f73655f757064ull /* "pose_upd" */
typedef struct mal_dr_args {
  int B, H, W, n_iters;
  float min_depth, max_depth, smooth_weight;
  int flags;
  const float *color0, *color_m1, *color_p1;      /* (B,3,H,W) */
  const float *K, *inv_K;                         /* (B,16) */
  const float *disp[MAL_DR_MAX_ITERS];            /* (B,1,H,W) */
  const float *T_m1[MAL_DR_MAX_ITERS], *T_p1[MAL_DR_MAX_ITERS]; /* (B,16) */
  const float *consistency_mask;                  /* (B,H,W); required when n_iters > 1 unless MAL_DR_NO_MOTION_MASK */
  const float *noise[MAL_DR_MAX_ITERS];           /* (B,1,H,W) N(0,1) per iteration, nullable */
  /* MAL_DR_NOISE_PHILOX: key; step = *noise_counter when noise_counter != NULL (a device word the step's last kernel
   * advances by one, so a replayed HIP graph draws fresh noise every replay), else noise_step */
  uint64_t noise_seed, noise_step; uint64_t* noise_counter;
  float *losses;                                  /* 4*MAL_DR_MAX_ITERS + 4 */
  float *loss_total;                              /* nullable: receives the total */
  const float *g_total;                           /* backward: device scalar, nullable = 1 */
  float *g_disp[MAL_DR_MAX_ITERS];                /* backward outputs, nullable each */
  float *g_T_m1[MAL_DR_MAX_ITERS], *g_T_p1[MAL_DR_MAX_ITERS];
  void *ws; size_t ws_bytes; void *stream;
  /* One call covers the iterations of ONE scale of opt.scales (upstream's default list is [0,1,2,3]: scale 0 and 2 with
   * n_losses+1 iterations, scale 1 skipped, scale 3 iteration 0 only, dualrefine/trainer.py:403-407,536-547; the caller sums
   * the calls' totals and divides by len(scales), :694).  scale > 0: disp[it] is the iteration's disparity UPSAMPLED to
   * (H,W) (trainer.py:411-412; mal_upsample_bilinear) -- what is warped and what the consistency term reads --, while the
   * smoothness term (:620-624) is taken on disp_lo[it], (B,1,H>>scale,W>>scale), against color0_s = inputs[("color",0,scale)],
   * (B,3,H>>scale,W>>scale); pass smooth_weight = disparity_smoothness / 2**scale.  Backward then writes g_disp[it] =
   * d total / d (upsampled disparity) WITHOUT the smoothness term and g_disp_lo[it] = the smoothness term's gradient at the
   * scale's own size (the caller adds the adjoint upsampling of the first: mal_upsample_bilinear_adjoint). */
  int scale;
  const float *color0_s;
  const float *disp_lo[MAL_DR_MAX_ITERS];
  float *g_disp_lo[MAL_DR_MAX_ITERS];
  /* nullable: the workspace of an earlier mal_dr_loss_fwd call of the SAME step (same images, B, H, W, flags) -- the texel
   * copies of the three images and the identity term are taken from it instead of being formed again (a step over several
   * scales packs once).  Honoured when this call's smoothness term does not ride on that sweep (scale > 0 or n_iters > 2). */
  const void *texels_from;
  /* parity instrumentation (tests), per iteration: the per-pixel decisions of that iteration's pass, as mal_step_args.dec_teacher
   * (int32 (MAL_DEC_PLANES,B,H,W); MAL_DEC_WIN, _TAP0/1, _L1).  NULL: the uninstrumented kernels; bit-identical results. */
  uint32_t *dec[MAL_DR_MAX_ITERS];
  /* MAL_DR_POSE_UPDATE */
  const float *pu_disp_m1, *pu_disp_p1;           /* (B,1,H,W) */
  const float *pu_T_m1, *pu_T_p1;                 /* (B,16) */
  const float *pu_noise;                          /* (B,1,H,W) N(0,1), nullable; must be NULL with MAL_DR_NOISE_PHILOX */
  const float *g_pu_total;                        /* backward: device scalar, nullable = 1 */
  float *g_pu_disp_m1, *g_pu_disp_p1;             /* backward outputs, nullable each (a NULL output is a detached operand) */
  float *g_pu_T_m1, *g_pu_T_p1;
  uint32_t *pu_dec;                               /* parity instrumentation, as dec[] */
  float *pu_loss_total;                           /* nullable: receives the pose-update loss (= losses[4*MAL_DR_MAX_ITERS + 2]) */
  /* An operand of the pose-update pass that IS an iteration's operand (upstream's default pairing: pu_disp_m1 = disp[n_iters-1],
   * pu_disp_p1 = disp[0], pu_T_m1 = T_m1[n_iters-1], pu_T_p1 = T_p1[0]) can have its pose-update gradient ADDED into that
   * iteration's output by the assembly launch instead of leaving as an output of its own that the caller then adds:
   * k + 1 = "add into iteration k's g_disp / g_T_m1 / g_T_p1" (the matching g_pu_* must then be NULL), 0 = separate output. */
  int pu_disp_m1_into, pu_disp_p1_into, pu_T_m1_into, pu_T_p1_into;
} mal_dr_args;
size_t mal_dr_workspace_bytes(int B, int H, int W, int n_iters);
int mal_dr_loss_fwd(const mal_dr_args* args);
int mal_dr_loss_bwd(const mal_dr_args* args);

/* F.interpolate(x, [H, W], mode="bilinear", align_corners=False) of a (B,1,h,w) map and its adjoint (a gather in a
 * fixed order), as the step uses them (tests) */
int mal_upsample_bilinear(const float* x, int B, int h, int w, int H, int W, float* out, void* stream);
int mal_upsample_bilinear_adjoint(const float* g_out, int B, int h, int w, int H, int W, float* g_x, void* stream);

/* ---- the glue between two convolutions of the depth decoder (mal_amd/networks.py DepthDecoder) as ONE pass each way:
 * F.pad(cat([interpolate(F.elu(x), scale_factor=up, mode="nearest"), skip], 1), (1,1,1,1), mode="reflect") and its adjoint.
 * x (B,C,h,w); skip (B,Cs,up*h,up*w), nullable when Cs = 0; out and g_out (B,C+Cs,up*h+2,up*w+2).  up in {1,2}, elu in
 * {0,1} (0: no activation).  The adjoint is a gather in a fixed order (mal_amd/csrc/mal_glue.hip states it; no atomics,
 * no zero fill); it reads x only with elu = 1 (a' = x > 0 ? 1 : expm1f(x) + 1), and a NULL gx or gskip is not computed.
 * MAL_EINVAL: a null required pointer, up/elu out of range, B, C, h or w < 1, Cs < 0, Cs > 0 without skip, up*h < 2 or
 * up*w < 2 (reflection needs two rows), or a padded tensor of 2^31 elements or more (32-bit indices).
 * The planning function is pure host code with the same shape checks: the workgroups the forward launches for that shape,
 * those of the adjoint that computes gx (need_x) and/or gskip (need_skip; ignored with Cs = 0; neither: 0 blocks, no
 * launch), and the floats of the flat output one workgroup covers per sweep.  Both entry points take their grids from it;
 * a grid that covers less than the output is strided over.  Every output pointer is nullable. */
int mal_decoder_join_plan(int B, int C, int Cs, int h, int w, int up, int need_x, int need_skip, int* blocks_fwd,
                          int* blocks_bwd, int* floats_per_block);
int mal_decoder_join_fwd(const float* x, const float* skip, float* out, int B, int C, int Cs, int h, int w, int up, int elu,
                         void* stream);
int mal_decoder_join_bwd(const float* g_out, const float* x, float* gx, float* gskip, int B, int C, int Cs, int h, int w,
                         int up, int elu, void* stream);

/* ---- the glue behind a ResNet convolution (mal_amd/networks.py BasicBlock, the encoders' stems) as TWO launches each way:
 * nn.BatchNorm2d -> (+ residual) -> (ReLU), y = relu(gamma * (x - mean) * invstd + beta + residual), and its adjoint.
 * x, residual (nullable), y, g_out, dx, dr (B,C,H,W) fp32 contiguous; gamma, beta, running_*, dgamma, dbeta (C) fp32;
 * save_mean, save_invstd (C) fp64: the batch statistics stay fp64 from the first element to the last use, and every
 * per-element expression is evaluated in fp64 on the fp32 operands and rounded once.
 * training = 1: batch statistics (biased variance for y, save_mean and save_invstd = 1/sqrt(var + eps) written), and the
 * module's side effects on the device: running_mean = (1-momentum)*running_mean + momentum*mean, running_var likewise with
 * the UNBIASED variance, *num_batches_tracked += 1.  training = 0: mean = running_mean, invstd = 1/sqrt(running_var + eps),
 * nothing but y is written (num_batches_tracked, save_*, ws may be NULL).  The statistics pass writes per-(channel, block)
 * partials (n, mean, M2) to ws and the apply pass combines them in a fixed order (Chan's formula, fp64; no atomics:
 * mal_amd/csrc/mal_bn.hip states the order), so equal inputs give equal bits.
 * The adjoint (training statistics only): g' = relu ? g_out * [y > 0] : g_out on the saved OUTPUT y (read only with relu = 1),
 * dbeta = sum g', dgamma = sum g' * xh, dx = gamma*invstd*(g' - dbeta/N - xh*dgamma/N), dr = g'; each of dx, dr, dgamma, dbeta
 * is nullable and a NULL one is neither computed nor written (all four NULL: MAL_OK, no launch); with dx, dgamma and dbeta all
 * NULL nothing is reduced and ws may be NULL.
 * The planning function is pure host code: blocks per channel (a function of N = B*H*W: the largest power of two <= 32 that
 * leaves each block 2048 elements) and the workspace both directions need for that shape; either output pointer nullable.
 * MAL_EINVAL: a null required pointer, B, C, H or W < 1, a tensor of 2^31 elements or more (32-bit offsets), training or relu
 * outside {0,1}, eps negative or not finite, momentum outside [0,1], N < 2 where batch statistics are taken (training forward;
 * a backward that reduces).  MAL_EWORKSPACE: ws_bytes below what the planning function returns. */
int mal_bn_join_plan(int B, int C, int H, int W, int* blocks_per_channel, size_t* ws_bytes);
int mal_bn_join_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, int64_t* num_batches_tracked, float* y, double* save_mean, double* save_invstd, int B,
                    int C, int H, int W, double eps, double momentum, int training, int relu, void* ws, size_t ws_bytes,
                    void* stream);
int mal_bn_join_bwd(const float* g_out, const float* x, const float* y, const float* gamma, const double* save_mean,
                    const double* save_invstd, float* dx, float* dr, float* dgamma, float* dbeta, int B, int C, int H, int W,
                    int relu, void* ws, size_t ws_bytes, void* stream);

/* ---- the max-pool behind a ResNet stem (mal_amd/networks.py: the three encoders) as ONE launch each way:
 * p = F.max_pool2d(y, kernel_size=3, stride=2, padding=1) and its adjoint.  y, g_y, dy (B,C,H,W) fp32 contiguous; p, g_p
 * (B,C,OH,OW) fp32 and code (B,C,OH,OW) bytes, OH = (H-1)/2 + 1, OW = (W-1)/2 + 1.
 * The winner of a window is ATen's: row-major over the window clipped to the plane, starting from -inf and the window's first
 * element, a value replaces the running maximum when val > max || isnan(val) (the first of equal maxima wins; a NaN wins and
 * a later NaN replaces it; a window of all -inf keeps its first element).  code, when not NULL, receives the winner's
 * position in the UNCLIPPED window, kh*3 + kw in 0..8; with code NULL (no gradient wanted) only p is written.
 * The adjoint is a gather over the codes: dy[h,w] = g_y[h,w] (+0 with g_y NULL: the cotangent that reaches y from its other
 * consumer) plus g_p of each of the at most four windows whose code points at (h,w), added in ascending (oh, ow) -- a fixed
 * order, no atomics, no zero fill, no read of y, no workspace; equal inputs give equal bits on either route.
 * Routes: 4 outputs per thread forward when W % 8 == 0, y and p are 16-byte and code 4-byte aligned; 4 elements of dy per
 * thread backward when W % 4 == 0, g_p, g_y and dy are 16-byte and code 4-byte aligned; one per thread otherwise.
 * The planning function is pure host code with the same shape checks: the output size, the workgroups of either launch
 * (256 threads; at most 2048, a larger tensor is strided over) and what a thread owns (4 or 1), for pointers that are
 * (aligned = 1) or are not (0) aligned as above; every output pointer is nullable.
 * MAL_EINVAL: a null required pointer (y, p; g_p, code, dy), B, C, H or W < 1, or y of 2^31 elements or more (32-bit offsets). */
int mal_stem_pool_plan(int B, int C, int H, int W, int aligned, int* OH, int* OW, int* blocks_fwd, int* blocks_bwd,
                       int* per_thread_fwd, int* per_thread_bwd);
int mal_stem_pool_fwd(const float* y, float* p, uint8_t* code, int B, int C, int H, int W, void* stream);
int mal_stem_pool_bwd(const float* g_p, const float* g_y, const uint8_t* code, float* dy, int B, int C, int H, int W,
                      void* stream);

/* ---- torch.optim.Adam's update (plain Adam: no weight decay, no amsgrad, no maximize) over a flat gradient buffer as ONE
 * launch (mal_amd/optim.py: FlatAdam).  The parameters stay where they are: `table` is a DEVICE array of n_chunks entries, one
 * per parameter tensor (fp32, contiguous): where it lives, the offset of its gradient in `grad` -- and of its moments in
 * exp_avg / exp_avg_sq, flat buffers of flat_elements floats each with the same offsets -- and its element count.  A call
 * updates the entries [first, first + count) (count 0: MAL_OK, no launch); range_elements, the sum of their counts, sizes the
 * grid and nothing else.  Per element, fp32, every operator one correctly rounded operation, no fused multiply-add, ATen's order:
 *   m' = m + (g - m) * c1;  v' = v * beta2 + (c2 * g) * g;  den = sqrt(v') / bs + eps;  p' = p + a * (m' / den)
 * with c1 = 1 - beta1, c2 = 1 - beta2, bs = sqrt(1 - beta2^t), a = -lr / (1 - beta1^t) formed by the caller in double and
 * rounded once.  t (the step number, >= 1) is checked, not used.  zero_grad != 0: each gradient element is overwritten with
 * +0 after it was read.  16-byte accesses with the flat side on the 16-byte grid, the 0..3 elements in front of and behind
 * them one by one; nothing outside a chunk is read or written, and an entry with a null pointer or with offset + count >
 * flat_elements is skipped.  No atomics: bit-reproducible, and any split into consecutive ranges gives the same bits.
 * The planning function is pure host code: the workgroups (at most 2048, tile T of the range belongs to workgroup T % blocks)
 * and threads of the launch for a range of n_chunks entries with total_elements elements, the elements of a tile (2048: a
 * chunk's tile 0 also owns its head and tail), the entries staged in LDS at a time and sizeof(mal_adam_chunk); every output
 * pointer is nullable.
 * MAL_EINVAL: a null pointer; a table off the 8-byte or a flat buffer off the 4-byte grid; n_chunks < 1; a range outside the
 * table; flat_elements < 1 or a total of 2^31 elements or more (32-bit offsets); range_elements < 0 or > flat_elements;
 * t < 1; bs not finite or not positive.  All checked before any HIP call. */
typedef struct mal_adam_chunk {
  float* param;      /* the parameter tensor's storage */
  uint32_t offset;   /* of its gradient and moments in the flat buffers, in elements */
  uint32_t count;    /* elements */
} mal_adam_chunk;
int mal_adam_plan(int n_chunks, long long total_elements, int* blocks, int* threads, int* tile_elements, int* table_window,
                  int* chunk_bytes);
int mal_adam_flat(const mal_adam_chunk* table, int n_chunks, int first, int count, long long range_elements, float* grad,
                  float* exp_avg, float* exp_avg_sq, long long flat_elements, int t, float c1, float beta2, float c2, float bs,
                  float eps, float a, int zero_grad, void* stream);

/* ---- N2: the temporal-hint producer's per-sample arithmetic, manydepth/dyn_utils.py:6-119 --------
 * (fill_dynamic_obj + generate_dynamic_instance), given the matched instance masks of the two warped frames
 * (num,H,W as bytes, non-zero = set; Mask2Former stays outside, the matcher is mal_match below).  Per instance the displacement
 * is half the larger-magnitude difference of the bounding-box edges between the frames (rows: low/top, columns:
 * right/left; index 0 is invisible to the extents, as upstream; half-to-even; replace=1 zeroes |d| < 3); "last"
 * patches move by +d, "next" by -d, overlapping copies add, pixels vacated by an instance show the other frame.
 * Outputs: ori_last / ori_next (C,H,W) = the reference's return values; delta [num][2] (row, column) and
 * flags [H*W] are what mal_dyn_instance_bwd needs.  C <= 4, num <= MAL_MAX_INSTANCES.                     */
size_t mal_dyn_workspace_bytes(int num);
int mal_dyn_instance_fwd(const uint8_t* mask_last, const uint8_t* mask_next, int num, const float* img_last,
                         const float* img_next, int C, int H, int W, int replace, float* ori_last, float* ori_next,
                         int32_t* delta, uint8_t* flags, void* ws, size_t ws_bytes, void* stream);
/* cotangents of (ori_last, ori_next) -> gradients w.r.t. (img_last, img_next), either nullable */
int mal_dyn_instance_bwd(const uint8_t* mask_last, const uint8_t* mask_next, int num, const int32_t* delta,
                         const uint8_t* flags, const float* g_ori_last, const float* g_ori_next, int C, int H, int W,
                         float* g_img_last, float* g_img_next, void* stream);

/* The same for several samples of a batch in one call (three launches forward, one backward for up to 16 samples; more
 * are chunked): one item per sample with matched instances; the fields are the arguments of the two functions above. */
typedef struct mal_dyn_item {
  const uint8_t* mask_last; const uint8_t* mask_next; int num;
  const float* img_last; const float* img_next;  /* forward in */
  float* ori_last; float* ori_next;              /* forward out */
  int32_t* delta; uint8_t* flags;                /* forward out, backward in */
  void* ws; size_t ws_bytes;                     /* forward scratch: mal_dyn_workspace_bytes(num) */
  const float* g_ori_last; const float* g_ori_next; float* g_img_last; float* g_img_next;  /* backward */
  /* optional: instance i is row idx_last[i] / idx_next[i] (device int64) of mask_last / mask_next -- the matcher's
   * selection (dyn_utils.py:147-150) applied inside the kernels instead of by a gather per sample and frame; NULL = row i */
  const int64_t* idx_last; const int64_t* idx_next;
  /* forward: ori_last / ori_next already hold img_last / img_next (the step's warp pass wrote both copies): only the pixels
   * of the instances' region are written */
  int prefilled;
  /* backward IN PLACE (g_img_* == g_ori_*: the cotangent buffers become the gradients): only region pixels change; they
   * are formed in g_tmp_* (C,H,W scratch, contents irrelevant) by one launch and moved by a second */
  float* g_tmp_last; float* g_tmp_next;
  /* backward, third form: g_ori_* are SNAPSHOTS valid at region pixels only (mal_step_args.g_syn_region_*), g_img_* the
   * buffers that hold the cotangent everywhere: one launch writes the region pixels of g_img_* (no scratch, no move) */
  int region_only;
  /* rows of mask_last / mask_next (0 = unknown): with them a selection idx_*[i] outside [0, rows) is clamped into the
   * tensor instead of being dereferenced (the torch indexing it replaces raised IndexError) */
  int n_last, n_next;
} mal_dyn_item;
int mal_dyn_batch_fwd(const mal_dyn_item* items, int n_items, int C, int H, int W, int replace, void* stream);
int mal_dyn_batch_bwd(const mal_dyn_item* items, int n_items, int C, int H, int W, void* stream);

/* ---- N2, the matcher: HungarianMatcher.memory_efficient_forward, manydepth/matcher.py:89-173 --------------------------
 * Instances of the two warped frames (n, m) against the confident instances of the target frame (0): masks (num,H,W) as
 * bytes (MAL_MATCH_U8: bool / uint8, non-zero = set) or float32 (MAL_MATCH_F32: BINARY floats, as Mask2Former emits them,
 * mask2former/maskformer_model.py:371), classes int64.  C1 (n_n,n_0) / C2 (n_m,n_0) fp32 =
 *   cost_class [class differs] + cost_dice (1 - (2 sum sigmoid(a) t + 1) / (sum sigmoid(a) + sum t + 1))
 * formed in fp64 from integer pixel counts (sigmoid(1) as torch's fp32 sigmoid gives it) and rounded once; cost_mask is
 * accepted and unused, as upstream (:121-122,130), but all three zero is refused (:86).  Each matrix is solved as a
 * rectangular linear assignment (min(rows, columns) pairs, fp64, shortest augmenting paths: what scipy runs); every
 * target column j assigned in both problems yields one pair slice_n[k] = row_n(j), slice_m[k] = row_m(j), in ASCENDING j
 * (upstream: CPython's iteration order of a set).  slice_n / slice_m: MAL_MATCH_MAX int64 each; result: 4 int32 =
 * count, non-binary (1 if a float32 mask element is neither 0 nor 1: upstream's sigmoid of it has no integer form and
 * the outputs are not to be used), 0, 0.  An empty side gives count 0.  Three launches and a 16-byte memset on `stream`;
 * no atomics, bit-reproducible.  ws: mal_match_workspace_bytes.  Sizes beyond MAL_MATCH_MAX are MAL_EINVAL. */
enum { MAL_MATCH_U8 = 0, MAL_MATCH_F32 = 1 };
typedef struct mal_match_args {
  const void* masks_n; const void* masks_m; const void* masks_0;  /* nullable where the count is 0 */
  int kind_n, kind_m, kind_0;                                     /* MAL_MATCH_U8 / MAL_MATCH_F32 */
  int n_n, n_m, n_0, H, W;
  const int64_t* class_n; const int64_t* class_m; const int64_t* class_0;
  double cost_class, cost_mask, cost_dice;
  float* C1; float* C2;                 /* out */
  int64_t* slice_n; int64_t* slice_m;   /* out: the first `count` of MAL_MATCH_MAX slots */
  int32_t* result;                      /* out: count, non-binary, 0, 0 */
  void* ws; size_t ws_bytes;
  void* stream;
} mal_match_args;
size_t mal_match_workspace_bytes(int n_n, int n_m, int n_0, int H, int W); /* 0 for sizes mal_match refuses */
int mal_match(const mal_match_args* args);

/* ---- N2, the segmenter's tail: Mask2Former's instance inference, mask2former/maskformer_model.py:219-227 + :344-380 ----
 * pred_logits (N,Q,K+1) and pred_masks (N,Q,h,w) fp32 as the network returns them -> per image the `topk` best (query,
 * class) pairs with their full-size BINARY masks as bytes, what mal_match and mal_dyn_batch_* read.  No float plane is
 * written.  Output size (H,W): 4(h-1) < H <= 4h and likewise W, the crop of the x4 plane to the image (upstream pads its
 * input to a multiple of 32 and the mask features sit at stride 4, so F.interpolate(mode="bilinear", align_corners=False)
 * is always exactly x4 there); any other size is MAL_EINVAL.
 * Selection: p = softmax over the K+1 logits of a query (fp64 inside, rounded once to fp32), last column dropped; the
 * topk largest of the Q*K values in DESCENDING p, ties by ASCENDING flat index q*K + c (upstream's topk(sorted=False)
 * leaves the order open); then the optional thing filter (thing[c] != 0 keeps class c, :360-367), survivors compacted
 * in order -> count[n] slots.  The same query may fill several slots; each slot has its own mask.
 * Masks: v = x4 bilinear value (ATen's rule: source = max((o + 0.5)/4 - 0.5, 0), neighbour clamped), byte = v > 0.
 * mask_score = float(sum of sigmoid(v) over the set pixels, fp64 partials in a fixed order) / (float(set pixels) + 1e-6f),
 * 0 for an empty mask; score = cls_score * mask_score (fp32).  Slots from count[n] on: classes 0, query -1, scores 0,
 * masks not written.  Bounds: 1 <= topk <= min(Q*K, MAL_MATCH_MAX), Q*K <= MAL_INSTANCES_MAX_QK, K+1 <=
 * MAL_INSTANCES_MAX_K1, N <= MAL_INSTANCES_MAX_N, h*w <= 2^24.  Three launches on `stream`; no allocation, no readback, no
 * float atomics, bit-reproducible.  ws: mal_instances_workspace_bytes. */
typedef struct mal_instances_args {
  const float* pred_logits;  /* (N,Q,K+1) */
  const float* pred_masks;   /* (N,Q,h,w) */
  const uint8_t* thing;      /* K bytes, nullable: keep every class */
  int N, Q, K, h, w, H, W, topk;
  int32_t* count;            /* out (N) */
  uint8_t* masks;            /* out (N,topk,H,W), 0 or 1 */
  float* scores;             /* out (N,topk) */
  int64_t* classes;          /* out (N,topk) */
  int32_t* query;            /* out (N,topk) */
  float* cls_score;          /* out (N,topk) */
  float* mask_score;         /* out (N,topk) */
  void* ws; size_t ws_bytes;
  void* stream;
} mal_instances_args;
size_t mal_instances_workspace_bytes(int N, int Q, int K, int h, int w, int H, int W, int topk); /* 0 for sizes mal_instances refuses */
int mal_instances(const mal_instances_args* args);

/* ---- N2, inside the segmenter: multi-scale deformable attention, FORWARD ONLY (the segmenter is frozen and runs under
 * no_grad: manydepth/trainer.py:354, manydepth/dyn_utils.py:185-186).  The operator of Mask2Former's pixel decoder,
 * mask2former/modeling/pixel_decoder/ops, whose upstream extension is CUDA-only.  All tensors fp32, contiguous, upstream's
 * layouts.  Per (n, q, m):  out = sum_l sum_p w * bilinear(value_l, x * W_l - 0.5, y * H_l - 0.5), zero padding,
 * align_corners=False: the arithmetic of ms_deformable_im2col_gpu_kernel (ops/src/cuda/ms_deform_im2col_cuda.cuh:242-304),
 * the function ms_deform_attn_core_pytorch (ops/functions/ms_deform_attn_func.py:52-72) computes.  A sample counts only when
 * y > -1 && x > -1 && y < H && x < W; every range test is made in float before any conversion to an index, so NaN and
 * infinite locations contribute zero.
 * mal_msda_fwd: sampling_locations (N,Lq,M,L,P,2) in (x, y) order and attention_weights (N,Lq,M,L,P) as given;
 * reference_points and ref_dim are not read.
 * mal_msda_fused_fwd: the module's default route (ops/modules/ms_deform_attn.py:102-112).  sampling_locations holds the
 * raw OFFSETS (N,Lq,M,L,P,2) and attention_weights the raw LOGITS (N,Lq,M,L*P) of the two linear layers; the kernel takes
 * the max-subtracted softmax over L*P and forms the locations from reference_points (N,Lq,L,ref_dim): ref_dim 2:
 * ref + off / (W_l, H_l); ref_dim 4: ref[:2] + off / P * ref[2:] * 0.5 -- in torch's roundings (true divisions, no fma).
 * spatial_shapes and level_start_index are DEVICE arrays read by the kernel (no readback: the call can be captured in a
 * graph).  A level is used only if 1 <= H_l, W_l <= min(S, 2^24), level_start_index[l] >= 0 and level_start_index[l] +
 * H_l W_l <= S; any other level contributes zero and reads nothing.
 * Bounds: 1 <= L <= MAL_MSDA_MAX_L, 1 <= P <= MAL_MSDA_MAX_P, L*P <= MAL_MSDA_MAX_LP, 1 <= D <= MAL_MSDA_MAX_D, M >= 1,
 * N, S, Lq >= 1, ref_dim 2 or 4 (fused), and value, out and sampling_locations below 2^31 elements each; anything else is
 * MAL_ESHAPE.  A null args or a null required pointer is MAL_EINVAL (checked first, before any HIP call).  float4 loads and
 * stores when D % 4 == 0 and value and out are 16-byte aligned, one channel per lane otherwise.  One launch on `stream`; no
 * workspace, no allocation, no atomics, bit-reproducible.
 * The planning function is pure host code with the same shape checks (MAL_ESHAPE for exactly the shapes both entry points
 * refuse; ref_dim is not a shape): for value and out that are (aligned = 1) or are not (0) on the 16-byte grid, the channels
 * a lane owns (4 or 1), the rows (n, q, m) a workgroup of 256 threads owns -- 256 / (D / vec), at most 4096 / (3 L P + 1) by
 * the LDS budget, at most N Lq M --, the workgroups of the launch and its dynamic LDS bytes.  Both entry points take their
 * launch from it; every output pointer is nullable. */
typedef struct mal_msda_args {
  const float* value;               /* (N,S,M,D) */
  const int64_t* spatial_shapes;    /* device (L,2): H_l, W_l */
  const int64_t* level_start_index; /* device (L) */
  const float* sampling_locations;  /* (N,Lq,M,L,P,2); fused: the offsets */
  const float* attention_weights;   /* (N,Lq,M,L,P);   fused: the logits */
  const float* reference_points;    /* fused only: (N,Lq,L,ref_dim) */
  int N, S, M, D, L, P, Lq, ref_dim;
  float* out;                       /* (N,Lq,M*D) */
  void* stream;
} mal_msda_args;
int mal_msda_plan(int N, int S, int Lq, int M, int D, int L, int P, int aligned, int* vec, int* rows, int* blocks,
                  size_t* lds_bytes);
int mal_msda_fwd(const mal_msda_args* args);
int mal_msda_fused_fwd(const mal_msda_args* args);

/* ---- N2b: DynamicDepth's occlusion-aware forward warp, FORWARD ONLY (upstream calls it under torch.no_grad():
 * dynamicdepth/trainer.py:494,502,517,525 and :825,840): dynamicdepth/rigid_warp.py:534-597, whose z-buffer upstream takes
 * from torch_sparse's CUDA-only coalesce.  All float tensors fp32 and contiguous.
 * Stage 1 (splat): every pixel of depth (B,H,W) is cut into upscale^2 sub-points that share its depth (nearest upsampling =
 * integer division of the sub-point's coordinates); each is back-projected with inverse(K_u) (K_u: the first two rows of K
 * times upscale), moved by pose[q] (B,3,4), divided by max(Z, 1e-3) and projected with the unscaled K; the coordinates are
 * TRUNCATED to a cell, and a cell keeps the largest 1/Z it receives.  A sub-point counts iff x > -1 && x < W && y > -1 &&
 * y < H, tested in float before any conversion (coordinates in (-1, 0) belong to cell 0; NaN and +-inf count nowhere).  The
 * z-buffer is a plane of the bit patterns of 1/Z updated with a 32-bit integer atomicMax: independent of arrival order,
 * bitwise reproducible; 0 = empty.
 * Stage 2 (resolve): depth_w = 1 / zbuf (0 in holes), then the inverse warp of rigid_warp.py:337-373 with the inverted pose
 * after upstream's mat2euler -> euler2mat round trip: bilinear, zero padding, align_corners=True.  Outputs, per pose q:
 * img_w * valid (P,B,C,H,W), depth_w * valid (P,B,H,W), valid = [zbuf != 0] * [max|coord| <= 1] (P,B,H,W), and optionally the
 * raw z-buffer (P,B,H,W uint32 bit patterns).
 * Composition (trainer.py:503-511, optional, per pose): with dst[q] (B,C,H,W) given, dst = 0 on all channels where mask[q]
 * (B,H,W bytes, nullable) is 1, then PER ELEMENT dst = img_w where img_w > 0 (0 instead with MAL_FWARP_NO_REPROJ).  select
 * (B bytes, nullable) is read on the device: dst of a sample whose byte is 0 is left untouched (the outputs are still
 * written), which replaces upstream's host read of non_cv_aug and keeps the call capturable.
 * The per-sample matrices (both inverses of K, the inverted pose, its Euler round trip, K pose_inv) are formed on the device
 * in fp64 and rounded to fp32 once; the per-pixel chains are fp32 in upstream's order, no fma.
 * One call enqueues a clear of the z-buffer and three launches on `stream`; nothing is allocated, nothing synchronises.
 * Bounds: H, W >= 2, 1 <= upscale <= MAL_FWARP_MAX_UPSCALE, 1 <= C <= MAL_FWARP_MAX_C, 1 <= n_pose <= MAL_FWARP_MAX_POSES,
 * 1 <= B <= 65535, every tensor below 2^31 elements; anything else is MAL_ESHAPE.  A null args or required pointer is
 * MAL_EINVAL (checked first); both before any HIP call.  ws: mal_forward_warp_workspace_bytes (0 for a refused shape).
 * mal_forward_warp_plan is pure host code with the same shape checks: elements a lane loads at once (1), the tile of source
 * (splat) or target (resolve) pixels a 256-thread workgroup owns, the tiles per row and per column of one (pose, sample)
 * plane, the workgroups of either launch and its dynamic LDS bytes (0); every output pointer is nullable.
 * mal_inverse_warp is stage 2 alone (rigid_warp.py:337-373, Euler mode, zero padding): depth (B,H,W) and pose (B,6) =
 * (tx, ty, tz, rx, ry, rz) are the caller's; out (B,C,H,W) is the unmasked sample, valid (B,H,W) bytes.  Its ws holds the
 * matrices only: mal_forward_warp_workspace_bytes(B, H, W, 1) is always enough. */
#define MAL_FWARP_MAX_POSES 4
#define MAL_FWARP_MAX_UPSCALE 4
#define MAL_FWARP_MAX_C 4
#define MAL_FWARP_NO_REPROJ 1     /* flags: composition writes 0 where img_w > 0 (--no_reproj_doj) */
typedef struct mal_fwarp_args {
  const float* img;                         /* (B,C,H,W) */
  const float* depth;                       /* (B,H,W) */
  const float* K;                           /* (B,3,3) */
  const float* pose[MAL_FWARP_MAX_POSES];   /* n_pose x (B,3,4) */
  int B, C, H, W, upscale, n_pose, flags;
  float* img_w;                             /* out (n_pose,B,C,H,W) */
  float* depth_w;                           /* out (n_pose,B,H,W) */
  float* valid;                             /* out (n_pose,B,H,W) */
  uint32_t* zbuf;                           /* out, nullable (n_pose,B,H,W) */
  float* dst[MAL_FWARP_MAX_POSES];          /* in/out, nullable (B,C,H,W) each */
  const uint8_t* mask[MAL_FWARP_MAX_POSES]; /* nullable (B,H,W) each */
  const uint8_t* select;                    /* nullable (B) */
  void* ws; size_t ws_bytes;
  void* stream;
} mal_fwarp_args;
size_t mal_forward_warp_workspace_bytes(int B, int H, int W, int n_pose);
int mal_forward_warp_plan(int B, int C, int H, int W, int upscale, int n_pose, int* vec, int* tile_w, int* tile_h,
                          int* tiles_x, int* tiles_y, int* blocks, size_t* lds_bytes);
int mal_forward_warp(const mal_fwarp_args* args);
int mal_inverse_warp(const float* img, const float* depth, const float* pose, const float* K, int B, int C, int H, int W,
                     float* out, uint8_t* valid, void* ws, size_t ws_bytes, void* stream);

/* ---- N3: ManyDepth's cost volume as MAL's student encoder builds it (forward only; upstream runs it under
 * no_grad): manydepth/networks/resnet_encoder.py:152-233 match_features + :296-312 of the encoder's forward.
 * current_feats (B,C,h,w) and lookup_feats (B,F,C,h,w) planar as the encoder produces them, C = 64 (with option
 * "costvol_impl" 0, the first formulation, both CHANNEL-LAST instead: mal_costvol_channel_last() says which); poses (B,F,16) relative poses (an
 * all-zero pose = missing frame, skipped); K / inv_K (B,16) at the matching resolution; depth_bins (D <= 256).
 * cost_volume (B,D,h,w) = match_features' first return value (mean |warped - current| x border masks, averaged
 * over the frames that hit, missing bins set to the pixel's maximum when set_missing_to_max); nullable outputs:
 * missing_mask (B,D,h,w) = its second return value; masked_cost_volume = cost_volume x confidence (:311);
 * lowest_cost (B,h,w) = 1 / depth of the first minimum, zeros read as 100 (:303-307); confidence_mask (B,h,w). */
int mal_costvol_channel_last(void);
int mal_cost_volume(const float* current_feats, const float* lookup_feats, const float* poses, const float* K,
                    const float* inv_K, const float* depth_bins, int B, int F, int C, int D, int h, int w, float eps,
                    int set_missing_to_max, float* cost_volume, float* missing_mask, float* masked_cost_volume,
                    float* lowest_cost, float* confidence_mask, void* stream);

/* ---- DynamicDepth's occlusion-aware cost volume (forward only): dynamicdepth/networks/resnet_encoder.py:148-249
 * match_features + :299-312 of the encoder's forward.  Everything mal_cost_volume takes (planar features only), and:
 * lookup_images (B*F,3,H,W), the images the lookup features were taken from (required when set_1 or pool; their sum over
 * the channels < 0.15 marks the holes the forward warp left, resized by nearest to 48x128 whatever h, w are);
 * aug_mask (B) nullable = all zero: a sample whose value is not 0 gets no occlusion handling (read on the device);
 * cv_min: the frames fuse by minimum, a frame's cost of 0 reads as 1 and a fused cost of exactly 1 as missing (else
 * ManyDepth's mean over the frames that hit); set_1: occluded samples become 1.0 on every channel; else pool: they become,
 * per channel, the maximum of 0 and the non-occluded samples of the (2 pool_r + 1)^3 window over (bin, y, x).  A cell is
 * occluded when the bilinear sample of occ[b] > 0 at its sampling position is > pool_th (occ[b]: the image of FLAT index b,
 * as upstream indexes it, not b*F+f).  pool_r in 0..2 (MAL_EINVAL otherwise); shapes as mal_cost_volume (MAL_ESHAPE).
 * ws: mal_cost_volume_dyn_workspace_bytes (0 for a refused shape): the occlusion images and one byte per (b,f,d,y,x);
 * needed only when set_1 or pool.  The call enqueues two launches (four with set_1 or pool) on `stream`; it reads nothing
 * back, allocates nothing and does not synchronise. */
size_t mal_cost_volume_dyn_workspace_bytes(int B, int F, int D, int h, int w);
int mal_cost_volume_dyn(const float* current_feats, const float* lookup_feats, const float* poses, const float* K,
                        const float* inv_K, const float* depth_bins, int B, int F, int C, int D, int h, int w, float eps,
                        int set_missing_to_max, const float* lookup_images, int H, int W, const float* aug_mask,
                        int cv_min, int set_1, int pool, int pool_r, float pool_th, float* cost_volume,
                        float* missing_mask, float* masked_cost_volume, float* lowest_cost, float* confidence_mask,
                        void* ws, size_t ws_bytes, void* stream);

/* ---- N4 (forward): DualRefine's epipolar correlation lookup, dualrefine/networks/depth_pose.py:433-435.
 * mal_epipolar_coords = Reprojections.depth2epipolarcoords (dualrefine/networks/utils/utils.py:180-217, --gap_factor
 * depth): depth (B,1,h,w), poses (B,16) relative poses, K (B,16) at that resolution, r = --corr_radius, L = --num_levels
 * (<= 4), softplus_delta = softplus of the module's learnable delta, ratio = --gap_factor_depth_ratio ->
 * coords (B,2,L,2r+1,h,w) pixel coordinates in the other view, max_dx (B,1,h,w), depths (B,1,L*(2r+1),h,w).
 * mal_coord_sample_l1 = CoordSampler.__call__ (dualrefine/networks/corr.py:25-50): fmap1 (B,C,h,w), f2_pyramid[l]
 * (B,C,h>>l,w>>l) (avg_pool2d(2,2) levels, corr.py:19-23), coords as above with d1 hypotheses per level ->
 * out (B, L*heads*d1, h, w): per level and channel group (heads) the mean of |fmap1 - bilinear zero-padded sample|. */
int mal_epipolar_coords(const float* depth, const float* poses, const float* K, int B, int h, int w, int r, int L,
                        float softplus_delta, float ratio, float* coords, float* max_dx, float* depths, void* stream);
/* _iproj / pose / _proj for given depth hypotheses (Reprojections.depthbins2coords, utils.py:251-253): depths (B,1,D,h,w)
 * -> coords (B,2,1,D,h,w). */
int mal_epipolar_coords_of_depths(const float* depths, const float* poses, const float* K, int B, int D, int h, int w,
                                 float* coords, void* stream);
int mal_coord_sample_l1(const float* fmap1, const float* const* f2_pyramid, const float* coords, int B, int C, int h, int w,
                        int L, int d1, int heads, float* out, void* stream);
/* VJPs of the two lookup functions (the DEQ solver differentiates through them in training,
 * dualrefine/networks/depth_pose.py:426-455).  mal_epipolar_coords_bwd: cotangents of (coords, max_dx, depths) --
 * the last two nullable -- -> g_depth (B,1,h,w), g_poses (B,16; row 3 zero), g_dd (1) = d / d softplus(delta); fixed
 * summation order.  mal_coord_sample_l1_bwd: cotangent of the lookup's output -> g_fmap1 (B,C,h,w), g_f2_pyramid[l]
 * (level shapes), g_coords; g_fmap1 / g_f2_pyramid[l] are ACCUMULATED into (zero them first); any of the three may be
 * NULL.  With ws and planes that fit the LDS the sums are exact integer (fixed-point) accumulations per (sample, channel)
 * plane -- order-independent --; otherwise float atomics, as ATen's grid_sampler backward. */
size_t mal_epipolar_coords_bwd_workspace_bytes(int B, int h, int w);
int mal_epipolar_coords_bwd(const float* depth, const float* poses, const float* K, const float* g_coords,
                            const float* g_max_dx, const float* g_depths, int B, int h, int w, int r, int L,
                            float softplus_delta, float ratio, float* g_depth, float* g_poses, float* g_dd,
                            void* ws, size_t ws_bytes, void* stream);
int mal_coord_sample_l1_bwd(const float* fmap1, const float* const* f2_pyramid, const float* coords, const float* g_out,
                            int B, int C, int h, int w, int L, int d1, int heads, float* g_fmap1,
                            float* const* g_f2_pyramid, float* g_coords, void* ws, size_t ws_bytes, void* stream);
size_t mal_coord_sample_l1_bwd_workspace_bytes(int B); /* ws nullable: without it the feature cotangents use global atomics */
/* The pose refinement step of the same loop (depth_pose.py:450-455), forward:
 * mal_epipolar_gradcoords = Reprojections.depth2gradcoords (utils.py:219-236): c_p (B,2,1,5,h,w) = the projection and its
 * +-1 px neighbours in x and y, P2 (B,4,h*w) = the transformed points.
 * mal_direct_align_normal_eq = PoseUpdate.direct_align up to the solve (utils.py:303-355; robust != 0: with the
 * --robust_pose_loss weights of :344-355, scaled_barron(0, 0.1) of the squared residual x the in-image test):
 * src_feat / tgt_feat (B,C,h,w), src_w / tgt_w (B,1,h,w) (tgt_w is sampled at the projection as :388-390), weight (B,1,h,w)
 * nullable, K (B,16), p2 = c_p, P2 as above -> H (B,6,6) = sum_px w J^T J and b (B,6) = sum_px -res w J of the
 * feature-metric Gauss-Newton step; ws: mal_direct_align_workspace_bytes(B,h,w). */
int mal_epipolar_gradcoords(const float* depth, const float* poses, const float* K, int B, int h, int w, float* c_p, float* P2,
                            void* stream);
size_t mal_direct_align_workspace_bytes(int B, int h, int w);
/* The rest of direct_align (utils.py:357-368): 6x6 Cholesky solve with upstream's fall-backs (general solve, then the
 * unchanged pose), se3_exp (dualrefine/layers.py:29-55), new_poses (B,16) = exp(update) @ poses; update (B,6). */
int mal_direct_align_update(const float* H, const float* b, const float* poses, int B, float* new_poses, float* update,
                            void* stream);
int mal_direct_align_normal_eq(const float* src_feat, const float* tgt_feat, const float* src_w, const float* tgt_w,
                               const float* weight, const float* K, const float* p2, const float* P2, int B, int C, int h, int w,
                               int robust, float* H, float* b, void* ws, size_t ws_bytes, void* stream);
/* VJPs of the three (the last unrolled solver step differentiates through the pose update, depth_pose.py:450-455).
 * mal_epipolar_gradcoords_bwd: cotangents of c_p and P2 (nullable) -> g_depth (B,1,h,w), g_poses (B,16); fixed order.
 * mal_direct_align_normal_eq_bwd: cotangents of H (B,36) and b (B,6) -> every output nullable: g_src_feat (B,C,h,w),
 * g_tgt_feat (B,C,h,w) and g_tgt_w (B,1,h,w) (ZERO on entry: accumulated with float atomics, as ATen's grid_sampler
 * backward), g_src_w, g_weight (B,1,h,w), g_p2 (B,2,1,5,h,w), g_P2 (B,4,h*w; row 3 zero).  K receives no gradient.
 * mal_direct_align_update_bwd: cotangents of new_poses (B,16) and update (B,6; nullable) -> g_H (B,36; symmetrised on the
 * Cholesky path as torch.linalg.cholesky's backward), g_b (B,6), g_poses (B,16). */
size_t mal_epipolar_gradcoords_bwd_workspace_bytes(int B, int h, int w);
int mal_epipolar_gradcoords_bwd(const float* depth, const float* poses, const float* K, const float* g_c_p, const float* g_P2,
                                int B, int h, int w, float* g_depth, float* g_poses, void* ws, size_t ws_bytes, void* stream);
int mal_direct_align_normal_eq_bwd(const float* src_feat, const float* tgt_feat, const float* src_w, const float* tgt_w,
                                   const float* weight, const float* K, const float* p2, const float* P2, const float* g_H,
                                   const float* g_b, int B, int C, int h, int w, int robust, float* g_src_feat,
                                   float* g_tgt_feat, float* g_src_w, float* g_tgt_w, float* g_weight, float* g_p2, float* g_P2,
                                   void* ws, size_t ws_bytes, void* stream);
size_t mal_direct_align_bwd_workspace_bytes(int B, int h, int w); /* ws nullable: without it g_tgt_feat is scattered with global atomics */
int mal_direct_align_update_bwd(const float* H, const float* b, const float* poses, const float* g_new_poses,
                                const float* g_update, int B, float* g_H, float* g_b, float* g_poses, void* stream);

/* ---- library options (mal_set_option / mal_get_option): exactly these names; value ranges in brackets, "0|1" switches take
 * any int (nonzero = 1).  All of them are scheduling choices: none changes what a step computes.
 * Task decomposition -- set before a step's first call and leave it until its _bwd (MAL_ESTALE otherwise):
 * "march_rows"  [0..4096] output rows per wavefront task of the marching gradient passes; 0 (default) = automatic: the
 *               smallest count >= 8 whose tasks fit one resident round of the device (CUs x 8 waves); values < 8 act as 8;
 * "march_rows_fwd" [0..4096] the same for the forward-only passes; 0 (default) = as "march_rows";
 * "pack_rows"   [8..4096] rows per task of the identity / packing sweep (default 10; the partials are sized for >= 8);
 * "device_cus"  [0..65536] decompose as if the device had this many compute units (0, default: ask the device; a value
 *               > 0 needs no device query, e.g. 32 = one MI355X CPX partition, 304 = MI300X);
 * "march_halo1" 0|1 (default 1): the gradient passes of the whole-step lists warp ONE row beyond each end of a task's
 *               segment and hand the boundary rows' missing terms over through scratch rows; 0: two rows, no hand-over (A/B);
 * "march_flip"  0|1 (default 1): odd row segments of the marching kernels walk bottom-up, so the two tasks sharing a
 *               segment boundary reach it together and the halo rows are served by the L2; 0 = all top-down;
 * "syn_rows"    [2..64] rows per task of the fused sweep given a region map (default 4; >= 8: the automatic decomposition);
 * Formulations and overlap:
 * "pass_impl"   [0..2] formulation of the fused pass: 1 = register-marching (default); 0 / 2 = the LDS-tiled first
 *               versions (256 threads x 4 px, 512 threads x 2 px; -DMAL_EXPERIMENTS builds only);
 * "march_lean"  0|1 (default 1): the teacher / student passes of the whole-step lists run the instantiations without the code
 *               of the optional operands they never pass (march_teacher_kernel, march_student_kernel); 0: generic (A/B);
 * "costvol_impl" [0..1] 1 (default): cost volume with planar features, lane = pixel; 0: channel-last, lane = channel;
 * "photo_impl"  [0..1] mal_photo_fwd/bwd: 1 = marching kernels, two candidates per launch (default for SSIM + min);
 *               0 = one pixel per thread (ATen's summation order; always used for MAL_F_NO_SSIM / MAL_F_AVG);
 * "epi_bwd_planes" [0..2] 2 (default): the feature-map cotangents of the N4 VJPs are accumulated per (sample, channel) plane
 *               in LDS when the planes fit, the lookup's with TWO channel planes per workgroup where 2 x the planes fit;
 *               1: one plane per workgroup; 0: global float atomics everywhere (the first formulation, kept for A/B);
 * "dyn_small_blocks" 0|1 (default 1): the temporal-hint producer's extents kernel in small workgroups; 0: 1024 threads (A/B);
 * "step_overlap" [0..2] 1 (default): with MAL_STEP_TEMPORAL the ensemble pass runs on a side stream beside the producer
 *               (forked after the warp pass, joined before the student pass; events, capturable); 0: in line; 2: beside the
 *               fused sweep (slower: kept for A/B);
 * "student_overlap" [0..2] (default 2): with MAL_STEP_TEMPORAL the student's marching pass (without its consistency /
 *               distillation epilogue, which becomes a pointwise launch after the join) is forked beside the producer behind
 *               the ensemble pass; 2: the two forked passes are ONE launch that runs only the samples whose weight
 *               1 - augmentation mask is not zero (decided on the device at run time; an augmented sample's terms are exact
 *               zeros) -- only when the step returns none of multi_reproj, ens_reproj, consistency_mask_out, dec_student and
 *               runs without MAL_STEP_MAIN_TEMPORAL, MAL_STEP_DUAL_DISTIL, ens_disp, with B <= 64; otherwise as 1;
 *               1: a launch each, every sample computed (same-binary A/B); 0: in line after the fused sweep, epilogue
 *               inside the pass (kept for A/B);
 * "side_order"  0..2 (default 0): 1 = of the forked passes the student's goes first, the ensemble pass behind it (slower);
 *               2 = the merged launch of "student_overlap" 2 picks the arrangement on the device from the live samples:
 *               as 0 when one resident round of wave slots holds the live tasks of both passes, otherwise the student's
 *               tasks first and the ensemble pass behind them in 8-row segments (same results; a launch per pass: as 0);
 * "side_priority" 0|1 (default 0): 1 = the side stream is created with the device's lowest priority (slower); read only when
 *               a caller stream's side stream is first created;
 * "tail_overlap" 0|1 (default 1): a --temporal step's backward chain runs on the side stream behind the fused sweep, beside
 *               the epilogue and the reduction of the forward (mal_loss_step_tail_begin);
 * "sweeps_batched" 0|1 (default 1): --temporal --main_temporal: both passes' fused sweeps as one launch; 0: two (A/B);
 * "ms_fold"     0|1 (default 1): the four-scale step's noise maps and upsampling ride on its first sweep; 0: launches of
 *               their own (A/B);
 * "syn_queue"   0|1: the fused sweep takes its tasks from a classified dispatch order (slower, default 0;
 *               -DMAL_EXPERIMENTS builds only);
 * "temporal_spec" 0|1: with MAL_STEP_TEMPORAL the pass in front of the producer already takes the teacher's gradient and the
 *               sweep behind the producer's backward only redoes the tasks near the region map (default 0;
 *               -DMAL_EXPERIMENTS builds only);
 * "march3"      0|1: the teacher's gradient pass as three cooperating wavefronts per strip, rows handed over through LDS
 *               (slower; default 0; -DMAL_EXPERIMENTS builds only);
 * Probes (timing / debugging experiments, results not meant to be used):
 * "debug", "epi_probe" (any int; default 0). */
int mal_set_option(const char* name, int value);
int mal_get_option(const char* name, int* value); /* the current value of an option mal_set_option accepts; MAL_EINVAL for
                                                   any other name */
/* Options are PROCESS-WIDE switches for same-box A/B measurements, not per-call configuration: set them before the first
 * step and leave them; a second trainer in the process sees the same values.  Setting one is serialised by a mutex;
 * launches read them without further synchronisation.  The formulations that were measured slower (pass_impl 0 / 2,
 * march3, temporal_spec, syn_queue) are compiled only into a library built with -DMAL_EXPERIMENTS (MAL_EXPERIMENTS=1
 * python -m mal_amd.build); the default library refuses those switches with MAL_EINVAL.  The one-shot arms below
 * (mal_profile_next_pass, mal_decisions_next_pass) are process-wide too (a step's backward runs on autograd's worker
 * thread, not on the arming one) and are taken with an atomic exchange: exactly one pass consumes an arm. */
int mal_build_has_experiments(void); /* 1 when the library contains the -DMAL_EXPERIMENTS formulations */
/* sizeof of the argument blocks as THIS library was compiled (0 mal_step_args, 1 mal_ms_args, 2 mal_dr_args, 3 mal_dyn_item,
 * 4 mal_step_scales_args, 5 mal_eval_seg, 6 mal_eval_args, 7 mal_match_args, 8 mal_instances_args, 9 mal_msda_args,
 * 10 mal_fwarp_args, 11 mal_eval_dyn_args; else 0): a binding in another language checks its own layout against it once, at load (mal_amd/_lib.py does). */
size_t mal_struct_bytes(int which);

/* ---- validation metrics: manydepth/trainer.py:836-1064 (Trainer.val) + evaluate_depth.py:35-53 (compute_errors) ----------
 * The ground truth of a split is packed once (mal_amd/evaluate.py): per image a segment of `slots` packed points.  Sparse
 * (LiDAR) segments hold the flat index y*gt_w+x of each valid point (mask and crop applied) and its value; dense segments
 * (CityScapes windows) hold the rw-wide rectangle at (x0, y0) of the resized image row by row, with 0 where the mask is
 * false.  `gt` is f64 when gt_f64, else fp32; med_gt is np.median of the image's valid ground truth (exact, in its dtype) --
 * or, packed for mal_eval_dyn_accumulate below, torch.median's lower middle value. */
typedef struct mal_eval_seg {
  int64_t off;     /* first packed slot of the image */
  int slots;       /* packed slots (sparse: = n) */
  int n;           /* valid points (>= 1) */
  int gt_h, gt_w;  /* size the prediction is resized to (cv2.resize INTER_LINEAR, float32) */
  int x0, y0, rw;  /* dense: the rectangle in the resized image; sparse: 0 */
  int dense;
  double med_gt;
} mal_eval_seg;

/* One batch of predictions: disp (B,1,H,W) are the network's sigmoid outputs for images first .. first+B-1.
 * Per valid point: disp_to_depth(disp, min_depth_disp, max_depth_disp)[0] (as mal_disp_to_depth), the 4-tap resize,
 * 1/x, x scale_factor; then per image an exact median, the ratio (median_scaling), the clamp to [clamp_min, clamp_max]
 * and compute_errors.  img_out[i*8 + 0..7] = abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, ratio (ratio = 1 without
 * median scaling) for each image i of the batch; nothing else is written but `pred` (fp32 scratch: the batch's slots,
 * seg[first+B-1].off + slots - seg[first].off of them).  resize_ulp moves each resized disparity by that many ulps
 * (a measurement hook; 0 in use). */
typedef struct mal_eval_args {
  int n_images, first, B, H, W;
  int gt_f64, median_scaling, resize_ulp;
  double min_depth_disp, max_depth_disp;  /* as the Python floats upstream passes: 1/min_depth is formed in f64 */
  float scale_factor, clamp_min, clamp_max;
  const mal_eval_seg* seg;  /* device, [n_images] */
  const int32_t* idx;       /* device, sparse flat indices (NULL if every segment is dense) */
  const void* gt;           /* device, packed ground truth */
  const float* disp;
  float* pred;
  double* img_out;          /* device, [n_images][8] */
  void* stream;
} mal_eval_args;

int mal_eval_accumulate(const mal_eval_args* args);
/* np.array(errors).mean(0): out7 = the mean of img_out[i*8 + 0..6] over the n_images images, in image order */
int mal_eval_mean(const double* img_out, int n_images, double* out7, void* stream);
/* compute_errors(gt, pred) on two device arrays of n values (each fp32 or f64, numpy's promotion: f64 arithmetic if
 * either is f64, logs in each input's own dtype): out7 = abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 as f64.
 * Deterministic two-stage sum; ws >= mal_eval_errors_workspace_bytes(n). */
size_t mal_eval_errors_workspace_bytes(size_t n);
int mal_eval_errors(const void* gt, int gt_f64, const void* pred, int pred_f64, size_t n, double* out7, void* ws,
                    size_t ws_bytes, void* stream);

/* ---- DynamicDepth's validation: dynamicdepth/trainer.py:1158-1257 (compute_depth_losses), :881-886 (val's aggregation),
 * layers.py:244-262 (compute_depth_errors) ---------------------------------------------------------------------------------
 * The packing is the one above (mal_amd/dyn_eval.py); med_gt holds torch.median's LOWER middle value of the image's valid
 * ground truth, and n < 2^24.  One batch: disp (B,1,H,W) sigmoid outputs and mask (B,1,mh,mw) object masks of images
 * first .. first+B-1.  Per valid point: disp_to_depth(disp, min_depth, max_depth)[1] at the four taps (as
 * mal_disp_to_depth), F.interpolate(mode="bilinear", align_corners=False) evaluated pointwise, clamp(1e-3, 80), and the
 * region byte F.interpolate(mask) (nearest) != 0.  Per image: torch.median of the predictions, the ratio, the float32
 * multiply, the second clamp, and compute_depth_errors over the valid points and over those with the region byte set.
 * img_out[i*MAL_EVAL_DYN_ROW + ..]: 0..6 abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 over the valid points; 7..13 the same
 * over the object region (all 0 when it is empty); 14 ratio; 15 n_all; 16 n_doj; 17 the median of the prediction.
 * Scratch, the batch's slots (seg[first+B-1].off + slots - seg[first].off) each: pred (the clamped prediction before
 * scaling), region (the bytes), scaled (NULL, or the prediction after scaling and the second clamp). */
#define MAL_EVAL_DYN_ROW 18
#define MAL_EVAL_DYN_MEAN 17
#define MAL_EVAL_MASK_F32 0
#define MAL_EVAL_MASK_U8 1
typedef struct mal_eval_dyn_args {
  int n_images, first, B, H, W;
  int mh, mw, mask_dtype;       /* MAL_EVAL_MASK_* */
  int gt_f64, reserved;
  double min_depth, max_depth;  /* as the Python floats upstream passes to disp_to_depth: 1/min is formed in f64 */
  const mal_eval_seg* seg;      /* device, [n_images] */
  const int32_t* idx;           /* device, sparse flat indices (NULL if every segment is dense) */
  const void* gt;               /* device, packed ground truth */
  const float* disp;
  const void* mask;
  float* pred;
  unsigned char* region;
  float* scaled;                /* nullable */
  double* img_out;              /* device, [n_images][MAL_EVAL_DYN_ROW] */
  void* stream;
} mal_eval_dyn_args;

int mal_eval_dyn_accumulate(const mal_eval_dyn_args* args);
/* out[0..6] the means of img_out[.][0..6] over the n_images images; out[7..13] the sums of img_out[.][7..13] over the images
 * with n_doj > 0 divided by their number (NaN when there is none, upstream's 0/0); out[14] that number (doj/count);
 * out[15] dojpxs, out[16] allpxs (the totals of n_doj and n_all).  In image order. */
int mal_eval_dyn_mean(const double* img_out, int n_images, double* out, void* stream);

/* ---- measurement hooks (bench.py): HIP events recorded immediately before / after the main
 * kernel of the NEXT mal_pass_fused call, on its stream (one-shot; cleared by that call). */
void* mal_event_create(void);
int mal_event_destroy(void* ev);
int mal_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on `stop` */
int mal_profile_next_pass(void* start, void* stop);
/* The task decomposition march_launch picks for a fused pass over (B,H,W) with `flags` (MAL_F_GRAD decides the halo) on
 * the current device: strips x segs wavefront tasks per sample, `rows` output rows per task, `iterations` of the row
 * loop a full task runs (rows + its halo rows).  bench.py prices the kernel's vector-ALU time with it. */
int mal_march_geometry(int B, int H, int W, int flags, int* strips, int* segs, int* rows, int* iterations);
/* Shader clock under load: two wavefronts of packed FMAs on every SIMD for `iters` rounds of 64 instructions; wave 0
 * leaves out3[0] = shader-clock ticks (s_memtime) and out3[1] = ticks of the constant 100 MHz counter (s_memrealtime)
 * around its loop (out3: 3 device words, the third is scratch).  clock_MHz = 100 * out3[0] / out3[1]. */
int mal_clock_probe(unsigned long long* out3, int iters, void* stream);
/* Parity instrumentation for the operator-level fused pass (tests): the next mal_pass_fused call whose flags are
 * GRAD|AUTOMASK|POSE_GRAD (no epilogue) or GRAD|EPILOGUE (no automask, no pose gradient) writes its per-pixel decisions
 * into `planes` (MAL_DEC_PLANES x B*H*W uint32, MAL_DEC_* above; the smoothness planes stay untouched) -- one shot. */
int mal_decisions_next_pass(uint32_t* planes);

#ifdef __cplusplus
}
#endif
#endif /* MAL_HIP_H */
