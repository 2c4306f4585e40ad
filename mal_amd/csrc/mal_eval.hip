// Validation metrics of upstream's trainer on the device: Trainer.val's per-image rule (manydepth/trainer.py:952-1064)
// and compute_errors (manydepth/evaluate_depth.py:35-53, manydepth/layers.py:260-278).
//
//   mal_eval_accumulate   one batch of disparities: per valid ground-truth point disp_to_depth + cv2.resize (INTER_LINEAR,
//                         float32) evaluated pointwise + 1/x + scale factor; per image an exact median (radix select on the
//                         float bits, LDS histograms, one workgroup per image), ratio, clamp, the seven error sums
//   mal_eval_mean         np.array(errors).mean(0), in image order
//   mal_eval_errors       compute_errors on two flat arrays, deterministic two-stage sums
//
// Every sum is per thread in a fixed stride order, then a fixed shuffle tree, then the waves in order: the same inputs give
// the same bits, and a batch writes only its own images' slots, so the order in which batches arrive does not matter.
// Decisions (median, ratio, clamp, thresh < 1.25^k) are taken in the dtype numpy takes them in (DESIGN.md "Validation").
#include "mal_eval_core.h"

using namespace mal;

namespace {

constexpr int kErrThreads = 256;
constexpr int kErrBlocks = 1024;

// the scaled disparity of disp_to_depth at a source pixel (mal_disp_to_depth's arithmetic)
MAL_DEV float scaled_at(const float* __restrict__ S, int i, float min_disp, float range) {
  return min_disp + range * S[i];
}

// cv2.resize(src (sh,sw) float32, (dw, dh), INTER_LINEAR) at destination pixel (x, y), in the operation order of
// OpenCV's two-pass resizeGeneric_ (HResizeLinear, then VResizeLinear): per row sx/fx from
// float((x + 0.5) * scale_x - 0.5); a horizontal tap past either border becomes the edge pixel with weight 0 (the right
// border is a plain copy); the rows are clamped to the image and keep their fractional weight.  -ffp-contract=off: each
// pass is a*w0 + b*w1 with three roundings.
MAL_DEV float resize_at(const float* __restrict__ S, int sh, int sw, double scale_x, double scale_y, int x, int y,
                        float min_disp, float range) {
  float fx = (float)(((double)x + 0.5) * scale_x - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  bool copy = false;
  if (sx < 0) { fx = 0.f; sx = 0; }
  if (sx >= sw - 1) { fx = 0.f; sx = sw - 1; copy = true; }
  float fy = (float)(((double)y + 0.5) * scale_y - 0.5);
  int sy = (int)floorf(fy);
  fy -= (float)sy;
  const int r0 = min(max(sy, 0), sh - 1), r1 = min(max(sy + 1, 0), sh - 1);
  const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
  float h0, h1;
  if (copy) {
    h0 = scaled_at(S, r0 * sw + sx, min_disp, range);
    h1 = scaled_at(S, r1 * sw + sx, min_disp, range);
  } else {
    h0 = scaled_at(S, r0 * sw + sx, min_disp, range) * a0 + scaled_at(S, r0 * sw + sx + 1, min_disp, range) * a1;
    h1 = scaled_at(S, r1 * sw + sx, min_disp, range) * a0 + scaled_at(S, r1 * sw + sx + 1, min_disp, range) * a1;
  }
  return h0 * b0 + h1 * b1;
}

template <typename T>
__global__ __launch_bounds__(kPredThreads) void eval_predict_kernel(mal_eval_args a, float min_disp, float range) {
  const int j = blockIdx.y;
  const mal_eval_seg sg = a.seg[a.first + j];
  const int64_t base = a.seg[a.first].off;  // a.pred holds the batch's slots only
  const float* S = a.disp + (size_t)j * a.H * a.W;
  uint32_t* out = (uint32_t*)a.pred + (sg.off - base);
  const T* g = (const T*)a.gt + sg.off;
  const double scale_x = 1.0 / ((double)sg.gt_w / (double)a.W), scale_y = 1.0 / ((double)sg.gt_h / (double)a.H);
  for (int i = blockIdx.x * kPredThreads + threadIdx.x; i < sg.slots; i += gridDim.x * kPredThreads) {
    if (sg.dense && !(g[i] > (T)0)) { out[i] = kInvalid; continue; }
    int x, y;
    slot_xy(sg, a.idx, i, x, y);
    float v = resize_at(S, a.H, a.W, scale_x, scale_y, x, y, min_disp, range);
    if (a.resize_ulp) v = __uint_as_float(__float_as_uint(v) + (uint32_t)a.resize_ulp);  // v > 0: bits are monotone
    const float p = div_(1.0f, v) * a.scale_factor;  // pred_depth = 1 / pred_disp; *= pred_depth_scale_factor
    out[i] = __float_as_uint(p);
  }
}

// the four sums and three counts of compute_errors, accumulated in f64 per thread
struct ErrSums {
  double abs_rel = 0.0, sq_rel = 0.0, sq = 0.0, sq_log = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
};

// gt and pred in their own dtypes (point_terms); the counts are kept as doubles
template <typename G, typename P>
MAL_DEV void add_point(ErrSums& s, G g, P p) {
  double t[4];
  int c[3];
  point_terms<G, P>(g, p, t, c);
  s.abs_rel += t[0];
  s.sq_rel += t[1];
  s.sq += t[2];
  s.sq_log += t[3];
  s.c1 += (double)c[0];
  s.c2 += (double)c[1];
  s.c3 += (double)c[2];
}

// per-image metrics from the sums: f64 as numpy's means; with float32 arithmetic the four means are float32 (a1..a3 are
// means of booleans: f64 either way)
MAL_DEV void finish_errors(const double* s7, double n, bool f32, double* out) {
  finish_means4(s7, n, f32, out);
  out[4] = s7[4] / n;
  out[5] = s7[5] / n;
  out[6] = s7[6] / n;
}

// workgroup-wide fixed-order sum of the seven accumulators; the result is valid in thread 0
__device__ void block_sum7(const ErrSums& s, double (*s_red)[kImgWaves], int nwaves, double* out7) {
  const double v[7] = {s.abs_rel, s.sq_rel, s.sq, s.sq_log, s.c1, s.c2, s.c3};
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int k = 0; k < 7; ++k) {
    const double t = wave_sum_d(v[k]);
    if (lane == 0) s_red[k][w] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 0; k < 7; ++k) {
      double t = 0.0;
      for (int i = 0; i < nwaves; ++i) t += s_red[k][i];
      out7[k] = t;
    }
}

// One workgroup per image of the batch: exact median of the predictions (np.median), ratio, scale, clamp, errors.
template <typename T>
__global__ __launch_bounds__(kImgThreads) void eval_image_kernel(mal_eval_args a) {
  __shared__ uint32_t hist[4096];
  __shared__ int s_wave[kImgWaves];
  __shared__ int s_bin, s_below;
  __shared__ uint32_t s_min;
  __shared__ double s_red[7][kImgWaves];
  const int img = a.first + blockIdx.x;
  const mal_eval_seg sg = a.seg[img];
  const uint32_t* pb = (const uint32_t*)a.pred + (sg.off - a.seg[a.first].off);
  const T* gt = (const T*)a.gt + sg.off;
  const int tid = threadIdx.x;
  constexpr bool gt64 = sizeof(T) == 8;
  if (tid == 0) { s_bin = 0; s_below = 0; }

  double ratio = 1.0;
  float ratio_f = 1.0f;
  if (a.median_scaling) {
    // np.median's lower middle value: rank k1 = (n-1)/2
    const int n = sg.n, k1 = (n - 1) / 2;
    const Selected sel = radix_select(pb, sg.slots, k1, hist, s_wave, &s_bin, &s_below);
    const uint32_t v1 = sel.bits;
    uint32_t v2 = v1;
    // even count: the upper middle is v1 again unless every copy of v1 lies at or below rank k1
    if ((n & 1) == 0 && (k1 - sel.k_left) + sel.cnt_eq < k1 + 2) {
      if (tid == 0) s_min = kInvalid;
      __syncthreads();
      uint32_t m = kInvalid;
      for (int i = tid; i < sg.slots; i += kImgThreads) {
        const uint32_t u = pb[i];
        if (u != kInvalid && u > v1 && u < m) m = u;
      }
      for (int o = 32; o > 0; o >>= 1) m = min(m, (uint32_t)__shfl_down(m, o, 64));
      if ((tid & 63) == 0) atomicMin(&s_min, m);
      __syncthreads();
      v2 = s_min;
    }
    // np.median of float32: the middle value, or the float32 mean of the two middle values
    const float med = (n & 1) ? __uint_as_float(v1) : (__uint_as_float(v1) + __uint_as_float(v2)) / 2.0f;
    if (gt64) ratio = sg.med_gt / (double)med;         // float64 / float32 -> float64
    else { ratio_f = (float)sg.med_gt / med; ratio = (double)ratio_f; }
  }

  ErrSums s;
  for (int i = tid; i < sg.slots; i += kImgThreads) {
    const uint32_t u = pb[i];
    if (u == kInvalid) continue;
    float p = __uint_as_float(u);
    if (a.median_scaling) p = gt64 ? (float)((double)p * ratio) : p * ratio_f;  // pred_depth *= ratio
    if (p < a.clamp_min) p = a.clamp_min;
    if (p > a.clamp_max) p = a.clamp_max;
    add_point<T, float>(s, gt[i], p);
  }
  double sums[7];
  block_sum7(s, s_red, kImgWaves, sums);
  if (tid == 0) {
    double* o = a.img_out + (size_t)img * 8;
    finish_errors(sums, (double)sg.n, !gt64, o);
    o[7] = ratio;
  }
}

__global__ void eval_mean_kernel(const double* img_out, int n_images, double* out7) {
  const int k = threadIdx.x;
  if (k >= 7) return;
  double s = 0.0;
  for (int i = 0; i < n_images; ++i) s += img_out[(size_t)i * 8 + k];
  out7[k] = s / (double)n_images;
}

template <typename G, typename P>
__global__ __launch_bounds__(kErrThreads) void eval_errors_stage1(const G* gt, const P* pred, size_t n, double* part) {
  __shared__ double s_red[7][kImgWaves];
  ErrSums s;
  for (size_t i = blockIdx.x * (size_t)kErrThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kErrThreads)
    add_point<G, P>(s, gt[i], pred[i]);
  double sums[7];
  block_sum7(s, s_red, kErrThreads / 64, sums);
  if (threadIdx.x == 0)
    for (int k = 0; k < 7; ++k) part[(size_t)blockIdx.x * 8 + k] = sums[k];
}

__global__ void eval_errors_stage2(const double* part, int nblocks, size_t n, int f32, double* out7) {
  __shared__ double s7[7];
  const int k = threadIdx.x;
  if (k < 7) {
    double s = 0.0;
    for (int i = 0; i < nblocks; ++i) s += part[(size_t)i * 8 + k];
    s7[k] = s;
  }
  __syncthreads();
  if (k == 0) {
    double o[7];
    finish_errors(s7, (double)n, f32 != 0, o);
    for (int i = 0; i < 7; ++i) out7[i] = o[i];
  }
}

int err_blocks(size_t n) {
  size_t g = (n + kErrThreads - 1) / kErrThreads;
  return (int)(g < 1 ? 1 : (g > (size_t)kErrBlocks ? kErrBlocks : g));
}

template <typename G, typename P>
void launch_errors(const void* gt, const void* pred, size_t n, double* part, int nb, hipStream_t st) {
  hipLaunchKernelGGL((eval_errors_stage1<G, P>), dim3(nb), dim3(kErrThreads), 0, st, (const G*)gt, (const P*)pred, n, part);
}

}  // namespace

extern "C" int mal_eval_accumulate(const mal_eval_args* a) {
  if (!a || !a->seg || !a->gt || !a->disp || !a->pred || !a->img_out) return MAL_EINVAL;
  if (a->n_images <= 0 || a->B <= 0 || a->first < 0 || a->first > a->n_images - a->B) return MAL_EINVAL;
  if (a->H < 1 || a->W < 1 || (double)a->B * a->H * a->W > 2.0e9) return MAL_ESHAPE;
  if (!(a->scale_factor > 0.f) || !(a->scale_factor < INFINITY)) return MAL_EINVAL;
  if (!(a->min_depth_disp > 0.0) || !(a->max_depth_disp > a->min_depth_disp) || !(a->max_depth_disp < INFINITY))
    return MAL_EINVAL;
  if (!(a->clamp_min > 0.f) || !(a->clamp_max > a->clamp_min)) return MAL_EINVAL;
  if (a->resize_ulp < -4 || a->resize_ulp > 4) return MAL_EINVAL;
  if (a->B > 65535) return MAL_EINVAL;
  hipStream_t st = (hipStream_t)a->stream;
  // disp_to_depth's constants: 1/max and 1/min - 1/max in f64 from the Python floats, then float32 (torch's scalar args)
  const float min_disp = (float)(1.0 / a->max_depth_disp);
  const float range = (float)(1.0 / a->min_depth_disp - 1.0 / a->max_depth_disp);
  mal_eval_args args = *a;
  dim3 pg(kPredBlocksPerImage, a->B);
  if (a->gt_f64) {
    hipLaunchKernelGGL(eval_predict_kernel<double>, pg, dim3(kPredThreads), 0, st, args, min_disp, range);
    hipLaunchKernelGGL(eval_image_kernel<double>, dim3(a->B), dim3(kImgThreads), 0, st, args);
  } else {
    hipLaunchKernelGGL(eval_predict_kernel<float>, pg, dim3(kPredThreads), 0, st, args, min_disp, range);
    hipLaunchKernelGGL(eval_image_kernel<float>, dim3(a->B), dim3(kImgThreads), 0, st, args);
  }
  return launch_status();
}

extern "C" int mal_eval_mean(const double* img_out, int n_images, double* out7, void* stream) {
  if (!img_out || !out7 || n_images <= 0) return MAL_EINVAL;
  hipLaunchKernelGGL(eval_mean_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, img_out, n_images, out7);
  return launch_status();
}

extern "C" size_t mal_eval_errors_workspace_bytes(size_t n) {
  if (n == 0) return 0;
  return (size_t)err_blocks(n) * 8 * sizeof(double);
}

extern "C" int mal_eval_errors(const void* gt, int gt_f64, const void* pred, int pred_f64, size_t n, double* out7, void* ws,
                               size_t ws_bytes, void* stream) {
  if (!gt || !pred || !out7 || !ws || n == 0) return MAL_EINVAL;
  if (ws_bytes < mal_eval_errors_workspace_bytes(n)) return MAL_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nb = err_blocks(n);
  double* part = (double*)ws;
  if (gt_f64 && pred_f64) launch_errors<double, double>(gt, pred, n, part, nb, st);
  else if (gt_f64) launch_errors<double, float>(gt, pred, n, part, nb, st);
  else if (pred_f64) launch_errors<float, double>(gt, pred, n, part, nb, st);
  else launch_errors<float, float>(gt, pred, n, part, nb, st);
  hipLaunchKernelGGL(eval_errors_stage2, dim3(1), dim3(64), 0, st, (const double*)part, nb, n, (gt_f64 || pred_f64) ? 0 : 1, out7);
  return launch_status();
}
