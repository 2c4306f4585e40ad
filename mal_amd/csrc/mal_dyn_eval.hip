// DynamicDepth's validation on the device: Trainer.compute_depth_losses (dynamicdepth/trainer.py:1158-1257) with
// layers.compute_depth_errors (dynamicdepth/layers.py:244-262) and the aggregation of Trainer.val (:756-905).
//
//   mal_eval_dyn_accumulate  one batch of disparities and object masks, two launches:
//     eval_dyn_predict_kernel  per packed ground-truth point: disp_to_depth's DEPTH at the four taps, ATen's
//                              upsample_bilinear2d (align_corners=False) in its device kernel's operation order,
//                              clamp(1e-3, 80); and the point's region byte: doj_mask by ATen's nearest rule, != 0
//     eval_dyn_image_kernel    one workgroup per image: torch.median (the LOWER middle value, radix select on the float
//                              bits), the ratio, the in-place float32 multiply, the second clamp, and in one pass the sums
//                              of compute_depth_errors over all valid points and over those inside the object region
//   mal_eval_dyn_mean        Trainer.val's aggregation over the rows, in image order
//
// The select, the scan, the packed-slot decode, the per-point terms and the promoted means are csrc/mal_eval_core.h's, shared
// with csrc/mal_eval.hip; this file holds what is DynamicDepth's: the decisions are taken in the dtype torch
// takes them in.  Nothing is allocated, read back or synchronised; a batch writes only its own images' rows, so grouping and
// order of the batches do not matter.
#include "mal_eval_core.h"

using namespace mal;

namespace {

constexpr int kRow = MAL_EVAL_DYN_ROW;
constexpr int kSums = 8, kCounts = 8;       // 4 + 4 sums; 3 + 3 threshold counts, n_all, n_doj
constexpr float kClampMin = 1e-3f, kClampMax = 80.f;  // trainer.py:1189, :1220: literals, not options

// torch.clamp: min(max(x, lo), hi) with NaN propagated
MAL_DEV float clamp_t(float v) {
  if (v < kClampMin) v = kClampMin;
  if (v > kClampMax) v = kClampMax;
  return v;
}

// ATen's area_pixel_compute_source_index (align_corners=False, not cubic) and the taps of upsample_bilinear2d's device
// kernel: src = max(0, scale * (dst + 0.5) - 0.5), i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1
MAL_DEV void taps_of(float scale, int dst, int in, int& i0, int& i1, float& l0, float& l1) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  const int t = (int)s;
  l1 = s - (float)t;
  l0 = 1.f - l1;
  i0 = min(t, in - 1);  // t <= in - 1 for every dst < out; the min only keeps a read inside the plane
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
}

// ATen's nearest_neighbor_compute_source_index
MAL_DEV int nearest_of(float scale, int dst, int in) { return min((int)floorf((float)dst * scale), in - 1); }

template <typename T, typename M>
__global__ __launch_bounds__(kPredThreads) void eval_dyn_predict_kernel(mal_eval_dyn_args a, float min_disp, float range) {
  const int j = blockIdx.y;
  const mal_eval_seg sg = a.seg[a.first + j];
  const int64_t base = a.seg[a.first].off;  // pred / region / scaled hold the batch's slots only
  const float* S = a.disp + (size_t)j * a.H * a.W;
  const M* Mk = (const M*)a.mask + (size_t)j * a.mh * a.mw;
  uint32_t* out = (uint32_t*)a.pred + (sg.off - base);
  unsigned char* reg = a.region + (sg.off - base);
  const T* g = (const T*)a.gt + sg.off;
  // compute_scales_value<float>: (float)in / out
  const float sy = (float)a.H / (float)sg.gt_h, sx = (float)a.W / (float)sg.gt_w;
  const float my = (float)a.mh / (float)sg.gt_h, mx = (float)a.mw / (float)sg.gt_w;
  for (int i = blockIdx.x * kPredThreads + threadIdx.x; i < sg.slots; i += gridDim.x * kPredThreads) {
    if (sg.dense && !(g[i] > (T)0)) { out[i] = kInvalid; reg[i] = 0; continue; }
    int x, y;
    slot_xy(sg, a.idx, i, x, y);
    int y0, y1, x0, x1;
    float l0y, l1y, l0x, l1x;
    taps_of(sy, y, a.H, y0, y1, l0y, l1y);
    taps_of(sx, x, a.W, x0, x1, l0x, l1x);
    const float d00 = depth_of(S[y0 * a.W + x0], min_disp, range), d01 = depth_of(S[y0 * a.W + x1], min_disp, range);
    const float d10 = depth_of(S[y1 * a.W + x0], min_disp, range), d11 = depth_of(S[y1 * a.W + x1], min_disp, range);
    const float v = l0y * (l0x * d00 + l1x * d01) + l1y * (l0x * d10 + l1x * d11);
    out[i] = __float_as_uint(clamp_t(v));
    const int ny = nearest_of(my, y, a.mh), nx = nearest_of(mx, x, a.mw);
    reg[i] = Mk[ny * a.mw + nx] != (M)0 ? 1 : 0;
  }
}

// one region's metrics from its sums: the four means in the promoted dtype; a1..a3 are .float().mean(): count / n in
// float32 (both exact below 2^24, which the packing guarantees)
MAL_DEV void finish_errors(const double* s4, const int* c3, int ni, bool f32, double* out) {
  finish_means4(s4, (double)ni, f32, out);
  for (int k = 0; k < 3; ++k) out[4 + k] = (double)((float)c3[k] / (float)ni);
}

// One workgroup per image of the batch.
template <typename T>
__global__ __launch_bounds__(kImgThreads) void eval_dyn_image_kernel(mal_eval_dyn_args a) {
  __shared__ uint32_t hist[4096];
  __shared__ int s_wave[kImgWaves];
  __shared__ int s_bin, s_below;
  __shared__ double s_red[kSums][kImgWaves];
  __shared__ int s_cnt[kCounts][kImgWaves];
  const int img = a.first + blockIdx.x;
  const mal_eval_seg sg = a.seg[img];
  const int64_t rel = sg.off - a.seg[a.first].off;
  const uint32_t* pb = (const uint32_t*)a.pred + rel;
  const unsigned char* reg = a.region + rel;
  float* scaled = a.scaled ? a.scaled + rel : nullptr;
  const T* gt = (const T*)a.gt + sg.off;
  const int tid = threadIdx.x;
  constexpr bool gt64 = sizeof(T) == 8;
  if (tid == 0) { s_bin = 0; s_below = 0; }

  // torch.median: element (n - 1) / 2 of the sorted values (the clamp leaves them in [1e-3, 80]: positive floats)
  const float med = __uint_as_float(radix_select(pb, sg.slots, (sg.n - 1) / 2, hist, s_wave, &s_bin, &s_below).bits);
  // depth_pred *= median(gt[mask]) / median(depth_pred[mask]): the quotient of two 0-dim tensors is taken in their promoted
  // dtype (f64 with f64 ground truth); the in-place multiply of the float32 map casts that 0-dim operand to float32 first
  // (TensorIterator's common dtype is the dimensioned operand's), so the ratio is rounded to float32 BEFORE the multiply
  const double ratio = gt64 ? sg.med_gt / (double)med : (double)((float)sg.med_gt / med);
  const float ratio_f = (float)ratio;

  double s[kSums];
  int c[kCounts];
  for (int q = 0; q < kSums; ++q) s[q] = 0.0;
  for (int q = 0; q < kCounts; ++q) c[q] = 0;
  for (int i = tid; i < sg.slots; i += kImgThreads) {
    const uint32_t u = pb[i];
    if (u == kInvalid) {
      if (scaled) scaled[i] = 0.f;
      continue;
    }
    const float p = clamp_t(__uint_as_float(u) * ratio_f);
    if (scaled) scaled[i] = p;
    double t[4];
    int f[3];
    point_terms<T, float>(gt[i], p, t, f);
    const bool in = reg[i] != 0;  // the object region takes the same terms: sums per thread in f64 (f64's own for f64 ground truth)
    for (int q = 0; q < 4; ++q) {
      s[q] += t[q];
      if (in) s[4 + q] += t[q];
    }
    for (int q = 0; q < 3; ++q) {
      c[q] += f[q];
      if (in) c[3 + q] += f[q];
    }
    c[6] += 1;
    c[7] += in ? 1 : 0;
  }
  // fixed shuffle tree, then the waves in order
  const int lane = tid & 63, w = tid >> 6;
  for (int q = 0; q < kSums; ++q) {
    const double t = wave_sum_d(s[q]);
    if (lane == 0) s_red[q][w] = t;
  }
  for (int q = 0; q < kCounts; ++q) {
    int t = c[q];
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
    if (lane == 0) s_cnt[q][w] = t;
  }
  __syncthreads();
  if (tid == 0) {
    double t[kSums];
    int n[kCounts];
    for (int q = 0; q < kSums; ++q) {
      double v = 0.0;
      for (int i = 0; i < kImgWaves; ++i) v += s_red[q][i];
      t[q] = v;
    }
    for (int q = 0; q < kCounts; ++q) {
      int v = 0;
      for (int i = 0; i < kImgWaves; ++i) v += s_cnt[q][i];
      n[q] = v;
    }
    double* o = a.img_out + (size_t)img * kRow;
    finish_errors(t, n, n[6], !gt64, o);
    if (n[7] > 0) finish_errors(t + 4, n + 3, n[7], !gt64, o + 7);
    else
      for (int q = 7; q < 14; ++q) o[q] = 0.0;  // upstream's NaNs of an empty region are never added (:1249)
    o[14] = ratio;
    o[15] = (double)n[6];
    o[16] = (double)n[7];
    o[17] = (double)med;
  }
}

// Trainer.val's aggregation (:881-886 over what :1231-1252 accumulated), in image order
__global__ void eval_dyn_mean_kernel(const double* img_out, int n_images, double* out) {
  const int k = threadIdx.x;
  if (k >= MAL_EVAL_DYN_MEAN) return;
  double s = 0.0, cnt = 0.0;
  for (int i = 0; i < n_images; ++i) {
    const double* r = img_out + (size_t)i * kRow;
    const bool doj = r[16] > 0.0;
    if (doj) cnt += 1.0;
    if (k < 7) s += r[k];
    else if (k < 14) s += doj ? r[k] : 0.0;
    else if (k == 15) s += r[16];
    else if (k == 16) s += r[15];
  }
  if (k < 7) out[k] = s / (double)n_images;
  else if (k < 14) out[k] = s / cnt;  // doj/count == 0: 0/0 = NaN, as upstream's division
  else if (k == 14) out[k] = cnt;
  else out[k] = s;
}

template <typename T, typename M>
void launch(const mal_eval_dyn_args& a, float min_disp, float range, hipStream_t st) {
  hipLaunchKernelGGL((eval_dyn_predict_kernel<T, M>), dim3(kPredBlocksPerImage, a.B), dim3(kPredThreads), 0, st, a, min_disp,
                     range);
  hipLaunchKernelGGL(eval_dyn_image_kernel<T>, dim3(a.B), dim3(kImgThreads), 0, st, a);
}

}  // namespace

extern "C" int mal_eval_dyn_accumulate(const mal_eval_dyn_args* a) {
  if (!a || !a->seg || !a->gt || !a->disp || !a->mask || !a->pred || !a->region || !a->img_out) return MAL_EINVAL;
  if (a->n_images <= 0 || a->B < 1 || a->first < 0 || a->first > a->n_images - a->B) return MAL_EINVAL;
  if (a->H < 1 || a->W < 1 || a->mh < 1 || a->mw < 1) return MAL_EINVAL;
  if ((double)a->B * a->H * a->W > 2.0e9 || (double)a->B * a->mh * a->mw > 2.0e9 || a->B > 65535) return MAL_ESHAPE;
  if (a->mask_dtype != MAL_EVAL_MASK_F32 && a->mask_dtype != MAL_EVAL_MASK_U8) return MAL_EINVAL;
  if (!(a->min_depth > 0.0) || !(a->max_depth > a->min_depth) || !(a->max_depth < INFINITY)) return MAL_EINVAL;
  hipStream_t st = (hipStream_t)a->stream;
  // disp_to_depth's constants: 1/max and 1/min - 1/max in f64 from the Python floats, then float32 (torch's scalar args)
  const float min_disp = (float)(1.0 / a->max_depth);
  const float range = (float)(1.0 / a->min_depth - 1.0 / a->max_depth);
  const bool u8 = a->mask_dtype == MAL_EVAL_MASK_U8;
  if (a->gt_f64) {
    if (u8) launch<double, unsigned char>(*a, min_disp, range, st);
    else launch<double, float>(*a, min_disp, range, st);
  } else {
    if (u8) launch<float, unsigned char>(*a, min_disp, range, st);
    else launch<float, float>(*a, min_disp, range, st);
  }
  return launch_status();
}

extern "C" int mal_eval_dyn_mean(const double* img_out, int n_images, double* out, void* stream) {
  if (!img_out || !out || n_images <= 0) return MAL_EINVAL;
  hipLaunchKernelGGL(eval_dyn_mean_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, img_out, n_images, out);
  return launch_status();
}
