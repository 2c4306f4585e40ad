// What the two depth evaluators (mal_eval.hip: MAL's Trainer.val with numpy's rules; mal_dyn_eval.hip: DynamicDepth's
// compute_depth_losses with torch's) share on the device, defined once: the launch constants, the packed-slot decode, the
// exact select on the float bits, the per-point error terms and the promoted-dtype means.  The files keep what differs: the
// resize rule, clamps, ratio rounding, regions, row layout, mean kernels.  A select spread over several workgroups
//  would replace radix_select here, for both.
#pragma once
#include "mal_common.h"
#include "mal_device.h"

namespace mal {

constexpr int kImgThreads = 1024;   // per-image workgroup: 16 waves
constexpr int kImgWaves = kImgThreads / 64;
constexpr int kPredThreads = 256;
constexpr int kPredBlocksPerImage = 32;
constexpr uint32_t kInvalid = 0xffffffffu;  // pred slot of a dense pixel outside the mask

// np.log / torch.log of a float32 array, as the correctly rounded value (numpy's SIMD logf is within a few ulp of it)
MAL_DEV float logf_cr(float x) { return (float)log((double)x); }

// pixel (x, y) of the full ground truth that packed slot i of a segment stands for: a dense window's slots run row by row
// from (x0, y0); a sparse segment carries its flat indices
MAL_DEV void slot_xy(const mal_eval_seg& sg, const int* __restrict__ idx, int i, int& x, int& y) {
  if (sg.dense) {
    y = sg.y0 + i / sg.rw;
    x = sg.x0 + (i - (i / sg.rw) * sg.rw);
  } else {
    const int f = idx[sg.off + i];
    y = f / sg.gt_w;
    x = f - y * sg.gt_w;
  }
}

// exclusive prefix sum over the workgroup (wave scan with shuffles, then the waves in order)
__device__ inline int block_excl_scan(int v, int* s_wave) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) s_wave[w] = x;
  __syncthreads();
  int b = 0;
  for (int i = 0; i < w; ++i) b += s_wave[i];
  __syncthreads();
  return b + x - v;
}

// bits: the value of rank k; k_left: k minus the number of values below it; cnt_eq: how many values equal it
struct Selected {
  uint32_t bits;
  int k_left, cnt_eq;
};

// The value of rank k (0-based) among the valid slots of pb, by a radix select on the bits of positive floats (monotone):
// 12 + 12 + 8 bits, one LDS histogram per pass.  The whole workgroup of kImgThreads calls it; hist[4096], s_wave[kImgWaves],
// *s_bin and *s_below are the caller's LDS (both zeroed by the caller before the call), and every thread gets the result.
MAL_DEV Selected radix_select(const uint32_t* __restrict__ pb, int slots, int k, uint32_t* hist, int* s_wave, int* s_bin,
                              int* s_below) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0, pmask = 0;
  int cnt_eq = 0;
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 20 : (pass == 1 ? 8 : 0);
    const int nb = pass == 2 ? 256 : 4096;
    for (int i = tid; i < nb; i += kImgThreads) hist[i] = 0u;
    __syncthreads();
    for (int i = tid; i < slots; i += kImgThreads) {
      const uint32_t u = pb[i];
      if (u != kInvalid && (u & pmask) == prefix) atomicAdd(&hist[(u >> shift) & (uint32_t)(nb - 1)], 1u);
    }
    __syncthreads();
    const int per = (nb + kImgThreads - 1) / kImgThreads;
    const int b0 = tid * per, b1 = min(b0 + per, nb);
    int local = 0;
    for (int b = b0; b < b1; ++b) local += (int)hist[b];
    const int excl = block_excl_scan(local, s_wave);
    if (k >= excl && k < excl + local) {
      int c = excl;
      for (int b = b0; b < b1; ++b) {
        if (k < c + (int)hist[b]) { *s_bin = b; *s_below = c; break; }
        c += (int)hist[b];
      }
    }
    __syncthreads();
    const int b = *s_bin;
    prefix |= (uint32_t)b << shift;
    pmask |= (uint32_t)(nb - 1) << shift;
    k -= *s_below;
    if (pass == 2) cnt_eq = (int)hist[b];
    __syncthreads();
  }
  return {prefix, k, cnt_eq};
}

// One point's four terms (abs_rel, sq_rel, squared difference, squared log difference) and three comparisons
// thresh < 1.25^k of compute_errors / compute_depth_errors under numpy's and torch's promotion alike: float64 arithmetic if
// either operand is float64 (the other is widened), the log of each operand in its own dtype
template <typename G, typename P>
MAL_DEV void point_terms(G g, P p, double* t, int* c) {
  if constexpr (sizeof(G) == 8 || sizeof(P) == 8) {
    const double gd = (double)g, pd = (double)p;
    const double d = gd - pd;
    t[0] = fabs(d) / gd;
    t[1] = (d * d) / gd;
    t[2] = d * d;
    const double lgg = sizeof(G) == 8 ? log(gd) : (double)logf_cr((float)g);
    const double lgp = sizeof(P) == 8 ? log(pd) : (double)logf_cr((float)p);
    const double l = lgg - lgp;
    t[3] = l * l;
    const double th = fmax(gd / pd, pd / gd);
    c[0] = th < 1.25 ? 1 : 0;
    c[1] = th < 1.5625 ? 1 : 0;
    c[2] = th < 1.953125 ? 1 : 0;
  } else {
    const float gf = (float)g, pf = (float)p;
    const float d = gf - pf;
    t[0] = (double)(fabsf(d) / gf);
    t[1] = (double)((d * d) / gf);
    t[2] = (double)(d * d);
    const float l = logf_cr(gf) - logf_cr(pf);
    t[3] = (double)(l * l);
    const float th = fmaxf(gf / pf, pf / gf);
    c[0] = th < 1.25f ? 1 : 0;
    c[1] = th < 1.5625f ? 1 : 0;
    c[2] = th < 1.953125f ? 1 : 0;
  }
}

// abs_rel, sq_rel, rmse, rmse_log from the four f64 sums over n points: means in the promoted dtype (float32 when both
// operands were).  a1..a3 are means of booleans, which numpy and torch type differently: each file has its own rule
MAL_DEV void finish_means4(const double* s4, double n, bool f32, double* out) {
  if (f32) {
    out[0] = (double)(float)(s4[0] / n);
    out[1] = (double)(float)(s4[1] / n);
    out[2] = (double)sqrtf((float)(s4[2] / n));
    out[3] = (double)sqrtf((float)(s4[3] / n));
  } else {
    out[0] = s4[0] / n;
    out[1] = s4[1] / n;
    out[2] = sqrt(s4[2] / n);
    out[3] = sqrt(s4[3] / n);
  }
}

}  // namespace mal
