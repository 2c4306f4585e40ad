// The reduction and assembly tails of the one-call loss steps (mal_step.hip, mal_step_ms.hip, mal_dr_step.hip), defined
// once.  Every sum below is taken in a FIXED order with no floating-point atomics: the steps are bit-equal between runs and
// between the one-call and the operator routes because of it, so an order or a rounding point changes here or nowhere.
// Workgroups of 256 threads throughout.
#pragma once
#include "mal_common.h"
#include "mal_device.h"

namespace mal {

// ---- per-sample sums: 8 slots x 32 strided partial sums, then a 32-term sum per slot
// thread (slot j = tid & 7, sub = tid >> 3) continues its running sum over the partials sub, sub + 32, ... < n of one source;
// a caller chains its sources into one accumulator (independent loads: issued together)
MAL_DEV double tail_strided_sum(double acc, const double* q, size_t stride, int n, int sub) {
#pragma unroll 8
  for (int t = sub; t < n; t += 32) acc += q[(size_t)t * stride];
  return acc;
}
// ... and out[j] = the sum of slot j's 32 partial sums in `sub` order
MAL_DEV void tail_sample_sums(double acc, double* s_part /*[256]*/, double* out /*[8]*/) {
  const int tid = threadIdx.x;
  s_part[tid] = acc;
  __syncthreads();
  if (tid < 8) {
    double a = 0.0;
    for (int k = 0; k < 32; ++k) a += s_part[k * 8 + tid];
    out[tid] = a;
  }
}

// ---- pose gradients of sample b: g_T[f] = K_b^T [gP_f ; 0] from the per-task pose partials bgP[task][24].  24 sums of
// per_sample partials: 10 threads per value (240 of 256), then a 10-term sum (fixed order), then the product: thread
// tid < 32 returns entry e = tid & 15 of frame f = tid >> 4 (the others 0); the caller stores it in its own layout and scale
MAL_DEV double tail_pose_block(const float* bgP, int per_sample, const float* K, int b, double* s_part /*[256]*/,
                               double* s_gP /*[24]*/) {
  const int tid = threadIdx.x;
  const int v = tid % 24, sub = tid / 24;
  double acc = 0.0;
  if (sub < 10) {
#pragma unroll 8
    for (int t = sub; t < per_sample; t += 10) acc += (double)bgP[((size_t)b * per_sample + t) * 24 + v];
  }
  s_part[tid] = acc;
  __syncthreads();
  if (tid < 24) {
    double a = 0.0;
    for (int k = 0; k < 10; ++k) a += s_part[k * 24 + tid];
    s_gP[tid] = a;
  }
  __syncthreads();
  double a = 0.0;
  if (tid < 32) {
    const int f = tid >> 4, e = tid & 15, k = e >> 2, j = e & 3;
    const float* Kb = K + b * 16;
    for (int i = 0; i < 3; ++i) a += (double)Kb[i * 4 + k] * s_gP[f * 12 + i * 4 + j];
  }
  return a;
}

// ---- true in the workgroup of a 1-D grid that gets here last (ticket: a counter the step's first launch reset); every thread
// of it then sees what all the others stored before their call.  Publishing relies on this order: (1) the workgroup barrier --
// __syncthreads() is a workgroup-scope release/acquire, so every thread's stores above happen-before lane 0's fence (barrier
// cumulativity); (2) ONE agent-scope release fence by lane 0 (an L2 write-back: cheap once per workgroup, 40 us when all 256
// threads of 768 workgroups issued a __threadfence() each); (3) the ticket atomic; (4) an agent-scope acquire in the one
// workgroup that continues.
MAL_DEV bool tail_last_workgroup(unsigned* ticket) {
  __shared__ unsigned s_last;
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    s_last = atomicAdd(ticket, 1u);
  }
  __syncthreads();
  if (s_last != gridDim.x - 1) return false;
  __threadfence();  // (the one workgroup that continues: acquire what the others published)
  return true;
}

// ---- smoothness of the mean-normalised disparity (layers.py:210-223, loss_utils.py:119-121); q = a sample's 8 sums (slot 6:
// sum gn * disp, slot 7: sum disp), hw = pixels of the map the term is taken on
// 1 / (mean + 1e-7) as every consumer of a mean forms it
MAL_DEV float tail_inv_mean(double mean) { return div_(1.0f, (float)mean + 1e-7f); }
// the mean-coupling term of the smoothness gradient, dot / (hw (mean + eps)^2) with dot = sum gn * disp
MAL_DEV double tail_smooth_corr(double dot, double mean, double hw) {
  const double m = (double)((float)mean + 1e-7f);
  return dot / (hw * m * m);
}
// statistics of the smoothness gradient of one sample: the mean and the coupling term
MAL_DEV void tail_smooth_stats(const double* q, double hw, double* mean_out, double* corr_out) {
  const double mean = q[7] / hw;
  *mean_out = mean;
  *corr_out = tail_smooth_corr(q[6], mean, hw);
}
// slot j as it enters the sum over samples: slots 4, 5 (smoothness) weighted by the sample's 1 / (mean + 1e-7)
MAL_DEV double tail_weighted_slot(const double* q, int j, double hw) {
  double v = q[j];
  if (j == 4 || j == 5) v = v * (double)tail_inv_mean(q[7] / hw);
  return v;
}

// ---- the last workgroup of mal_step.hip / mal_step_ms.hip: from the per-sample sums ps[pass][b][8] (pass = net * S + s; its
// smoothness term lives on the (H >> s, W >> s) map) the statistics stats[pass * B + b] = mean, stats[(passes + pass) * B + b]
// = coupling term, and tot[pass][j] = the weighted slots added in sample order.  One thread per (pass, sample, slot) fetches and
// weighs its term (a single round trip for all of them), 8 threads per pass then add the B terms; beyond kTailStage terms the
// summing threads re-fetch theirs instead of finding them staged in LDS.  Ends with a barrier.
constexpr int kTailStage = 1024;
MAL_DEV void tail_sum_over_samples(const double* ps, int passes, int S, int B, int H, int W, double* stats, double (*tot)[8]) {
  __shared__ double s_term[kTailStage];
  const int tid = threadIdx.x, n = passes * B;
  auto hw_of = [&](int pass) { const int s = pass % S; return (double)((H >> s) * (W >> s)); };
  const bool staged = n * 8 <= kTailStage;
  for (int i = tid; staged && i < n * 8; i += 256) s_term[i] = tail_weighted_slot(ps + (size_t)(i >> 3) * 8, i & 7, hw_of((i >> 3) / B));
  for (int i = tid; i < n; i += 256) tail_smooth_stats(ps + (size_t)i * 8, hw_of(i / B), stats + i, stats + n + i);
  __syncthreads();
  if (tid < passes * 8) {
    const int pass = tid >> 3, j = tid & 7;
    const double hw = hw_of(pass);
    double a = 0.0;
    for (int b = 0; b < B; ++b)
      a += staged ? s_term[((size_t)pass * B + b) * 8 + j] : tail_weighted_slot(ps + ((size_t)pass * B + b) * 8, j, hw);
    tot[pass][j] = a;
  }
  __syncthreads();
}

// ---- one-row halo of the marching gradient passes (MarchParams::bnd): workgroup i = (sample, segment, first / last row) adds
// the neighbouring task's scratch row to that row of the pass's gradient map in place (one add per element)
MAL_DEV void tail_fold_boundary_row(float* G, const float* bnd, int i, int H, int W, int rows, int segs) {
  const int which = i & 1, bs = i >> 1, seg = bs % segs, b = bs / segs;
  if ((which == 0 && seg == 0) || (which == 1 && seg == segs - 1)) return;  // the image's own border: nobody beyond it
  const int y = which == 0 ? seg * rows : min(seg * rows + rows, H) - 1;
  float* g = G + ((size_t)b * H + y) * W;
  const float* r = bnd + ((size_t)(b * segs + seg) * 2 + which) * W;
  for (int x = threadIdx.x; x < W; x += 256) g[x] += r[x];
}

// ---- per-pixel terms of the assembly kernels
// the unnormalised reprojection gradient at pixel i (column x), completed by the neighbouring task's scratch row where its row
// is a segment boundary (brow: march_boundary_row, nullable)
MAL_DEV float tail_boundary_G(const float* G, const float* brow, size_t i, int x) { return brow ? G[i] + brow[x] : G[i]; }
// d (weighted smoothness) / d disp: gn = d / d normalised disparity, inv = tail_inv_mean(mean_b), corr = the coupling term
MAL_DEV float tail_smooth_grad(float cS, float gn, float inv, float corr) { return cS * (gn * inv - corr); }

}  // namespace mal
