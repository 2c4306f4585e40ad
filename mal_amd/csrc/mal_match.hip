// The temporal-hint producer's instance matcher: manydepth/matcher.py:89-173, `HungarianMatcher.memory_efficient_forward`
// (instances of the two warped frames `n`, `m` against the confident instances `0` of the target frame).
//
// Upstream forms two dense fp32 einsums over (N, H*W) sigmoid copies of the masks, takes both cost matrices to the host,
// runs scipy's linear_sum_assignment twice, intersects the assigned target columns in Python and copies the two index
// lists back.  The masks it is given are BINARY floats ((mask_pred > 0).float(), mask2former/maskformer_model.py:371), so
// sigmoid takes two values only and both sums of the dice term are exact functions of three integers per pair:
//   c11 = |a & t|, cnt_a = |a|, cnt_t = |t|
//   sum sigma(a) t = 0.5 (cnt_t - c11) + s1 c11        sum sigma(a) = 0.5 (HW - cnt_a) + s1 cnt_a       s1 = sigmoid(1.0f)
// Three launches on the caller's stream, no atomics, integer sums and a fixed reduction order (bit-reproducible):
//   match_pack_kernel    every mask of the three sets -> a row of ceil(HW/64) 64-bit words (a wave reads 64 consecutive
//                        elements, __ballot(x != 0) is the word; the tail word is zero-padded) and its population count
//                        per band of words; a float32 element that is neither 0 nor 1 sets the sticky word result[1]
//   match_cost_kernel    both matrices: per (row, 8 target columns) a wave runs over the words, popcount(a & t), wave
//                        reduction; the cost is formed in fp64 from the three integers and rounded ONCE to fp32
//   match_assign_kernel  one workgroup, one wavefront per matrix: rectangular linear assignment by shortest augmenting
//                        paths with duals (Jonker-Volgenant as Crouse states it, what scipy runs), fp64, candidate
//                        columns over the lanes (two per lane above 64), lowest index on a tie; then the target columns
//                        assigned in both problems, in ascending order -> slice_n, slice_m, result[0] = count
#include "mal_common.h"
#include "mal_device.h"

namespace mal {

constexpr int kPackBands = 8;     // bands of words per mask in the packing launch (one workgroup each)
constexpr int kPackThreads = 256;
constexpr int kCostTile = 8;      // target columns per wave of the cost launch: the row's word stays in a register
// torch's fp32 sigmoid of 1.0f (0x3f3b26a8), the only value of sigma(a) besides 0.5f on a binary mask
constexpr double kSigmoid1 = 0.731058597564697265625;

struct MatchParams {
  const void* masks[3];        // n, m, 0
  int kind[3];                 // MAL_MATCH_U8 / MAL_MATCH_F32
  int num[3];
  const long long* cls[3];
  int HW, nw;                  // elements and 64-bit words per mask
  unsigned long long* words;   // [num_n + num_m + num_0][nw]
  int* cnt;                    // [num_n + num_m + num_0][kPackBands]
  double w_class, w_dice;
  float* C[2];                 // (num_n, num_0), (num_m, num_0)
  long long* slice[2];
  int* result;                 // count, non-binary, 0, 0
};

__global__ __launch_bounds__(kPackThreads) void match_pack_kernel(MatchParams p) {
  __shared__ int s_cnt[kPackThreads / 64];
  const int g = blockIdx.y, band = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int set = g < p.num[0] ? 0 : (g < p.num[0] + p.num[1] ? 1 : 2);
  const int i = g - (set == 0 ? 0 : (set == 1 ? p.num[0] : p.num[0] + p.num[1]));
  const int per = (p.nw + kPackBands - 1) / kPackBands, w_lo = band * per, w_hi = min(w_lo + per, p.nw);
  unsigned long long* out = p.words + (size_t)g * p.nw;
  const bool f32 = p.kind[set] == MAL_MATCH_F32;
  const float* mf = (const float*)p.masks[set] + (size_t)i * p.HW;
  const uint8_t* mb = (const uint8_t*)p.masks[set] + (size_t)i * p.HW;
  int cnt = 0;  // wave-uniform: the ballot is
  bool bad = false;
  constexpr int kWaves = kPackThreads / 64;
  for (int w = w_lo + wave; w < w_hi; w += 4 * kWaves) {  // four words per trip: the loads are issued together
    bool on[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ww = w + q * kWaves;
      const long long k = (long long)ww * 64 + lane;
      on[q] = false;
      if (ww < w_hi && k < p.HW) {
        if (f32) { const float x = mf[k]; on[q] = x != 0.f; bad |= x != 0.f && x != 1.f; }
        else on[q] = mb[k] != 0;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ww = w + q * kWaves;
      if (ww >= w_hi) break;  // wave-uniform
      const unsigned long long bits = __ballot(on[q]);
      if (lane == 0) out[ww] = bits;
      cnt += __popcll(bits);
    }
  }
  if (bad) p.result[1] = 1;  // every writer stores the same value
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int k = 0; k < kPackThreads / 64; ++k) s += s_cnt[k];
    p.cnt[g * kPackBands + band] = s;
  }
}

MAL_DEV int match_count(const int* cnt, int g) {
  int s = 0;
  for (int k = 0; k < kPackBands; ++k) s += cnt[g * kPackBands + k];
  return s;
}

__global__ __launch_bounds__(64) void match_cost_kernel(MatchParams p) {
  const int r = blockIdx.y, j0 = blockIdx.x * kCostTile, lane = threadIdx.x;
  const int which = r < p.num[0] ? 0 : 1, i = which ? r - p.num[0] : r;
  const int n0 = p.num[2], g0 = p.num[0] + p.num[1];
  const unsigned long long* a = p.words + (size_t)r * p.nw;
  const unsigned long long* t = p.words + (size_t)(g0 + j0) * p.nw;
  int acc[kCostTile];
#pragma unroll
  for (int c = 0; c < kCostTile; ++c) acc[c] = 0;
  for (int w = lane; w < p.nw; w += 64) {
    const unsigned long long aw = a[w];
#pragma unroll
    for (int c = 0; c < kCostTile; ++c)
      if (j0 + c < n0) acc[c] += __popcll(aw & t[(size_t)c * p.nw + w]);
  }
#pragma unroll
  for (int c = 0; c < kCostTile; ++c)
    for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
  const double cnt_a = (double)match_count(p.cnt, r);
  const double sum_a = 0.5 * ((double)p.HW - cnt_a) + kSigmoid1 * cnt_a;  // sum of sigmoid(a)
  const long long cls_a = p.cls[which][i];
#pragma unroll
  for (int c = 0; c < kCostTile; ++c) {
    const int j = j0 + c;
    if (lane != c || j >= n0) continue;
    const double c11 = (double)acc[c], cnt_t = (double)match_count(p.cnt, g0 + j);
    const double inter = 0.5 * (cnt_t - c11) + kSigmoid1 * c11;            // sum of sigmoid(a) * t
    const double dice = 1.0 - (2.0 * inter + 1.0) / (sum_a + cnt_t + 1.0);  // matcher.py:19-23
    const double cost = p.w_class * (cls_a != p.cls[2][j] ? 1.0 : 0.0) + p.w_dice * dice;
    p.C[which][(size_t)i * n0 + j] = (float)cost;
  }
}

// value of a per-lane pair of registers (element e lives in lane e & 63, register e >> 6) at index e (wave-uniform or
// per lane); call it where the whole wave is active
template <typename T>
MAL_DEV T match_at(const T (&r)[2], int e) {
  const T lo = __shfl(r[0], e & 63, 64), hi = __shfl(r[1], e & 63, 64);
  return e < 64 ? lo : hi;
}

// One wavefront solves min sum_i cost(i, col(i)) over nr <= nc <= MAL_MATCH_MAX (every row assigned, distinct columns);
// cost(i, j) = C[i * si + j * sj].  On return col_of[k] of a lane is the column of row lane + 64 k (or -1 beyond nr) and
// row_of[k] the row of column lane + 64 k (or -1).  Crouse, "On implementing 2D rectangular assignment algorithms" (2016),
// the algorithm of scipy.optimize.linear_sum_assignment; every loop is bounded by the matrix dimensions.
MAL_DEV void match_solve(const float* C, int nr, int nc, int si, int sj, int (&col_of)[2], int (&row_of)[2]) {
  const int lane = threadIdx.x & 63;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  double u[2] = {0.0, 0.0}, v[2] = {0.0, 0.0};  // duals of rows / columns lane, lane + 64
  col_of[0] = col_of[1] = row_of[0] = row_of[1] = -1;
  for (int cur = 0; cur < nr; ++cur) {
    double spc[2] = {inf, inf};  // shortest path cost to each column
    int path[2] = {-1, -1};
    bool sc[2] = {false, false};  // column scanned
    double min_val = 0.0;
    int i = cur, sink = -1;
    for (int it = 0; it < nc && sink < 0; ++it) {
      const double ui = match_at(u, i);
      double best = inf;
      int best_j = 0x7fffffff;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int j = lane + 64 * k;
        if (j < nc && !sc[k]) {
          const double r = min_val + (double)C[(size_t)i * si + (size_t)j * sj] - ui - v[k];
          if (r < spc[k]) { spc[k] = r; path[k] = i; }
          if (spc[k] < best) { best = spc[k]; best_j = j; }  // (k = 1 holds the higher index: ties stay with k = 0)
        }
      }
      for (int o = 32; o > 0; o >>= 1) {  // minimum over the wave, the lowest column on a tie
        const double ob = __shfl_xor(best, o, 64);
        const int oj = __shfl_xor(best_j, o, 64);
        if (ob < best || (ob == best && oj < best_j)) { best = ob; best_j = oj; }
      }
      if (best_j == 0x7fffffff) break;  // no finite candidate: cannot happen with finite costs
      min_val = best;
      const int j = best_j;
      if (lane == (j & 63)) sc[j >> 6] = true;
      const int r4 = match_at(row_of, j);
      if (r4 < 0) sink = j; else i = r4;
    }
    if (sink < 0) break;
    // duals: rows reached (cur and the rows of the scanned columns), columns scanned
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int row = lane + 64 * k, c = col_of[k];
      const int cc = c < 0 ? 0 : c;
      // (both registers are read by EVERY lane and selected afterwards: a shuffle inside a branch on the lane's own column
      // would read from lanes the branch has switched off)
      const int sci[2] = {(int)sc[0], (int)sc[1]};
      const double spc_c = match_at(spc, cc);
      const int sc_c = match_at(sci, cc);
      if (row == cur) u[k] += min_val;
      else if (c >= 0 && sc_c) u[k] += min_val - spc_c;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (sc[k]) v[k] -= min_val - spc[k];
    // augment along the path from the sink back to cur
    int j = sink;
    for (int it = 0; it <= nr; ++it) {
      const int ri = match_at(path, j);
      if (lane == (j & 63)) row_of[j >> 6] = ri;
      const int old = match_at(col_of, ri);
      if (lane == (ri & 63)) col_of[ri >> 6] = j;
      j = old;
      if (ri == cur || j < 0) break;
    }
  }
}

__global__ __launch_bounds__(128) void match_assign_kernel(MatchParams p) {
  __shared__ int s_row[2][MAL_MATCH_MAX];  // per problem: the instance assigned to each target column, or -1
  const int which = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nr = p.num[which], n0 = p.num[2];
  int col_of[2], row_of[2];
  // augment over the smaller dimension: the solver's rows are the instances, or (transposed) the targets
  const bool tr = n0 < nr;
  if (tr) match_solve(p.C[which], n0, nr, 1, n0, col_of, row_of);
  else match_solve(p.C[which], nr, n0, n0, 1, col_of, row_of);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int t = lane + 64 * k;
    if (t < MAL_MATCH_MAX) s_row[which][t] = t < n0 ? (tr ? col_of[k] : row_of[k]) : -1;
  }
  __syncthreads();
  if (which != 0) return;
  int base = 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int t = lane + 64 * k;
    const int a = s_row[0][t], b = s_row[1][t];
    const bool both = a >= 0 && b >= 0;
    const unsigned long long m = __ballot(both);
    if (both) {
      const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
      p.slice[0][pos] = a;
      p.slice[1][pos] = b;
    }
    base += __popcll(m);
  }
  if (lane == 0) p.result[0] = base;
}

}  // namespace mal

using namespace mal;

static size_t match_words(int H, int W) { return ((size_t)H * (size_t)W + 63) / 64; }

static bool match_sizes_ok(int n_n, int n_m, int n_0, int H, int W) {
  if (n_n < 0 || n_m < 0 || n_0 < 0 || n_n > MAL_MATCH_MAX || n_m > MAL_MATCH_MAX || n_0 > MAL_MATCH_MAX) return false;
  if (H <= 0 || W <= 0 || (double)H * (double)W > 2.0e9) return false;  // int32 element index, + 63 included
  return true;
}

extern "C" size_t mal_match_workspace_bytes(int n_n, int n_m, int n_0, int H, int W) {
  if (!match_sizes_ok(n_n, n_m, n_0, H, W)) return 0;
  const size_t total = (size_t)n_n + n_m + n_0;
  return align256(total * match_words(H, W) * sizeof(unsigned long long)) + align256(total * kPackBands * sizeof(int)) + 256;
}

extern "C" int mal_match(const mal_match_args* a) {
  if (!a) return MAL_EINVAL;
  if (!match_sizes_ok(a->n_n, a->n_m, a->n_0, a->H, a->W)) return MAL_EINVAL;
  const int num[3] = {a->n_n, a->n_m, a->n_0};
  const void* masks[3] = {a->masks_n, a->masks_m, a->masks_0};
  const int kind[3] = {a->kind_n, a->kind_m, a->kind_0};
  const int64_t* cls[3] = {a->class_n, a->class_m, a->class_0};
  for (int s = 0; s < 3; ++s) {
    if (kind[s] != MAL_MATCH_U8 && kind[s] != MAL_MATCH_F32) return MAL_EINVAL;
    if (num[s] > 0 && (!masks[s] || !cls[s])) return MAL_EINVAL;
  }
  if (!a->slice_n || !a->slice_m || !a->result || !a->ws) return MAL_EINVAL;
  if ((a->n_n > 0 && a->n_0 > 0 && !a->C1) || (a->n_m > 0 && a->n_0 > 0 && !a->C2)) return MAL_EINVAL;
  if (!(a->cost_class == a->cost_class) || !(a->cost_mask == a->cost_mask) || !(a->cost_dice == a->cost_dice)) return MAL_EINVAL;
  if (a->cost_class == 0.0 && a->cost_mask == 0.0 && a->cost_dice == 0.0) return MAL_EINVAL;  // matcher.py:86
  if (a->ws_bytes < mal_match_workspace_bytes(a->n_n, a->n_m, a->n_0, a->H, a->W)) return MAL_EWORKSPACE;
  hipStream_t st = (hipStream_t)a->stream;
  const int total = a->n_n + a->n_m + a->n_0;
  MatchParams p;
  for (int s = 0; s < 3; ++s) {
    p.masks[s] = masks[s]; p.kind[s] = kind[s]; p.num[s] = num[s]; p.cls[s] = (const long long*)cls[s];
  }
  p.HW = a->H * a->W;
  p.nw = (int)match_words(a->H, a->W);
  char* base = (char*)(((uintptr_t)a->ws + 255) & ~(uintptr_t)255);
  p.words = (unsigned long long*)base;
  p.cnt = (int*)(base + align256((size_t)total * p.nw * sizeof(unsigned long long)));
  p.w_class = a->cost_class; p.w_dice = a->cost_dice;
  p.C[0] = a->C1; p.C[1] = a->C2;
  p.slice[0] = (long long*)a->slice_n; p.slice[1] = (long long*)a->slice_m;
  p.result = a->result;
  if (hipMemsetAsync(a->result, 0, 4 * sizeof(int32_t), st) != hipSuccess) return MAL_ELAUNCH;
  if (total == 0) return MAL_OK;
  hipLaunchKernelGGL(match_pack_kernel, dim3(kPackBands, total), dim3(kPackThreads), 0, st, p);
  if (a->n_0 == 0 || a->n_n + a->n_m == 0) return launch_status();
  hipLaunchKernelGGL(match_cost_kernel, dim3((a->n_0 + kCostTile - 1) / kCostTile, a->n_n + a->n_m), dim3(64), 0, st, p);
  // an empty side: count = 0 (the memset), the solver is not launched
  if (a->n_n > 0 && a->n_m > 0) hipLaunchKernelGGL(match_assign_kernel, dim3(1), dim3(128), 0, st, p);
  return launch_status();
}
