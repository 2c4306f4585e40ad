// Multi-scale deformable attention, forward only: the operator of Mask2Former's pixel decoder
// (mask2former/modeling/pixel_decoder/ops), whose upstream extension is CUDA-only.  The arithmetic is that of
// ms_deformable_im2col_gpu_kernel (ops/src/cuda/ms_deform_im2col_cuda.cuh:242-304), which is the function
// ms_deform_attn_core_pytorch (ops/functions/ms_deform_attn_func.py:52-72) computes through grid_sample:
//   out[n, q, m, :] = sum_l sum_p w[n,q,m,l,p] * bilinear(value_l[n, :, m, :], x * W_l - 0.5, y * H_l - 0.5)
// zero padding, align_corners=False; a sample counts only when y > -1 && x > -1 && y < H && x < W, and each corner is
// tested for range before it is read.  Every test is made in float before any float -> int conversion: a NaN or infinite
// location fails the first test, contributes zero and never forms an index.
//
// One kernel, two routes:
//   plain   sampling_locations (N,Lq,M,L,P,2) and attention_weights (N,Lq,M,L,P) as given
//   fused   the two linear layers' raw outputs, offsets (N,Lq,M,L,P,2) and logits (N,Lq,M,L*P), plus reference_points
//           (N,Lq,L,2|4): the max-subtracted softmax over L*P and the location arithmetic of
//           ops/modules/ms_deform_attn.py:104-112 happen in LDS, in the roundings torch makes (true divisions, no fma)
//
// Work decomposition.  A "row" is one (n, q, m): D contiguous output floats, L*P samples whose 2 L P location floats and
// L P weights are contiguous too.  A lane owns VEC consecutive channels of a row (VEC = 4: float4 loads and stores when
// D % 4 == 0 and the pointers are 16-byte aligned; VEC = 1 otherwise), so D / VEC lanes cover a row and, at M = 8, D = 32, one
// wave covers one query's 256 channels: each corner fetch is one 128-byte segment per lane group and the wave's store is
// 1 KiB contiguous.  A workgroup owns `rows` consecutive rows (linear in q: queries of one level are spatial neighbours and
// share value rows in L2); it first loads their locations and weights into LDS with coalesced loads, then every lane reads
// its row's samples from there (a broadcast inside the lane group).  No atomics, no readback; spatial_shapes and
// level_start_index are read on the device, as upstream does, so the call can be captured in a graph.
//
// Guard: a level is used only if 1 <= H, W <= min(S, 2^24), start >= 0 and start + H*W <= S (64-bit arithmetic that cannot
// overflow after the first test); otherwise it contributes zero and reads nothing.
#include "mal_common.h"

namespace mal {

constexpr int kMsdaThreads = 256;
constexpr int kMsdaLdsFloats = 4096;  // locations + weights (+ softmax sums) of a workgroup's rows: 16 KiB at most

struct MsdaParams {
  const float* value;         // (N, S, M, D)
  const long long* shapes;    // (L, 2)  H_l, W_l
  const long long* start;     // (L)
  const float* loc;           // plain: locations (N,Lq,M,L,P,2); fused: offsets, same layout
  const float* wgt;           // plain: weights (N,Lq,M,L,P);     fused: logits, same layout
  const float* ref;           // fused: (N, Lq, L, ref_dim)
  float* out;                 // (N, Lq, M*D)
  int N, S, M, D, L, P, Lq, ref_dim;
  int rows;                   // rows per workgroup
  long long total_rows;       // N * Lq * M
};

struct MsdaLevel { int H, W; long long start; bool ok; };

__device__ __forceinline__ MsdaLevel msda_level(const MsdaParams& p, int l) {
  MsdaLevel v;
  const long long H = p.shapes[2 * l], W = p.shapes[2 * l + 1], st = p.start[l];
  // (H, W <= 2^24: (float)H and (float)W are exact, so the float range tests below are the integer ones)
  v.ok = H >= 1 && W >= 1 && H <= (long long)p.S && W <= (long long)p.S && H <= (1ll << 24) && W <= (1ll << 24) && st >= 0 &&
         st <= (long long)p.S && st + H * W <= (long long)p.S;
  v.H = (int)H; v.W = (int)W; v.start = st;
  return v;
}

template <int VEC> struct MsdaVec;
template <> struct MsdaVec<1> {
  typedef float T;
  static __device__ __forceinline__ T zero() { return 0.f; }
  static __device__ __forceinline__ T mul(float a, T v) { return a * v; }
  static __device__ __forceinline__ T add(T a, T b) { return a + b; }
};
template <> struct MsdaVec<4> {
  typedef float4 T;
  static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ T mul(float a, T v) { return make_float4(a * v.x, a * v.y, a * v.z, a * v.w); }
  static __device__ __forceinline__ T add(T a, T b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
};

template <int VEC, bool FUSED>
__global__ __launch_bounds__(kMsdaThreads) void msda_fwd_kernel(MsdaParams p) {
  typedef MsdaVec<VEC> V;
  typedef typename V::T vec_t;
  extern __shared__ __align__(16) float s_mem[];
  const int LP = p.L * p.P, tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * p.rows;
  const int nrows = (int)min((long long)p.rows, p.total_rows - row0);  // >= 1 by the grid size
  float* s_loc = s_mem;                       // [rows][LP][2]
  float* s_w = s_mem + (size_t)p.rows * LP * 2;  // [rows][LP]
  // the workgroup's locations and weights: two contiguous pieces of global memory
  {
    const float* g_loc = p.loc + row0 * LP * 2;
    const float* g_w = p.wgt + row0 * LP;
    for (int i = tid; i < nrows * LP * 2; i += kMsdaThreads) s_loc[i] = g_loc[i];
    for (int i = tid; i < nrows * LP; i += kMsdaThreads) s_w[i] = g_w[i];
  }
  __syncthreads();
  if (FUSED) {
    float* s_sum = s_w + (size_t)p.rows * LP;  // [rows]
    // softmax over the L*P logits of a row (ms_deform_attn.py:104): e = exp(x - max) in place, their sum in index order
    if (tid < nrows) {
      float* x = s_w + tid * LP;
      float m = x[0];
      for (int k = 1; k < LP; ++k) m = fmaxf(m, x[k]);
      float s = 0.f;
      for (int k = 0; k < LP; ++k) {
        const float e = expf(x[k] - m);
        x[k] = e;
        s += e;
      }
      s_sum[tid] = s;
    }
    __syncthreads();
    // per sample: the weight e / sum and the location (:106-112), in place
    for (int i = tid; i < nrows * LP; i += kMsdaThreads) {
      const int r = i / LP, k = i - r * LP, l = k / p.P;
      s_w[i] = s_w[i] / s_sum[r];
      const long long nq = (row0 + r) / p.M;
      const float* rp = p.ref + (nq * p.L + l) * p.ref_dim;
      const float ox = s_loc[2 * i], oy = s_loc[2 * i + 1];
      float x, y;
      if (p.ref_dim == 2) {  // ref + off / (W_l, H_l)
        x = rp[0] + ox / (float)p.shapes[2 * l + 1];
        y = rp[1] + oy / (float)p.shapes[2 * l];
      } else {               // ref[:2] + off / P * ref[2:] * 0.5
        x = rp[0] + ox / (float)p.P * rp[2] * 0.5f;
        y = rp[1] + oy / (float)p.P * rp[3] * 0.5f;
      }
      s_loc[2 * i] = x;
      s_loc[2 * i + 1] = y;
    }
    __syncthreads();
  }
  const int lpr = p.D / VEC;  // lanes per row
  const int r = tid / lpr, c = (tid - r * lpr) * VEC;
  if (r >= nrows) return;     // (no barrier below)
  const long long row = row0 + r;
  const int m = (int)(row % p.M);
  const long long n = row / ((long long)p.M * p.Lq);
  const int MD = p.M * p.D;
  const float* vbase = p.value + (size_t)n * p.S * MD + (size_t)m * p.D + c;
  const float* lc = s_loc + (size_t)r * LP * 2;
  const float* wt = s_w + (size_t)r * LP;
  vec_t acc = V::zero();
  for (int l = 0; l < p.L; ++l) {
    const MsdaLevel lv = msda_level(p, l);
    if (!lv.ok) continue;  // uniform over the grid
    const float Hf = (float)lv.H, Wf = (float)lv.W;
    const float* vl = vbase + (size_t)lv.start * MD;
    for (int k = 0; k < p.P; ++k) {
      const int i = l * p.P + k;
      const float y = lc[2 * i + 1] * Hf - 0.5f, x = lc[2 * i] * Wf - 0.5f;
      if (!(y > -1.f && x > -1.f && y < Hf && x < Wf)) continue;  // NaN fails here
      const float yl = floorf(y), xl = floorf(x);  // in [-1, H-1] and [-1, W-1]
      const float lh = y - yl, lw = x - xl, hh = 1.f - lh, hw = 1.f - lw;
      const bool y0 = yl >= 0.f, y1 = yl + 1.f <= Hf - 1.f, x0 = xl >= 0.f, x1 = xl + 1.f <= Wf - 1.f;
      const int iy = (int)yl, ix = (int)xl;
      const float* at = vl + ((ptrdiff_t)iy * lv.W + ix) * MD;  // formed, not read, when a corner is outside
      vec_t v1 = V::zero(), v2 = V::zero(), v3 = V::zero(), v4 = V::zero();
      if (y0 && x0) v1 = *(const vec_t*)at;
      if (y0 && x1) v2 = *(const vec_t*)(at + MD);
      if (y1 && x0) v3 = *(const vec_t*)(at + (ptrdiff_t)lv.W * MD);
      if (y1 && x1) v4 = *(const vec_t*)(at + (ptrdiff_t)lv.W * MD + MD);
      const float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
      const vec_t val = V::add(V::add(V::add(V::mul(w1, v1), V::mul(w2, v2)), V::mul(w3, v3)), V::mul(w4, v4));
      acc = V::add(acc, V::mul(wt[i], val));
    }
  }
  *(vec_t*)(p.out + (size_t)row * p.D + c) = acc;
}

}  // namespace mal

using namespace mal;

struct MsdaPlan { int vec, rows, blocks; size_t lds; };

// the launch of either route for a shape, pure host code: both entry points and mal_msda_plan take their numbers from here
static int msda_plan(int N, int S, int Lq, int M, int D, int L, int P, bool aligned, MsdaPlan* pl) {
  if (N < 1 || S < 1 || Lq < 1 || M < 1) return MAL_ESHAPE;
  if (L < 1 || L > MAL_MSDA_MAX_L || P < 1 || P > MAL_MSDA_MAX_P || L * P > MAL_MSDA_MAX_LP) return MAL_ESHAPE;
  if (D < 1 || D > MAL_MSDA_MAX_D) return MAL_ESHAPE;
  // every tensor below 2^31 elements: value, output, locations
  const double lim = 2147483647.0;
  const double md = (double)M * D;
  if ((double)N * S * md > lim || (double)N * Lq * md > lim || (double)N * Lq * M * L * P * 2.0 > lim) return MAL_ESHAPE;
  const long long total_rows = (long long)N * Lq * M;
  pl->vec = D % 4 == 0 && aligned ? 4 : 1;
  const int lpr = D / pl->vec;
  const int per_row = L * P * 3 + 1;  // LDS floats of a row: locations, weights, the softmax sum
  int rows = kMsdaThreads / lpr;
  if (rows > kMsdaLdsFloats / per_row) rows = kMsdaLdsFloats / per_row;  // >= 42
  if ((long long)rows > total_rows) rows = (int)total_rows;
  pl->rows = rows;
  pl->blocks = (int)((total_rows + rows - 1) / rows);  // (total_rows < 2^31 by the bound on the output)
  pl->lds = (size_t)rows * per_row * sizeof(float);
  return MAL_OK;
}

extern "C" int mal_msda_plan(int N, int S, int Lq, int M, int D, int L, int P, int aligned, int* vec, int* rows, int* blocks,
                             size_t* lds_bytes) {
  MsdaPlan pl;
  const int rc = msda_plan(N, S, Lq, M, D, L, P, aligned != 0, &pl);
  if (rc != MAL_OK) return rc;
  if (vec) *vec = pl.vec;
  if (rows) *rows = pl.rows;
  if (blocks) *blocks = pl.blocks;
  if (lds_bytes) *lds_bytes = pl.lds;
  return MAL_OK;
}

static int msda_launch(const mal_msda_args* a, bool fused) {
  if (!a) return MAL_EINVAL;
  if (!a->value || !a->spatial_shapes || !a->level_start_index || !a->sampling_locations || !a->attention_weights || !a->out)
    return MAL_EINVAL;
  if (fused && !a->reference_points) return MAL_EINVAL;
  if (fused && a->ref_dim != 2 && a->ref_dim != 4) return MAL_ESHAPE;
  MsdaPlan pl;
  const int rc = msda_plan(a->N, a->S, a->Lq, a->M, a->D, a->L, a->P, (((uintptr_t)a->value | (uintptr_t)a->out) & 15) == 0, &pl);
  if (rc != MAL_OK) return rc;
  MsdaParams p;
  p.value = a->value; p.shapes = (const long long*)a->spatial_shapes; p.start = (const long long*)a->level_start_index;
  p.loc = a->sampling_locations; p.wgt = a->attention_weights; p.ref = a->reference_points; p.out = a->out;
  p.N = a->N; p.S = a->S; p.M = a->M; p.D = a->D; p.L = a->L; p.P = a->P; p.Lq = a->Lq; p.ref_dim = a->ref_dim;
  p.total_rows = (long long)a->N * a->Lq * a->M;
  p.rows = pl.rows;
  const bool vec4 = pl.vec == 4;
  const unsigned grid = (unsigned)pl.blocks;
  const size_t lds = pl.lds;
  hipStream_t st = (hipStream_t)a->stream;
  if (vec4) {
    if (fused) hipLaunchKernelGGL((msda_fwd_kernel<4, true>), dim3(grid), dim3(kMsdaThreads), lds, st, p);
    else hipLaunchKernelGGL((msda_fwd_kernel<4, false>), dim3(grid), dim3(kMsdaThreads), lds, st, p);
  } else {
    if (fused) hipLaunchKernelGGL((msda_fwd_kernel<1, true>), dim3(grid), dim3(kMsdaThreads), lds, st, p);
    else hipLaunchKernelGGL((msda_fwd_kernel<1, false>), dim3(grid), dim3(kMsdaThreads), lds, st, p);
  }
  return launch_status();
}

extern "C" int mal_msda_fwd(const mal_msda_args* a) { return msda_launch(a, false); }

extern "C" int mal_msda_fused_fwd(const mal_msda_args* a) { return msda_launch(a, true); }
