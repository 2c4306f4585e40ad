// The max-pool behind the stem of a ResNet (mal_amd/networks.py: the three encoders) as one launch each way:
//
//   p = F.max_pool2d(y, kernel_size=3, stride=2, padding=1)        y (B,C,H,W) fp32 contiguous
//
// p (B,C,OH,OW), OH = (H-1)/2 + 1, OW = (W-1)/2 + 1.  Window (oh, ow) covers rows 2oh-1 .. 2oh+1 and columns 2ow-1 .. 2ow+1
// clipped to the plane (padding is -inf: it never wins and never ties).
//
// THE WINNER of a window, ATen's rule (max_pool_forward_nchw; the CPU kernel has the same one):
//   m = -inf, winner = the first element of the clipped window; then row-major over the clipped window
//   a value replaces m when  val > m || isnan(val)
// so the FIRST of equal maxima wins, a NaN wins and a later NaN replaces it, and a window of all -inf keeps its first
// element.  The forward writes, beside p, one byte per output: the winner's position in the UNCLIPPED window, kh*3 + kw
// (0..8), where ATen saves an int64 flat index.  Without a code pointer (no gradient wanted) only p is written.
//
// THE BACKWARD is a gather over codes: element (h, w) of dy lies in at most four windows,
//   rows     oh = h>>1 with kh = (h&1) + 1, and for odd h also oh = (h>>1) + 1 with kh = 0 (if oh < OH)
//   columns  ow = w>>1 with kw = (w&1) + 1, and for odd w also ow = (w>>1) + 1 with kw = 0 (if ow < OW)
// and receives g_p[window] from each whose code is kh*3 + kw.  SUMMATION ORDER, fixed (no atomics, no zero fill, no read of
// y, no workspace; two runs give the same bits, and so do the two routes below):
//   acc = g_y[h, w] (the cotangent that reaches y from its other consumer; +0 without one), then the windows in ascending
//   (oh, ow), one fp32 addition each.
//
// Routes.  Forward: a thread owns 4 consecutive outputs of a row (two 16-byte loads and one float per input row, one
// 16-byte store of p, one 4-byte store of codes) when W % 8 == 0 and the pointers are aligned, one output otherwise.
// Backward: a thread owns 4 consecutive elements of dy (one 16-byte store; per window row one 8-byte and one 4-byte load
// of g_p, a 2-byte and a 1-byte load of codes) when W % 4 == 0 and the pointers are aligned, one element otherwise.
// Units are numbered flat (plane-major, then row, then column), the grid is capped at kPoolMaxBlocks workgroups and
// strided over; mal_stem_pool_plan says what the launches are.
//
// Every element offset is a 32-bit unsigned: the entry points refuse tensors of 2^31 elements or more.
#include "mal_common.h"
#include <math.h>

namespace mal {

constexpr int kPoolThreads = 256;
constexpr int kPoolMaxBlocks = 2048;  // 8 workgroups per compute unit; a larger tensor is strided over

struct PoolGeom {
  unsigned H, W, OH, OW;
  unsigned units;  // of this launch: outputs (forward) or elements of dy (backward), divided by the route's width
};

__device__ __forceinline__ void pool_take(bool valid, float v, unsigned k, float& m, unsigned& code) {
  if (valid && (v > m || v != v)) { m = v; code = k; }
}

// ---------------------------------------------------------------------------------------------------------- forward
// One output per thread.  An invalid (clipped) position is read at a clamped, valid address and never taken.
__global__ __launch_bounds__(kPoolThreads) void pool_fwd1_kernel(const float* __restrict__ y, float* __restrict__ p,
                                                                 uint8_t* __restrict__ code, PoolGeom g) {
  const unsigned stride = gridDim.x * kPoolThreads;
  for (unsigned u = blockIdx.x * kPoolThreads + threadIdx.x; u < g.units; u += stride) {
    const unsigned row = u / g.OW, ow = u - row * g.OW;
    const unsigned plane = row / g.OH, oh = row - plane * g.OH;
    const float* src = y + plane * (g.H * g.W);
    const bool top = oh > 0, bottom = 2 * oh + 1 < g.H, left = ow > 0, right = 2 * ow + 1 < g.W;
    float m = -INFINITY;
    unsigned c = (top ? 0u : 3u) + (left ? 0u : 1u);
#pragma unroll
    for (unsigned kh = 0; kh < 3; ++kh) {
      const bool vh = kh == 0 ? top : (kh == 2 ? bottom : true);
      const unsigned hh = vh ? 2 * oh + kh - 1 : 2 * oh;
#pragma unroll
      for (unsigned kw = 0; kw < 3; ++kw) {
        const bool vw = kw == 0 ? left : (kw == 2 ? right : true);
        const unsigned ww = vw ? 2 * ow + kw - 1 : 2 * ow;
        pool_take(vh && vw, src[hh * g.W + ww], kh * 3 + kw, m, c);
      }
    }
    p[u] = m;
    if (code) code[u] = (uint8_t)c;
  }
}

// Four consecutive outputs per thread; W % 8 == 0 (so OW % 4 == 0, and no window is clipped on the right), y and p 16-byte
// aligned, code 4-byte aligned.  Outputs 4q .. 4q+3 of a row read columns 8q-1 .. 8q+7.
__global__ __launch_bounds__(kPoolThreads) void pool_fwd4_kernel(const float* __restrict__ y, float* __restrict__ p,
                                                                 uint8_t* __restrict__ code, PoolGeom g) {
  const unsigned stride = gridDim.x * kPoolThreads;
  const unsigned OWQ = g.OW >> 2;
  for (unsigned u = blockIdx.x * kPoolThreads + threadIdx.x; u < g.units; u += stride) {
    const unsigned row = u / OWQ, q = u - row * OWQ;
    const unsigned plane = row / g.OH, oh = row - plane * g.OH;
    const float* src = y + plane * (g.H * g.W) + 8 * q;
    const bool top = oh > 0, bottom = 2 * oh + 1 < g.H, left = q > 0;
    float r[3][9];
#pragma unroll
    for (unsigned kh = 0; kh < 3; ++kh) {
      const bool vh = kh == 0 ? top : (kh == 2 ? bottom : true);
      const float* line = src + (vh ? 2 * oh + kh - 1 : 2 * oh) * g.W;
      const float4 a = *reinterpret_cast<const float4*>(line);
      const float4 b = *reinterpret_cast<const float4*>(line + 4);
      r[kh][0] = left ? line[-1] : a.x;
      r[kh][1] = a.x; r[kh][2] = a.y; r[kh][3] = a.z; r[kh][4] = a.w;
      r[kh][5] = b.x; r[kh][6] = b.y; r[kh][7] = b.z; r[kh][8] = b.w;
    }
    float m[4];
    unsigned c[4];
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) {
      const bool vl = j > 0 || left;
      m[j] = -INFINITY;
      c[j] = (top ? 0u : 3u) + (vl ? 0u : 1u);
#pragma unroll
      for (unsigned kh = 0; kh < 3; ++kh) {
        const bool vh = kh == 0 ? top : (kh == 2 ? bottom : true);
#pragma unroll
        for (unsigned kw = 0; kw < 3; ++kw) pool_take(vh && (kw > 0 || vl), r[kh][2 * j + kw], kh * 3 + kw, m[j], c[j]);
      }
    }
    *reinterpret_cast<float4*>(p + 4 * u) = make_float4(m[0], m[1], m[2], m[3]);
    if (code) *reinterpret_cast<uint32_t*>(code + 4 * u) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
  }
}

// --------------------------------------------------------------------------------------------------------- backward
struct PoolBwd {
  const float* g_p;
  const float* g_y;  // nullable
  const uint8_t* code;
  float* dy;
};

template <int V>
__global__ __launch_bounds__(kPoolThreads) void pool_bwd_kernel(PoolBwd a, PoolGeom g) {
  const unsigned stride = gridDim.x * kPoolThreads;
  const unsigned WQ = g.W / V;
  for (unsigned u = blockIdx.x * kPoolThreads + threadIdx.x; u < g.units; u += stride) {
    const unsigned row = u / WQ, q = u - row * WQ;
    const unsigned plane = row / g.H, h = row - plane * g.H;
    float acc[V];
    if (V == 4) {
      float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (a.g_y) t = *reinterpret_cast<const float4*>(a.g_y + 4 * u);
      acc[0] = t.x; acc[1 % V] = t.y; acc[2 % V] = t.z; acc[3 % V] = t.w;
    } else {
      acc[0] = a.g_y ? a.g_y[u] : 0.0f;
    }
    const unsigned oh0 = h >> 1;
    const unsigned nrows = ((h & 1u) && oh0 + 1 < g.OH) ? 2u : 1u;
    for (unsigned r = 0; r < nrows; ++r) {  // ascending oh
      const unsigned k0 = r == 0 ? ((h & 1u) + 1u) * 3u : 0u;  // kh * 3 of this element in that window row
      const unsigned base = (plane * g.OH + oh0 + r) * g.OW;
      if (V == 4) {  // columns 4q .. 4q+3 lie in the windows ow = 2q, 2q+1 and (the last one, kw = 0) 2q+2
        const unsigned o = base + 2 * q;
        const float2 gp = *reinterpret_cast<const float2*>(a.g_p + o);
        const unsigned cd = *reinterpret_cast<const uint16_t*>(a.code + o);
        const unsigned c0 = cd & 255u, c1 = cd >> 8;
        const bool third = 2 * q + 2 < g.OW;
        const float gp2 = third ? a.g_p[o + 2] : 0.0f;
        const unsigned c2 = third ? a.code[o + 2] : 9u;
        if (c0 == k0 + 1) acc[0] += gp.x;
        if (c0 == k0 + 2) acc[1 % V] += gp.x;
        if (c1 == k0) acc[1 % V] += gp.y;
        if (c1 == k0 + 1) acc[2 % V] += gp.y;
        if (c1 == k0 + 2) acc[3 % V] += gp.y;
        if (c2 == k0) acc[3 % V] += gp2;
      } else {
        const unsigned ow0 = q >> 1;
        if (a.code[base + ow0] == k0 + (q & 1u) + 1u) acc[0] += a.g_p[base + ow0];
        if ((q & 1u) && ow0 + 1 < g.OW && a.code[base + ow0 + 1] == k0) acc[0] += a.g_p[base + ow0 + 1];
      }
    }
    if (V == 4) *reinterpret_cast<float4*>(a.dy + 4 * u) = make_float4(acc[0], acc[1 % V], acc[2 % V], acc[3 % V]);
    else a.dy[u] = acc[0];
  }
}

// ------------------------------------------------------------------------------------------------------------- host
struct PoolPlan {
  int OH, OW;
  int v_fwd, v_bwd;            // outputs / elements of dy per thread
  unsigned units_fwd, units_bwd;
  int blocks_fwd, blocks_bwd;
};

static int pool_blocks(unsigned units) {
  const unsigned b = (units + kPoolThreads - 1) / kPoolThreads;
  return (int)(b < (unsigned)kPoolMaxBlocks ? b : (unsigned)kPoolMaxBlocks);
}

static int pool_plan(int B, int C, int H, int W, bool aligned_fwd, bool aligned_bwd, PoolPlan* pl) {
  if (B < 1 || C < 1 || H < 1 || W < 1) return MAL_EINVAL;
  const long double tot = (long double)B * C * (long double)H * W;
  if (tot >= 2147483648.0L) return MAL_EINVAL;  // 32-bit offsets
  pl->OH = (H - 1) / 2 + 1;
  pl->OW = (W - 1) / 2 + 1;
  pl->v_fwd = (aligned_fwd && W % 8 == 0) ? 4 : 1;
  pl->v_bwd = (aligned_bwd && W % 4 == 0) ? 4 : 1;
  const unsigned planes = (unsigned)B * (unsigned)C;
  pl->units_fwd = planes * (unsigned)pl->OH * (unsigned)(pl->OW / pl->v_fwd);
  pl->units_bwd = planes * (unsigned)H * (unsigned)(W / pl->v_bwd);
  pl->blocks_fwd = pool_blocks(pl->units_fwd);
  pl->blocks_bwd = pool_blocks(pl->units_bwd);
  return MAL_OK;
}

static bool pool_aligned(const void* p, unsigned n) { return ((uintptr_t)p & (uintptr_t)(n - 1)) == 0; }

static PoolGeom pool_geom(int H, int W, const PoolPlan& pl, unsigned units) {
  PoolGeom g;
  g.H = (unsigned)H; g.W = (unsigned)W; g.OH = (unsigned)pl.OH; g.OW = (unsigned)pl.OW;
  g.units = units;
  return g;
}

}  // namespace mal

using namespace mal;

extern "C" int mal_stem_pool_plan(int B, int C, int H, int W, int aligned, int* OH, int* OW, int* blocks_fwd, int* blocks_bwd,
                                  int* per_thread_fwd, int* per_thread_bwd) {
  PoolPlan pl;
  const int rc = pool_plan(B, C, H, W, aligned != 0, aligned != 0, &pl);
  if (rc) return rc;
  if (OH) *OH = pl.OH;
  if (OW) *OW = pl.OW;
  if (blocks_fwd) *blocks_fwd = pl.blocks_fwd;
  if (blocks_bwd) *blocks_bwd = pl.blocks_bwd;
  if (per_thread_fwd) *per_thread_fwd = pl.v_fwd;
  if (per_thread_bwd) *per_thread_bwd = pl.v_bwd;
  return MAL_OK;
}

extern "C" int mal_stem_pool_fwd(const float* y, float* p, uint8_t* code, int B, int C, int H, int W, void* stream) {
  PoolPlan pl;
  const bool aligned = pool_aligned(y, 16) && pool_aligned(p, 16) && pool_aligned(code, 4);
  const int rc = pool_plan(B, C, H, W, aligned, false, &pl);
  if (rc) return rc;
  if (!y || !p) return MAL_EINVAL;
  const PoolGeom g = pool_geom(H, W, pl, pl.units_fwd);
  hipStream_t st = (hipStream_t)stream;
  if (pl.v_fwd == 4) hipLaunchKernelGGL(pool_fwd4_kernel, dim3(pl.blocks_fwd), dim3(kPoolThreads), 0, st, y, p, code, g);
  else hipLaunchKernelGGL(pool_fwd1_kernel, dim3(pl.blocks_fwd), dim3(kPoolThreads), 0, st, y, p, code, g);
  return launch_status();
}

extern "C" int mal_stem_pool_bwd(const float* g_p, const float* g_y, const uint8_t* code, float* dy, int B, int C, int H, int W,
                                 void* stream) {
  PoolPlan pl;
  const bool aligned = pool_aligned(g_p, 16) && pool_aligned(g_y, 16) && pool_aligned(dy, 16) && pool_aligned(code, 4);
  const int rc = pool_plan(B, C, H, W, false, aligned, &pl);
  if (rc) return rc;
  if (!g_p || !code || !dy) return MAL_EINVAL;
  const PoolGeom g = pool_geom(H, W, pl, pl.units_bwd);
  const PoolBwd a = {g_p, g_y, code, dy};
  hipStream_t st = (hipStream_t)stream;
  if (pl.v_bwd == 4) hipLaunchKernelGGL((pool_bwd_kernel<4>), dim3(pl.blocks_bwd), dim3(kPoolThreads), 0, st, a, g);
  else hipLaunchKernelGGL((pool_bwd_kernel<1>), dim3(pl.blocks_bwd), dim3(kPoolThreads), 0, st, a, g);
  return launch_status();
}
