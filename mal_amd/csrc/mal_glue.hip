// The glue between two decoder convolutions (mal_amd/networks.py DepthDecoder) as one pass each way:
//
//   conv -> ELU -> interpolate(x2, nearest) -> cat([x, skip], 1) -> ReflectionPad2d(1) -> conv
//
// fp32, NCHW contiguous.  up in {1,2}, elu in {0,1}, skip optional.  H = up*h, W = up*w, Hp = H+2, Wp = W+2,
//   src(p) = 1 if p == 0; H-2 if p == H+1; else p-1        (columns: the same with W)
//
// Forward (join_fwd_kernel), out (B, C+Cs, Hp, Wp):
//   c <  C: out[b,c,p,q] = act(x[b,c, src(p)/up, src(q)/up])      act(v) = v > 0 ? v : expm1f(v)  (elu), else v
//   c >= C: out[b,c,p,q] = skip[b,c-C, src(p), src(q)]
// `out` is one contiguous array, so it is written as such: a thread owns 4 consecutive floats of the FLAT output (one
// 16-byte store whatever (W+2) % 4 is, when the base pointer is 16-byte aligned; 4 scalar stores otherwise) and walks
// (q, p, c, b) as an odometer across the row / plane / sample ends inside its 4 floats.  The grid is capped and strided
// over; the odometer of the stride is computed on the host, so the only divisions are the three that place a thread's
// first unit.  The loads are gathers of 4-byte words that a wave reads from one or two contiguous row pieces.
//
// Backward (join_bwd_kernel): a gather -- no atomics, no zero fill.  g is shaped like out.  An interior row r receives
// from the padded rows R(r) = {r+1} u {0 if r == 1} u {H+1 if r == H-2}, columns alike.  THE SUMMATION ORDER, fixed:
//   rowsum(p, c) = (g[p, c+1] + g[p, 0] if c == 1) + g[p, W+1] if c == W-2          left to right, absent terms skipped
//   S(r, c)      = (rowsum(r+1, c) + rowsum(0, c) if r == 1) + rowsum(H+1, c) if r == H-2
//   gskip[b,k,r,c] = S(r, c) of plane C+k
//   gx[b,c,i,j]    = a' * S(i, j)                                                       (up = 1)
//                  = a' * (((S(2i,2j) + S(2i,2j+1)) + S(2i+1,2j)) + S(2i+1,2j+1))     (up = 2)
//   a' = x > 0 ? 1 : expm1f(x) + 1   (elu; ATen's y + 1 on the forward's own y), the product is left out without elu
// An element sums at most 16 terms (up = 2, h = w = 1), 12 with up = 2 and one of h, w equal to 1, at most 9 otherwise.
// -ffp-contract=off (mal_amd/build.py): no product above is fused into an addition.  The outputs are two contiguous arrays,
// each written in flat units of 4 floats as in the forward; x is read with the same 16-byte unit as gx is written.  A null
// gx or gskip is not computed.
//
// Every flat index and every element offset is a 32-bit unsigned: the entry points refuse tensors of 2^31 elements or more.
#include "mal_common.h"
#include <math.h>

namespace mal {

constexpr int kJoinBlocks = 2048;  // 256 CUs x 8 workgroups of 256 threads; more work is strided over
constexpr int kJoinBlockFloats = 4 * 256;  // of the flat output, per workgroup and sweep

// (d0 fastest) digits of a flat index over an array of shape (.., r2, r1, r0); d3 is the unbounded leading digit
struct Odo { unsigned d0, d1, d2, d3; };
struct OdoSpace {
  unsigned r0, r1, r2;  // radices
  unsigned n;           // elements
  Odo stride;           // digits of the grid's stride (4 * threads of the grid)
  int vec;              // 16-byte accesses allowed (base pointers aligned)
};

__device__ __forceinline__ Odo odo_of(unsigned flat, const OdoSpace& s) {
  Odo o;
  unsigned t = flat / s.r0;
  o.d0 = flat - t * s.r0;
  unsigned u = t / s.r1;
  o.d1 = t - u * s.r1;
  o.d3 = u / s.r2;
  o.d2 = u - o.d3 * s.r2;
  return o;
}
// +1; returns which digit was the last to change (0: d0 only)
__device__ __forceinline__ int odo_inc(Odo& o, const OdoSpace& s) {
  if (++o.d0 != s.r0) return 0;
  o.d0 = 0;
  if (++o.d1 != s.r1) return 1;
  o.d1 = 0;
  if (++o.d2 != s.r2) return 2;
  o.d2 = 0;
  ++o.d3;
  return 3;
}
// + the grid stride: each digit of the stride is below its radix, so one conditional subtraction per digit carries
__device__ __forceinline__ void odo_add(Odo& o, const OdoSpace& s) {
  unsigned c;
  o.d0 += s.stride.d0; c = o.d0 >= s.r0; o.d0 -= c ? s.r0 : 0u;
  o.d1 += s.stride.d1 + c; c = o.d1 >= s.r1; o.d1 -= c ? s.r1 : 0u;
  o.d2 += s.stride.d2 + c; c = o.d2 >= s.r2; o.d2 -= c ? s.r2 : 0u;
  o.d3 += s.stride.d3 + c;
}

struct JoinShape { unsigned C, Cs, h, w; };

__device__ __forceinline__ unsigned refl_src(unsigned p, unsigned n) {  // n = unpadded extent
  return p == 0 ? 1u : (p == n + 1 ? n - 2 : p - 1);
}

template <bool ELU>
__device__ __forceinline__ float join_act(float v) {
  return ELU ? (v > 0.0f ? v : expm1f(v)) : v;
}

// ---------------------------------------------------------------------------------------------------------- forward
template <int UP, bool ELU>
__global__ __launch_bounds__(256) void join_fwd_kernel(const float* __restrict__ x, const float* __restrict__ skip,
                                                       float* __restrict__ out, JoinShape g, OdoSpace sp) {
  const unsigned H = UP * g.h, W = UP * g.w;
  const unsigned step = 4u * gridDim.x * 256u;
  unsigned flat = 4u * (blockIdx.x * 256u + threadIdx.x);
  if (flat >= sp.n) return;
  Odo o = odo_of(flat, sp);  // (q, p, c, b)
  for (; flat < sp.n; flat += step, odo_add(o, sp)) {
    Odo e = o;
    float v[4];
    const float* row = nullptr;
    bool from_x = true, fresh = true;
    const unsigned left = sp.n - flat;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if ((unsigned)k < left) {
        if (fresh) {  // a new source row: only here are the row offsets multiplied out
          const unsigned sr = refl_src(e.d1, H);
          from_x = e.d2 < g.C;
          row = from_x ? x + ((e.d3 * g.C + e.d2) * g.h + sr / UP) * g.w
                       : skip + ((e.d3 * g.Cs + (e.d2 - g.C)) * H + sr) * W;
        }
        const unsigned sc = refl_src(e.d0, W);
        v[k] = from_x ? join_act<ELU>(row[sc / UP]) : row[sc];
        fresh = odo_inc(e, sp) != 0;
      } else {
        v[k] = 0.0f;
      }
    }
    if (sp.vec && left >= 4) {
      *reinterpret_cast<float4*>(out + flat) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((unsigned)k < left) out[flat + k] = v[k];
    }
  }
}

// --------------------------------------------------------------------------------------------------------- backward
__device__ __forceinline__ float join_rowsum(const float* __restrict__ row, unsigned c, unsigned W) {
  float s = row[c + 1];
  if (c == 1) s += row[0];
  if (c == W - 2) s += row[W + 1];
  return s;
}
// S(r, c) of one padded plane
__device__ __forceinline__ float join_gather(const float* __restrict__ plane, unsigned r, unsigned c, unsigned H, unsigned W) {
  const unsigned Wp = W + 2;
  float s = join_rowsum(plane + (r + 1) * Wp, c, W);
  if (r == 1) s += join_rowsum(plane, c, W);
  if (r == H - 2) s += join_rowsum(plane + (H + 1) * Wp, c, W);
  return s;
}

template <int UP, bool ELU>
__global__ __launch_bounds__(256) void join_bwd_kernel(const float* __restrict__ gin, const float* __restrict__ x,
                                                       float* __restrict__ gx, float* __restrict__ gskip, JoinShape g,
                                                       OdoSpace spx, OdoSpace sps) {
  const unsigned H = UP * g.h, W = UP * g.w, Ct = g.C + g.Cs;
  const unsigned plane_elems = (H + 2) * (W + 2);
  const unsigned step = 4u * gridDim.x * 256u;
  const unsigned first = 4u * (blockIdx.x * 256u + threadIdx.x);
  if (gx && first < spx.n) {  // (j, i, c, b) over gx
    unsigned flat = first;
    Odo o = odo_of(flat, spx);
    for (; flat < spx.n; flat += step, odo_add(o, spx)) {
      Odo e = o;
      const unsigned left = spx.n - flat;
      const bool wide = spx.vec && left >= 4;
      float xv[4] = {1.0f, 1.0f, 1.0f, 1.0f};
      if (ELU) {
        if (wide) {
          const float4 t = *reinterpret_cast<const float4*>(x + flat);
          xv[0] = t.x; xv[1] = t.y; xv[2] = t.z; xv[3] = t.w;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if ((unsigned)k < left) xv[k] = x[flat + k];
        }
      }
      float v[4];
      const float* plane = nullptr;
      bool fresh = true;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if ((unsigned)k < left) {
          if (fresh) plane = gin + (e.d3 * Ct + e.d2) * plane_elems;
          const unsigned r = UP * e.d1, c = UP * e.d0;
          float s = join_gather(plane, r, c, H, W);
          if (UP == 2) {
            s += join_gather(plane, r, c + 1, H, W);
            s += join_gather(plane, r + 1, c, H, W);
            s += join_gather(plane, r + 1, c + 1, H, W);
          }
          if (ELU) {
            const float a = xv[k] > 0.0f ? 1.0f : expm1f(xv[k]) + 1.0f;
            s = a * s;
          }
          v[k] = s;
          fresh = odo_inc(e, spx) >= 2;
        } else {
          v[k] = 0.0f;
        }
      }
      if (wide) {
        *reinterpret_cast<float4*>(gx + flat) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if ((unsigned)k < left) gx[flat + k] = v[k];
      }
    }
  }
  if (gskip && first < sps.n) {  // (c, r, k, b) over gskip
    unsigned flat = first;
    Odo o = odo_of(flat, sps);
    for (; flat < sps.n; flat += step, odo_add(o, sps)) {
      Odo e = o;
      const unsigned left = sps.n - flat;
      float v[4];
      const float* plane = nullptr;
      bool fresh = true;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if ((unsigned)k < left) {
          if (fresh) plane = gin + (e.d3 * Ct + g.C + e.d2) * plane_elems;
          v[k] = join_gather(plane, e.d1, e.d0, H, W);
          fresh = odo_inc(e, sps) >= 2;
        } else {
          v[k] = 0.0f;
        }
      }
      if (sps.vec && left >= 4) {
        *reinterpret_cast<float4*>(gskip + flat) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if ((unsigned)k < left) gskip[flat + k] = v[k];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- host
static unsigned join_blocks(size_t n) {
  const size_t b = (n + kJoinBlockFloats - 1) / kJoinBlockFloats;
  return (unsigned)(b < (size_t)kJoinBlocks ? (b ? b : 1) : (size_t)kJoinBlocks);
}

static OdoSpace odo_space(unsigned r0, unsigned r1, unsigned r2, size_t n, unsigned blocks, bool aligned) {
  OdoSpace s;
  s.r0 = r0; s.r1 = r1; s.r2 = r2; s.n = (unsigned)n; s.vec = aligned ? 1 : 0;
  unsigned st = 4u * blocks * 256u;
  s.stride.d0 = st % r0; st /= r0;
  s.stride.d1 = st % r1; st /= r1;
  s.stride.d2 = st % r2; s.stride.d3 = st / r2;
  return s;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// the checks both entry points share; *n_out = elements of the padded tensor
static int join_check(int B, int C, int Cs, int h, int w, int up, int elu, size_t* n_out) {
  if ((up != 1 && up != 2) || (elu != 0 && elu != 1) || B < 1 || C < 1 || h < 1 || w < 1 || Cs < 0) return MAL_EINVAL;
  // extents first in 64 bits: h, w up to INT_MAX must not wrap before they are refused
  const int64_t H = (int64_t)up * h, W = (int64_t)up * w;
  if (H < 2 || W < 2) return MAL_EINVAL;
  const long double n = (long double)B * ((long double)C + Cs) * (long double)(H + 2) * (long double)(W + 2);
  if (n >= 2147483648.0L) return MAL_EINVAL;  // 32-bit flat indices, and room for the last grid stride
  *n_out = (size_t)B * (size_t)(C + Cs) * (size_t)(H + 2) * (size_t)(W + 2);
  return MAL_OK;
}

// the block counts of both launches, the one place they are decided (mal_decoder_join_plan reports them).  The backward's
// two index spaces share one grid, sized by the larger of the outputs that are asked for; 0: nothing to launch
struct JoinPlan {
  size_t nx, ns;  // elements of gx and of gskip
  unsigned blocks_fwd, blocks_bwd;
};
static JoinPlan join_plan(int B, int C, int Cs, int h, int w, int up, size_t n_out, bool need_x, bool need_skip) {
  JoinPlan p;
  p.nx = (size_t)B * C * h * w;
  p.ns = (size_t)B * Cs * (size_t)(up * h) * (size_t)(up * w);
  p.blocks_fwd = join_blocks(n_out);
  const size_t most = (need_x ? p.nx : 0) > (need_skip ? p.ns : 0) ? p.nx : p.ns;
  p.blocks_bwd = (need_x || need_skip) ? join_blocks(most) : 0u;
  return p;
}

}  // namespace mal

using namespace mal;

extern "C" int mal_decoder_join_plan(int B, int C, int Cs, int h, int w, int up, int need_x, int need_skip, int* blocks_fwd,
                                     int* blocks_bwd, int* floats_per_block) {
  size_t n = 0;
  const int rc = join_check(B, C, Cs, h, w, up, 0, &n);
  if (rc) return rc;
  if ((need_x != 0 && need_x != 1) || (need_skip != 0 && need_skip != 1)) return MAL_EINVAL;
  const JoinPlan p = join_plan(B, C, Cs, h, w, up, n, need_x != 0, need_skip != 0 && Cs > 0);
  if (blocks_fwd) *blocks_fwd = (int)p.blocks_fwd;
  if (blocks_bwd) *blocks_bwd = (int)p.blocks_bwd;
  if (floats_per_block) *floats_per_block = kJoinBlockFloats;
  return MAL_OK;
}

extern "C" int mal_decoder_join_fwd(const float* x, const float* skip, float* out, int B, int C, int Cs, int h, int w, int up,
                                    int elu, void* stream) {
  size_t n = 0;
  const int rc = join_check(B, C, Cs, h, w, up, elu, &n);
  if (rc) return rc;
  if (!x || !out || (Cs > 0 && !skip)) return MAL_EINVAL;
  const unsigned blocks = join_plan(B, C, Cs, h, w, up, n, false, false).blocks_fwd;
  const JoinShape g = {(unsigned)C, (unsigned)Cs, (unsigned)h, (unsigned)w};
  const OdoSpace sp = odo_space((unsigned)(up * w + 2), (unsigned)(up * h + 2), (unsigned)(C + Cs), n, blocks, aligned16(out));
  hipStream_t st = (hipStream_t)stream;
#define MAL_JOIN_FWD(U, E) hipLaunchKernelGGL((join_fwd_kernel<U, E>), dim3(blocks), dim3(256), 0, st, x, skip, out, g, sp)
  if (up == 2) { if (elu) MAL_JOIN_FWD(2, true); else MAL_JOIN_FWD(2, false); }
  else         { if (elu) MAL_JOIN_FWD(1, true); else MAL_JOIN_FWD(1, false); }
#undef MAL_JOIN_FWD
  return launch_status();
}

extern "C" int mal_decoder_join_bwd(const float* g_out, const float* x, float* gx, float* gskip, int B, int C, int Cs, int h,
                                    int w, int up, int elu, void* stream) {
  size_t n = 0;
  const int rc = join_check(B, C, Cs, h, w, up, elu, &n);
  if (rc) return rc;
  if (!g_out || (elu && !x)) return MAL_EINVAL;
  if (Cs == 0) gskip = nullptr;
  if (!gx && !gskip) return MAL_OK;
  const JoinPlan p = join_plan(B, C, Cs, h, w, up, n, gx != nullptr, gskip != nullptr);
  const size_t nx = p.nx, ns = p.ns;
  const unsigned blocks = p.blocks_bwd;
  const JoinShape g = {(unsigned)C, (unsigned)Cs, (unsigned)h, (unsigned)w};
  const OdoSpace spx = odo_space((unsigned)w, (unsigned)h, (unsigned)C, nx, blocks, aligned16(gx) && (!elu || aligned16(x)));
  const OdoSpace sps = odo_space((unsigned)(up * w), (unsigned)(up * h), (unsigned)(Cs > 0 ? Cs : 1), ns, blocks, aligned16(gskip));
  hipStream_t st = (hipStream_t)stream;
#define MAL_JOIN_BWD(U, E) \
  hipLaunchKernelGGL((join_bwd_kernel<U, E>), dim3(blocks), dim3(256), 0, st, g_out, x, gx, gskip, g, spx, sps)
  if (up == 2) { if (elu) MAL_JOIN_BWD(2, true); else MAL_JOIN_BWD(2, false); }
  else         { if (elu) MAL_JOIN_BWD(1, true); else MAL_JOIN_BWD(1, false); }
#undef MAL_JOIN_BWD
  return launch_status();
}
