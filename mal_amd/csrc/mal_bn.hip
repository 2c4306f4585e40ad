// The glue behind a ResNet convolution (mal_amd/networks.py BasicBlock, the encoders' stems) as two launches each way:
//
//   conv -> BatchNorm2d -> (+ residual) -> (ReLU)
//
// fp32, NCHW contiguous.  x (B,C,H,W), N = B*H*W elements per channel.  Per channel c, nn.BatchNorm2d's arithmetic:
//   training:  mean = sum(x)/N,  var = sum((x-mean)^2)/N  (biased),  invstd = 1/sqrt(var + eps)
//   eval:      mean = running_mean,  invstd = 1/sqrt(running_var + eps)
//   xh = (x - mean) * invstd,   pre = (xh * gamma + beta) (+ r),   y = relu ? (pre < 0 ? 0 : pre) : pre,  rounded to fp32 ONCE
//   training side effects: running_mean = (1-m)*running_mean + m*mean,  running_var = (1-m)*running_var + m*var*N/(N-1),
//                          num_batches_tracked += 1 (int64)
// Backward (training):  g' = relu ? (y > 0 ? g : 0) : g          (the mask is read from the saved OUTPUT, as ATen's ReLU does)
//   dbeta = sum(g'),  dgamma = sum(g' * xh),  dx = (gamma*invstd) * ((g' - dbeta/N) - xh * (dgamma/N)),  dr = g'
//
// A channel's N elements are B pieces of H*W floats, (H*W)*C apart.  They are cut into UNITS of V floats (V = 4: one
// 16-byte access, when H*W % 4 == 0 and every pointer is 16-byte aligned; V = 1 otherwise), numbered b-major, and the units
// into S = blocks-per-channel contiguous ranges (bn_split: a function of N alone, a power of two).  A thread walks its range
// with stride 256 and carries (b, q) as an odometer, so the only division is the one that places its first unit.
//
// THE SUMMATION ORDER, fixed (no atomics, no arrival order; two runs give the same bits):
//   thread:  its units in ascending order; the V values of a unit are merged as ONE group (mean and M2 of the group first)
//   wave:    lane l takes lane l+32, then l+16, ... l+1 (__shfl_down); lane 0 holds the wave's value
//   block:   wave 0, 1, 2, 3 in that order -> the partial of (c, s), written to the workspace
//   channel: the NEXT launch's prologue: lane s of wave 0 loads partial s (lanes >= S: empty), the same wave tree
// Statistics are merged with Chan's formula on (n, mean, M2) in fp64 from the first element on -- never E[x^2] - mean^2 --
// and STAY fp64: save_mean and save_invstd are (C) doubles, and the per-element expressions above are evaluated in fp64 on
// the fp32 operands (the memory system, not the vector ALU, bounds all four kernels), so y, dx, dgamma and dbeta carry one
// fp32 rounding each instead of the statistics' (mean 100, std 1: the fp32 mean alone costs 4e-6 of a standard deviation;
// N = 2: dx is a difference that cancels to eps/var of its terms).  Only the running statistics are the module's fp32.
//
// Every element offset is a 32-bit unsigned: the entry points refuse tensors of 2^31 elements or more.
#include "mal_common.h"
#include <math.h>

namespace mal {

constexpr int kBnThreads = 256;
constexpr int kBnMaxSplit = 32;         // <= 64: one wave combines a channel's partials
constexpr int kBnMinBlockElems = 2048;  // a block below this is launch latency and little else

struct BnGeom {
  unsigned C, R;        // channels; units per (b, c) plane
  unsigned U, upb;      // units per channel; units per block
  unsigned S;           // blocks per channel
  unsigned st_q, st_b;  // 256 = st_b * R + st_q
};

struct Chan { double n, mean, m2; };

// a, then b
__device__ __forceinline__ Chan chan_merge(Chan a, const Chan b) {
  const double n = a.n + b.n;
  if (b.n > 0.0) {
    const double f = b.n / n, d = b.mean - a.mean;
    a.mean = a.mean + d * f;
    a.m2 = (a.m2 + b.m2) + (d * d) * (a.n * f);
  }
  a.n = n;
  return a;
}

__device__ __forceinline__ Chan chan_wave(Chan a) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    Chan b;
    b.n = __shfl_down(a.n, off);
    b.mean = __shfl_down(a.mean, off);
    b.m2 = __shfl_down(a.m2, off);
    a = chan_merge(a, b);
  }
  return a;  // lane 0
}

__device__ __forceinline__ double sum_wave(double a) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) a += __shfl_down(a, off);
  return a;  // lane 0
}

// the walk of one thread over its block's units
struct BnWalk {
  unsigned u, end, b, q;
  __device__ __forceinline__ BnWalk(const BnGeom& g, unsigned s) {
    u = s * g.upb + threadIdx.x;
    const unsigned e = (s + 1) * g.upb;
    end = e < g.U ? e : g.U;
    b = u / g.R;
    q = u - b * g.R;
  }
  __device__ __forceinline__ bool more() const { return u < end; }
  template <int V>
  __device__ __forceinline__ unsigned offset(const BnGeom& g, unsigned c) const { return ((b * g.C + c) * g.R + q) * V; }
  __device__ __forceinline__ void next(const BnGeom& g) {
    u += kBnThreads;
    q += g.st_q;
    b += g.st_b;
    if (q >= g.R) { q -= g.R; ++b; }
  }
};

template <int V>
__device__ __forceinline__ void bn_load(const float* __restrict__ p, unsigned off, float (&v)[V]) {
  if (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p + off);
    v[0] = t.x; v[1 % V] = t.y; v[2 % V] = t.z; v[3 % V] = t.w;
  } else {
    v[0] = p[off];
  }
}
template <int V>
__device__ __forceinline__ void bn_store(float* __restrict__ p, unsigned off, const float (&v)[V]) {
  if (V == 4) *reinterpret_cast<float4*>(p + off) = make_float4(v[0], v[1 % V], v[2 % V], v[3 % V]);
  else p[off] = v[0];
}

// ------------------------------------------------------------------------------------------------ forward: statistics
template <int V>
__global__ __launch_bounds__(kBnThreads) void bn_stats_kernel(const float* __restrict__ x, double* __restrict__ part, BnGeom g) {
  const unsigned c = blockIdx.x / g.S, s = blockIdx.x - c * g.S;
  Chan a = {0.0, 0.0, 0.0};
  float nf = 0.0f;
  for (BnWalk w(g, s); w.more(); w.next(g)) {
    float v[V];
    bn_load<V>(x, w.template offset<V>(g, c), v);
    double mg, m2g;
    if (V == 4) {  // the group of 4: sum exact in fp64, then the squares about its mean
      const double x0 = v[0], x1 = v[1 % V], x2 = v[2 % V], x3 = v[3 % V];
      mg = ((x0 + x1) + (x2 + x3)) * 0.25;
      const double d0 = x0 - mg, d1 = x1 - mg, d2 = x2 - mg, d3 = x3 - mg;
      m2g = (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    } else {
      mg = v[0];
      m2g = 0.0;
    }
    const float nn = nf + (float)V;          // counts are exact in fp32 (< 2^24 per thread)
    const double f = (double)((float)V / nn);  // the weight V/n: one fp32 division per unit, 6e-8 off at worst
    const double d = mg - a.mean;
    a.mean = a.mean + d * f;
    a.m2 = (a.m2 + m2g) + (d * d) * ((double)nf * f);
    nf = nn;
  }
  a.n = (double)nf;
  a = chan_wave(a);
  __shared__ double sh[kBnThreads / 64][3];
  const unsigned wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) { sh[wave][0] = a.n; sh[wave][1] = a.mean; sh[wave][2] = a.m2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    Chan t = {sh[0][0], sh[0][1], sh[0][2]};
    for (int k = 1; k < kBnThreads / 64; ++k) t = chan_merge(t, Chan{sh[k][0], sh[k][1], sh[k][2]});
    double* o = part + (size_t)blockIdx.x * 3;
    o[0] = t.n; o[1] = t.mean; o[2] = t.m2;
  }
}

// --------------------------------------------------------------------------------------------------- forward: apply
struct BnFwd {
  const float *x, *r, *gamma, *beta;
  float *running_mean, *running_var;
  long long* nbt;
  float* y;
  double *save_mean, *save_invstd;
  const double* part;
  double eps, momentum;
};

template <int V, bool TRAIN, bool RELU, bool RES>
__global__ __launch_bounds__(kBnThreads) void bn_apply_kernel(BnFwd a, BnGeom g) {
  const unsigned c = blockIdx.x / g.S, s = blockIdx.x - c * g.S;
  double mean, invstd;
  if (TRAIN) {
    __shared__ double sh[2];
    if (threadIdx.x < 64) {
      Chan t = {0.0, 0.0, 0.0};
      if (threadIdx.x < g.S) {
        const double* p = a.part + ((size_t)c * g.S + threadIdx.x) * 3;
        t.n = p[0]; t.mean = p[1]; t.m2 = p[2];
      }
      t = chan_wave(t);
      if (threadIdx.x == 0) {
        const double m = t.mean;
        const double is = 1.0 / sqrt(t.m2 / t.n + a.eps);
        sh[0] = m; sh[1] = is;
        if (s == 0) {  // the channel's designated block: the saved statistics and the module's side effects
          a.save_mean[c] = m;
          a.save_invstd[c] = is;
          const double mo = a.momentum;
          a.running_mean[c] = (float)((1.0 - mo) * (double)a.running_mean[c] + mo * t.mean);
          a.running_var[c] = (float)((1.0 - mo) * (double)a.running_var[c] + mo * (t.m2 / (t.n - 1.0)));
          if (c == 0) *a.nbt = *a.nbt + 1;
        }
      }
    }
    __syncthreads();
    mean = sh[0]; invstd = sh[1];
  } else {
    mean = (double)a.running_mean[c];
    invstd = 1.0 / sqrt((double)a.running_var[c] + a.eps);
  }
  const double ga = (double)a.gamma[c], be = (double)a.beta[c];
  for (BnWalk w(g, s); w.more(); w.next(g)) {
    const unsigned off = w.template offset<V>(g, c);
    float v[V], r[V];
    bn_load<V>(a.x, off, v);
    if (RES) bn_load<V>(a.r, off, r);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      double pre = (((double)v[k] - mean) * invstd) * ga + be;
      if (RES) pre = pre + (double)r[k];
      v[k] = (float)(RELU ? (pre < 0.0 ? 0.0 : pre) : pre);
    }
    bn_store<V>(a.y, off, v);
  }
}

// -------------------------------------------------------------------------------------------------- backward: reduce
template <int V, bool RELU>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_reduce_kernel(const float* __restrict__ gout, const float* __restrict__ x,
                                                                   const float* __restrict__ y,
                                                                   const double* __restrict__ save_mean,
                                                                   const double* __restrict__ save_invstd,
                                                                   double* __restrict__ part, BnGeom g) {
  const unsigned c = blockIdx.x / g.S, s = blockIdx.x - c * g.S;
  const double mean = save_mean[c], invstd = save_invstd[c];
  double sg = 0.0, sgx = 0.0;
  for (BnWalk w(g, s); w.more(); w.next(g)) {
    const unsigned off = w.template offset<V>(g, c);
    float gv[V], xv[V], yv[V];
    bn_load<V>(gout, off, gv);
    bn_load<V>(x, off, xv);
    if (RELU) bn_load<V>(y, off, yv);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float gp = RELU ? (yv[k] > 0.0f ? gv[k] : 0.0f) : gv[k];
      const double xh = ((double)xv[k] - mean) * invstd;
      sg += (double)gp;
      sgx += (double)gp * xh;
    }
  }
  sg = sum_wave(sg);
  sgx = sum_wave(sgx);
  __shared__ double sh[kBnThreads / 64][2];
  const unsigned wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) { sh[wave][0] = sg; sh[wave][1] = sgx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t0 = sh[0][0], t1 = sh[0][1];
    for (int k = 1; k < kBnThreads / 64; ++k) { t0 += sh[k][0]; t1 += sh[k][1]; }
    double* o = part + (size_t)blockIdx.x * 2;
    o[0] = t0; o[1] = t1;
  }
}

// --------------------------------------------------------------------------------------------------- backward: apply
struct BnBwd {
  const float *gout, *x, *y, *gamma;
  const double *save_mean, *save_invstd;
  float *dx, *dr, *dgamma, *dbeta;
  const double* part;  // null: dr alone is wanted, nothing was reduced
  double n;
};

template <int V, bool RELU>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_apply_kernel(BnBwd a, BnGeom g) {
  const unsigned c = blockIdx.x / g.S, s = blockIdx.x - c * g.S;
  double mg = 0.0, mgx = 0.0;
  if (a.part) {
    __shared__ double sh[2];
    if (threadIdx.x < 64) {
      double t0 = 0.0, t1 = 0.0;
      if (threadIdx.x < g.S) {
        const double* p = a.part + ((size_t)c * g.S + threadIdx.x) * 2;
        t0 = p[0]; t1 = p[1];
      }
      t0 = sum_wave(t0);
      t1 = sum_wave(t1);
      if (threadIdx.x == 0) {
        sh[0] = t0 / a.n; sh[1] = t1 / a.n;
        if (s == 0) {
          if (a.dbeta) a.dbeta[c] = (float)t0;
          if (a.dgamma) a.dgamma[c] = (float)t1;
        }
      }
    }
    __syncthreads();
    mg = sh[0]; mgx = sh[1];
  }
  if (!a.dx && !a.dr) return;
  const double mean = a.save_mean[c], invstd = a.save_invstd[c];
  const double scale = (double)a.gamma[c] * invstd;
  for (BnWalk w(g, s); w.more(); w.next(g)) {
    const unsigned off = w.template offset<V>(g, c);
    float gv[V], xv[V], yv[V];
    bn_load<V>(a.gout, off, gv);
    if (RELU) bn_load<V>(a.y, off, yv);
#pragma unroll
    for (int k = 0; k < V; ++k) gv[k] = RELU ? (yv[k] > 0.0f ? gv[k] : 0.0f) : gv[k];
    if (a.dr) bn_store<V>(a.dr, off, gv);
    if (a.dx) {
      bn_load<V>(a.x, off, xv);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const double xh = ((double)xv[k] - mean) * invstd;
        xv[k] = (float)(scale * (((double)gv[k] - mg) - xh * mgx));
      }
      bn_store<V>(a.dx, off, xv);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- host
// blocks per channel: the largest power of two that leaves every block kBnMinBlockElems elements, at most kBnMaxSplit.
// A function of N alone: the boundaries are N = kBnMinBlockElems * {2, 4, 8, 16, 32}.
static int bn_split(int64_t n) {
  int s = 1;
  while (s < kBnMaxSplit && (int64_t)kBnMinBlockElems * (2 * s) <= n) s *= 2;
  return s;
}

static int bn_check(int B, int C, int H, int W, int64_t* n_out) {
  if (B < 1 || C < 1 || H < 1 || W < 1) return MAL_EINVAL;
  const long double tot = (long double)B * C * (long double)H * W;
  if (tot >= 2147483648.0L) return MAL_EINVAL;  // 32-bit offsets
  *n_out = (int64_t)B * H * W;
  return MAL_OK;
}

static size_t bn_ws_bytes(int C, int S) { return align256((size_t)C * S * 3 * sizeof(double)); }

static BnGeom bn_geom(int B, int C, int H, int W, int S, int V) {
  BnGeom g;
  g.C = (unsigned)C;
  g.R = (unsigned)(H * W / V);
  g.U = (unsigned)B * g.R;
  g.S = (unsigned)S;
  g.upb = (g.U + g.S - 1) / g.S;
  g.st_q = (unsigned)kBnThreads % g.R;
  g.st_b = (unsigned)kBnThreads / g.R;
  return g;
}

static bool bn_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace mal

using namespace mal;

extern "C" int mal_bn_join_plan(int B, int C, int H, int W, int* blocks_per_channel, size_t* ws_bytes) {
  int64_t n = 0;
  const int rc = bn_check(B, C, H, W, &n);
  if (rc) return rc;
  const int S = bn_split(n);
  if (blocks_per_channel) *blocks_per_channel = S;
  if (ws_bytes) *ws_bytes = bn_ws_bytes(C, S);
  return MAL_OK;
}

extern "C" int mal_bn_join_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, int64_t* num_batches_tracked, float* y, double* save_mean, double* save_invstd,
                               int B, int C, int H, int W, double eps, double momentum, int training, int relu, void* ws,
                               size_t ws_bytes, void* stream) {
  int64_t n = 0;
  const int rc = bn_check(B, C, H, W, &n);
  if (rc) return rc;
  if ((training != 0 && training != 1) || (relu != 0 && relu != 1)) return MAL_EINVAL;
  if (!(eps >= 0.0) || !(eps < (double)INFINITY) || !(momentum >= 0.0 && momentum <= 1.0)) return MAL_EINVAL;
  if (!x || !gamma || !beta || !running_mean || !running_var || !y) return MAL_EINVAL;
  const int S = bn_split(n);
  if (training) {
    if (n < 2 || !num_batches_tracked || !save_mean || !save_invstd || !ws) return MAL_EINVAL;
    if (ws_bytes < bn_ws_bytes(C, S)) return MAL_EWORKSPACE;
  }
  const bool vec = (H * W) % 4 == 0 && bn_aligned16(x) && bn_aligned16(y) && (!residual || bn_aligned16(residual));
  const BnGeom g = bn_geom(B, C, H, W, S, vec ? 4 : 1);
  const unsigned blocks = (unsigned)C * (unsigned)S;
  hipStream_t st = (hipStream_t)stream;
  BnFwd a = {x, residual, gamma, beta, running_mean, running_var, (long long*)num_batches_tracked, y, save_mean, save_invstd,
             (const double*)ws, eps, momentum};
  if (training) {
    if (vec) hipLaunchKernelGGL((bn_stats_kernel<4>), dim3(blocks), dim3(kBnThreads), 0, st, x, (double*)ws, g);
    else hipLaunchKernelGGL((bn_stats_kernel<1>), dim3(blocks), dim3(kBnThreads), 0, st, x, (double*)ws, g);
  }
#define MAL_BN_APPLY(V, T, RL, RS) hipLaunchKernelGGL((bn_apply_kernel<V, T, RL, RS>), dim3(blocks), dim3(kBnThreads), 0, st, a, g)
#define MAL_BN_APPLY_RS(V, T, RL) do { if (residual) MAL_BN_APPLY(V, T, RL, true); else MAL_BN_APPLY(V, T, RL, false); } while (0)
#define MAL_BN_APPLY_RL(V, T) do { if (relu) MAL_BN_APPLY_RS(V, T, true); else MAL_BN_APPLY_RS(V, T, false); } while (0)
#define MAL_BN_APPLY_T(V) do { if (training) MAL_BN_APPLY_RL(V, true); else MAL_BN_APPLY_RL(V, false); } while (0)
  if (vec) MAL_BN_APPLY_T(4); else MAL_BN_APPLY_T(1);
#undef MAL_BN_APPLY_T
#undef MAL_BN_APPLY_RL
#undef MAL_BN_APPLY_RS
#undef MAL_BN_APPLY
  return launch_status();
}

extern "C" int mal_bn_join_bwd(const float* g_out, const float* x, const float* y, const float* gamma, const double* save_mean,
                               const double* save_invstd, float* dx, float* dr, float* dgamma, float* dbeta, int B, int C, int H,
                               int W, int relu, void* ws, size_t ws_bytes, void* stream) {
  int64_t n = 0;
  const int rc = bn_check(B, C, H, W, &n);
  if (rc) return rc;
  if (relu != 0 && relu != 1) return MAL_EINVAL;
  if (!g_out || !x || !gamma || !save_mean || !save_invstd || (relu && !y)) return MAL_EINVAL;
  if (!dx && !dr && !dgamma && !dbeta) return MAL_OK;
  const bool reduce = dx || dgamma || dbeta;
  const int S = bn_split(n);
  if (reduce) {
    if (n < 2 || !ws) return MAL_EINVAL;
    if (ws_bytes < bn_ws_bytes(C, S)) return MAL_EWORKSPACE;
  }
  const bool vec = (H * W) % 4 == 0 && bn_aligned16(g_out) && bn_aligned16(x) && (!relu || bn_aligned16(y)) &&
                   (!dx || bn_aligned16(dx)) && (!dr || bn_aligned16(dr));
  const BnGeom g = bn_geom(B, C, H, W, S, vec ? 4 : 1);
  const unsigned blocks = (unsigned)C * (unsigned)S;
  hipStream_t st = (hipStream_t)stream;
  BnBwd a = {g_out, x, y, gamma, save_mean, save_invstd, dx, dr, dgamma, dbeta, reduce ? (const double*)ws : nullptr,
             (double)n};
#define MAL_BN_BWD(V, RL)                                                                                                   \
  do {                                                                                                                      \
    if (reduce)                                                                                                             \
      hipLaunchKernelGGL((bn_bwd_reduce_kernel<V, RL>), dim3(blocks), dim3(kBnThreads), 0, st, g_out, x, y, save_mean,      \
                         save_invstd, (double*)ws, g);                                                                      \
    hipLaunchKernelGGL((bn_bwd_apply_kernel<V, RL>), dim3(blocks), dim3(kBnThreads), 0, st, a, g);                          \
  } while (0)
  if (vec) { if (relu) MAL_BN_BWD(4, true); else MAL_BN_BWD(4, false); }
  else     { if (relu) MAL_BN_BWD(1, true); else MAL_BN_BWD(1, false); }
#undef MAL_BN_BWD
  return launch_status();
}
