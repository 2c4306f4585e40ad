// torch.optim.Adam's update (plain Adam: no weight decay, no amsgrad, no maximize) over the harness's flat gradient buffer as
// ONE launch per step (mal_amd/optim.py: FlatAdam; upstream trains with torch.optim.Adam(params, lr), manydepth/trainer.py).
//
// The parameters stay where torch put them: a device-resident CHUNK TABLE, built once, says for every parameter tensor where
// it lives, where its gradient lies in the flat buffer (mal_amd.dp.FlatGradBucket.flat) and how many elements it has.
// exp_avg and exp_avg_sq are two flat buffers of the optimizer's own with the bucket's offsets.  A launch updates the table
// entries [first, first + count): a later change can update one exchange piece while the next is still on the wire.
//
// ARITHMETIC, fp32, one correctly rounded operation per operator, no fused multiply-add (the library is built with
// -ffp-contract=off; hipcc's default division and square root are correctly rounded and keep denormals), in ATen's order
// (lerp_ with a weight below 0.5, mul_ + addcmul_, sqrt / bias_correction2_sqrt + eps, addcdiv_):
//   m' = m + (g - m) * c1            c1 = fp32(1 - beta1)
//   v' = v * beta2 + (c2 * g) * g    c2 = fp32(1 - beta2)
//   den = sqrt(v') / bs + eps        bs = fp32(sqrt(1 - beta2^t))
//   p' = p + a * (m' / den)          a  = fp32(-lr / (1 - beta1^t))
// The six scalars are formed on the host in double, rounded once and passed as kernel arguments.  With zero_grad the
// gradient element is overwritten with +0 after it was read (the bucket's memset of the next step, for 4 bytes more per
// parameter here instead of 8 there).  No atomics, no reduction: two runs give the same bits, and so does any split of the
// table into consecutive ranges.
//
// DECOMPOSITION.  A chunk of n elements at flat offset `off` is cut into
//   head   the elements in front of the first 16-byte boundary of the gradient's address (0..3, at most n),
//   body   nv = (n - head) / 4 vectors of four floats,
//   tail   the 0..3 elements behind the body,
// and the body into TILES of kAdamTile elements (256 threads x kAdamUnroll vectors); a chunk has max(1, ceil(nv / 512))
// tiles and tile 0 also owns head and tail, one element per thread.  The tiles of the range are numbered in table order and
// tile T belongs to workgroup T % gridDim.x: every workgroup walks the range's entries (staged through LDS 256 at a time)
// and keeps the running tile count, all in scalar registers.  The grid is min(kAdamMaxBlocks, ceil(elements / kAdamTile) +
// count) -- a bound on the number of tiles that needs the range's element total only, which the caller knows;
// mal_adam_plan returns it.  The total sizes the grid and nothing else: what is read and written follows from the table alone.
//
// ACCESS WIDTH.  The flat offsets are whatever the bucket assigned (RepDepth has one-element biases: most offsets are odd),
// so a parameter's own address and its gradient's are in general NOT congruent modulo 16 bytes.  The head is peeled so that
// the three flat streams (g, m, v: three of the four reads, two or three of the three or four writes) are on the 16-byte
// grid; the parameter stream is then accessed through a four-float type of 4-byte alignment, for which the compiler emits
// the same global_load_dwordx4 / global_store_dwordx4 (global memory instructions of gfx9 need dword alignment only).  All
// four streams go through that type, so flat buffers that are themselves off the 16-byte grid are correct too.  Every
// access lies inside its chunk; an entry that does not fit the flat buffers (offset + count > flat_elements) or has a null
// parameter pointer is skipped, not clamped.
//
// STORE FLAVOUR.  p, m and v are not read again before the next step (tens of milliseconds of other traffic later) and g by
// nobody, so no line written here is worth a place in a cache -- but every store flavour's bytes leave the L2 in the same
// pass (MI355X: plain / nt keep the line, sc1 drops it, the fabric traffic is equal) and nt / sc1 loads are at best equal to
// plain ones at 16 bytes per lane.  Plain loads and stores; DESIGN.md has the measured rate.
//
// Every element offset is a 32-bit unsigned: the entry points refuse totals of 2^31 elements or more.
#include "mal_common.h"
#include <math.h>

namespace mal {

constexpr int kAdamThreads = 256;
constexpr int kAdamUnroll = 2;                               // 16-byte vectors per thread and stream in one tile
constexpr int kAdamTileVecs = kAdamThreads * kAdamUnroll;    // 512
constexpr int kAdamTile = kAdamTileVecs * 4;                 // 2048 elements
constexpr int kAdamMaxBlocks = 2048;                         // 8 workgroups per compute unit; longer ranges are strided over
constexpr int kAdamWindow = 256;                             // table entries staged in LDS at a time

typedef float f4v __attribute__((ext_vector_type(4)));
typedef f4v f4u __attribute__((aligned(4)));  // four floats at dword alignment: one dwordx4 access
// A table entry's pointer reaches the kernel as data, so the compiler cannot know its address space and would emit flat_
// instructions for it: say that it is global memory.
#define MAL_GLOBAL __attribute__((address_space(1)))

struct AdamScalars { float c1, beta2, c2, bs, eps, a; };

struct AdamArgs {
  const mal_adam_chunk* table;
  unsigned first, count;
  float* g;
  float* m;
  float* v;
  unsigned flat_elements;
  AdamScalars s;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamScalars& s) {
  m = m + (g - m) * s.c1;
  v = v * s.beta2 + (s.c2 * g) * g;
  const float den = sqrtf(v) / s.bs + s.eps;
  p = p + s.a * (m / den);
}

__device__ __forceinline__ void adam_four(f4v& p, const f4v& g, f4v& m, f4v& v, const AdamScalars& s) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float pp = p[k], mm = m[k], vv = v[k];
    adam_one(pp, g[k], mm, vv, s);
    p[k] = pp; m[k] = mm; v[k] = vv;
  }
}

__device__ __forceinline__ unsigned adam_uniform(unsigned x) { return (unsigned)__builtin_amdgcn_readfirstlane((int)x); }

template <bool ZERO>
__global__ __launch_bounds__(kAdamThreads) void adam_flat_kernel(AdamArgs a) {
  __shared__ mal_adam_chunk win[kAdamWindow];
  const unsigned G = gridDim.x, b = blockIdx.x, tid = threadIdx.x;
  unsigned r = 0;  // tiles of the entries walked so far, modulo G (r < G)
  for (unsigned w0 = 0; w0 < a.count; w0 += kAdamWindow) {
    const unsigned wn = a.count - w0 < (unsigned)kAdamWindow ? a.count - w0 : (unsigned)kAdamWindow;
    if (w0) __syncthreads();  // the previous window has been walked by every wave
    if (tid < wn) win[tid] = a.table[a.first + w0 + tid];
    __syncthreads();
    for (unsigned e = 0; e < wn; ++e) {
      // the same entry in every lane: keep it, and all that follows from it, in scalar registers
      const mal_adam_chunk c = win[e];
      const uintptr_t pa = (uintptr_t)c.param;
      const uintptr_t pu = (uintptr_t)adam_uniform((unsigned)pa) | ((uintptr_t)adam_uniform((unsigned)(pa >> 32)) << 32);
      const unsigned off = adam_uniform(c.offset), n = adam_uniform(c.count);
      if (n == 0 || pu == 0 || off > a.flat_elements || n > a.flat_elements - off) continue;  // r is not advanced: no tiles
      MAL_GLOBAL float* p = (MAL_GLOBAL float*)pu;
      MAL_GLOBAL float* g = (MAL_GLOBAL float*)a.g + off;
      MAL_GLOBAL float* m = (MAL_GLOBAL float*)a.m + off;
      MAL_GLOBAL float* v = (MAL_GLOBAL float*)a.v + off;
      unsigned head = (unsigned)((16u - (unsigned)((uintptr_t)g & 15u)) & 15u) >> 2;
      if (head > n) head = n;
      const unsigned nv = (n - head) >> 2;
      const unsigned tail0 = head + 4u * nv;  // first element of the tail
      const unsigned nscalar = n - 4u * nv;   // head + tail, at most 6
      unsigned tiles = (nv + kAdamTileVecs - 1) / kAdamTileVecs;
      if (tiles == 0) tiles = 1;
      for (unsigned t = b >= r ? b - r : b + (G - r); t < tiles; t += G) {
        if (t == 0 && tid < nscalar) {
          const unsigned i = tid < head ? tid : tail0 + (tid - head);
          float pp = p[i], mm = m[i], vv = v[i];
          const float gg = g[i];
          adam_one(pp, gg, mm, vv, a.s);
          p[i] = pp; m[i] = mm; v[i] = vv;
          if (ZERO) g[i] = 0.0f;
        }
        MAL_GLOBAL f4u* P = (MAL_GLOBAL f4u*)(p + head);
        MAL_GLOBAL f4u* Gv = (MAL_GLOBAL f4u*)(g + head);
        MAL_GLOBAL f4u* M = (MAL_GLOBAL f4u*)(m + head);
        MAL_GLOBAL f4u* V = (MAL_GLOBAL f4u*)(v + head);
        const unsigned i0 = t * kAdamTileVecs + tid;
        f4v xp[kAdamUnroll], xg[kAdamUnroll], xm[kAdamUnroll], xv[kAdamUnroll];
#pragma unroll
        for (int j = 0; j < kAdamUnroll; ++j) {
          const unsigned i = i0 + j * kAdamThreads;
          if (i < nv) { xg[j] = Gv[i]; xm[j] = M[i]; xv[j] = V[i]; xp[j] = P[i]; }
        }
#pragma unroll
        for (int j = 0; j < kAdamUnroll; ++j) {
          const unsigned i = i0 + j * kAdamThreads;
          if (i < nv) {
            adam_four(xp[j], xg[j], xm[j], xv[j], a.s);
            P[i] = xp[j]; M[i] = xm[j]; V[i] = xv[j];
            if (ZERO) { const f4v z = {0.0f, 0.0f, 0.0f, 0.0f}; Gv[i] = z; }
          }
        }
      }
      r = (r + tiles) % G;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- host
static int adam_plan(int n_chunks, long long elements, int* blocks) {
  if (n_chunks < 1 || elements < 0 || elements >= 2147483648LL) return MAL_EINVAL;  // 32-bit offsets
  const long long bound = (elements + kAdamTile - 1) / kAdamTile + n_chunks;  // >= the tiles of n_chunks entries with that total
  *blocks = (int)(bound < (long long)kAdamMaxBlocks ? bound : (long long)kAdamMaxBlocks);
  return MAL_OK;
}

}  // namespace mal

using namespace mal;

extern "C" int mal_adam_plan(int n_chunks, long long total_elements, int* blocks, int* threads, int* tile_elements,
                             int* table_window, int* chunk_bytes) {
  int nb = 0;
  const int rc = adam_plan(n_chunks, total_elements, &nb);
  if (rc) return rc;
  if (blocks) *blocks = nb;
  if (threads) *threads = kAdamThreads;
  if (tile_elements) *tile_elements = kAdamTile;
  if (table_window) *table_window = kAdamWindow;
  if (chunk_bytes) *chunk_bytes = (int)sizeof(mal_adam_chunk);
  return MAL_OK;
}

extern "C" int mal_adam_flat(const mal_adam_chunk* table, int n_chunks, int first, int count, long long range_elements,
                             float* grad, float* exp_avg, float* exp_avg_sq, long long flat_elements, int t, float c1,
                             float beta2, float c2, float bs, float eps, float a, int zero_grad, void* stream) {
  if (!table || !grad || !exp_avg || !exp_avg_sq) return MAL_EINVAL;
  if ((((uintptr_t)table) & 7u) || ((((uintptr_t)grad) | ((uintptr_t)exp_avg) | ((uintptr_t)exp_avg_sq)) & 3u)) return MAL_EINVAL;
  if (n_chunks < 1 || first < 0 || count < 0 || first > n_chunks || count > n_chunks - first) return MAL_EINVAL;
  if (flat_elements < 1 || flat_elements >= 2147483648LL || range_elements > flat_elements) return MAL_EINVAL;
  if (t < 1 || !(bs > 0.0f) || !isfinite(bs)) return MAL_EINVAL;
  int nb = 0;
  const int rc = adam_plan(count > 0 ? count : 1, range_elements, &nb);
  if (rc) return rc;
  if (count == 0) return MAL_OK;  // an empty range: nothing to launch
  AdamArgs k;
  k.table = table; k.first = (unsigned)first; k.count = (unsigned)count;
  k.g = grad; k.m = exp_avg; k.v = exp_avg_sq; k.flat_elements = (unsigned)flat_elements;
  k.s.c1 = c1; k.s.beta2 = beta2; k.s.c2 = c2; k.s.bs = bs; k.s.eps = eps; k.s.a = a;
  hipStream_t st = (hipStream_t)stream;
  if (zero_grad) hipLaunchKernelGGL((adam_flat_kernel<true>), dim3(nb), dim3(kAdamThreads), 0, st, k);
  else hipLaunchKernelGGL((adam_flat_kernel<false>), dim3(nb), dim3(kAdamThreads), 0, st, k);
  return launch_status();
}
