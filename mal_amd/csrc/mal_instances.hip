// Mask2Former's instance inference tail for the temporal-hint producer: mask2former/maskformer_model.py:219-227 (the x4
// bilinear upsample of all Q mask-logit planes) + :344-380 (`instance_inference`: softmax, top-k over the flattened Q*K
// scores, gather of the chosen planes, `mask_pred > 0`, the sigmoid copy and two full-size products and sums for the mask
// score, the "thing" filter).  Upstream materialises the upsampled fp32 logits of every query, then the float masks, then
// the sigmoids; here no float plane is ever written: the byte masks the matcher and the synthesis kernels read are the
// only full-size output.  Three launches on the caller's stream, integer atomics on LDS only (their order does not reach
// the result), fixed-order fp64 partial sums, no readback (bit-reproducible):
//   inst_select_kernel  one workgroup per image: softmax statistics per query (fp64 sum of exp(x - max)), every class
//                       probability rounded ONCE to fp32, its bits and the flat index q*K + c in one 64-bit key (keys are
//                       distinct: a tie in the score goes to the lower index), the T-th largest key by a bitwise radix
//                       descent (one ballot-count per bit), the T keys above it ranked among themselves -> slots in
//                       descending score; then the thing filter, survivors compacted in order -> count, classes, query,
//                       cls_score
//   inst_mask_kernel    per (slot, image, 256 source texels): a lane owns one source texel = a 4x4 block of output pixels,
//                       reads its clamped 3x3 neighbourhood, forms the 16 values with the x4 weights (1/8 3/8 5/8 7/8),
//                       stores each row of four bytes as one dword (byte stores when W is not a multiple of 4: the rows
//                       are not dword-aligned then), counts the set pixels and sums sigmoid(v) over them in fp64: lane ->
//                       wave (xor shuffles) -> workgroup (LDS, wave order) -> one partial per workgroup
//   inst_finish_kernel  one lane per slot adds the workgroups' partials in index order; mask_score, score in fp32
#include "mal_common.h"
#include "mal_device.h"

namespace mal {

constexpr int kInstMaskThreads = 256;

struct InstParams {
  const float* logits;       // (N, Q, K+1)
  const float* planes;       // (N, Q, h, w)
  const uint8_t* thing;      // K bytes or null
  int N, Q, K, h, w, H, W, T;
  int nblk;                  // workgroups per slot of the mask launch
  int ibits;                 // bits of the index field of a key
  double* stats;             // ws: [N][Q][2]  max, sum of exp
  int* part_cnt;             // ws: [N][T][nblk]
  double* part_sum;          // ws: [N][T][nblk]
  int32_t* count;            // (N)
  uint8_t* masks;            // (N, T, H, W)
  float* scores;             // (N, T)
  long long* classes;        // (N, T)
  int32_t* query;            // (N, T)
  float* cls_score;          // (N, T)
  float* mask_score;         // (N, T)
};

// THREADS * PER >= Q*K.  Element e (flat index q*K + c) lives in thread e % THREADS, register e / THREADS.
template <int THREADS, int PER>
__global__ __launch_bounds__(THREADS) void inst_select_kernel(InstParams p) {
  constexpr int kWaves = THREADS / 64;
  __shared__ int s_cnt[2][kWaves];
  __shared__ unsigned long long s_sel[MAL_MATCH_MAX], s_sorted[MAL_MATCH_MAX];
  __shared__ int s_fill, s_keep[2];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K, K1 = p.K + 1, nel = p.Q * p.K, T = p.T;
  const float* lg = p.logits + (size_t)n * p.Q * K1;
  double* st = p.stats + (size_t)n * p.Q * 2;
  if (tid == 0) s_fill = 0;
  if (tid < MAL_MATCH_MAX) s_sel[tid] = 0ull;
  for (int q = tid; q < p.Q; q += THREADS) {
    const float* x = lg + (size_t)q * K1;
    float m = x[0];
    for (int c = 1; c < K1; ++c) m = fmaxf(m, x[c]);
    double s = 0.0;
    for (int c = 0; c < K1; ++c) s += exp((double)x[c] - (double)m);
    st[2 * q] = (double)m;
    st[2 * q + 1] = s;
  }
  __syncthreads();  // (the statistics are read back by this workgroup only)
  unsigned long long key[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int e = k * THREADS + tid;
    key[k] = 0ull;  // below every real key: their index field is >= 1
    if (e < nel) {
      const int q = e / K, c = e - q * K;
      const float pr = (float)(exp((double)lg[(size_t)q * K1 + c] - st[2 * q]) / st[2 * q + 1]);
      key[k] = ((unsigned long long)__float_as_uint(pr) << p.ibits) | (unsigned long long)(nel - e);
    }
  }
  // the T-th largest key: a probability is <= 1.0f = 0x3f800000, so bit 29 + ibits is the highest that can be set
  unsigned long long P = 0ull;
  for (int b = 29 + p.ibits; b >= 0; --b) {
    const unsigned long long trial = P | (1ull << b);
    int c = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) c += __popcll(__ballot(key[k] >= trial));
    if (lane == 0) s_cnt[b & 1][wave] = c;
    __syncthreads();  // one barrier per bit: the buffer written two rounds later is this one, and no wave gets there before every wave has left this round
    int tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) tot += s_cnt[b & 1][w];
    if (tot >= T) P = trial;
  }
  // exactly T keys are >= P (they are distinct and T <= Q*K); any order into the list, the rank decides the slot
#pragma unroll
  for (int k = 0; k < PER; ++k)
    if (key[k] >= P && key[k] != 0ull) {
      const int at = atomicAdd(&s_fill, 1);
      if (at < MAL_MATCH_MAX) s_sel[at] = key[k];
    }
  __syncthreads();
  if (tid < T) {
    const unsigned long long mine = s_sel[tid];
    int rank = 0;
    for (int u = 0; u < T; ++u) rank += s_sel[u] > mine ? 1 : 0;
    s_sorted[rank] = mine;
  }
  __syncthreads();
  // the thing filter AFTER the top-k (maskformer_model.py:360-367), survivors compacted in order; T <= 128: waves 0 and 1
  const bool live = tid < T;
  const unsigned long long mine = live ? s_sorted[tid] : 0ull;
  const int e = min(max(nel - (int)(mine & ((1ull << p.ibits) - 1ull)), 0), nel - 1);
  const int q = e / K, c = e - q * K;
  const bool keep = live && (p.thing == nullptr || p.thing[c] != 0);
  const unsigned long long bal = __ballot(keep);
  if (lane == 0 && wave < 2) s_keep[wave] = __popcll(bal);
  __syncthreads();
  const int total = s_keep[0] + s_keep[1];
  const size_t o = (size_t)n * T;
  if (keep) {
    const int pos = (wave == 1 ? s_keep[0] : 0) + __popcll(bal & ((1ull << lane) - 1ull));
    p.classes[o + pos] = c;
    p.query[o + pos] = q;
    p.cls_score[o + pos] = __uint_as_float((unsigned)(mine >> p.ibits));
  }
  if (tid == 0) p.count[n] = total;
  // the slots behind the survivors get defined contents (the mask launch skips them, the finishing launch zeroes their scores)
  for (int t = total + tid; t < T; t += THREADS) {
    p.classes[o + t] = 0;
    p.query[o + t] = -1;
    p.cls_score[o + t] = 0.f;
  }
}

// One lane per source texel (i, j) = output rows 4i..4i+3, columns 4j..4j+3.  ATen's rule (UpSampleBilinear2d,
// align_corners=False, scale 1/4): source = max((o + 0.5)/4 - 0.5, 0), so columns 4j, 4j+1 take texels (j-1, j) with the
// weight 5/8, 7/8 on j and columns 4j+2, 4j+3 take (j, j+1) with 1/8, 3/8 on j+1; at the borders the neighbour index is
// clamped to the texel itself, where ATen has weight 0 on one tap (first two) or both taps equal (last two): the same value.
template <bool DWORD>
__global__ __launch_bounds__(kInstMaskThreads) void inst_mask_kernel(InstParams p) {
  __shared__ int s_c[kInstMaskThreads / 64];
  __shared__ double s_s[kInstMaskThreads / 64];
  const int slot = blockIdx.y, n = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (slot >= p.count[n]) return;  // workgroup-uniform
  const int q = p.query[(size_t)n * p.T + slot];
  const int h = p.h, w = p.w, H = p.H, W = p.W;
  const float* src = p.planes + ((size_t)n * p.Q + q) * h * w;
  uint8_t* dst = p.masks + ((size_t)n * p.T + slot) * H * W;
  const int u = blockIdx.x * kInstMaskThreads + tid;
  int cnt = 0;
  double sum = 0.0;
  if (u < h * w) {
    const int i = u / w, j = u - i * w;
    const int im = max(i - 1, 0), ip = min(i + 1, h - 1), jm = max(j - 1, 0), jp = min(j + 1, w - 1);
    float r[3][4];  // the three source rows, interpolated along x at the four columns
    const int rows[3] = {im, i, ip};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float* s = src + (size_t)rows[k] * w;
      const float a = s[jm], b = s[j], c = s[jp];
      r[k][0] = 0.375f * a + 0.625f * b;
      r[k][1] = 0.125f * a + 0.875f * b;
      r[k][2] = 0.875f * b + 0.125f * c;
      r[k][3] = 0.625f * b + 0.375f * c;
    }
#pragma unroll
    for (int dy = 0; dy < 4; ++dy) {
      const int y = 4 * i + dy;
      if (y >= H) break;
      const float w0 = dy == 0 ? 0.375f : (dy == 1 ? 0.125f : (dy == 2 ? 0.875f : 0.625f));
      const float w1 = 1.f - w0;
      const int ka = dy < 2 ? 0 : 1;  // rows (i-1, i) or (i, i+1)
      float v[4];
      unsigned word = 0u;
#pragma unroll
      for (int dx = 0; dx < 4; ++dx) {
        v[dx] = w0 * r[ka][dx] + w1 * r[ka + 1][dx];
        if (v[dx] > 0.f && 4 * j + dx < W) word |= 1u << (8 * dx);
      }
      if (word) {  // most rows of four of most planes hold no set pixel: a wave without one skips the sigmoids
#pragma unroll
        for (int dx = 0; dx < 4; ++dx)
          if ((word >> (8 * dx)) & 1u) {
            // sigmoid(v) of a set pixel: v > 0, exp(-v) in (0, 1]; hardware exp2 and reciprocal, each ~1 ulp
            cnt += 1;
            sum += (double)__frcp_rn(1.f + __expf(-v[dx]));
          }
      }
      uint8_t* row = dst + (size_t)y * W + 4 * j;
      if (DWORD) {
        *(unsigned*)row = word;  // W == 4w: every row of four is whole and dword-aligned
      } else {
#pragma unroll
        for (int dx = 0; dx < 4; ++dx)
          if (4 * j + dx < W) row[dx] = (uint8_t)((word >> (8 * dx)) & 1u);
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    sum += __shfl_xor(sum, o, 64);
  }
  if (lane == 0) { s_c[wave] = cnt; s_s[wave] = sum; }
  __syncthreads();
  if (tid == 0) {
    int c = 0;
    double s = 0.0;
    for (int k = 0; k < kInstMaskThreads / 64; ++k) { c += s_c[k]; s += s_s[k]; }
    const size_t at = ((size_t)n * p.T + slot) * p.nblk + blockIdx.x;
    p.part_cnt[at] = c;
    p.part_sum[at] = s;
  }
}

__global__ __launch_bounds__(MAL_MATCH_MAX) void inst_finish_kernel(InstParams p) {
  const int n = blockIdx.x, slot = threadIdx.x;
  if (slot >= p.T) return;
  const size_t o = (size_t)n * p.T + slot;
  float ms = 0.f, sc = 0.f;
  if (slot < p.count[n]) {
    long long c = 0;
    double s = 0.0;
    for (int k = 0; k < p.nblk; ++k) { c += p.part_cnt[o * p.nblk + k]; s += p.part_sum[o * p.nblk + k]; }
    ms = c > 0 ? (float)s / ((float)c + 1e-6f) : 0.f;  // maskformer_model.py:377 (0 / 1e-6 there)
    sc = p.cls_score[o] * ms;               // :378
  }
  p.mask_score[o] = ms;
  p.scores[o] = sc;
}

}  // namespace mal

using namespace mal;

static bool inst_sizes_ok(int N, int Q, int K, int h, int w, int H, int W, int T) {
  if (N <= 0 || N > MAL_INSTANCES_MAX_N || Q <= 0 || K <= 0 || h <= 0 || w <= 0 || T <= 0) return false;
  if (K + 1 > MAL_INSTANCES_MAX_K1 || (long long)Q * K > MAL_INSTANCES_MAX_QK) return false;
  if (T > MAL_MATCH_MAX || (long long)T > (long long)Q * K) return false;
  if ((long long)h * w > (1ll << 24)) return false;  // (h*w and 16*h*w as int32)
  if (H <= 4 * (h - 1) || H > 4 * h || W <= 4 * (w - 1) || W > 4 * w) return false;  // the crop of the x4 plane only
  return true;
}

static int inst_nblk(int h, int w) { return (int)(((long long)h * w + kInstMaskThreads - 1) / kInstMaskThreads); }

extern "C" size_t mal_instances_workspace_bytes(int N, int Q, int K, int h, int w, int H, int W, int topk) {
  if (!inst_sizes_ok(N, Q, K, h, w, H, W, topk)) return 0;
  const size_t parts = (size_t)N * topk * inst_nblk(h, w);
  return align256((size_t)N * Q * 2 * sizeof(double)) + align256(parts * sizeof(double)) + align256(parts * sizeof(int)) + 256;
}

extern "C" int mal_instances(const mal_instances_args* a) {
  if (!a) return MAL_EINVAL;
  if (!inst_sizes_ok(a->N, a->Q, a->K, a->h, a->w, a->H, a->W, a->topk)) return MAL_EINVAL;
  if (!a->pred_logits || !a->pred_masks || !a->count || !a->masks || !a->scores || !a->classes || !a->query ||
      !a->cls_score || !a->mask_score || !a->ws)
    return MAL_EINVAL;
  if (a->ws_bytes < mal_instances_workspace_bytes(a->N, a->Q, a->K, a->h, a->w, a->H, a->W, a->topk)) return MAL_EWORKSPACE;
  hipStream_t st = (hipStream_t)a->stream;
  InstParams p;
  p.logits = a->pred_logits; p.planes = a->pred_masks; p.thing = a->thing;
  p.N = a->N; p.Q = a->Q; p.K = a->K; p.h = a->h; p.w = a->w; p.H = a->H; p.W = a->W; p.T = a->topk;
  p.nblk = inst_nblk(a->h, a->w);
  const int nel = a->Q * a->K;
  p.ibits = 1;
  while ((1 << p.ibits) <= nel) ++p.ibits;  // the index field holds 1..nel
  const size_t parts = (size_t)a->N * a->topk * p.nblk;
  char* base = (char*)(((uintptr_t)a->ws + 255) & ~(uintptr_t)255);
  p.stats = (double*)base; base += align256((size_t)a->N * a->Q * 2 * sizeof(double));
  p.part_sum = (double*)base; base += align256(parts * sizeof(double));
  p.part_cnt = (int*)base;
  p.count = a->count; p.masks = a->masks; p.scores = a->scores; p.classes = (long long*)a->classes; p.query = a->query;
  p.cls_score = a->cls_score; p.mask_score = a->mask_score;
  if (nel <= 1024) hipLaunchKernelGGL((inst_select_kernel<256, 4>), dim3(a->N), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((inst_select_kernel<1024, 16>), dim3(a->N), dim3(1024), 0, st, p);
  const dim3 grid((unsigned)p.nblk, (unsigned)a->topk, (unsigned)a->N);
  if (a->W == 4 * a->w && ((uintptr_t)a->masks & 3) == 0)
    hipLaunchKernelGGL(inst_mask_kernel<true>, grid, dim3(kInstMaskThreads), 0, st, p);
  else
    hipLaunchKernelGGL(inst_mask_kernel<false>, grid, dim3(kInstMaskThreads), 0, st, p);
  hipLaunchKernelGGL(inst_finish_kernel, dim3(a->N), dim3(MAL_MATCH_MAX), 0, st, p);
  return launch_status();
}
