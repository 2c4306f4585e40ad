// DynamicDepth's hole-aware reprojection loss on MATERIALISED candidates, forward and backward
// (dynamicdepth/trainer.py:958-975 compute_reprojection_loss with --zero_img, :1058-1064 --selec_reproj; both on by default).
//
//   mal_photo_holes_fwd   hole test per candidate, r_c on the zeroed pair, min / mean / selection, automask, sums
//   mal_holes_commit      target <- target * !(union of the holes): the in-place `target[mask] = 0` of upstream, as a
//                         pointwise launch BEHIND the one that read the target's 3x3 windows
//   mal_photo_holes_bwd   d sum(rp*w) / d candidate, gathered over the 3x3 neighbours from the saved choice and weight
//
// A hole is a pixel whose warped colour sums to less than 0.1 over the three channels (the forward warp of DESIGN.md 16 leaves
// exact zeros there).  With MAL_F_ZERO_IMG the candidate AND the target are zeroed at the candidate's holes before r is
// taken; the target keeps the zeros, so candidate c sees the union U_c = h_0 | .. | h_c.  The zeroed pixels lie inside the
// 3x3 SSIM windows of their neighbours: r changes around a hole, not only in it.
//
// One workgroup per 32x8 tile of output pixels.  It stages the EFFECTIVE images -- candidate c and the target as candidate c
// sees it, zeroed, with the reflection pad already applied -- and the hole bits in LDS with a halo of one pixel (forward) or
// two (backward: a pixel's gradient needs the windows of its eight neighbours).  Every tap of the 2 x 3 channel windows is
// then an LDS read; global memory is read once per tile pixel.  The arithmetic is that of the one-pixel-per-thread kernels
// of mal_photo.hip in the same order (ATen's row-major window sums, ((c0+c1)+c2)/3), so with both flags off, or with no pixel
// under the threshold, the outputs are those of mal_photo_fwd / _bwd under photo_impl = 0 bit for bit.
#include "mal_common.h"
#include "mal_device.h"

namespace mal {

constexpr int kHoleTW = 32, kHoleTH = 8;       // output pixels of a workgroup: 256 threads, one pixel each
constexpr int kHoleHaloFwd = 1, kHoleHaloBwd = 2;
constexpr int kHoleMaxCand = 2;
constexpr float kHoleThreshold = 0.1f;

struct HoleParams {
  const float* target; const float* cand[kHoleMaxCand]; int n_cand;
  const float* ident; const float* noise; const float* ext_mask;
  int B, H, W, flags, tiles_x, tiles_y;
  uint8_t* holes;                 // [n_cand][B][H][W]
  float* min_reproj; uint8_t* choice; float* weight_out; double* block_sums;
  // backward
  const uint8_t* holes_in; const uint8_t* choice_in; const float* weight_in; const float* scale; const double* sums;
  float* g_cand[kHoleMaxCand];
};

// The effective images of one tile: p[c][ch] candidate c, t[c][ch] the target as candidate c meets it, hb the hole bits
// (bit c = h_c).  Position (ly, lx) is image pixel (y0 - HALO + ly, x0 - HALO + lx) REFLECTED into the image (ReflectionPad2d(1);
// positions two outside are clamped and never read by an in-image window).
template <int HALO>
struct HoleTile {
  static constexpr int TW = kHoleTW + 2 * HALO, TH = kHoleTH + 2 * HALO, N = TW * TH;
  float p[kHoleMaxCand][3][N];
  float t[kHoleMaxCand][3][N];
  uint8_t hb[N];
};

// FROM_BYTES: the hole bits are the saved bytes of the forward (backward) instead of the test on the candidate (forward)
template <int HALO, bool FROM_BYTES>
MAL_DEV void hole_tile_load(HoleTile<HALO>& s, const HoleParams& p, int b, int y0, int x0) {
  typedef HoleTile<HALO> T;
  const int H = p.H, W = p.W, HW = H * W;
  const bool zero = p.flags & MAL_F_ZERO_IMG, test = p.flags & (MAL_F_ZERO_IMG | MAL_F_SELECT);
  const size_t img_b = (size_t)b * 3 * HW, map_b = (size_t)b * HW, plane = (size_t)p.B * HW;
  for (int i = threadIdx.x; i < T::N; i += blockDim.x) {
    const int ly = i / T::TW, lx = i - ly * T::TW;
    const int gy = min(max(reflect1(y0 - HALO + ly, H), 0), H - 1);
    const int gx = min(max(reflect1(x0 - HALO + lx, W), 0), W - 1);
    const int pix = gy * W + gx;
    float tv[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) tv[ch] = p.target[img_b + (size_t)ch * HW + pix];
    unsigned bits = 0u, uni = 0u;
#pragma unroll
    for (int c = 0; c < kHoleMaxCand; ++c) {
      if (c >= p.n_cand) break;
      float pv[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) pv[ch] = p.cand[c][img_b + (size_t)ch * HW + pix];
      bool h = false;
      if (test) h = FROM_BYTES ? p.holes_in[(size_t)c * plane + map_b + pix] != 0 : ((pv[0] + pv[1]) + pv[2]) < kHoleThreshold;
      bits |= h ? (1u << c) : 0u;
      uni |= (zero && h) ? 1u : 0u;        // U_c: the target keeps the zeros of the candidates before c
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        s.p[c][ch][i] = (zero && h) ? 0.0f : pv[ch];
        s.t[c][ch][i] = uni ? 0.0f : tv[ch];
      }
    }
    s.hb[i] = (uint8_t)bits;
  }
}

// the five window sums around tile position o = ly * TW + lx, row-major as window_sums of mal_photo.hip
template <int TW>
MAL_DEV float tile_ssim(const float* __restrict__ x, const float* __restrict__ y, int o, SsimStats* st) {
  float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
  for (int i = -1; i <= 1; ++i)
#pragma unroll
    for (int j = -1; j <= 1; ++j) {
      const float xv = x[o + i * TW + j], yv = y[o + i * TW + j];
      a += xv; b += yv; aa += xv * xv; bb += yv * yv; ab += xv * yv;
    }
  return ssim_from_sums(a, b, aa, bb, ab, st);
}

// r(P'_c, T_c) at tile position o: reproj_at of mal_photo.hip on the staged pair
template <int HALO>
MAL_DEV float tile_reproj(const HoleTile<HALO>& s, int c, int o, bool no_ssim) {
  float ssum = 0.f, lsum = 0.f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float l1 = fabsf(s.t[c][ch][o] - s.p[c][ch][o]);
    lsum = ch == 0 ? l1 : lsum + l1;
    if (!no_ssim) {
      const float v = clamp01(tile_ssim<HoleTile<HALO>::TW>(s.p[c][ch], s.t[c][ch], o, nullptr));
      ssum = ch == 0 ? v : ssum + v;
    }
  }
  const float l1m = div3_(lsum);
  if (no_ssim) return l1m;
  return 0.85f * div3_(ssum) + 0.15f * l1m;
}

__global__ __launch_bounds__(256) void photo_holes_fwd_kernel(HoleParams p) {
  constexpr int HALO = kHoleHaloFwd;
  typedef HoleTile<HALO> T;
  __shared__ T s;
  __shared__ double s_red[4][2];
  const int per_b = p.tiles_x * p.tiles_y;
  const int b = blockIdx.x / per_b, tt = blockIdx.x - b * per_b;
  const int y0 = (tt / p.tiles_x) * kHoleTH, x0 = (tt % p.tiles_x) * kHoleTW;
  hole_tile_load<HALO, false>(s, p, b, y0, x0);
  __syncthreads();
  const int ty = threadIdx.x / kHoleTW, tx = threadIdx.x - ty * kHoleTW;
  const int gy = y0 + ty, gx = x0 + tx;
  const bool no_ssim = p.flags & MAL_F_NO_SSIM, avg = p.flags & MAL_F_AVG, automask = p.flags & MAL_F_AUTOMASK;
  double acc_rw = 0.0, acc_w = 0.0;
  if (gy < p.H && gx < p.W) {
    const int o = (ty + HALO) * T::TW + tx + HALO;
    const size_t i = (size_t)b * p.H * p.W + (size_t)gy * p.W + gx;
    const unsigned bits = s.hb[o];
    float r[kHoleMaxCand] = {0.f, 0.f};
#pragma unroll
    for (int c = 0; c < kHoleMaxCand; ++c)
      if (c < p.n_cand) r[c] = tile_reproj<HALO>(s, c, o, no_ssim);
    float rp = r[0];
    int win = 0;
    if (avg) {
      if (p.n_cand == 2) rp = rp + r[1];
      rp = div_(rp, (float)p.n_cand);
      win = MAL_HOLE_CHOICE_AVG;
    } else if (p.n_cand == 2 && r[1] < rp) { rp = r[1]; win = 1; }   // first minimum wins (torch.min)
    if (p.flags & MAL_F_SELECT) {  // trainer.py:1062-1064, in upstream's order: the later assignment overrides
      if (bits & 1u) { rp = r[1]; win = 1; }
      if (bits & 2u) { rp = r[0]; win = 0; }
      if ((bits & 3u) == 3u) { rp = 0.0f; win = MAL_HOLE_CHOICE_NONE; }
    }
    float w = 1.0f;
    if (automask) {
      float idn = p.ident[i];
      if (p.noise) idn += p.noise[i] * 0.00001f;
      w = (rp <= idn) ? 1.0f : 0.0f;
    }
    if (p.ext_mask) w *= p.ext_mask[i];
    if (p.holes) {
      const size_t plane = (size_t)p.B * p.H * p.W;
      for (int c = 0; c < p.n_cand; ++c) p.holes[(size_t)c * plane + i] = (uint8_t)((bits >> c) & 1u);
    }
    if (p.min_reproj) p.min_reproj[i] = rp;
    if (p.choice) p.choice[i] = (uint8_t)win;
    if (p.weight_out) p.weight_out[i] = w;
    acc_rw = (double)(rp * w);
    acc_w = (double)w;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double r0 = wave_sum_d(acc_rw), r1 = wave_sum_d(acc_w);
  if (lane == 0) { s_red[wv][0] = r0; s_red[wv][1] = r1; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int j = threadIdx.x;
    p.block_sums[(size_t)blockIdx.x * 2 + j] = (s_red[0][j] + s_red[1][j]) + (s_red[2][j] + s_red[3][j]);
  }
}

// out[j] = sum_i partial[i*2 + j], j < 2, in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void holes_reduce_kernel(const double* partial, int nparts, double* out) {
  __shared__ double s[256];
  const int tid = threadIdx.x;
  for (int j = 0; j < 2; ++j) {
    double acc = 0.0;
    for (int i = tid; i < nparts; i += 256) acc += partial[(size_t)i * 2 + j];
    s[tid] = acc;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
      if (tid < k) s[tid] += s[tid + k];
      __syncthreads();
    }
    if (tid == 0) out[j] = s[0];
    __syncthreads();
  }
}

// target[b][ch][pix] <- 0 where any candidate of the call has a hole
__global__ __launch_bounds__(256) void holes_commit_kernel(float* target, const uint8_t* holes, int n_cand, int B, int HW) {
  const size_t n = (size_t)B * HW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned u = holes[i];
    if (n_cand == 2) u |= holes[n + i];
    if (!u) continue;
    const size_t b = i / HW, pix = i - b * HW;
    float* t = target + b * 3 * HW + pix;
    t[0] = 0.0f; t[HW] = 0.0f; t[2 * (size_t)HW] = 0.0f;
  }
}

// The weight of a call whose identity term did not exist yet when its rp was taken (upstream evaluates the identity pair
// AFTER the warped pair, on the target the warped pair zeroed): w = [rp <= ident + 1e-5 noise] * ext_mask, and the sums.
__global__ __launch_bounds__(256) void holes_weight_kernel(const float* min_reproj, const float* ident, const float* noise,
                                                           const float* ext_mask, size_t n, float* weight_out,
                                                           double* block_sums) {
  __shared__ double s_red[4][2];
  double acc_rw = 0.0, acc_w = 0.0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float rp = min_reproj[i];
    float w = 1.0f;
    if (ident) {
      float idn = ident[i];
      if (noise) idn += noise[i] * 0.00001f;
      w = (rp <= idn) ? 1.0f : 0.0f;
    }
    if (ext_mask) w *= ext_mask[i];
    weight_out[i] = w;
    acc_rw += (double)(rp * w);
    acc_w += (double)w;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double r0 = wave_sum_d(acc_rw), r1 = wave_sum_d(acc_w);
  if (lane == 0) { s_red[wv][0] = r0; s_red[wv][1] = r1; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int j = threadIdx.x;
    block_sums[(size_t)blockIdx.x * 2 + j] = (s_red[0][j] + s_red[1][j]) + (s_red[2][j] + s_red[3][j]);
  }
}

MAL_DEV float hole_sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }
// multiplicity of neighbour offset d of pixel q along an axis of length n (adjoint of ReflectionPad2d(1)), as mal_photo.hip
MAL_DEV float hole_refl_mult(int q, int d, int n) {
  const int pq = q + d;
  if (pq < 0 || pq >= n) return 0.f;
  if (d == -1 && q == 1) return 2.f;
  if (d == 1 && q == n - 2) return 2.f;
  return 1.f;
}

__global__ __launch_bounds__(256) void photo_holes_bwd_kernel(HoleParams p) {
  constexpr int HALO = kHoleHaloBwd;
  typedef HoleTile<HALO> T;
  constexpr int MW = kHoleTW + 2, MH = kHoleTH + 2;   // choice and weight: the tile and its eight-neighbour ring
  __shared__ T s;
  __shared__ float s_w[MH * MW];
  __shared__ uint8_t s_ch[MH * MW];
  __shared__ float s_part[kHoleMaxCand][3][3][MH * MW];   // d S / d (mu_x, E[x^2], E[xy]) of the pixel's window
  __shared__ uint8_t s_ok[kHoleMaxCand][3][MH * MW];
  const int H = p.H, W = p.W, HW = H * W;
  const int per_b = p.tiles_x * p.tiles_y;
  const int b = blockIdx.x / per_b, tt = blockIdx.x - b * per_b;
  const int y0 = (tt / p.tiles_x) * kHoleTH, x0 = (tt % p.tiles_x) * kHoleTW;
  hole_tile_load<HALO, true>(s, p, b, y0, x0);
  for (int i = threadIdx.x; i < MH * MW; i += blockDim.x) {
    const int ly = i / MW, lx = i - ly * MW;
    const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;   // outside: not a pixel, contributes nothing
    const size_t g = (size_t)b * HW + (size_t)(in ? gy : 0) * W + (in ? gx : 0);
    s_w[i] = in ? p.weight_in[g] : 0.0f;
    s_ch[i] = in ? p.choice_in[g] : (uint8_t)MAL_HOLE_CHOICE_NONE;
  }
  __syncthreads();
  const bool no_ssim = p.flags & MAL_F_NO_SSIM, zero = p.flags & MAL_F_ZERO_IMG;
  // The SSIM partials of a pixel p belong to p alone, and up to nine gathering pixels need them: they are formed once per
  // position of the ring-extended tile -- only for the candidate that feeds rp there, only where the weight is not 0 -- and
  // staged.  s_ok: the partials exist (p is live for (c, ch) and its SSIM value lies inside the clamp).
  if (!no_ssim) {
    for (int i = threadIdx.x; i < MH * MW; i += blockDim.x) {
      const int ly = i / MW, lx = i - ly * MW;
      const int op = (ly + HALO - 1) * T::TW + lx + HALO - 1;
      const int who = s_ch[i];
      const bool live_px = s_w[i] != 0.f;
      for (int c = 0; c < p.n_cand; ++c) {
        const bool live = live_px && p.g_cand[c] && (who == c || who == MAL_HOLE_CHOICE_AVG);
        for (int ch = 0; ch < 3; ++ch) {
          uint8_t ok = 0;
          if (live) {
            SsimStats st;
            tile_ssim<T::TW>(s.p[c][ch], s.t[c][ch], op, &st);
            if (st.gate != 0.f) {
              const SsimGrad gr = ssim_partials(st);
              s_part[c][ch][0][i] = gr.dmx; s_part[c][ch][1][i] = gr.dsxx; s_part[c][ch][2][i] = gr.dsxy;
              ok = 1;
            }
          }
          s_ok[c][ch][i] = ok;
        }
      }
    }
    __syncthreads();
  }
  const int ty = threadIdx.x / kHoleTW, tx = threadIdx.x - ty * kHoleTW;
  const int gy = y0 + ty, gx = x0 + tx;
  if (gy >= H || gx >= W) return;   // (behind the last barrier)
  float sc = p.scale ? *p.scale : 1.0f;
  if (p.sums) sc = (float)((double)sc / (p.sums[1] + 1e-7));
  const float sc_avg = sc / (float)p.n_cand;     // a pixel that took the mean hands each candidate 1/n of its weight
  const int o = (ty + HALO) * T::TW + tx + HALO;
  const int m0 = (ty + 1) * MW + tx + 1;
  const unsigned bits = s.hb[o];
  const float l1w = no_ssim ? (1.0f / 3.0f) : (0.15f / 3.0f);
  for (int c = 0; c < p.n_cand; ++c) {
    float* g = p.g_cand[c];
    if (!g) continue;
    g += (size_t)b * 3 * HW + (size_t)gy * W + gx;
    if (zero && ((bits >> c) & 1u)) {  // the masked copy was written over: no path back to the candidate
      g[0] = 0.0f; g[HW] = 0.0f; g[2 * (size_t)HW] = 0.0f;
      continue;
    }
    for (int ch = 0; ch < 3; ++ch) {
      const float xq = s.p[c][ch][o], yq = s.t[c][ch][o];
      float a_sel = 0.f, a_avg = 0.f;
      if (!no_ssim) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const float m = hole_refl_mult(gy, dy, H) * hole_refl_mult(gx, dx, W);
            if (m == 0.f) continue;
            const int ip = m0 + dy * MW + dx;
            if (!s_ok[c][ch][ip]) continue;   // another candidate feeds rp there, weight 0, or SSIM outside the clamp
            const float kk = -0.5f * (0.85f / 3.0f) * s_w[ip] * m * (1.0f / 9.0f);
            const float term = kk * (s_part[c][ch][0][ip] + 2.0f * xq * s_part[c][ch][1][ip] + yq * s_part[c][ch][2][ip]);
            if (s_ch[ip] == c) a_sel += term; else a_avg += term;
          }
      }
      const int who = s_ch[m0];
      if (who == c) a_sel += hole_sgn(xq - yq) * l1w * s_w[m0];
      else if (who == MAL_HOLE_CHOICE_AVG) a_avg += hole_sgn(xq - yq) * l1w * s_w[m0];
      g[(size_t)ch * HW] = a_avg * sc_avg + a_sel * sc;
    }
  }
}

static int hole_checks(int n_cand, int B, int H, int W, int flags) {
  if (B <= 0 || H < 2 || W < 2) return MAL_EINVAL;
  if (n_cand < 1 || n_cand > kHoleMaxCand) return MAL_EINVAL;
  if ((flags & MAL_F_SELECT) && n_cand != 2) return MAL_EINVAL;
  if (flags & ~(MAL_F_AUTOMASK | MAL_F_NO_SSIM | MAL_F_AVG | MAL_F_ZERO_IMG | MAL_F_SELECT)) return MAL_EINVAL;
  return check_shape(B, H, W);
}

static void hole_tiles(HoleParams& p) {
  p.tiles_x = (p.W + kHoleTW - 1) / kHoleTW;
  p.tiles_y = (p.H + kHoleTH - 1) / kHoleTH;
}

static int hole_ew_grid(size_t n, int cap) {
  const size_t g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > (size_t)cap ? (size_t)cap : g));
}

}  // namespace mal

using namespace mal;

extern "C" int mal_photo_holes_plan(int B, int H, int W, int* tile_w, int* tile_h, int* halo_fwd, int* halo_bwd, int* blocks,
                                    size_t* lds_fwd, size_t* lds_bwd) {
  const int rc = hole_checks(1, B, H, W, 0);
  if (rc) return rc;
  HoleParams p = {};
  p.H = H; p.W = W;
  hole_tiles(p);
  if (tile_w) *tile_w = kHoleTW;
  if (tile_h) *tile_h = kHoleTH;
  if (halo_fwd) *halo_fwd = kHoleHaloFwd;
  if (halo_bwd) *halo_bwd = kHoleHaloBwd;
  if (blocks) *blocks = B * p.tiles_x * p.tiles_y;
  if (lds_fwd) *lds_fwd = sizeof(HoleTile<kHoleHaloFwd>) + 4 * 2 * sizeof(double);
  if (lds_bwd) *lds_bwd = sizeof(HoleTile<kHoleHaloBwd>) + (size_t)(kHoleTW + 2) * (kHoleTH + 2) * ((1 + kHoleMaxCand * 9) * sizeof(float) + 1 + kHoleMaxCand * 3);
  return MAL_OK;
}

extern "C" int mal_photo_holes_fwd(const float* target, const float* const* cand, int n_cand, const float* ident,
                                   const float* noise, const float* ext_mask, int B, int H, int W, int flags, uint8_t* holes,
                                   float* min_reproj, uint8_t* choice, float* weight_out, double* sums, void* ws,
                                   size_t ws_bytes, void* stream) {
  int rc = hole_checks(n_cand, B, H, W, flags);
  if (rc) return rc;
  if (!target || !cand || !sums || !ws) return MAL_EINVAL;
  for (int c = 0; c < n_cand; ++c) if (!cand[c]) return MAL_EINVAL;
  if ((flags & MAL_F_AUTOMASK) && !ident) return MAL_EINVAL;
  if ((flags & MAL_F_ZERO_IMG) && !holes) return MAL_EINVAL;   // the commit and the backward read them
  Workspace w = carve(ws, B, H, W);
  if (ws_bytes < w.bytes) return MAL_EWORKSPACE;
  HoleParams p = {};
  p.target = target; p.n_cand = n_cand;
  for (int c = 0; c < n_cand; ++c) p.cand[c] = cand[c];
  p.ident = ident; p.noise = noise; p.ext_mask = ext_mask; p.B = B; p.H = H; p.W = W; p.flags = flags;
  p.holes = holes; p.min_reproj = min_reproj; p.choice = choice; p.weight_out = weight_out; p.block_sums = w.block_sums;
  hole_tiles(p);
  const int grid = B * p.tiles_x * p.tiles_y;   // 2 doubles each; block_sums holds 8 per 60x8 strip piece (ws_blocks)
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(photo_holes_fwd_kernel, dim3(grid), dim3(256), 0, st, p);
  rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(holes_reduce_kernel, dim3(1), dim3(256), 0, st, w.block_sums, grid, sums);
  return launch_status();
}

extern "C" int mal_holes_commit(float* target, const uint8_t* holes, int n_cand, int B, int H, int W, void* stream) {
  int rc = hole_checks(n_cand, B, H, W, 0);
  if (rc) return rc;
  if (!target || !holes) return MAL_EINVAL;
  hipLaunchKernelGGL(holes_commit_kernel, dim3(hole_ew_grid((size_t)B * H * W, 4096)), dim3(256), 0, (hipStream_t)stream,
                     target, holes, n_cand, B, H * W);
  return launch_status();
}

extern "C" int mal_holes_weight(const float* min_reproj, const float* ident, const float* noise, const float* ext_mask, int B,
                                int H, int W, float* weight_out, double* sums, void* ws, size_t ws_bytes, void* stream) {
  int rc = hole_checks(1, B, H, W, 0);
  if (rc) return rc;
  if (!min_reproj || !weight_out || !sums || !ws || (noise && !ident)) return MAL_EINVAL;
  Workspace w = carve(ws, B, H, W);
  if (ws_bytes < w.bytes) return MAL_EWORKSPACE;
  const size_t n = (size_t)B * H * W;
  const int grid = hole_ew_grid(n, 2048);   // 2 doubles each in the 4096 of scratch
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(holes_weight_kernel, dim3(grid), dim3(256), 0, st, min_reproj, ident, noise, ext_mask, n, weight_out,
                     w.scratch);
  rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(holes_reduce_kernel, dim3(1), dim3(256), 0, st, w.scratch, grid, sums);
  return launch_status();
}

extern "C" int mal_photo_holes_bwd(const float* target, const float* const* cand, int n_cand, const uint8_t* holes,
                                   const uint8_t* choice, const float* weight, const float* scale, const double* sums, int B,
                                   int H, int W, int flags, float* const* g_cand, void* stream) {
  int rc = hole_checks(n_cand, B, H, W, flags);
  if (rc) return rc;
  if (!target || !cand || !choice || !weight || !g_cand) return MAL_EINVAL;
  if ((flags & (MAL_F_ZERO_IMG | MAL_F_SELECT)) && !holes) return MAL_EINVAL;
  HoleParams p = {};
  p.target = target; p.n_cand = n_cand;
  for (int c = 0; c < n_cand; ++c) { if (!cand[c]) return MAL_EINVAL; p.cand[c] = cand[c]; p.g_cand[c] = g_cand[c]; }
  p.B = B; p.H = H; p.W = W; p.flags = flags; p.holes_in = holes; p.choice_in = choice; p.weight_in = weight;
  p.scale = scale; p.sums = sums;
  hole_tiles(p);
  hipLaunchKernelGGL(photo_holes_bwd_kernel, dim3(B * p.tiles_x * p.tiles_y), dim3(256), 0, (hipStream_t)stream, p);
  return launch_status();
}
