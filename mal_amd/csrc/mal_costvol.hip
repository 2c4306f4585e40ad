// N3: ManyDepth's cost volume as MAL's student encoder builds it, forward only (upstream runs
// it under torch.no_grad()): manydepth/networks/resnet_encoder.py:152-233 `match_features` and the lines of
// `ResnetEncoderMatching.forward` that consume it (:296-312).
//
// Upstream loops over the batch in Python and, per sample and lookup frame, replicates the 64-channel feature
// map 96 times, back-projects / projects 96 x h x w points through ~10 ATen launches, grid_samples 189 MB and
// reduces it again.  Here: features channel-last (B,h,w,64), one wavefront per output pixel, two launches.
//
//   costvol_match_kernel   phase 1: lane = depth bin.  Each lane back-projects the pixel to ITS bin's depth,
//                          projects it into the lookup frame (layers.py:163-199), unnormalises (zeros padding,
//                          align_corners=True), and keeps the four tap offsets (clamped), the four weights
//                          (zeroed for taps outside the image) and the border mask of resnet_encoder.py:199-211.
//                          phase 2: lane = channel.  For every bin the tap data is broadcast from its lane, the
//                          four taps are four coalesced 256-byte loads, |warped - current| is summed over the
//                          wave, and the bin's lane accumulates mean * mask and the hit count over the frames.
//                          Result: cost / (counts + 1e-7) per (bin, pixel).
//   costvol_finish_kernel  per pixel over the bins: missing = (cost == 0), missing bins take the pixel's maximum
//                          (:221-226), confidence = every bin seen (:255-262, 299-300), lowest_cost = 1 / depth
//                          of the first minimum with zeros read as 100 (:303-307), volume x confidence (:311).
#include "mal_common.h"
#include "mal_device.h"
#include "mal_sample.h"

namespace mal {

constexpr int kCvC = 64;  // feature channels = lanes (ResNet-18 stage 1, num_ch_enc[1])

struct CostVolParams {
  const float* cur;    // (B,h,w,64)
  const float* look;   // (B,F,h,w,64)
  const float* K; const float* invK;  // (B,16) at the matching resolution
  const float* poses;  // (B,F,16)
  const float* bins;   // (D)
  int B, F, D, h, w; float eps; int set_missing_to_max;
  float* cost;         // (B,D,h,w) normalised cost, then (finish) the returned volume
  float* missing;      // (B,D,h,w) nullable
  float* masked;       // (B,D,h,w) nullable: volume x confidence
  float* lowest_cost;  // (B,h,w) nullable
  float* confidence;   // (B,h,w) nullable
};

struct TapSet { int o[4]; float w[4]; float edge; };

// pix_locs of one (pixel, depth): X = depth * ray (layers.py:163-168), project and normalise (:184-199).  The one place this
// chain is written: the feature taps below and the occlusion mask of the DynamicDepth variant sample at the same position.
MAL_DEV void grid_position(const float* P, const float* ray, float depth, float eps, int w, int h, float& gx, float& gy) {
  const float X[3] = {depth * ray[0], depth * ray[1], depth * ray[2]};
  float c[3];
  for (int i = 0; i < 3; ++i) {
    float acc = P[4 * i] * X[0];
    acc = fma_(P[4 * i + 1], X[1], acc);
    acc = fma_(P[4 * i + 2], X[2], acc);
    c[i] = fma_(P[4 * i + 3], 1.0f, acc);
  }
  const float zp = c[2] + eps;
  const float u = div_safe_(c[0], zp), v = div_safe_(c[1], zp);
  gx = (div_(u, (float)(w - 1)) - 0.5f) * 2.0f;
  gy = (div_(v, (float)(h - 1)) - 0.5f) * 2.0f;
}

// the reference's chain for one (pixel, depth): grid_position, grid_sample's unnormalise (align_corners=True), the border mask
// of resnet_encoder.py:199-205 on the sampling position, and the zero-padded taps of mal_sample.h (element offsets)
MAL_DEV TapSet taps_for(const float* P, const float* ray, float depth, float eps, int w, int h) {
  TapSet t;
  float gx, gy;
  grid_position(P, ray, depth, eps, w, h, gx, gy);
  const float wm1 = (float)(w - 1), hm1 = (float)(h - 1);
  const float ix = (gx + 1.0f) * (wm1 * 0.5f), iy = (gy + 1.0f) * (hm1 * 0.5f);
  const float xv = (gx / 2.0f + 0.5f) * wm1, yv = (gy / 2.0f + 0.5f) * hm1;
  t.edge = (xv >= 2.0f && xv <= (float)(w - 2) && yv >= 2.0f && yv <= (float)(h - 2)) ? 1.0f : 0.0f;
  const Corners c = corners_of(ix, iy, w, h);
  for (int k = 0; k < 4; ++k) t.o[k] = c.o[k];
  tap_weights(c, frac_one_minus(ix, iy, c), t.w);
  return t;
}

// 64-lane sum with DPP only (no LDS crossbar): pairs, quads, half rows, rows, then the two row broadcasts;
// the total lands in lane 63
template <int CTRL, int ROW_MASK>
MAL_DEV float dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}
MAL_DEV float wave_sum_dpp(float v) {
  v = dpp_add<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
  v = dpp_add<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
  v = dpp_add<0x141, 0xf>(v);  // row_half_mirror
  v = dpp_add<0x140, 0xf>(v);  // row_mirror: every lane holds its row's sum
  v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 into rows 1, 3
  v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 into rows 2, 3
  return v;
}

MAL_DEV float bcast(float v, int lane) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane)); }
MAL_DEV int bcasti(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

MAL_DEV bool frame_missing(const float* T) {  // an all-zero pose is a missing lookup frame (:176-178); uniform per (b, f)
  float tsum = 0.f;
  for (int i = 0; i < 16; ++i) tsum += T[i];
  return tsum == 0.f;
}

MAL_DEV bool inner_pixel(int x, int y, int w, int h) { return y >= 2 && y < h - 2 && x >= 2 && x < w - 2; }  // resnet_encoder.py:208-210

// the sample's inverse intrinsics (kept: the pooled fill derives its neighbours' rays from them) and the pixel's ray
MAL_DEV void pixel_ray(const CostVolParams& p, int b, int x, int y, float ik[9], float ray[3]) {
  for (int e = 0; e < 9; ++e) ik[e] = p.invK[b * 16 + (e / 3) * 4 + (e % 3)];
  ray_of(ik, (float)x, (float)y, ray);
}

__global__ __launch_bounds__(256) void costvol_match_kernel(CostVolParams p) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int h = p.h, w = p.w, hw = h * w;
  const int xg = blockIdx.x * 4 + wv, y = blockIdx.y, b = blockIdx.z;
  if (xg >= w) return;
  const int pix = y * w + xg;
  const int rounds = (p.D + 63) / 64;
  float* out = p.cost + (size_t)b * p.D * hw + pix;
  if (!inner_pixel(xg, y, w, h)) {  // every difference is masked: cost 0 / (0 + 1e-7) = 0
    for (int k = 0; k < rounds; ++k)
      if (k * 64 + lane < p.D) out[(size_t)(k * 64 + lane) * hw] = 0.f;
    return;
  }
  const float curv = p.cur[((size_t)b * hw + pix) * kCvC + lane];
  float ray[3], ik[9];
  pixel_ray(p, b, xg, y, ik, ray);
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, cnt[4] = {0.f, 0.f, 0.f, 0.f};  // bins lane, lane+64, ... (D <= 256)
  for (int f = 0; f < p.F; ++f) {
    const float* T = p.poses + ((size_t)b * p.F + f) * 16;
    if (frame_missing(T)) continue;
    float P[12];
    compose_P(p.K + b * 16, T, P);
    const float* lf = p.look + (((size_t)b * p.F + f) * hw) * kCvC + lane;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= rounds) break;
      const int dmine = k * 64 + lane;
      const TapSet t = taps_for(P, ray, p.bins[min(dmine, p.D - 1)], p.eps, w, h);  // phase 1: lane = bin
      const int nb = min(64, p.D - k * 64);
      for (int j = 0; j < nb; ++j) {                                                   // phase 2: lane = channel
        if (bcast(t.edge, j) == 0.f) continue;  // masked out (wave-uniform): the difference would be multiplied by 0
        const int o0 = bcasti(t.o[0], j), o1 = bcasti(t.o[1], j), o2 = bcasti(t.o[2], j), o3 = bcasti(t.o[3], j);
        const float wj[4] = {bcast(t.w[0], j), bcast(t.w[1], j), bcast(t.w[2], j), bcast(t.w[3], j)};
        const float o = blend4(lf[(size_t)o0 * kCvC], lf[(size_t)o1 * kCvC], lf[(size_t)o2 * kCvC], lf[(size_t)o3 * kCvC], wj);
        const float s = wave_sum_dpp(fabsf(o - curv));        // lane 63 holds the sum
        const float diff = bcast(s, 63) * (1.0f / (float)kCvC) * bcast(t.edge, j);
        if (lane == j) { acc[k] += diff; cnt[k] += diff > 0.f ? 1.0f : 0.f; }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < rounds && k * 64 + lane < p.D) out[(size_t)(k * 64 + lane) * hw] = div_(acc[k], cnt[k] + 1e-7f);
}

// Second formulation (default): features stay PLANAR (B,C,h,w) as the encoder produces them -- no relayout -- and
// lane = pixel: a wavefront owns 64 consecutive pixels and kCvG consecutive depth bins.  Per lookup frame every lane
// derives its taps for its bins once (phase 1 of the first formulation, without the broadcast), then walks the 64
// channel planes: per (bin, channel) four dword loads whose lanes fall in adjacent addresses (neighbouring pixels
// sample neighbouring positions) and that move only a little from bin to bin (the epipolar line), so they hit the
// L1 -- and 6 VALU operations, with no cross-lane reduction at all (the channel sum is a per-lane running sum).
// bins per wavefront, (4 offsets + 4 weights) registers each.  Measured at B=12 48x160 D=96: 2..6 bins 0.50 ms, 8 0.52,
// 12 0.88, 16 1.28 (spills); forcing three or four waves per SIMD through the launch bounds is slower (0.65-0.74 ms:
// the compiler's wide version keeps more loads in flight); loading a row's two taps as one unaligned 8-byte pair is
// slower too (0.58 ms).
constexpr int kCvG = 6;

// ---- the parts of a lane = pixel matching kernel, written once: costvol_match_px_kernel and costvol_match_dyn_kernel are
// match_px below and nothing else; costvol_match_pool_kernel (an LDS tile, thread = pixel) uses them around its tile code.
// One frame's taps of a pixel for its kCvG bins: byte offsets, weights, the border mask (0 outside the inner region) and
// zeroed channel sums.  Returns whether any bin of this lane carries a cost.
MAL_DEV bool frame_taps(const CostVolParams& p, const float* P, const float* ray, int d0, bool inner, unsigned off[kCvG][4],
                        float wt[kCvG][4], float edge[kCvG], float sum[kCvG]) {
  bool any = false;
#pragma unroll
  for (int j = 0; j < kCvG; ++j) {
    const TapSet t = taps_for(P, ray, p.bins[min(d0 + j, p.D - 1)], p.eps, p.w, p.h);
#pragma unroll
    for (int k = 0; k < 4; ++k) { off[j][k] = (unsigned)t.o[k] * 4u; wt[j][k] = t.w[k]; }
    edge[j] = inner ? t.edge : 0.f;
    sum[j] = 0.f;
    any = any || edge[j] != 0.f;
  }
  return any;
}

// the plain loop: sum over the 64 channel planes of |warped lookup - current| for the pixel's kCvG bins
MAL_DEV void channel_sums(const float* lf, const float* cf, int hw, int pix, const unsigned (*off)[4], const float (*wt)[4],
                          float sum[kCvG]) {
  for (int ch = 0; ch < kCvC; ++ch) {
    const char* pl = reinterpret_cast<const char*>(lf + (size_t)ch * hw);
    const float cv = cf[(size_t)ch * hw + pix];
#pragma unroll
    for (int j = 0; j < kCvG; ++j) sum[j] += fabsf(plane_sample(pl, off[j], wt[j]) - cv);
  }
}

// Frames fuse by the mean over the hits (ManyDepth; DynamicDepth without cv_min) or by minimum (cv_min, :226: a difference
// of 0 reads as 1 = no change, and an untouched 1 is stored as 0).
template <bool CVMIN>
MAL_DEV void fuse_init(float acc[kCvG], float cnt[kCvG]) {
#pragma unroll
  for (int j = 0; j < kCvG; ++j) { acc[j] = CVMIN ? 1.f : 0.f; cnt[j] = 0.f; }
}
template <bool CVMIN>
MAL_DEV void fuse_frame(const float sum[kCvG], const float edge[kCvG], float acc[kCvG], float cnt[kCvG]) {
#pragma unroll
  for (int j = 0; j < kCvG; ++j) {
    const float diff = sum[j] * (1.0f / (float)kCvC) * edge[j];
    if (CVMIN) {
      const float dm = diff == 0.f ? 1.0f : diff;
      acc[j] = (dm < acc[j] || dm != dm) ? dm : acc[j];  // torch.minimum
    } else {
      acc[j] += diff;
      cnt[j] += diff > 0.f ? 1.0f : 0.f;
    }
  }
}
template <bool CVMIN>
MAL_DEV void store_bins(const CostVolParams& p, int b, int pix, int d0, bool live, const float acc[kCvG], const float cnt[kCvG]) {
  const int hw = p.h * p.w;
  float* out = p.cost + (size_t)b * p.D * hw + pix;
#pragma unroll
  for (int j = 0; j < kCvG; ++j)  // mean: 0 / 1e-7 = 0 outside the inner region
    if (live && d0 + j < p.D) out[(size_t)(d0 + j) * hw] =CVMIN ? (acc[j] == 1.0f ? 0.f : acc[j]) : div_(acc[j], cnt[j] + 1e-7f);
}

// The matching loop of a wavefront that owns 64 consecutive pixels and kCvG bins.  OCC = false: the plain loop and nothing
// else.  OCC = true: DynamicDepth's set_1 -- only in a wavefront that holds a masked cell (byte of m) with a live border mask,
// the masked cells take |1 - current| per channel; aug (nullable) switches that off per sample, read here.
template <bool OCC, bool CVMIN>
MAL_DEV void match_px(const CostVolParams& p, const unsigned char* m, const float* aug) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int h = p.h, w = p.w, hw = h * w;
  const int pix0 = (blockIdx.x * 4 + wv) * 64, grp = blockIdx.y, b = blockIdx.z;
  if (pix0 >= hw) return;
  const bool live = pix0 + lane < hw;
  const int pix = min(pix0 + lane, hw - 1);
  const int y = pix / w, x = pix - y * w;
  const bool inner = inner_pixel(x, y, w, h);
  const int d0 = grp * kCvG;
  float ray[3], ik[9];
  pixel_ray(p, b, x, y, ik, ray);
  float acc[kCvG], cnt[kCvG];
  fuse_init<CVMIN>(acc, cnt);
  const float* cf = p.cur + (size_t)b * kCvC * hw;
  const bool occ_on = OCC && !(aug && aug[b] != 0.f);  // :192, on the device; wave-uniform
  for (int f = 0; f < p.F; ++f) {
    const float* T = p.poses + ((size_t)b * p.F + f) * 16;
    if (frame_missing(T)) continue;
    float P[12];
    compose_P(p.K + b * 16, T, P);
    unsigned off[kCvG][4];
    float wt[kCvG][4], edge[kCvG], sum[kCvG];
    const bool any = frame_taps(p, P, ray, d0, inner, off, wt, edge, sum);
    if (__ballot(any) == 0ull) continue;  // every (pixel, bin) of this wave is masked out: diffs 0, which cv_min reads as no change
    channel_sums(p.look + ((size_t)b * p.F + f) * kCvC * hw, cf, hw, pix, off, wt, sum);
    if (OCC && occ_on) {
      // a masked cell whose border mask is 0 keeps a difference of 0 whatever it samples
      const unsigned char* mf = m + ((size_t)b * p.F + f) * p.D * hw;
      bool need[kCvG], anyneed = false;
#pragma unroll
      for (int j = 0; j < kCvG; ++j) {
        need[j] = d0 + j < p.D && edge[j] != 0.f && mf[(size_t)(d0 + j) * hw + pix] != 0;
        anyneed = anyneed || need[j];
      }
      if (__ballot(anyneed) != 0ull) {  // set_1 (the pooled fill has a kernel of its own)
        float s1 = 0.f;
        for (int ch = 0; ch < kCvC; ++ch) s1 += fabsf(1.0f - cf[(size_t)ch * hw + pix]);
#pragma unroll
        for (int j = 0; j < kCvG; ++j) sum[j] = need[j] ? s1 : sum[j];
      }
    }
    fuse_frame<CVMIN>(sum, edge, acc, cnt);
  }
  store_bins<CVMIN>(p, b, pix, d0, live, acc, cnt);
}

__global__ __launch_bounds__(256) void costvol_match_px_kernel(CostVolParams p) { match_px<false, false>(p, nullptr, nullptr); }


// 64 pixels per workgroup, the bins split over its four wavefronts (lane = pixel: every access is a coalesced row
// piece of one bin plane); the pixel's maximum / hit count / first minimum are combined through LDS in bin order
__global__ __launch_bounds__(256) void costvol_finish_kernel(CostVolParams p) {
  __shared__ float s_mx[4][64], s_best[4][64];
  __shared__ int s_seen[4][64], s_arg[4][64];
  const int hw = p.h * p.w, lane = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  const bool live = i < p.B * hw;
  const int ii = live ? i : p.B * hw - 1;
  const int b = ii / hw, pix = ii - b * hw;
  const int per = (p.D + 3) / 4, d_lo = min(part * per, p.D), d_hi = min(d_lo + per, p.D);
  float* c = p.cost + (size_t)b * p.D * hw + pix;
  float mx = -INFINITY;
  int seen = 0;
#pragma unroll 8
  for (int d = d_lo; d < d_hi; ++d) {
    const float v = c[(size_t)d * hw];
    mx = fmaxf(mx, v);
    seen += v > 0.f ? 1 : 0;  // (cost * (1 - missing) > 0): a missing bin is exactly 0
  }
  s_mx[part][lane] = mx; s_seen[part][lane] = seen;
  __syncthreads();
  mx = fmaxf(fmaxf(s_mx[0][lane], s_mx[1][lane]), fmaxf(s_mx[2][lane], s_mx[3][lane]));
  seen = (s_seen[0][lane] + s_seen[1][lane]) + (s_seen[2][lane] + s_seen[3][lane]);
  const float conf = seen == p.D ? 1.0f : 0.0f;
  float best = INFINITY;
  int arg = 0;
#pragma unroll 4
  for (int d = d_lo; d < d_hi; ++d) {
    const float v = c[(size_t)d * hw];
    const float miss = v == 0.f ? 1.0f : 0.0f;
    const float filled = p.set_missing_to_max ? v * (1.0f - miss) + mx * miss : v;
    const float viz = filled == 0.f ? 100.0f : filled;
    if (viz < best) { best = viz; arg = d; }  // first minimum, as torch.min
    if (live) {
      const size_t o = (size_t)b * p.D * hw + (size_t)d * hw + pix;
      c[(size_t)d * hw] = filled;
      if (p.missing) p.missing[o] = miss;
      if (p.masked) p.masked[o] = filled * conf;
    }
  }
  s_best[part][lane] = best; s_arg[part][lane] = arg;
  __syncthreads();
  if (part == 0 && live) {
    for (int k = 1; k < 4; ++k)
      if (s_best[k][lane] < best) { best = s_best[k][lane]; arg = s_arg[k][lane]; }  // strict: the earlier bin wins a tie
    if (p.confidence) p.confidence[i] = conf;
    if (p.lowest_cost) p.lowest_cost[i] = div_(1.0f, p.bins[arg]);
  }
}

// ---- DynamicDepth's occlusion-aware variant (dynamicdepth/networks/resnet_encoder.py:148-249), DESIGN.md 17 -------------
// Four launches when set_1 or pool is on, two otherwise:
//   costvol_occ_image_kernel  (:160) one thread per cell of the 48x128 occlusion image of every lookup image: nearest source
//                             pixel as ATen picks it, channel sum (c0 + c1) + c2 < 0.15f, one byte.
//   costvol_occ_mask_kernel   (:194-195) m(b,f,d,y,x): the bilinear sample (zero padding, align_corners) of occ[b] -- the
//                             image of FLAT index b, upstream's indexing, not b*F+f -- at the cell's sampling position,
//                             compared strictly with pool_th; one byte per cell, every pixel (the pool reads border pixels
//                             as neighbours).  Skipped for augmented samples and missing frames, whose bytes are never read.
//   costvol_match_dyn_kernel  options off and set_1: match_px above, the very body of costvol_match_px_kernel; with set_1 -- only
//                             in a wavefront that holds a masked cell with a live border mask -- the masked cells take
//                             |1 - current| per channel.
//   costvol_match_pool_kernel pool: an LDS tile of 8 x 32 pixels x 6 bins with a halo of r (described at the kernel); a
//                             neighbour's sample comes from taps_for with ITS ray and bin and from plane_sample, the function
//                             the centre uses, so the maximum is exact and does not depend on the tiling.
//                             Frames fuse by minimum (cv_min) or by the mean over the hits, in both.
//   costvol_finish_kernel     unchanged.
constexpr int kOccH = 48, kOccW = 128;  // resnet_encoder.py:160: fixed, whatever the matching resolution is

struct CostVolDynParams {
  CostVolParams cv;
  const float* images;   // (B*F,3,H,W)
  const float* aug;      // (B) nullable: != 0 switches the occlusion handling off for the sample
  int H, W;
  float pool_th;
  unsigned char* occ;    // (B*F,48,128)
  unsigned char* m;      // (B,F,D,h,w)
};

__global__ __launch_bounds__(256) void costvol_occ_image_kernel(CostVolDynParams q) {
  const int i = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (i >= kOccH * kOccW) return;
  const int oy = i / kOccW, ox = i - oy * kOccW;
  // ATen's nearest rule: floor(dst * (float)(in / out)) clamped to in - 1
  const int sy = min((int)floorf((float)oy * ((float)q.H / (float)kOccH)), q.H - 1);
  const int sx = min((int)floorf((float)ox * ((float)q.W / (float)kOccW)), q.W - 1);
  const float* im = q.images + (size_t)n * 3 * q.H * q.W + (size_t)sy * q.W + sx;
  const size_t pl = (size_t)q.H * q.W;
  const float s = (im[0] + im[pl]) + im[2 * pl];
  q.occ[(size_t)n * kOccH * kOccW + i] = s < 0.15f ? 1 : 0;
}

__global__ __launch_bounds__(256) void costvol_occ_mask_kernel(CostVolDynParams q) {
  const CostVolParams& p = q.cv;
  const int h = p.h, w = p.w, hw = h * w;
  const int pix = blockIdx.x * 256 + threadIdx.x, d = blockIdx.y, bf = blockIdx.z, b = bf / p.F;
  if (pix >= hw) return;
  if (q.aug && q.aug[b] != 0.f) return;
  const float* T = p.poses + (size_t)bf * 16;
  if (frame_missing(T)) return;
  const int y = pix / w, x = pix - y * w;
  float ray[3], ik[9], P[12];
  pixel_ray(p, b, x, y, ik, ray);
  compose_P(p.K + b * 16, T, P);
  float gx, gy;
  grid_position(P, ray, p.bins[d], p.eps, w, h, gx, gy);  // the position the feature taps are built from
  // grid_sample on the 48x128 image: zeros padding, bilinear, align_corners=True
  const float ix = ((gx + 1.0f) / 2.0f) * (float)(kOccW - 1), iy = ((gy + 1.0f) / 2.0f) * (float)(kOccH - 1);
  const Corners c = corners_of(ix, iy, kOccW, kOccH);
  const Frac fr = frac_one_minus(ix, iy, c);
  const unsigned char* oc = q.occ + (size_t)b * kOccH * kOccW;  // occ[b], not occ[b*F+f] (:194)
  float val = 0.f;
  if (!c.wild) {  // byte taps, unzeroed weights and plain adds: this sample keeps its own arithmetic
    auto tap = [&](int k) { return c.v[k] ? (float)oc[c.o[k]] : 0.f; };
    val = tap(0) * (fr.ex * fr.ey);
    val += tap(1) * (fr.tx * fr.ey);
    val += tap(2) * (fr.ex * fr.ty);
    val += tap(3) * (fr.tx * fr.ty);
  }
  q.m[((size_t)bf * p.D + d) * hw + pix] = val > q.pool_th ? 1 : 0;
}

template <bool OCC, bool CVMIN>
__global__ __launch_bounds__(256) void costvol_match_dyn_kernel(CostVolDynParams q) { match_px<OCC, CVMIN>(q.cv, q.m, q.aug); }


// The pooled fill as an LDS tile.  A workgroup owns 8 x 32 pixels (thread = pixel) and kCvG bins.  Options and frames are
// tested workgroup-uniformly; a tile without a masked cell that carries a cost runs the plain loop.  Otherwise the tile plus a
// halo of R in bin, y and x is spread over the threads (cell i of the haloed tile belongs to thread i mod 256): each thread
// derives ITS cells' taps once per frame with taps_for from the cell's own ray and bin, and per channel writes their samples
// -- plane_sample, the function of the plain loop; 0 for masked cells and for cells outside the volume, which is what they
// contribute to a maximum that already holds the masked centre's 0 -- into one of two LDS planes; after one barrier every
// thread takes, for each of its own cells, the plane's value (unmasked: the very sample the plain loop computes), or the
// maximum over the (2R+1)^3 window (masked), or 0 outright when the whole window is masked (found once per frame from the
// mask bytes).  The window maximum is taken separably -- along x, along y, along the bins: 3 (2R+1) reads instead of
// (2R+1)^3, the same value since a maximum does not depend on the order -- through two more LDS planes and two more
// barriers, and only in a tile that holds a masked cell with an unmasked neighbour.  The sample plane is double-buffered.
constexpr int kPtY = 8, kPtX = 32;

template <int R, bool CVMIN>
__global__ __launch_bounds__(256) void costvol_match_pool_kernel(CostVolDynParams q) {
  constexpr int TD = kCvG + 2 * R, TY = kPtY + 2 * R, TX = kPtX + 2 * R, NCELL = TD * TY * TX, NC = (NCELL + 255) / 256;
  __shared__ float s_v[2][NCELL];
  __shared__ float s_x[TD * TY * kPtX], s_y[TD * kPtY * kPtX];
  const CostVolParams& p = q.cv;
  const int tid = threadIdx.x, ly = tid / kPtX, lx = tid - ly * kPtX;
  const int h = p.h, w = p.w, hw = h * w;
  const int tiles_x = (w + kPtX - 1) / kPtX;
  const int ty0 = (blockIdx.x / tiles_x) * kPtY, tx0 = (blockIdx.x % tiles_x) * kPtX;
  const int grp = blockIdx.y, b = blockIdx.z, d0 = grp * kCvG;
  const bool live = ty0 + ly < h && tx0 + lx < w;
  const int y = min(ty0 + ly, h - 1), x = min(tx0 + lx, w - 1), pix = y * w + x;
  const bool inner = live && inner_pixel(x, y, w, h);
  float ray[3], ik[9];
  pixel_ray(p, b, x, y, ik, ray);
  float acc[kCvG], cnt[kCvG];
  fuse_init<CVMIN>(acc, cnt);
  const float* cf = p.cur + (size_t)b * kCvC * hw;
  const bool occ_on = !(q.aug && q.aug[b] != 0.f);  // :192, on the device; workgroup-uniform
  for (int f = 0; f < p.F; ++f) {
    const float* T = p.poses + ((size_t)b * p.F + f) * 16;
    if (frame_missing(T)) continue;  // workgroup-uniform
    float P[12];
    compose_P(p.K + b * 16, T, P);
    float edge[kCvG], sum[kCvG];
    bool any = false;
#pragma unroll
    for (int j = 0; j < kCvG; ++j) {
      edge[j] = inner ? taps_for(P, ray, p.bins[min(d0 + j, p.D - 1)], p.eps, w, h).edge : 0.f;
      sum[j] = 0.f;
      any = any || edge[j] != 0.f;
    }
    if (__syncthreads_or(any) == 0) continue;  // every difference of the tile is x 0
    const float* lf = p.look + ((size_t)b * p.F + f) * kCvC * hw;
    const unsigned char* mf = q.m + ((size_t)b * p.F + f) * p.D * hw;
    // what each own cell takes per channel: 0 its own sample, 1 the window maximum, 2 nothing but 0 (whole window masked)
    int state[kCvG];
    bool anyneed = false;
#pragma unroll
    for (int j = 0; j < kCvG; ++j) {
      const int dc = d0 + j;
      state[j] = 0;
      if (occ_on && dc < p.D && edge[j] != 0.f && mf[(size_t)dc * hw + pix] != 0) {
        bool open = false;  // an inner pixel: with R <= 2 the window stays inside the image in x and y
#pragma unroll 1
        for (int dn = max(dc - R, 0); dn <= min(dc + R, p.D - 1); ++dn)
#pragma unroll 1
          for (int dy = -R; dy <= R; ++dy)
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) open = open || mf[(size_t)dn * hw + pix + dy * w + dx] == 0;
        state[j] = open ? 1 : 2;
        anyneed = true;
      }
    }
    bool anyopen = false;
#pragma unroll
    for (int j = 0; j < kCvG; ++j) anyopen = anyopen || state[j] == 1;
    const bool tile_need = __syncthreads_or(anyneed) != 0, tile_open = __syncthreads_or(anyopen) != 0;
    unsigned coff[NC][4];
    float cwt[NC][4];
    unsigned zero = 0u;  // bit k: this thread's cell k contributes 0 (masked, outside the volume, or past the tile)
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      int cd = 0, cy = 0, cx = 0;
      bool valid;
      if (tile_need) {
        const int i = tid + k * 256, ii = min(i, NCELL - 1);
        const int dz = ii / (TY * TX), rem = ii - dz * (TY * TX), ry = rem / TX;
        cd = d0 - R + dz; cy = ty0 - R + ry; cx = tx0 - R + (rem - ry * TX);
        valid = i < NCELL && cd >= 0 && cd < p.D && cy >= 0 && cy < h && cx >= 0 && cx < w;
      } else {  // the plain loop: this thread's own cells
        cd = d0 + k; cy = y; cx = x;
        valid = k < kCvG;
      }
      cd = min(max(cd, 0), p.D - 1); cy = min(max(cy, 0), h - 1); cx = min(max(cx, 0), w - 1);
      if (tile_need && valid && mf[(size_t)cd * hw + cy * w + cx] != 0) valid = false;
      float nray[3];
      ray_of(ik, (float)cx, (float)cy, nray);
      const TapSet t = taps_for(P, nray, p.bins[cd], p.eps, w, h);
#pragma unroll
      for (int c = 0; c < 4; ++c) { coff[k][c] = (unsigned)t.o[c] * 4u; cwt[k][c] = t.w[c]; }
      if (!valid) zero |= 1u << k;
    }
    if (!tile_need) {
      channel_sums(lf, cf, hw, pix, coff, cwt, sum);  // NC >= kCvG: cells 0..kCvG-1 are this thread's own
    } else {
      for (int ch = 0; ch < kCvC; ++ch) {
        float* buf = s_v[ch & 1];
        const char* pl = reinterpret_cast<const char*>(lf + (size_t)ch * hw);
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          const int i = tid + k * 256;
          const float v = plane_sample(pl, coff[k], cwt[k]);
          if (i < NCELL) buf[i] = ((zero >> k) & 1u) ? 0.f : v;
        }
        __syncthreads();
        if (tile_open) {  // the window maximum, separably (a maximum does not depend on the order): along x, then y, then the bins
          for (int i = tid; i < TD * TY * kPtX; i += 256) {
            const int row = i / kPtX, cx = i - row * kPtX;
            const float* c0 = buf + row * TX + cx + R;
            float v = c0[0];
#pragma unroll
            for (int dx = 1; dx <= R; ++dx) v = fmaxf(v, fmaxf(c0[-dx], c0[dx]));
            s_x[i] = v;
          }
          __syncthreads();
          for (int i = tid; i < TD * kPtY * kPtX; i += 256) {
            const int dz = i / (kPtY * kPtX), rem = i - dz * (kPtY * kPtX), ry = rem / kPtX, cx = rem - ry * kPtX;
            const float* c0 = s_x + ((dz * TY) + ry + R) * kPtX + cx;
            float v = c0[0];
#pragma unroll
            for (int dy = 1; dy <= R; ++dy) v = fmaxf(v, fmaxf(c0[-dy * kPtX], c0[dy * kPtX]));
            s_y[i] = v;
          }
          __syncthreads();
        }
        const float cv = cf[(size_t)ch * hw + pix];
#pragma unroll
        for (int j = 0; j < kCvG; ++j) {
          float v = 0.f;
          if (state[j] == 0) {
            v = buf[((j + R) * TY + ly + R) * TX + lx + R];
          } else if (state[j] == 1) {  // the masked centre's own 0 is in the window
            const float* c0 = s_y + ((j + R) * kPtY + ly) * kPtX + lx;
            v = c0[0];
#pragma unroll
            for (int dd = 1; dd <= R; ++dd) v = fmaxf(v, fmaxf(c0[-dd * kPtY * kPtX], c0[dd * kPtY * kPtX]));
          }
          sum[j] += fabsf(v - cv);
        }
      }
    }
    fuse_frame<CVMIN>(sum, edge, acc, cnt);
  }
  store_bins<CVMIN>(p, b, pix, d0, live, acc, cnt);
}

}  // namespace mal

using namespace mal;

namespace mal { opt_t g_costvol_impl{1}; }  // 1 = planar features, lane = pixel (default); 0 = channel-last, lane = channel

extern "C" int mal_costvol_channel_last(void) { return g_costvol_impl == 0; }

// what both entry points refuse as a shape, and the record both fill
static int costvol_shape_status(int B, int F, int C, int D, int h, int w) {
  if (B <= 0 || F <= 0 || D <= 0 || h < 5 || w < 5) return MAL_ESHAPE;
  if (C != kCvC || D > 256) return MAL_ESHAPE;  // lanes = channels; four bins per lane at most
  if ((double)B * D * h * w > 2.0e9 / 4 || (double)B * F * h * w * C > 2.0e9 / 4) return MAL_ESHAPE;
  return MAL_OK;
}

static CostVolParams costvol_params(const float* current_feats, const float* lookup_feats, const float* poses, const float* K,
                                    const float* inv_K, const float* depth_bins, int B, int F, int D, int h, int w, float eps,
                                    int set_missing_to_max, float* cost_volume, float* missing_mask, float* masked_cost_volume,
                                    float* lowest_cost, float* confidence_mask) {
  CostVolParams p = {};
  p.cur = current_feats; p.look = lookup_feats; p.poses = poses; p.K = K; p.invK = inv_K; p.bins = depth_bins;
  p.B = B; p.F = F; p.D = D; p.h = h; p.w = w; p.eps = eps; p.set_missing_to_max = set_missing_to_max;
  p.cost = cost_volume; p.missing = missing_mask; p.masked = masked_cost_volume; p.lowest_cost = lowest_cost;
  p.confidence = confidence_mask;
  return p;
}

extern "C" int mal_cost_volume(const float* current_feats, const float* lookup_feats, const float* poses, const float* K,
                               const float* inv_K, const float* depth_bins, int B, int F, int C, int D, int h, int w,
                               float eps, int set_missing_to_max, float* cost_volume, float* missing_mask,
                               float* masked_cost_volume, float* lowest_cost, float* confidence_mask, void* stream) {
  const int st0 = costvol_shape_status(B, F, C, D, h, w);
  if (st0 != MAL_OK) return st0;
  if (!current_feats || !lookup_feats || !poses || !K || !inv_K || !depth_bins || !cost_volume) return MAL_EINVAL;
  const CostVolParams p = costvol_params(current_feats, lookup_feats, poses, K, inv_K, depth_bins, B, F, D, h, w, eps,
                                         set_missing_to_max, cost_volume, missing_mask, masked_cost_volume, lowest_cost,
                                         confidence_mask);
  hipStream_t st = (hipStream_t)stream;
  if (g_costvol_impl == 0)
    hipLaunchKernelGGL(costvol_match_kernel, dim3((w + 3) / 4, h, B), dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL(costvol_match_px_kernel, dim3((h * w + 255) / 256, (D + kCvG - 1) / kCvG, B), dim3(256), 0, st, p);
  hipLaunchKernelGGL(costvol_finish_kernel, dim3((B * h * w + 63) / 64), dim3(256), 0, st, p);
  return launch_status();
}

// ---- DynamicDepth's variant: occ images (B*F*48*128 bytes, 256-aligned) then one byte per (b,f,d,y,x)
static size_t dyn_occ_bytes(int B, int F) { return (((size_t)B * F * kOccH * kOccW) + 255) / 256 * 256; }

static int dyn_shape_status(int B, int F, int C, int D, int h, int w) {
  const int st = costvol_shape_status(B, F, C, D, h, w);
  if (st != MAL_OK) return st;
  if (B > 65535 || (long long)B * F > 65535) return MAL_ESHAPE;  // grid dimensions z (B) and of the occlusion launches (B*F)
  return MAL_OK;
}

extern "C" size_t mal_cost_volume_dyn_workspace_bytes(int B, int F, int D, int h, int w) {
  if (dyn_shape_status(B, F, kCvC, D, h, w) != MAL_OK) return 0;
  return dyn_occ_bytes(B, F) + (size_t)B * F * D * h * w;
}

extern "C" int mal_cost_volume_dyn(const float* current_feats, const float* lookup_feats, const float* poses, const float* K,
                                   const float* inv_K, const float* depth_bins, int B, int F, int C, int D, int h, int w,
                                   float eps, int set_missing_to_max, const float* lookup_images, int H, int W,
                                   const float* aug_mask, int cv_min, int set_1, int pool, int pool_r, float pool_th,
                                   float* cost_volume, float* missing_mask, float* masked_cost_volume, float* lowest_cost,
                                   float* confidence_mask, void* ws, size_t ws_bytes, void* stream) {
  const int st0 = dyn_shape_status(B, F, C, D, h, w);
  if (st0 != MAL_OK) return st0;
  if (pool_r < 0 || pool_r > 2) return MAL_EINVAL;  // --cv_pool_radius: a wider window leaves the image around inner pixels
  if (!current_feats || !lookup_feats || !poses || !K || !inv_K || !depth_bins || !cost_volume) return MAL_EINVAL;
  const bool occ = set_1 || pool;
  if (occ) {
    if (!lookup_images || !ws) return MAL_EINVAL;
    if (H <= 0 || W <= 0 || (double)B * F * 3 * H * W > 2.0e9) return MAL_ESHAPE;
    if (ws_bytes < mal_cost_volume_dyn_workspace_bytes(B, F, D, h, w)) return MAL_EINVAL;
  }
  CostVolDynParams q = {};
  CostVolParams& p = q.cv;
  p = costvol_params(current_feats, lookup_feats, poses, K, inv_K, depth_bins, B, F, D, h, w, eps, set_missing_to_max,
                     cost_volume, missing_mask, masked_cost_volume, lowest_cost, confidence_mask);
  q.images = lookup_images; q.aug = aug_mask; q.H = H; q.W = W;
  q.pool_th = pool_th;
  q.occ = (unsigned char*)ws; q.m = occ ? (unsigned char*)ws + dyn_occ_bytes(B, F) : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((h * w + 255) / 256, (D + kCvG - 1) / kCvG, B);
  if (occ) {
    hipLaunchKernelGGL(costvol_occ_image_kernel, dim3((kOccH * kOccW + 255) / 256, B * F), dim3(256), 0, st, q);
    hipLaunchKernelGGL(costvol_occ_mask_kernel, dim3((h * w + 255) / 256, D, B * F), dim3(256), 0, st, q);
    if (pool && !set_1) {
      const dim3 tg(((w + kPtX - 1) / kPtX) * ((h + kPtY - 1) / kPtY), (D + kCvG - 1) / kCvG, B);
#define MAL_POOL_LAUNCH(R) \
      if (cv_min) hipLaunchKernelGGL((costvol_match_pool_kernel<R, true>), tg, dim3(256), 0, st, q); \
      else hipLaunchKernelGGL((costvol_match_pool_kernel<R, false>), tg, dim3(256), 0, st, q)
      if (pool_r == 0) { MAL_POOL_LAUNCH(0); } else if (pool_r == 1) { MAL_POOL_LAUNCH(1); } else { MAL_POOL_LAUNCH(2); }
#undef MAL_POOL_LAUNCH
    } else if (cv_min) hipLaunchKernelGGL((costvol_match_dyn_kernel<true, true>), grid, dim3(256), 0, st, q);
    else hipLaunchKernelGGL((costvol_match_dyn_kernel<true, false>), grid, dim3(256), 0, st, q);
  } else {
    if (cv_min) hipLaunchKernelGGL((costvol_match_dyn_kernel<false, true>), grid, dim3(256), 0, st, q);
    else hipLaunchKernelGGL((costvol_match_dyn_kernel<false, false>), grid, dim3(256), 0, st, q);
  }
  hipLaunchKernelGGL(costvol_finish_kernel, dim3((B * h * w + 63) / 64), dim3(256), 0, st, p);
  return launch_status();
}
