// DynamicDepth's occlusion-aware forward warp (dynamicdepth/rigid_warp.py:534-597, called at trainer.py:502,517,525 and
// :825,840), forward only (upstream runs it under torch.no_grad(), trainer.py:494), and its second stage alone, the inverse
// warp of rigid_warp.py:337-373.  Upstream needs torch_sparse's CUDA coalesce for the z-buffer; here it is an integer
// atomicMax.
//
//   stage 1, splat    every source pixel is cut into up x up sub-points that share its depth (nearest upsampling is integer
//                     division of the sub-point's coordinates by up); each is back-projected with inverse(K_u), K_u = K with
//                     its first two rows times up, moved by pose (3x4), divided by max(Z, 1e-3) and projected with the
//                     UNSCALED K; its coordinates are TRUNCATED to a cell, and the cell keeps the largest 1/Z it receives.
//   stage 2, resolve  depth_w = 1 / zbuf (0 in holes); the source image is inverse-warped with depth_w and the inverted pose
//                     after upstream's mat2euler -> euler2mat round trip; outputs img_w * valid, depth_w * valid, valid.
//
// One mal_forward_warp enqueues four things on the caller's stream: a clear of the z-buffer, fwarp_prep_kernel,
// fwarp_splat_kernel, fwarp_resolve_kernel.  No allocation, no synchronisation, no readback; capturable.
//
// Arithmetic.  The per-sample matrices are formed once in fp64 by fwarp_prep_kernel and rounded to fp32 once (upstream:
// torch.inverse, atan2, sin and cos in fp32).  The per-sub-point and per-pixel chains are fp32 in upstream's order, a 3-term
// dot product summed left to right as ATen's bmm row does, true divisions, no fma (the library is built -ffp-contract=off).
// Every range test is made in float before any conversion to an index:  inside iff x > -1 && x < W && y > -1 && y < H, which
// is what .long() followed by upstream's `< 0` / `> hh-1` tests comes to for finite values (coordinates in (-1, 0) truncate
// to cell 0); NaN and +-inf fail it, contribute nothing and never form an index.
//
// Z-buffer.  A (P,B,H,W) plane of the BIT PATTERNS of 1/Z.  Z >= 1e-3, so 0 < 1/Z <= 1000 and unsigned integer order is float
// order; the update is a 32-bit integer atomicMax, so the plane does not depend on arrival order and is bitwise reproducible.
// 0 is "empty" (upstream too reads a dense 0 as a hole).
//
// Decomposition.  Splat: one thread owns one source pixel and its up^2 sub-points; sub-points that fall into the same cell
// are combined in registers (row runs, then column runs: neighbours in the sub-point grid are the ones that share a cell)
// and the survivors go straight to global memory with one atomicMax each.  Resolve: one thread per target pixel.  Both use
// 64x4-pixel tiles of 256 threads (a wave reads a 256-byte row piece of depth / zbuf); grid = (tiles, B, poses), so the two
// warps of a training step that share image and depth are one call.
#include "mal_common.h"

namespace mal {

constexpr int kFwTW = 64;    // tile width  (one wave = one 64-pixel row piece)
constexpr int kFwTH = 4;     // tile height (4 waves)
constexpr int kFwMats = 32;  // fp32 values prep leaves per (pose, sample): inv(K_u) 9, inv(K) 9, (K pose_inv)[:, :3] 9, [:, 3] 3

struct FwarpParams {
  const float* img;      // (B,C,H,W)
  const float* depth;    // (B,H,W)
  const float* K;        // (B,9)
  const float* pose[MAL_FWARP_MAX_POSES];        // forward: (B,12) each; inverse warp: pose[0] = (B,6)
  float* mats;           // workspace (P,B,kFwMats)
  unsigned* zbuf;        // workspace (P,B,H,W)
  float* img_w;          // (P,B,C,H,W)
  float* depth_w;        // (P,B,H,W)
  float* valid;          // (P,B,H,W)
  unsigned char* valid_u8;  // inverse warp: (B,H,W)
  unsigned* zbuf_out;    // nullable (P,B,H,W)
  float* dst[MAL_FWARP_MAX_POSES];               // nullable (B,C,H,W) each
  const unsigned char* mask[MAL_FWARP_MAX_POSES];  // nullable (B,H,W) each
  const unsigned char* select;                   // nullable (B)
  int B, C, H, W, up, P, tiles_x, no_reproj;
};

// inverse of a row-major 3x3 by cofactors: valid for any invertible matrix
__device__ inline void inv3(const double* m, double* o) {
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double id = 1.0 / (m[0] * c00 + m[1] * c01 + m[2] * c02);
  o[0] = c00 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  o[3] = c01 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  o[6] = c02 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

__device__ inline void mul3(const double* a, const double* b, double* o) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o[r * 3 + c] = a[r * 3] * b[c] + a[r * 3 + 1] * b[3 + c] + a[r * 3 + 2] * b[6 + c];
}

// upstream's euler2mat (rigid_warp.py:204-239): xmat @ ymat @ zmat
__device__ inline void euler_to_mat(double ex, double ey, double ez, double* R) {
  const double cx = cos(ex), sx = sin(ex), cy = cos(ey), sy = sin(ey), cz = cos(ez), sz = sin(ez);
  const double xm[9] = {1, 0, 0, 0, cx, -sx, 0, sx, cx};
  const double ym[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy};
  const double zm[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1};
  double xy[9];
  mul3(xm, ym, xy);
  mul3(xy, zm, R);
}

// One thread per (pose, sample).  FWD: pose is a 3x4 [R | t]; its inverse [R^-1 | -R^-1 t] goes through upstream's
// mat2euler (rigid_warp.py:175-200, the sy < 1e-6 branch included) and back through euler2mat, as forward_warp hands
// inverse_warp a 6-vector (:585-591).  Otherwise pose is that 6-vector (tx, ty, tz, rx, ry, rz) itself.
template <bool FWD>
__global__ void fwarp_prep_kernel(FwarpParams p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.P * p.B) return;
  const int q = i / p.B, b = i - q * p.B;
  double K[9], Ku[9], Kiu[9], Ki[9], R[9], t[3];
  for (int k = 0; k < 9; ++k) {
    const float kv = p.K[b * 9 + k];
    K[k] = (double)kv;
    Ku[k] = k < 6 ? (double)(kv * (float)p.up) : (double)kv;  // upstream scales the fp32 matrix before inverting it
  }
  inv3(Ku, Kiu);
  inv3(K, Ki);
  if (FWD) {
    const float* T = p.pose[q] + (size_t)b * 12;
    double Rf[9], Ri[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) Rf[r * 3 + c] = (double)T[r * 4 + c];
    inv3(Rf, Ri);
    for (int r = 0; r < 3; ++r)
      t[r] = -(Ri[r * 3] * (double)T[3] + Ri[r * 3 + 1] * (double)T[7] + Ri[r * 3 + 2] * (double)T[11]);
    const double sy = sqrt(Ri[0] * Ri[0] + Ri[3] * Ri[3]);
    const double s = sy < 1e-6 ? 1.0 : 0.0;
    const double ex = atan2(Ri[7], Ri[8]) * (1.0 - s) + atan2(-Ri[5], Ri[4]) * s;
    const double ey = atan2(-Ri[6], sy) * (1.0 - s) + atan2(-Ri[6], sy) * s;
    const double ez = atan2(Ri[3], Ri[0]) * (1.0 - s) + (Ri[3] * 0.0) * s;
    euler_to_mat(ex, ey, ez, R);
  } else {
    const float* v = p.pose[0] + (size_t)b * 6;
    t[0] = (double)v[0]; t[1] = (double)v[1]; t[2] = (double)v[2];
    euler_to_mat((double)v[3], (double)v[4], (double)v[5], R);
  }
  float* m = p.mats + (size_t)i * kFwMats;
  double A[9];
  mul3(K, R, A);
  for (int k = 0; k < 9; ++k) {
    m[k] = (float)Kiu[k];
    m[9 + k] = (float)Ki[k];
    m[18 + k] = (float)A[k];
  }
  for (int r = 0; r < 3; ++r) m[27 + r] = (float)(K[r * 3] * t[0] + K[r * 3 + 1] * t[1] + K[r * 3 + 2] * t[2]);
  m[30] = 0.f;
  m[31] = 0.f;
}

template <int UP>
__global__ __launch_bounds__(256) void fwarp_splat_kernel(FwarpParams p) {
  const int b = blockIdx.y, q = blockIdx.z;
  const int ty = blockIdx.x / p.tiles_x, tx = blockIdx.x - ty * p.tiles_x;
  const int x = tx * kFwTW + (threadIdx.x & (kFwTW - 1)), y = ty * kFwTH + (threadIdx.x / kFwTW);
  if (x >= p.W || y >= p.H) return;
  const int W = p.W, H = p.H;
  const float* ku = p.mats + (size_t)(q * p.B + b) * kFwMats;  // inverse(K_u)
  const float* K = p.K + (size_t)b * 9;
  const float* T = p.pose[q] + (size_t)b * 12;
  const float d = p.depth[((size_t)b * H + y) * W + x];
  const float fW = (float)W, fH = (float)H;
  int cell[UP * UP];
  unsigned val[UP * UP];
#pragma unroll
  for (int sv = 0; sv < UP; ++sv) {
#pragma unroll
    for (int su = 0; su < UP; ++su) {
      const float u = (float)(x * UP + su), v = (float)(y * UP + sv);
      const float c0 = (ku[0] * u + ku[1] * v + ku[2]) * d;
      const float c1 = (ku[3] * u + ku[4] * v + ku[5]) * d;
      const float c2 = (ku[6] * u + ku[7] * v + ku[8]) * d;
      const float X = (T[0] * c0 + T[1] * c1 + T[2] * c2) + T[3];
      const float Y = (T[4] * c0 + T[5] * c1 + T[6] * c2) + T[7];
      float Z = (T[8] * c0 + T[9] * c1 + T[10] * c2) + T[11];
      Z = Z < 1e-3f ? 1e-3f : Z;  // a NaN stays a NaN, as torch.clamp leaves it
      const float xn = X / Z, yn = Y / Z, zn = Z / Z;
      const float px = K[0] * xn + K[1] * yn + K[2] * zn;
      const float py = K[3] * xn + K[4] * yn + K[5] * zn;
      const bool inside = px > -1.f && px < fW && py > -1.f && py < fH;  // in float, before any conversion
      const int k = sv * UP + su;
      cell[k] = inside ? (int)py * W + (int)px : -1;  // truncation: (-1, 0) is cell 0
      val[k] = __float_as_uint(1.f / Z);
    }
  }
  // combine sub-points of one cell before anything is issued: runs along rows, then along columns
#pragma unroll
  for (int sv = 0; sv < UP; ++sv)
#pragma unroll
    for (int su = 1; su < UP; ++su) {
      const int k = sv * UP + su;
      if (cell[k] >= 0 && cell[k] == cell[k - 1]) {
        val[k] = val[k] > val[k - 1] ? val[k] : val[k - 1];
        cell[k - 1] = -1;
      }
    }
#pragma unroll
  for (int sv = 1; sv < UP; ++sv)
#pragma unroll
    for (int su = 0; su < UP; ++su) {
      const int k = sv * UP + su;
      if (cell[k] >= 0 && cell[k] == cell[k - UP]) {
        val[k] = val[k] > val[k - UP] ? val[k] : val[k - UP];
        cell[k - UP] = -1;
      }
    }
  unsigned* zb = p.zbuf + (size_t)(q * p.B + b) * H * W;
#pragma unroll
  for (int k = 0; k < UP * UP; ++k)
    if (cell[k] >= 0) atomicMax(zb + cell[k], val[k]);  // cell in [0, H*W) by the float range test above
}

// bilinear sample of one (H,W) plane at (ix, iy), zero padding, ATen's corner order and weights; the caller has shown
// ix in (-1, W) and iy in (-1, H)
__device__ inline float fw_bilinear(const float* pl, int H, int W, float ix, float iy) {
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
  const float fx1 = fx0 + 1.f, fy1 = fy0 + 1.f;
  const float nw = (fx1 - ix) * (fy1 - iy), ne = (ix - fx0) * (fy1 - iy), sw = (fx1 - ix) * (iy - fy0), se = (ix - fx0) * (iy - fy0);
  const bool xa = x0 >= 0, xb = x1 <= W - 1, ya = y0 >= 0, yb = y1 <= H - 1;
  float acc = 0.f;
  if (xa && ya) acc += pl[(size_t)y0 * W + x0] * nw;
  if (xb && ya) acc += pl[(size_t)y0 * W + x1] * ne;
  if (xa && yb) acc += pl[(size_t)y1 * W + x0] * sw;
  if (xb && yb) acc += pl[(size_t)y1 * W + x1] * se;
  return acc;
}

// FWD: depth from the z-buffer, masked outputs, optional composition.  Otherwise (mal_inverse_warp) the caller's depth, the
// unmasked image and a byte validity plane, as rigid_warp.py:337-373 returns them.
template <bool FWD>
__global__ __launch_bounds__(256) void fwarp_resolve_kernel(FwarpParams p) {
  const int b = blockIdx.y, q = blockIdx.z;
  const int ty = blockIdx.x / p.tiles_x, tx = blockIdx.x - ty * p.tiles_x;
  const int x = tx * kFwTW + (threadIdx.x & (kFwTW - 1)), y = ty * kFwTH + (threadIdx.x / kFwTW);
  if (x >= p.W || y >= p.H) return;
  const int W = p.W, H = p.H, C = p.C;
  const size_t hw = (size_t)H * W, pix = (size_t)y * W + x;
  const size_t plane = (size_t)(q * p.B + b);
  const float* m = p.mats + plane * kFwMats;
  const float* ki = m + 9;
  const float* A = m + 18;
  const float* tr = m + 27;
  bool fw = true;
  float dw;
  if (FWD) {
    const unsigned bits = p.zbuf[plane * hw + pix];
    if (p.zbuf_out) p.zbuf_out[plane * hw + pix] = bits;
    fw = bits != 0u;
    dw = fw ? 1.f / __uint_as_float(bits) : 0.f;
  } else {
    dw = p.depth[(size_t)b * hw + pix];
  }
  const float fx = (float)x, fy = (float)y;
  const float c0 = (ki[0] * fx + ki[1] * fy + ki[2]) * dw;
  const float c1 = (ki[3] * fx + ki[4] * fy + ki[5]) * dw;
  const float c2 = (ki[6] * fx + ki[7] * fy + ki[8]) * dw;
  const float X = (A[0] * c0 + A[1] * c1 + A[2] * c2) + tr[0];
  const float Y = (A[3] * c0 + A[4] * c1 + A[5] * c2) + tr[1];
  float Z = (A[6] * c0 + A[7] * c1 + A[8] * c2) + tr[2];
  Z = Z < 1e-3f ? 1e-3f : Z;
  const float gx = 2.f * (X / Z) / (float)(W - 1) - 1.f;
  const float gy = 2.f * (Y / Z) / (float)(H - 1) - 1.f;
  const bool iw = fabsf(gx) <= 1.f && fabsf(gy) <= 1.f;  // max|coord| <= 1; false for NaN
  const float ix = ((gx + 1.f) / 2.f) * (float)(W - 1), iy = ((gy + 1.f) / 2.f) * (float)(H - 1);  // align_corners=True
  const bool hit = ix > -1.f && ix < (float)W && iy > -1.f && iy < (float)H;  // else every corner is padding
  const float vf = (fw && iw) ? 1.f : 0.f;
  if (FWD) {
    p.depth_w[plane * hw + pix] = dw * vf;
    p.valid[plane * hw + pix] = vf;
  } else {
    p.valid_u8[(size_t)b * hw + pix] = iw ? 1 : 0;
  }
  float* dst = FWD ? p.dst[q] : nullptr;
  const bool compose = dst != nullptr && (p.select == nullptr || p.select[b] != 0);
  const bool cut = compose && p.mask[q] != nullptr && p.mask[q][(size_t)b * hw + pix] == 1;
  for (int c = 0; c < C; ++c) {
    const float s = hit ? fw_bilinear(p.img + ((size_t)b * C + c) * hw, H, W, ix, iy) : 0.f;
    const float w = FWD ? s * vf : s;
    p.img_w[(plane * C + c) * hw + pix] = w;
    if (compose) {  // trainer.py:506-510: the mask zeroes all channels, then each element takes img_w where img_w > 0
      float* e = dst + ((size_t)b * C + c) * hw + pix;
      if (w > 0.f) *e = p.no_reproj ? 0.f : w;
      else if (cut) *e = 0.f;
    }
  }
}

}  // namespace mal

using namespace mal;

struct FwarpPlan { int tiles_x, tiles_y; };

// shape checks and launch geometry of both entry points, pure host code
static int fwarp_plan(int B, int C, int H, int W, int up, int P, FwarpPlan* pl) {
  if (B < 1 || H < 1 || W < 1) return MAL_ESHAPE;
  if (H < 2 || W < 2) return MAL_ESHAPE;  // upstream divides by W - 1 and H - 1
  if (up < 1 || up > MAL_FWARP_MAX_UPSCALE || C < 1 || C > MAL_FWARP_MAX_C || P < 1 || P > MAL_FWARP_MAX_POSES) return MAL_ESHAPE;
  if (B > 65535) return MAL_ESHAPE;  // grid y
  const double lim = 2147483647.0;
  if ((double)P * B * C * H * W > lim || (double)P * B * H * W > lim) return MAL_ESHAPE;  // every tensor below 2^31 elements
  if ((double)H * up > 16777216.0 || (double)W * up > 16777216.0) return MAL_ESHAPE;      // sub-point coordinates exact in fp32
  pl->tiles_x = (W + kFwTW - 1) / kFwTW;
  pl->tiles_y = (H + kFwTH - 1) / kFwTH;
  return MAL_OK;
}

extern "C" int mal_forward_warp_plan(int B, int C, int H, int W, int upscale, int n_pose, int* vec, int* tile_w, int* tile_h,
                                     int* tiles_x, int* tiles_y, int* blocks, size_t* lds_bytes) {
  FwarpPlan pl;
  const int rc = fwarp_plan(B, C, H, W, upscale, n_pose, &pl);
  if (rc != MAL_OK) return rc;
  if (vec) *vec = 1;
  if (tile_w) *tile_w = kFwTW;
  if (tile_h) *tile_h = kFwTH;
  if (tiles_x) *tiles_x = pl.tiles_x;
  if (tiles_y) *tiles_y = pl.tiles_y;
  if (blocks) *blocks = pl.tiles_x * pl.tiles_y * B * n_pose;
  if (lds_bytes) *lds_bytes = 0;
  return MAL_OK;
}

static size_t fwarp_mats_bytes(int B, int P) { return align256((size_t)P * B * kFwMats * sizeof(float)); }

extern "C" size_t mal_forward_warp_workspace_bytes(int B, int H, int W, int n_pose) {
  FwarpPlan pl;
  if (fwarp_plan(B, 1, H, W, 1, n_pose, &pl) != MAL_OK) return 0;
  return fwarp_mats_bytes(B, n_pose) + align256((size_t)n_pose * B * H * W * sizeof(unsigned));
}

extern "C" int mal_forward_warp(const mal_fwarp_args* a) {
  if (!a) return MAL_EINVAL;
  if (!a->img || !a->depth || !a->K || !a->img_w || !a->depth_w || !a->valid || !a->ws) return MAL_EINVAL;
  if (a->n_pose >= 1 && a->n_pose <= MAL_FWARP_MAX_POSES)
    for (int q = 0; q < a->n_pose; ++q)
      if (!a->pose[q]) return MAL_EINVAL;
  FwarpPlan pl;
  const int rc = fwarp_plan(a->B, a->C, a->H, a->W, a->upscale, a->n_pose, &pl);
  if (rc != MAL_OK) return rc;
  if (a->ws_bytes < mal_forward_warp_workspace_bytes(a->B, a->H, a->W, a->n_pose)) return MAL_EWORKSPACE;
  FwarpParams p = {};
  p.img = a->img; p.depth = a->depth; p.K = a->K;
  for (int q = 0; q < a->n_pose; ++q) {
    p.pose[q] = a->pose[q];
    p.dst[q] = a->dst[q];
    p.mask[q] = a->mask[q];
  }
  p.mats = (float*)a->ws;
  p.zbuf = (unsigned*)((char*)a->ws + fwarp_mats_bytes(a->B, a->n_pose));
  p.img_w = a->img_w; p.depth_w = a->depth_w; p.valid = a->valid; p.zbuf_out = (unsigned*)a->zbuf;
  p.select = a->select;
  p.B = a->B; p.C = a->C; p.H = a->H; p.W = a->W; p.up = a->upscale; p.P = a->n_pose; p.tiles_x = pl.tiles_x;
  p.no_reproj = (a->flags & MAL_FWARP_NO_REPROJ) ? 1 : 0;
  hipStream_t st = (hipStream_t)a->stream;
  const size_t cells = (size_t)a->n_pose * a->B * a->H * a->W;
  if (hipMemsetAsync(p.zbuf, 0, cells * sizeof(unsigned), st) != hipSuccess) return MAL_ELAUNCH;
  const int pb = a->n_pose * a->B;
  hipLaunchKernelGGL((fwarp_prep_kernel<true>), dim3((pb + 63) / 64), dim3(64), 0, st, p);
  const dim3 grid((unsigned)(pl.tiles_x * pl.tiles_y), (unsigned)a->B, (unsigned)a->n_pose), block(kFwTW * kFwTH);
  switch (a->upscale) {
    case 1: hipLaunchKernelGGL((fwarp_splat_kernel<1>), grid, block, 0, st, p); break;
    case 2: hipLaunchKernelGGL((fwarp_splat_kernel<2>), grid, block, 0, st, p); break;
    case 3: hipLaunchKernelGGL((fwarp_splat_kernel<3>), grid, block, 0, st, p); break;
    default: hipLaunchKernelGGL((fwarp_splat_kernel<4>), grid, block, 0, st, p); break;
  }
  hipLaunchKernelGGL((fwarp_resolve_kernel<true>), grid, block, 0, st, p);
  return launch_status();
}

extern "C" int mal_inverse_warp(const float* img, const float* depth, const float* pose, const float* K, int B, int C, int H,
                                int W, float* out, unsigned char* valid, void* ws, size_t ws_bytes, void* stream) {
  if (!img || !depth || !pose || !K || !out || !valid || !ws) return MAL_EINVAL;
  FwarpPlan pl;
  const int rc = fwarp_plan(B, C, H, W, 1, 1, &pl);
  if (rc != MAL_OK) return rc;
  if (ws_bytes < fwarp_mats_bytes(B, 1)) return MAL_EWORKSPACE;
  FwarpParams p = {};
  p.img = img; p.depth = depth; p.K = K; p.pose[0] = pose;
  p.mats = (float*)ws;
  p.img_w = out; p.valid_u8 = valid;
  p.B = B; p.C = C; p.H = H; p.W = W; p.up = 1; p.P = 1; p.tiles_x = pl.tiles_x;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((fwarp_prep_kernel<false>), dim3((B + 63) / 64), dim3(64), 0, st, p);
  const dim3 grid((unsigned)(pl.tiles_x * pl.tiles_y), (unsigned)B, 1u), block(kFwTW * kFwTH);
  hipLaunchKernelGGL((fwarp_resolve_kernel<false>), grid, block, 0, st, p);
  return launch_status();
}
