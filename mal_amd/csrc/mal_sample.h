// Zero-padded bilinear sampling as the lookup kernels use it, defined once: the cost volume and DynamicDepth's variant
// (mal_costvol.hip), DualRefine's epipolar lookup, its VJPs and the pose-refinement step (mal_epipolar.hip).  Each caller
// keeps what is its own: how a sampling position (ix, iy) comes about (grid_position and the align_corners=True
// unnormalise there, the align_corners=False level position here), whether it keeps element or byte offsets, and what it
// does with the taps.  This header holds what they share: the four corners, the zeroed weights and one plane sample.
//
// Not served from here, on purpose: fw_bilinear (mal_fwarp.hip: its caller guarantees the range, conditional plain adds),
// the deformable-attention sampler (mal_msda.hip: the CUDA kernel's convention) and make_taps (mal_device.h: border clamp).
#pragma once
#include "mal_device.h"

namespace mal {

// Corner order everywhere: 0 = (y0, x0), 1 = (y0, x1), 2 = (y1, x0), 3 = (y1, x1).
struct Corners {
  float x0f, y0f;  // floor of the position, as floats: the fractions below are taken against these
  bool wild;       // the position is far outside the map, or NaN: every tap is padding
  int o[4];        // element offsets y * w + x of the corners, each clamped into the map (always loadable)
  bool v[4];       // the corner lies inside the map and the position is not wild
};

MAL_DEV Corners corners_of(float ix, float iy, int w, int h) {
  Corners c;
  c.x0f = floorf(ix); c.y0f = floorf(iy);
  // keep the int conversion defined for wild positions: [-2, size + 1] holds every floor with a tap inside the map
  const float xc = fminf(fmaxf(c.x0f, -2.0f), (float)w + 1.0f), yc = fminf(fmaxf(c.y0f, -2.0f), (float)h + 1.0f);
  const int x0 = (int)xc, y0 = (int)yc, x1 = x0 + 1, y1 = y0 + 1;
  c.wild = !(c.x0f == xc && c.y0f == yc);  // also true for NaN
  const bool vx0 = x0 >= 0 && x0 < w, vx1 = x1 >= 0 && x1 < w, vy0 = y0 >= 0 && y0 < h, vy1 = y1 >= 0 && y1 < h;
  const int cx0 = min(max(x0, 0), w - 1), cx1 = min(max(x1, 0), w - 1), cy0 = min(max(y0, 0), h - 1), cy1 = min(max(y1, 0), h - 1);
  c.o[0] = cy0 * w + cx0; c.o[1] = cy0 * w + cx1; c.o[2] = cy1 * w + cx0; c.o[3] = cy1 * w + cx1;
  c.v[0] = !c.wild && vx0 && vy0; c.v[1] = !c.wild && vx1 && vy0; c.v[2] = !c.wild && vx0 && vy1; c.v[3] = !c.wild && vx1 && vy1;
  return c;
}

// The fractions: tx, ty towards corner x1 / y1, ex, ey towards x0 / y0.  TWO conventions, not to be merged: for
// x0f >= 1 they differ in the last bit of ex, and each is what its reference executes.
struct Frac { float tx, ty, ex, ey; };
// the cost volume and its occlusion mask: ex = 1 - (ix - x0f)
MAL_DEV Frac frac_one_minus(float ix, float iy, const Corners& c) {
  Frac f;
  f.tx = ix - c.x0f; f.ex = 1.0f - f.tx; f.ty = iy - c.y0f; f.ey = 1.0f - f.ty;
  return f;
}
// the epipolar lookup, its VJPs and the pose-refinement step: ex = (x0f + 1) - ix
MAL_DEV Frac frac_next_minus(float ix, float iy, const Corners& c) {
  Frac f;
  f.tx = ix - c.x0f; f.ty = iy - c.y0f; f.ex = (c.x0f + 1.0f) - ix; f.ey = (c.y0f + 1.0f) - iy;
  return f;
}

// the bilinear weights, zero for a corner that is padding
MAL_DEV void tap_weights(const Corners& c, const Frac& f, float w[4]) {
  w[0] = c.v[0] ? f.ex * f.ey : 0.f;
  w[1] = c.v[1] ? f.tx * f.ey : 0.f;
  w[2] = c.v[2] ? f.ex * f.ty : 0.f;
  w[3] = c.v[3] ? f.tx * f.ty : 0.f;
}

// one sample from the four tap values: one multiply and three fmas, in this order, everywhere
MAL_DEV float blend4(float a, float b, float c, float d, const float w[4]) {
  float o = a * w[0];
  o = fma_(b, w[1], o);
  o = fma_(c, w[2], o);
  return fma_(d, w[3], o);
}
MAL_DEV float tap_load(const char* plane, unsigned byte_off) { return *reinterpret_cast<const float*>(plane + byte_off); }
// one sample of a feature plane through BYTE offsets (element offset * 4u, kept in registers across the channel loop)
MAL_DEV float plane_sample(const char* plane, const unsigned off[4], const float w[4]) {
  return blend4(tap_load(plane, off[0]), tap_load(plane, off[1]), tap_load(plane, off[2]), tap_load(plane, off[3]), w);
}

}  // namespace mal
