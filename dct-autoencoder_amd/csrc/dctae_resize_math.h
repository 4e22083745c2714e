// The arithmetic of the antialiased bilinear resize, the rule stated once
// (torch's interpolate(mode="bilinear", antialias=True, align_corners=False),
// the filter behind the reference's dataset crop, dataset.py:59-73): plain
// C++ for host and device, every operation an fp32 operation rounded on its
// own.  The `fp contract(off)` bodies keep that under any contraction setting
// of the caller, and the division is the correctly rounded one.  A host
// compiler builds this file alone (tests/test_resize_host.py does); the
// kernel of dctae_resize.hip calls the same functions.
//
// One axis n_in -> n_out, output index i:
//   scale = n_in / n_out, support = max(scale, 1), inv = 1 / scale (1 when scale < 1)
//   center = scale * (i + 0.5)
//   taps j in [lo, hi): lo = max(int(center - support + 0.5), 0),
//                       hi = min(int(center + support + 0.5), n_in)
//   raw(j) = max(0, 1 - |(j - center + 0.5) * inv|), sum = raw(lo) + ... in ascending j
//   weight(j) = raw(j) / sum
//   out[i] = weight(lo) * x[lo], then acc = acc + weight(j) * x[j] in ascending j
// The horizontal pass comes first, the vertical pass runs over its results.
#pragma once
#include "dctae_pixel.h"

namespace dctae {

// what every output index of one axis shares
struct ResizeAxis {
  float scale, support, inv;
};

// the taps of one output index: source indices [lo, hi) around center
struct ResizeWindow {
  int lo, hi;
  float center;
};

DCTAE_PX_HD inline ResizeAxis resize_axis(int n_in, int n_out) {
  ResizeAxis a;
  a.scale = (float)n_in / (float)n_out;
  const bool down = a.scale >= 1.0f;
  a.support = down ? a.scale : 1.0f;
  a.inv = down ? 1.0f / a.scale : 1.0f;
  return a;
}

DCTAE_PX_HD inline ResizeWindow resize_window(const ResizeAxis& a, int i, int n_in) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  ResizeWindow w;
  w.center = a.scale * ((float)i + 0.5f);
  const float fl = (w.center - a.support) + 0.5f;
  const float fh = (w.center + a.support) + 0.5f;
  const int lo = (int)fl, hi = (int)fh;   // truncation, as Python's int()
  w.lo = lo > 0 ? lo : 0;
  w.hi = hi < n_in ? hi : n_in;
  return w;
}

// the triangle filter at tap j, before normalisation
DCTAE_PX_HD inline float resize_raw_weight(const ResizeAxis& a, float center, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float x = (((float)j - center) + 0.5f) * a.inv;
  const float w = 1.0f - (x < 0.0f ? -x : x);
  return w > 0.0f ? w : 0.0f;
}

// the sum of the raw weights, in ascending j
DCTAE_PX_HD inline float resize_weight_sum(const ResizeAxis& a, const ResizeWindow& w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float s = 0.0f;
  for (int j = w.lo; j < w.hi; ++j) s = s + resize_raw_weight(a, w.center, j);
  return s;
}

DCTAE_PX_HD inline float resize_weight(const ResizeAxis& a, float center, float sum, int j) {
  return resize_raw_weight(a, center, j) / sum;
}

// one step of the filter's sum: the first tap starts it, every later one adds
// its rounded product to it
DCTAE_PX_HD inline float resize_tap(bool first, float acc, float w, float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float p = w * x;
  return first ? p : acc + p;
}

}  // namespace dctae
