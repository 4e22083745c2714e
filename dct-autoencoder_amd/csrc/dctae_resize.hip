// Antialiased bilinear resize of a ragged list of (3, H, W) images, fp32 or
// bytes, to fp32 images of any size, in one launch: the resize of the
// reference's dataset crop (dataset.py:59-73), include/dctae_resize.h.  The
// arithmetic is that of dctae_resize_math.h and nothing else; this unit only
// decides who computes which pixel.
//
// A block of four waves owns a 32 x 64 tile of one channel plane of one output
// image: lane l of every wave owns column l, wave g the rows 8g .. 8g + 7, each
// in a register accumulator.  The block streams the source rows that the
// tile's vertical windows cover in ascending order, 16 at a time: wave g
// stages rows 4g .. 4g + 3 of the group (the columns the tile's horizontal
// windows cover, converted to fp32 once) in LDS, starts the loads of the next
// group, and filters the staged rows to its 64 columns, the four rows sharing
// each tap's weight; the 16 x 64 results cross the waves through LDS, and
// every wave walks, for each of its rows, the group's source rows inside that
// row's window, adding weight * result to the row's accumulator.  The vertical
// sum so runs in ascending source row for any scale, and a horizontal window
// wider than the staging buffer is walked in pieces, the column sums carried
// across them in ascending order as well: no size of LDS bounds either scale.
// The vertical windows of a wave's rows are the same in all its lanes and are
// kept in scalar registers, so the loops over them branch on scalars.  No
// atomics, nothing shared between blocks, every output pixel stored once; a
// pixel's value depends on its own image alone.
//
// The block finds its image by bisecting the prefix sum of the images' tile
// counts (the one table of the plan: 48 bytes per image); channel and tile
// origin follow from the remainder.
#include "dctae_ctx.h"
#include "dctae_resize_math.h"
#include "../../include/dctae_resize.h"

using namespace dctae;

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 64;          // one column per lane
constexpr int kWaveRows = 8;        // output rows per wave
constexpr int kTileH = 4 * kWaveRows;
constexpr int kGroup = 16;          // source rows per round, four per wave
constexpr int kStageW = 320;        // staged source columns per piece (scale 4 and a window: 264)
constexpr int kStagePer = kStageW / 64;   // of them per lane
constexpr int kTaps = 16;           // windows up to this many taps keep their weights in LDS (scale 7)
constexpr int kMaxSide = 1 << 23;   // (float)i + 0.5f is exact below

struct ResizeImg {
  int64_t src, dst;    // element offsets of the image in the caller's buffers
  int32_t ih, iw, oh, ow;
  int32_t tiles_x, tiles_y;
  int32_t tile0;       // the image's first block; 3 * tiles_x * tiles_y follow
  int32_t pad;
};

template <typename Px>
__global__ __launch_bounds__(kThreads) void k_resize_aa(const ResizeImg* __restrict__ imgs, int n_img,
                                                        const Px* __restrict__ src_base,
                                                        float* __restrict__ dst_base) {
  __shared__ float s_px[kGroup][kStageW];
  __shared__ float s_t[kGroup][kTileW];
  __shared__ float s_wx[kTaps][kTileW];    // weight of tap t of column l
  __shared__ float s_wy[kTileH][kTaps];    // weight of tap t of row y
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x;
  int a = 0, z = n_img - 1;
  while (a < z) {
    const int m = (a + z + 1) >> 1;
    if (imgs[m].tile0 <= b)
      a = m;
    else
      z = m - 1;
  }
  const ResizeImg im = imgs[a];
  const int per = im.tiles_x * im.tiles_y;
  const int t = b - im.tile0;
  const int c = t / per, rem = t - c * per;
  const int ty = rem / im.tiles_x;
  const int oy0 = ty * kTileH, ox0 = (rem - ty * im.tiles_x) * kTileW;
  const Px* plane = src_base + im.src + (int64_t)c * im.ih * im.iw;
  float* out = dst_base + im.dst + (int64_t)c * im.oh * im.ow;
  const ResizeAxis ax = resize_axis(im.iw, im.ow), ay = resize_axis(im.ih, im.oh);

  // this lane's column, and the source columns [X0, X1) of the tile's columns
  const int ox = ox0 + lane;
  const bool col_ok = ox < im.ow;
  ResizeWindow wx{0, 0, 0.0f};
  if (col_ok) wx = resize_window(ax, ox, im.iw);
  const float sumx = resize_weight_sum(ax, wx);
  const int X0 = resize_window(ax, ox0, im.iw).lo;
  const int X1 = resize_window(ax, min(ox0 + kTileW, im.ow) - 1, im.iw).hi;

  // this wave's rows, and the source rows [R0, R1) of the tile's rows
  ResizeWindow wy[kWaveRows];
  float sumy[kWaveRows], acc[kWaveRows];
#pragma unroll
  for (int k = 0; k < kWaveRows; ++k) {
    const int oy = oy0 + wv * kWaveRows + k;
    wy[k] = ResizeWindow{0, 0, 0.0f};
    if (oy < im.oh) wy[k] = resize_window(ay, oy, im.ih);
    // the same in every lane: scalar loop bounds below
    wy[k].lo = __builtin_amdgcn_readfirstlane(wy[k].lo);
    wy[k].hi = __builtin_amdgcn_readfirstlane(wy[k].hi);
    wy[k].center = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(wy[k].center)));
    sumy[k] = 0.0f;
    acc[k] = 0.0f;
  }
  const int R0 = resize_window(ay, oy0, im.ih).lo;
  const int R1 = resize_window(ay, min(oy0 + kTileH, im.oh) - 1, im.ih).hi;

  // The weights of an axis whose windows all hold at most kTaps taps are
  // computed once into LDS (the same function calls, so the same bits);
  // wider windows compute each weight where it is used.  Thread i fills taps
  // i % 8, i % 8 + 8 of row i / 8; wave g taps g, g + 4, ... of its lanes' columns.
  const int trow = threadIdx.x >> 3;
  ResizeWindow wt{0, 0, 0.0f};
  if (oy0 + trow < im.oh) wt = resize_window(ay, oy0 + trow, im.ih);
  const bool tab_x = __syncthreads_and(wx.hi - wx.lo <= kTaps) != 0;
  const bool tab_y = __syncthreads_and(wt.hi - wt.lo <= kTaps) != 0;
  if (tab_x) {
    for (int k = wv; k < wx.hi - wx.lo; k += 4) s_wx[k][lane] = resize_weight(ax, wx.center, sumx, wx.lo + k);
  }
  if (tab_y) {
    const float st = resize_weight_sum(ay, wt);
    for (int k = threadIdx.x & 7; k < wt.hi - wt.lo; k += 8) s_wy[trow][k] = resize_weight(ay, wt.center, st, wt.lo + k);
  } else {
#pragma unroll
    for (int k = 0; k < kWaveRows; ++k) sumy[k] = resize_weight_sum(ay, wy[k]);
  }

  // the pixels of a piece (16 source rows x up to kStageW columns from c0) travel
  // through registers, kept as loaded: the next piece is in flight while this one is filtered
  float pf[4][kStagePer];
  auto fetch = [&](int rg, int c0) {
    // every load is unconditional, so all of them are in flight together: a row
    // past R1 or a column past the piece reads the last one instead, and its
    // value goes nowhere (such columns are not staged, such rows lie in no window)
    const int len = min(kStageW, X1 - c0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = min(rg + wv * 4 + q, R1 - 1);
      const Px* row = plane + (int64_t)r * im.iw + c0;
#pragma unroll
      for (int i = 0; i < kStagePer; ++i) pf[q][i] = load_px_raw(row + min(lane + 64 * i, len - 1));
    }
  };
  const int Rend = X1 > X0 ? R1 : R0;   // no columns, no rounds (every piece then holds a column)
  int rg = R0, c0 = X0;
  if (rg < Rend) fetch(rg, c0);
  float tacc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  while (rg < Rend) {
    const int len = min(kStageW, X1 - c0);
    const bool last = c0 + kStageW >= X1;   // the round's last piece
    const int rgn = last ? rg + kGroup : rg, c0n = last ? X0 : c0 + kStageW;
    __syncthreads();   // the previous piece and the previous round's s_t are read
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int i = 0; i < kStagePer; ++i) s_px[wv * 4 + q][lane + 64 * i] = px_value<Px>(pf[q][i]);   // past len: unread
    }
    if (rgn < Rend) fetch(rgn, c0n);
    __syncthreads();
    const int jb = max(wx.lo, c0), je = min(wx.hi, c0 + len);
    for (int j = jb; j < je; ++j) {
      const float w = tab_x ? s_wx[j - wx.lo][lane] : resize_weight(ax, wx.center, sumx, j);
      const bool first = j == wx.lo;
#pragma unroll
      for (int q = 0; q < 4; ++q) tacc[q] = resize_tap(first, tacc[q], w, s_px[wv * 4 + q][j - c0]);
    }
    if (last) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        s_t[wv * 4 + q][lane] = tacc[q];
        tacc[q] = 0.0f;
      }
      __syncthreads();
      // row by row of the wave's eight: the round's source rows inside its window, ascending
#pragma unroll
      for (int k = 0; k < kWaveRows; ++k) {
        const int ra = max(wy[k].lo, rg), rb = min(wy[k].hi, rg + kGroup);
        for (int r = ra; r < rb; ++r) {
          const float v = tab_y ? s_wy[wv * kWaveRows + k][r - wy[k].lo]
                                : resize_weight(ay, wy[k].center, sumy[k], r);
          acc[k] = resize_tap(r == wy[k].lo, acc[k], v, s_t[r - rg][lane]);
        }
      }
    }
    rg = rgn, c0 = c0n;
  }
  if (!col_ok) return;
#pragma unroll
  for (int k = 0; k < kWaveRows; ++k) {
    const int oy = oy0 + wv * kWaveRows + k;
    if (oy < im.oh) out[(int64_t)oy * im.ow + ox] = acc[k];
  }
}

// bytes [a0, a1) and [b0, b1) share one
inline bool ranges_meet(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

}  // namespace

// the call behind both entries; Px says what in_rgb points at and what in_off counts
template <typename Px>
static int resize_call(dctae_ctx* ctx, const char* own, const Px* in_rgb, const int64_t* in_off,
                       const int32_t* in_hw, int32_t n_in, const dctae_images_out* out, void* stream) {
  const std::string me = own;
  if (!out) return fail(ctx, DCTAE_EINVAL, me + ": NULL image descriptor");
  if (n_in != out->n_img)
    return fail(ctx, DCTAE_EINVAL, me + ": " + std::to_string(n_in) + " input images, " +
                                       std::to_string(out->n_img) + " output images");
  const int n = n_in;
  if (n < 0) return fail(ctx, DCTAE_EINVAL, me + ": n_img < 0");
  if (n == 0) return 0;
  if (!in_rgb || !in_off || !in_hw || !out->rgb_dev || !out->img_off || !out->hw)
    return fail(ctx, DCTAE_EINVAL, me + ": NULL image buffer");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  std::vector<ResizeImg> R(n);
  std::vector<uintptr_t> i0(n), i1(n);
  uintptr_t in_min = ~uintptr_t(0), in_max = 0;
  int64_t tiles = 0;
  for (int i = 0; i < n; ++i) {
    ResizeImg& r = R[i];
    r.ih = in_hw[2 * i], r.iw = in_hw[2 * i + 1], r.oh = out->hw[2 * i], r.ow = out->hw[2 * i + 1];
    if (r.ih <= 0 || r.iw <= 0 || r.oh <= 0 || r.ow <= 0)
      return fail(ctx, DCTAE_EINVAL, me + ": image " + std::to_string(i) + " has a side <= 0");
    if (r.ih > kMaxSide || r.iw > kMaxSide || r.oh > kMaxSide || r.ow > kMaxSide)
      return fail(ctx, DCTAE_EINVAL, me + ": image " + std::to_string(i) + " has a side above 2^23");
    r.src = in_off[i], r.dst = out->img_off[i];
    r.tiles_x = (r.ow + kTileW - 1) / kTileW, r.tiles_y = (r.oh + kTileH - 1) / kTileH;
    r.pad = 0;
    if (tiles > INT32_MAX) break;
    r.tile0 = (int32_t)tiles;
    tiles += 3ll * r.tiles_x * r.tiles_y;
    i0[i] = (uintptr_t)(in_rgb + r.src);
    i1[i] = i0[i] + (uintptr_t)3 * r.ih * r.iw * sizeof(Px);
    in_min = std::min(in_min, i0[i]), in_max = std::max(in_max, i1[i]);
  }
  if (tiles > INT32_MAX) return fail(ctx, DCTAE_EUNSUP, me + ": too many output tiles in one call");
  for (int i = 0; i < n; ++i) {
    const uintptr_t o0 = (uintptr_t)(out->rgb_dev + R[i].dst), o1 = o0 + (uintptr_t)3 * R[i].oh * R[i].ow * 4;
    if (!ranges_meet(o0, o1, in_min, in_max)) continue;
    for (int j = 0; j < n; ++j)
      if (ranges_meet(o0, o1, i0[j], i1[j]))
        return fail(ctx, DCTAE_EINVAL, me + ": output image " + std::to_string(i) + " overlaps input image " +
                                           std::to_string(j));
  }
  int rc;
  OrderedCall oc(ctx, s);   // the image table travels through the context's plan
  PlanBuf pb;
  const size_t r_off = pb.add(R.data(), R.size());
  uint8_t* pd;
  if ((rc = oc.upload(pb, &pd))) return rc;
  {
    Timer t(ctx, s, "resize_aa");
    k_resize_aa<Px><<<(unsigned)tiles, kThreads, 0, s>>>((const ResizeImg*)(pd + r_off), n, in_rgb, out->rgb_dev);
  }
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

extern "C" {

int dctae_resize_aa(dctae_ctx* ctx, const dctae_images* in, const dctae_images_out* out, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!in) return fail(ctx, DCTAE_EINVAL, "dctae_resize_aa: NULL image descriptor");
  return resize_call(ctx, "dctae_resize_aa", in->rgb_dev, in->img_off, in->hw, in->n_img, out, stream);
}

int dctae_resize_aa_u8(dctae_ctx* ctx, const dctae_images_u8* in, const dctae_images_out* out, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!in) return fail(ctx, DCTAE_EINVAL, "dctae_resize_aa_u8: NULL image descriptor");
  return resize_call(ctx, "dctae_resize_aa_u8", in->rgb_dev, in->img_off, in->hw, in->n_img, out, stream);
}

}  // extern "C"
