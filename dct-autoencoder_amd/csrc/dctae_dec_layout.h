// The decode family's layouts, each stated once: which path a batch takes, how
// the forward lays out the workspace of its targets (the images of a plain
// decode, the sorted frames of dctae_decode_frames) and how the backward lays
// out its own.  Plain C++17 with no HIP call and no dctae_ctx, so a host
// compiler builds it alone (tests/test_dec_layout_host.py does).
#pragma once
#include <algorithm>
#include <vector>

#include "dctae_internal.h"
#include "dctae_options.h"

namespace dctae {

// ---- path choice ----
// fft: every image 512 x 512 with equal kept tile columns and the recommended
// LFQ (dctae_idct.hip); the planner still asks fft_plan_for for the specialised
// plan.  rows512: 32 kept tile columns on the default row kernel
// (k_idct_rows512); band: U in the band layout (k_idct_cols512b), else row-major
struct DecPath {
  bool fft, rows512, band;
};
constexpr int kFftDecSide = 512;   // the side the FFT decode kernels are compiled for
// codes: the call decodes LFQ codes of cb_dim bits in ncb codebooks
inline DecPath decode_path(const Options& opt, int P, bool codes, int cb_dim, int ncb, const ImgDesc* D, int n_img) {
  bool fftdec = n_img > 0 && opt.fft_decode && P == 14 && (!codes || (cb_dim == 14 && ncb == 14));
  for (int i = 0; fftdec && i < n_img; ++i)
    fftdec = D[i].H == kFftDecSide && D[i].W == kFftDecSide && D[i].qh <= 32 && D[i].qw == D[0].qw;
  const bool rows512 = fftdec && opt.dec_rows_kernel == 3 && D[0].qw == 32;
  return {fftdec, rows512, rows512 && opt.dec_cols_kernel == 2};
}

// ---- forward workspace, in floats ----
struct DecLayout {
  int64_t wsf = 0;       // the targets' regions: what the GEMM path zeroes
  int64_t map_off = 0;   // the slot map, one slab of 3 maxph maxpw words per target
  int64_t map_n = 0;     //   (k_dec_map: the later packed slot wins at a duplicate place, FE:639-643)
  int64_t mm_off = 0;    // clip: two words per target
  int64_t total = 0;     // the scratch request
  std::vector<int2> row_blocks;   // FFT path: (target, y0) of every 16 rows
};

// ws_y / ws_t / ws_p of every target (GEMM path: Y, U and the ipt image, target
// by target, unrounded; FFT path: U alone, on 64-float boundaries), then the
// slot map and, with clip, the min / max words.  staged (clip to bytes): the
// kernels write fp32 targets into the workspace, rgb_off = where
inline DecLayout decode_layout(ImgDesc* T, int n, bool fft, int maxph, int maxpw, bool clip, bool staged) {
  DecLayout L;
  for (int g = 0; g < n; ++g) {
    ImgDesc& d = T[g];
    if (fft) {
      d.ws_t = L.wsf;
      L.wsf += up64(3ll * d.H * d.Kw);
      for (int y0 = 0; y0 < d.H; y0 += 16) L.row_blocks.push_back(make_int2(g, y0));
    } else {
      d.ws_y = L.wsf;
      L.wsf += 3ll * d.Kh * d.Kw;
      d.ws_t = L.wsf;
      L.wsf += 3ll * d.H * d.Kw;
      d.ws_p = L.wsf;
      L.wsf += 3ll * d.H * d.W;
    }
  }
  L.map_off = up64(L.wsf);
  L.map_n = (int64_t)n * 3 * maxph * maxpw;
  L.total = L.map_off + L.map_n;
  L.mm_off = up64(L.total);
  if (clip) L.total = L.mm_off + 2ll * n;
  for (int g = 0; staged && g < n; ++g) {
    T[g].rgb_off = up64(L.total);
    L.total = T[g].rgb_off + 3ll * T[g].H * T[g].W;
  }
  return L;
}

// ---- backward workspace (dctae_decode_backward), in floats ----
struct DecBwdLayout {
  int64_t y_floats;          // every Y first: one memset
  int64_t map_off, map_n;    // the slot map
  int64_t dc_off;            // the images' DC coefficients, 3 floats each
  size_t request;            // bytes
};
// every Y, then U / T and ipt / g_ipt per image, each on a 64-float boundary
inline DecBwdLayout decode_bwd_layout(ImgDesc* D, int n_img, int maxph, int maxpw) {
  DecBwdLayout L{};
  int64_t wsf = 0;
  for (int i = 0; i < n_img; ++i) {
    D[i].ws_y = wsf;
    wsf += up64(3ll * D[i].Kh * D[i].Kw);
  }
  L.y_floats = wsf;
  for (int i = 0; i < n_img; ++i) {
    D[i].ws_t = wsf;
    wsf += up64(3ll * D[i].H * D[i].Kw);
    D[i].ws_p = wsf;
    wsf += up64(3ll * D[i].H * D[i].W);
  }
  L.map_off = wsf;
  L.map_n = (int64_t)n_img * 3 * maxph * maxpw;
  L.dc_off = up64(L.map_off + L.map_n);
  L.request = std::max<size_t>((size_t)(L.dc_off + 3ll * n_img) * 4, 512);
  return L;
}

}  // namespace dctae
