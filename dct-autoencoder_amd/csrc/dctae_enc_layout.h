// The encode plan's layouts, each stated once: which kernel family serves a
// side of an image, which workspace regions the image needs, how a call's
// images are cut into chunk jobs and laid out in the workspace, and how the
// token staging is carved.  Plain C++17 with no HIP call and no dctae_ctx, so a
// host compiler builds it alone (tests/test_enc_layout_host.py does).
#pragma once
#include <algorithm>
#include <cassert>
#include <vector>

#include "dctae_internal.h"
#include "dctae_options.h"

namespace dctae {

// ---- routes: the kernel family of an image's row pass (length W) and column pass (length H) ----
enum class Route { kGemm, kBluestein, kFft, kBand };   // kBand: columns only (k_cols512b on the band layout T')
inline Route row_route(const ImgDesc& d) {
  return d.plan_w < 0 ? Route::kGemm : (d.bs & 1) ? Route::kBluestein : Route::kFft;
}
inline Route col_route(const ImgDesc& d) {
  return d.plan_h < 0 ? Route::kGemm : (d.bs & 2) ? Route::kBluestein : d.tband ? Route::kBand : Route::kFft;
}
inline bool all_fft(const ImgDesc& d) { return row_route(d) != Route::kGemm && col_route(d) != Route::kGemm; }

// ---- regions: what an image keeps in the workspace, in floats (0 = not kept) ----
struct Regions {
  int64_t t;     // T (3, H, Kw): always
  int64_t ipt;   // the colour-transformed image (3, H, W): rows on the GEMM
  int64_t y;     // the spectrum corner Y (3, Kh, Kw): columns on the GEMM or Bluestein (k_tile_epilogue reads it)
};
inline Regions regions_of(const ImgDesc& d) {
  const Route r = row_route(d), c = col_route(d);
  return {3ll * d.Kw * d.H, r == Route::kGemm ? 3ll * d.H * d.W : 0,
          c == Route::kGemm || c == Route::kBluestein ? 3ll * d.Kh * d.Kw : 0};
}
// the bytes the chunk cut counts for an image: 64 floats of slack per region kept
inline int64_t chunk_estimate(const ImgDesc& d) {
  const Regions r = regions_of(d);
  return (r.t + 64 + (r.ipt ? r.ipt + 64 : 0) + (r.y ? r.y + 64 : 0)) * 4;
}
// ---- chunk cut and workspace layout ----
struct JobRange {
  int i0, i1;         // images [i0, i1)
  int64_t amax_off;   // floats: |max| pairs per image, then k_rows_fused's per-image flags, "any" word, 8 tile counters
};
struct WsLayout {
  std::vector<JobRange> jobs;
  size_t ws_need = 0;   // bytes: the largest job (the jobs run one after another on the same workspace)
};

// chunks: FFT images are grouped so the intermediate T of a chunk stays in
// the 256 MiB Infinity Cache between the row and column kernels
inline std::vector<JobRange> cut_chunks(const ImgDesc* D, int n, const Options& opt) {
  std::vector<JobRange> jobs;
  for (int i = 0; i < n;) {
    JobRange j{i, i, 0};
    int64_t wsb = 0;
    while (i < n) {
      const int64_t w = chunk_estimate(D[i]);
      const int64_t cap = all_fft(D[i]) ? std::min<int64_t>(opt.chunk_bytes, opt.ws_limit) : opt.ws_limit;
      if (i > j.i0 && wsb + w > cap) break;
      wsb += w;
      ++i;
    }
    j.i1 = i;
    jobs.push_back(j);
  }
  return jobs;
}

// the chunk cut, then ws_t / ws_p / ws_y of every image (each job starts at 0)
inline WsLayout lay_out_workspace(ImgDesc* D, int n, const Options& opt) {
  WsLayout L;
  L.jobs = cut_chunks(D, n, opt);
  for (JobRange& j : L.jobs) {
    int64_t wsf = 0;
    for (int i = j.i0; i < j.i1; ++i) {
      ImgDesc& d = D[i];
      const Regions r = regions_of(d);
      if (opt.t_alias > 0 && i - j.i0 >= opt.t_alias) {   // profiling: T slots shared (wrong output)
        d.ws_t = D[j.i0 + (i - j.i0) % opt.t_alias].ws_t;
        d.ws_p = d.ws_y = wsf;
        continue;
      }
      d.ws_t = wsf;
      wsf += up64(r.t);
      d.ws_p = wsf;
      wsf += up64(r.ipt);
      d.ws_y = wsf;
      wsf += up64(r.y);
    }
    j.amax_off = wsf;
    wsf += up64(3ll * (j.i1 - j.i0) + 9);
    L.ws_need = std::max<size_t>(L.ws_need, (size_t)wsf * 4);
  }
  return L;
}

// ---- token staging of a packed call: byte offsets of its sections (flat token order) ----
struct StageLayout {
  size_t scores = 0, codes = 0, norm = 0, raw = 0;   // a section the call does not stage is empty
  size_t need = 0;   // the scratch request: the sections unrounded, and 4096 bytes that cover their 256-byte rounding
  StageLayout() = default;
  StageLayout(int64_t n_tok, int ncb, int PP, bool want_norm, bool raw_staged) {
    const size_t nt = (size_t)n_tok, patch = nt * 4 * PP;
    auto up256 = [](size_t v) { return (v + 255) & ~size_t(255); };
    need = nt * (4 + 2 * ncb) + (raw_staged ? patch : 0) + (want_norm ? patch : 0) + 4096;
    codes = scores + up256(nt * 4);
    norm = codes + up256(nt * 2 * ncb);
    raw = norm + (want_norm ? patch : 0);
    assert(raw + (raw_staged ? patch : 0) <= need);
  }
};

}  // namespace dctae
