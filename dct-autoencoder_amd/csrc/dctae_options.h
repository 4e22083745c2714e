// The context's option switches (dctae_set_option): one struct, one table, one
// apply function.  Plain C++17 with no HIP include, so a host compiler builds
// it alone (tests/test_options_host.py does).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/dctae.h"

namespace dctae {

// Every switch is an int64_t so that one table row type addresses them all;
// the boolean ones hold 0 / 1.
struct Options {
  int64_t fft_enabled = 1;
  // lengths without a Makhoul plan: Bluestein FFT (dctae_bluestein.hip) or the
  // MFMA GEMM.  Default GEMM: on config 4 (1024 ragged images up to 1024^2)
  // the Bluestein kernels measured 16.9 ms of device time against the GEMM
  // path's 12.0 ms (the transform doubles the FFT length; the fp32 MFMA GEMM
  // runs at ~60 TF/s at these sizes) -- DESIGN.md section "Bluestein".
  int64_t bluestein = 0;
  int64_t fft_spec_enabled = 1;
  int64_t t_alias = 0;     // profiling only: images share t_alias T slots (wrong output)
  int64_t bs_ablate = 0;   // profiling only: Bluestein kernels skip 1 loads, 2 FFTs, 4 post (wrong output)
  // profiling only (VERDICT r5 item 2's gate, with t_alias): on a band-path job,
  // 1 = rows only, 2 = columns only, 3 = rows of images [n/2, n) beside
  // columns of [0, n/2) on two streams, 4 = the pipelined step (rows [0, n/2);
  // rows [n/2, n) beside columns [0, n/2); columns [n/2, n); sort / pack),
  // 5 = rows of [n/2, n) alone, 6 = columns of [0, n/2) alone
  int64_t gate = 0;
  // 512-wide rows with 32 kept tile columns: 4 = k_rows512pk (default), 2 = the
  // general compile-time plan kernel k_fft_rows2<512> (serves max_patch_w < 32;
  // selectable here so the parity tests cover it on the headline shape)
  int64_t rows_kernel = 4;
  // 512 x 512 images at 32 x 32 kept tiles: 1 = the row pass writes the band
  // layout (band16 T'[c][y/16][kx][16 rows], t4_index in dctae_rows512.h) and
  // the columns run k_cols512b (16-byte loads,
  // DESIGN.md section 4); 0 = row-major T and k_fft_cols7
  int64_t cols512b = 1;
  // k_cols512b's codes-only encodes on k_cols512w (two strips per 7-wave block, no repeated column lanes)
  int64_t cols_wide = 0;   // measured slower
  // a batch of >= 64 band images: the first half's sort / pack on a side
  // stream beside the second half's column kernel
  int64_t sort_overlap = 0;
  // one job of uniform images whose rows and columns each run one compile-time
  // plan kernel (config 2's 224^2): the first half's columns and sort / pack on
  // a side stream beside the second half's rows and columns
  int64_t halves = 0;   // measured slower
  int64_t xcd_order = 1;             // column blocks of one (image, channel) on one XCD, back to back
  int64_t chunk_bytes = 1ll << 40;   // workspace per chunk of the FFT path (measured: one chunk is fastest)
  int64_t ws_limit = 8ll << 30;      // workspace bytes a chunk job may take
  // 2: rocPRIM block radix sort (<= 3072 tokens per image); 1: the bitonic
  // kernel that serves larger images (selectable for the parity tests)
  int64_t sort_kernel = 2;
  // odd 7-smooth sides (N <= 256, the column kernel's LDS) on the generic FFT
  // kernels in the real-FFT form (M = N); 0 (default): the GEMM DCT (or
  // Bluestein) -- measured faster: config 4 6.37-6.39 vs 6.41-6.44 ms with
  // the odd plans (their sides added ~40 us to each generic FFT launch, the
  // GEMM launches they left did not shrink)
  int64_t fft_odd = 0;
  // sides whose FFT plan has no compile-time kernel (spec 0: every 7-smooth N
  // other than 512 / 224) on the generic LDS Stockham kernels; 0 (default):
  // the MFMA GEMM DCT, measured faster on every shape tried (same box,
  // BatchEncoder ms: 256 x 448^2 2.23 -> 1.24, 512 x 256^2 1.19 -> 0.90,
  // 128 x 480 x 640 1.45 -> 0.80, 256 x 336^2 1.17 -> 0.92, 1024 x 128^2
  // 0.50 -> 0.49; config 4 6.36-6.39 -> 6.12-6.16)
  int64_t fft_generic = 0;
  int64_t fft_decode = 1;        // decode 512^2 batches on the FFT kernels (dctae_idct.hip)
  int64_t dec_rows_kernel = 3;   // decode rows at Kw = 448: 3 = k_idct_rows512, 2 = k_idct_rows2
  // decode columns with k_idct_rows512: 2 = k_idct_cols512b (band-layout U, default), 1 = k_idct_cols512
  int64_t dec_cols_kernel = 2;
  // DCT GEMMs (lengths without a Makhoul plan, dctae_dct2, decode): 1 = the
  // split-bf16 MFMA kernel k_gemm_x3 (fp32 accuracy, 0.375 of the MFMA time),
  // 0 = the fp32 MFMA kernel k_gemm_f32
  int64_t gemm_x3 = 1;
  // the encode's DCT GEMMs (with gemm_x3): 1 = k_gemm_h2 (fp16 MFMA, two-piece
  // operands scaled into the fp16 range, three products: half k_gemm_x3's
  // MFMAs), 0 = k_gemm_x3
  int64_t gemm_h2 = 1;
  // the encode's row GEMM (with gemm_h2): 1 = k_gemm_h2r (operands streamed to
  // LDS by buffer_load ... lds), 0 = k_gemm_h2<3, 1>
  int64_t gemm_dma = 1;
  // images with rows and columns on the GEMM DCT: 1 = colour transform, folds
  // and row GEMM in one pass (k_rows_fused), 0 = k_rgb_to_ipt + the row GEMM
  int64_t rows_fused = 1;
  // the encode's column GEMM (with gemm_h2): 1 = k_gemm_h2c (LDS DMA), 0 = k_gemm_h2<3, 2>
  int64_t cols_dma = 1;
  // images with both passes on the GEMM DCT: T / Y parity-planar (ImgDesc::tperm)
  int64_t tperm = 1;
  // debug: fill each of the five scratch buffers (workspace, staging, PatchNorm
  // statistics, VectorQuantize, LFQ projection) with NaN bits (0xff) when a
  // call first asks for it, so a read of a word the call did not write shows
  // in its outputs (env DCTAE_WS_POISON=1 sets it at context creation)
  int64_t ws_poison = 0;
  // LFQ projections on the fp16 form with the conf/patch14-l.json shapes
  // (192 < in, out <= 208 / 224): 1 = the W-stationary kernel k_lfq_ws
  // (dctae_lfq_ws.hip), 0 = k_lfq_proj_h2
  int64_t lfq_ws = 1;
};

// How a row's legal values are given: kBool stores value != 0; kRange takes
// [lo, hi]; kEither takes lo or hi and nothing between.
enum OptKind { kBool, kRange, kEither };

struct OptionRow {
  const char* key;   // the ABI name (include/dctae.h)
  int64_t Options::*member;
  OptKind kind;
  int64_t lo, hi;
  bool plan;        // read by describe / fft_plan_for / bs_plan_for / build_encode_plan: part of the plan-cache key
  bool profiling;   // wrong outputs on purpose: accepted only with DCTAE_PROFILING (make PROFILING=1)
};

constexpr int64_t kOptMax = INT64_MAX;

constexpr OptionRow kOptions[] = {
    // key               member                       kind     lo       hi       plan   profiling
    {"fft",             &Options::fft_enabled,      kBool,   0,       1,       true,  false},
    {"fft_spec",        &Options::fft_spec_enabled, kBool,   0,       1,       true,  false},
    {"bluestein",       &Options::bluestein,        kBool,   0,       1,       true,  false},
    {"t_alias",         &Options::t_alias,          kRange,  0,       kOptMax, true,  true},
    {"xcd_order",       &Options::xcd_order,        kBool,   0,       1,       true,  false},
    {"gemm_x3",         &Options::gemm_x3,          kBool,   0,       1,       true,  false},
    {"cols512b",        &Options::cols512b,         kBool,   0,       1,       true,  false},
    {"rows_kernel",     &Options::rows_kernel,      kEither, 2,       4,       true,  false},
    {"gemm_h2",         &Options::gemm_h2,          kBool,   0,       1,       true,  false},
    {"fft_odd",         &Options::fft_odd,          kBool,   0,       1,       true,  false},
    {"fft_generic",     &Options::fft_generic,      kBool,   0,       1,       true,  false},
    {"tperm",           &Options::tperm,            kBool,   0,       1,       true,  false},
    {"rows_fused",      &Options::rows_fused,       kBool,   0,       1,       true,  false},
    {"chunk_bytes",     &Options::chunk_bytes,      kRange,  1 << 20, kOptMax, true,  false},
    {"workspace_limit", &Options::ws_limit,         kRange,  1 << 20, kOptMax, true,  false},
    {"bs_ablate",       &Options::bs_ablate,        kRange,  0,       7,       false, true},
    {"gate",            &Options::gate,             kRange,  0,       6,       false, true},
    {"cols_wide",       &Options::cols_wide,        kBool,   0,       1,       false, false},
    {"sort_overlap",    &Options::sort_overlap,     kBool,   0,       1,       false, false},
    {"halves",          &Options::halves,           kBool,   0,       1,       false, false},
    {"fft_decode",      &Options::fft_decode,       kBool,   0,       1,       false, false},
    {"dec_rows_kernel", &Options::dec_rows_kernel,  kEither, 2,       3,       false, false},
    {"dec_cols_kernel", &Options::dec_cols_kernel,  kEither, 1,       2,       false, false},
    {"sort_kernel",     &Options::sort_kernel,      kEither, 1,       2,       false, false},
    {"gemm_dma",        &Options::gemm_dma,         kBool,   0,       1,       false, false},
    {"cols_dma",        &Options::cols_dma,         kBool,   0,       1,       false, false},
    {"lfq_ws",          &Options::lfq_ws,           kBool,   0,       1,       false, false},
    {"ws_poison",       &Options::ws_poison,        kBool,   0,       1,       false, false},
};

// Set option `key` to `value`: 0, DCTAE_EINVAL (unknown key or illegal value)
// or DCTAE_EUNSUP (a profiling switch in a shipped build), with the message in *err.
inline int apply_option(Options& o, const char* key, int64_t value, std::string* err) {
  for (const OptionRow& r : kOptions) {
    if (std::strcmp(r.key, key) != 0) continue;
#ifndef DCTAE_PROFILING
    // profiling switches make dctae_encode write WRONG outputs (shared T
    // slots, skipped loads / stores) and exist only in a profiling build
    // (`make PROFILING=1`, a separate library), never in the shipped one
    if (r.profiling) {
      *err = std::string("option ") + key + " exists only in a profiling build (make PROFILING=1)";
      return DCTAE_EUNSUP;
    }
#endif
    if (r.kind == kBool) value = value != 0;
    if (r.kind == kEither ? (value != r.lo && value != r.hi) : (value < r.lo || value > r.hi)) break;
    o.*r.member = value;
    return 0;
  }
  *err = std::string("unknown option or bad value: ") + key;
  return DCTAE_EINVAL;
}

// The plan-shaping switches, one key entry each, in table order.
template <class Vec>
inline void push_plan_options(const Options& o, Vec& key) {
  for (const OptionRow& r : kOptions)
    if (r.plan) key.push_back(o.*r.member);
}

}  // namespace dctae
