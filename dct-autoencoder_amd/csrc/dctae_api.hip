// C ABI of libdctae.so: context, planning, workspace and launch sequencing.
// See include/dctae.h for the contract of every entry point.
#include <cmath>
#include <complex>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dctae.h"
#include "dctae_internal.h"
#include "dctae_launch.h"
#include "dctae_model.h"

using namespace dctae;

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------

struct TimedLaunch {
  const char* name;
  hipEvent_t a, b;
};

struct TimingEntry {
  std::string name;
  double ms = 0.0;
  int64_t launches = 0;
};

struct dctae_ctx {
  int device = 0;
  std::string err;
  // DCT-II matrices C_N[rows][N] (fp32, from float64), keyed by (N, rows)
  std::map<std::pair<int, int>, float*> dct;
  // the same matrices pre-split for k_gemm_x3 (GemmProblem::Xs), by fp32 pointer
  struct X3Mat {
    uint16_t* d;
    int R, K, Rp, Kp;
    uint16_t* dh;   // k_gemm_h2: two fp16 planes [2][Rp][Kp] of the matrix scaled by 2^hexp
    int hexp;
  };
  std::map<const float*, X3Mat> dct_x3;
  // workspace (floats) and token staging (bytes), grow-only
  float* ws = nullptr;
  size_t ws_bytes = 0;
  uint8_t* stage = nullptr;
  size_t stage_bytes = 0;
  int64_t ws_limit = 8ll << 30;
  // plan: host (pinned) + device copies, last uploaded plan bytes for caching
  uint8_t* plan_host = nullptr;
  uint8_t* plan_dev = nullptr;
  size_t plan_cap = 0;
  std::vector<uint8_t> plan_last;
  uint64_t plan_last_id = 0, plan_counter = 0;
  hipEvent_t plan_evt = nullptr;
  hipEvent_t done_evt = nullptr;
  // sort_overlap: the first half's sort / pack on a side stream beside the
  // second half's column kernel (created on first use)
  hipStream_t side = nullptr;
  hipEvent_t side_in = nullptr, side_out = nullptr;
  hipStream_t last_stream = nullptr;
  bool have_done = false;
  int* err_dev = nullptr;
  ColorMats cm{};
  // FFT-DCT plans: tables (W_M^k, alpha/beta) in one device buffer
  float2* fft_tab = nullptr;
  int64_t fft_tab_cap = 0, fft_tab_used = 0;
  std::map<int, FftPlan> fft_plans;   // N -> plan (N = 0 entries never stored)
  std::map<int, FftPlan> bs_plans;    // N -> Bluestein plan (kind 1; kind 0 = none)
  std::map<int, int64_t> bs_tw;       // L -> offset of W_L^m in fft_tab
  bool fft_enabled = true;
  // lengths without a Makhoul plan: Bluestein FFT (dctae_bluestein.hip) or the
  // MFMA GEMM.  Default GEMM: on config 4 (1024 ragged images up to 1024^2)
  // the Bluestein kernels measured 16.9 ms of device time against the GEMM
  // path's 12.0 ms (the transform doubles the FFT length; the fp32 MFMA GEMM
  // runs at ~60 TF/s at these sizes) -- DESIGN.md section "Bluestein".
  bool bluestein = false;
  bool fft_spec_enabled = true;
  int t_alias = 0;                    // profiling only: images share t_alias T slots (wrong output)
  int bs_ablate = 0;                  // profiling only: Bluestein kernels skip 1 loads, 2 FFTs, 4 post (wrong output)
  // profiling only (VERDICT r5 item 2's gate, with t_alias): on a band-path job,
  // 1 = rows only, 2 = columns only, 3 = rows of images [n/2, n) beside
  // columns of [0, n/2) on two streams, 4 = the pipelined step (rows [0, n/2);
  // rows [n/2, n) beside columns [0, n/2); columns [n/2, n); sort / pack),
  // 5 = rows of [n/2, n) alone, 6 = columns of [0, n/2) alone
  int gate = 0;
  // 512-wide rows with 32 kept tile columns: 4 = k_rows512pk (default), 2 = the
  // general compile-time plan kernel k_fft_rows2<512> (serves max_patch_w < 32;
  // selectable here so the parity tests cover it on the headline shape)
  int rows_kernel = 4;
  // 512 x 512 images at 32 x 32 kept tiles: 1 = the row pass writes the band
  // layout (band16 T'[c][y/16][kx][16 rows], t4_index in dctae_rows512.h) and
  // the columns run k_cols512b (16-byte loads,
  // DESIGN.md section 4); 0 = row-major T and k_fft_cols7
  int cols512b = 1;
  // k_cols512b's codes-only encodes on k_cols512w (two strips per 7-wave block, no repeated column lanes)
  int cols_wide = 0;   // measured slower
  int sort_overlap = 0;
  // one job of uniform images whose rows and columns each run one compile-time
  // plan kernel (config 2's 224^2): the first half's columns and sort / pack on
  // a side stream beside the second half's rows and columns
  int halves = 0;   // flipped on after its GPU A/B
  int xcd_order = 1;                  // column blocks of one (image, channel) on one XCD, back to back
  size_t lds_limit = 64 * 1024;       // dynamic LDS the FFT kernels may use
  int64_t chunk_bytes = 1ll << 40;    // workspace per chunk of the FFT path (measured: one chunk is fastest)
  // 2: rocPRIM block radix sort (<= 3072 tokens per image); 1: the bitonic
  // kernel that serves larger images (selectable for the parity tests)
  int sort_kernel = 2;
  // odd 7-smooth sides (N <= 256, the column kernel's LDS) on the generic FFT
  // kernels in the real-FFT form (M = N); 0 (default): the GEMM DCT (or
  // Bluestein) -- measured faster: config 4 6.37-6.39 vs 6.41-6.44 ms with
  // the odd plans (their sides added ~40 us to each generic FFT launch, the
  // GEMM launches they left did not shrink)
  int fft_odd = 0;
  // sides whose FFT plan has no compile-time kernel (spec 0: every 7-smooth N
  // other than 512 / 224) on the generic LDS Stockham kernels; 0 (default):
  // the MFMA GEMM DCT, measured faster on every shape tried (same box,
  // BatchEncoder ms: 256 x 448^2 2.23 -> 1.24, 512 x 256^2 1.19 -> 0.90,
  // 128 x 480 x 640 1.45 -> 0.80, 256 x 336^2 1.17 -> 0.92, 1024 x 128^2
  // 0.50 -> 0.49; config 4 6.36-6.39 -> 6.12-6.16)
  int fft_generic = 0;
  int fft_decode = 1;                 // decode 512^2 batches on the FFT kernels (dctae_idct.hip)
  int dec_rows_kernel = 3;            // decode rows at Kw = 448: 3 = k_idct_rows512, 2 = k_idct_rows2
  // decode columns with k_idct_rows512: 2 = k_idct_cols512b (band-layout U, default), 1 = k_idct_cols512
  int dec_cols_kernel = 2;
  int n_cu = 256;
  // DCT GEMMs (lengths without a Makhoul plan, dctae_dct2, decode): 1 = the
  // split-bf16 MFMA kernel k_gemm_x3 (fp32 accuracy, 0.375 of the MFMA time),
  // 0 = the fp32 MFMA kernel k_gemm_f32
  int gemm_x3 = 1;
  // the encode's DCT GEMMs (with gemm_x3): 1 = k_gemm_h2 (fp16 MFMA, two-piece
  // operands scaled into the fp16 range, three products: half k_gemm_x3's
  // MFMAs), 0 = k_gemm_x3
  int gemm_h2 = 1;
  // the encode's row GEMM (with gemm_h2): 1 = k_gemm_h2r (operands streamed to
  // LDS by buffer_load ... lds), 0 = k_gemm_h2<3, 1>
  int gemm_dma = 1;
  // images with rows and columns on the GEMM DCT: 1 = colour transform, folds
  // and row GEMM in one pass (k_rows_fused), 0 = k_rgb_to_ipt + the row GEMM
  int rows_fused = 1;
  // the encode's column GEMM (with gemm_h2): 1 = k_gemm_h2c (LDS DMA), 0 = k_gemm_h2<3, 2>
  int cols_dma = 1;
  // images with both passes on the GEMM DCT: T / Y parity-planar (ImgDesc::tperm)
  int tperm = 1;
  // debug: fill the workspace and staging buffers with NaN bits (0xff) before
  // every call that sizes them, so a read of a word the call did not write
  // shows in its outputs (env DCTAE_WS_POISON=1 sets it at context creation)
  int ws_poison = 0;
  // LFQ projections on the fp16 form with the conf/patch14-l.json shapes
  // (192 < in, out <= 208 / 224): 1 = the W-stationary kernel k_lfq_ws
  // (dctae_lfq_ws.hip), 0 = k_lfq_proj_h2
  int lfq_ws = 1;
  // PatchNorm training scratch (token cell ids, per-cell lists, batch tables), grow-only
  uint8_t* st_ws = nullptr;
  // VectorQuantize scratch (projected vectors, codes, transformed codebook), grow-only
  uint8_t* vq_ws = nullptr;
  size_t vq_bytes = 0;
  // LFQ projection scratch (the pre-split weight planes), grow-only
  uint16_t* proj_ws = nullptr;
  size_t proj_bytes = 0;
  size_t st_bytes = 0;
  // cached encode plan
  std::vector<int64_t> enc_key;
  struct EncPlan* enc_plan = nullptr;
  // timing
  bool timing = false;
  std::vector<TimedLaunch> pending;
  std::vector<hipEvent_t> evt_pool;
  std::vector<TimingEntry> totals;
};

namespace {
void ctx_gemm(const dctae_ctx* ctx, int nc, const dctae::GemmProblem* probs, const dctae::TileRef* tiles, int n_tiles,
              hipStream_t s, int share = 0) {
  if (ctx->gemm_x3)
    dctae::launch_gemm_x3(nc, probs, tiles, n_tiles, s, share);
  else
    dctae::launch_gemm(nc, probs, tiles, n_tiles, s, share);
}
}  // namespace

namespace {

thread_local std::string g_err;

int fail(dctae_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  g_err = msg;
  return code;
}

#define HIPCHK(ctx, expr)                                                              \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return fail(ctx, DCTAE_EHIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)

// reference colour constants (util.py:21-43), built exactly like the
// reference does in fp32: Trgb2lms = MHPE @ MsRGB; Tlms2rgb = inverse; Mipt^-1.
// The Python layer overrides these with torch-computed bits (ctx->cm) so the
// matrix inverses carry the reference's exact fp32 values.
void default_colors(ColorMats& cm) {
  const double srgb[9] = {0.4124564, 0.3575761, 0.1804375, 0.2126729, 0.7151522, 0.0721750,
                          0.0193339, 0.1191920, 0.9503041};
  const double hpe[9] = {0.4002, 0.7076, -0.0807, -0.2280, 1.1500, 0.0612, 0, 0, 0.9184};
  const double ipt[9] = {0.4, 0.4, 0.2, 4.455, -4.851, 0.3960, 0.8056, 0.3572, -1.1628};
  double m[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0;
      for (int k = 0; k < 3; ++k) s += (double)(float)hpe[3 * i + k] * (double)(float)srgb[3 * k + j];
      m[3 * i + j] = s;
    }
  auto inv3 = [](const double* a, double* o) {
    double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) +
                 a[2] * (a[3] * a[7] - a[4] * a[6]);
    o[0] = (a[4] * a[8] - a[5] * a[7]) / det;
    o[1] = (a[2] * a[7] - a[1] * a[8]) / det;
    o[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    o[3] = (a[5] * a[6] - a[3] * a[8]) / det;
    o[4] = (a[0] * a[8] - a[2] * a[6]) / det;
    o[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    o[6] = (a[3] * a[7] - a[4] * a[6]) / det;
    o[7] = (a[1] * a[6] - a[0] * a[7]) / det;
    o[8] = (a[0] * a[4] - a[1] * a[3]) / det;
  };
  double mi[9], ii[9], ipd[9];
  for (int i = 0; i < 9; ++i) ipd[i] = (float)ipt[i];
  inv3(m, mi);
  inv3(ipd, ii);
  for (int i = 0; i < 9; ++i) {
    cm.rgb2lms[i] = (float)m[i];
    cm.lms2rgb[i] = (float)mi[i];
    cm.lms2ipt[i] = (float)ipt[i];
    cm.ipt2lms[i] = (float)ii[i];
  }
}

// the call-ordering event (order_after_previous / mark_done) only orders this
// context's calls across streams of one device: no system-scope fence (its
// cache write-back sat between back-to-back calls)
constexpr unsigned kDoneEvtFlags = hipEventDisableTiming | hipEventDisableSystemFence;

struct Timer {
  dctae_ctx* ctx;
  hipStream_t s;
  const char* name;
  hipEvent_t a = nullptr;
  Timer(dctae_ctx* c, hipStream_t st, const char* n) : ctx(c), s(st), name(n) {
    if (ctx->timing) {
      a = take();
      hipEventRecord(a, s);
    }
  }
  hipEvent_t take() {
    if (ctx->evt_pool.empty()) {
      hipEvent_t e;
      hipEventCreate(&e);
      return e;
    }
    hipEvent_t e = ctx->evt_pool.back();
    ctx->evt_pool.pop_back();
    return e;
  }
  ~Timer() {
    if (ctx->timing) {
      hipEvent_t b = take();
      hipEventRecord(b, s);
      ctx->pending.push_back({name, a, b});
    }
  }
};

// ---- plan serialisation ----------------------------------------------------
struct PlanBuf {
  std::vector<uint8_t> bytes;
  template <class T>
  size_t add(const T* p, size_t n) {
    size_t off = (bytes.size() + 255) & ~size_t(255);
    bytes.resize(off + n * sizeof(T));
    if (n) std::memcpy(bytes.data() + off, p, n * sizeof(T));
    return off;
  }
};

// order this call after the previous one on a possibly different stream
void order_after_previous(dctae_ctx* ctx, hipStream_t s) {
  if (ctx->have_done && ctx->last_stream != s) hipStreamWaitEvent(s, ctx->done_evt, 0);
}

void mark_done(dctae_ctx* ctx, hipStream_t s) {
  hipEventRecord(ctx->done_evt, s);
  ctx->last_stream = s;
  ctx->have_done = true;
}

int upload_plan(dctae_ctx* ctx, const PlanBuf& pb, hipStream_t s, uint64_t plan_id = 0) {
  const size_t n = pb.bytes.size();
  if (n == 0) return 0;
  if (plan_id != 0 && plan_id == ctx->plan_last_id) return 0;
  if (n == ctx->plan_last.size() && std::memcmp(pb.bytes.data(), ctx->plan_last.data(), n) == 0) {
    ctx->plan_last_id = plan_id;
    return 0;
  }
  if (n > ctx->plan_cap) {
    HIPCHK(ctx, hipDeviceSynchronize());
    if (ctx->plan_host) hipHostFree(ctx->plan_host);
    if (ctx->plan_dev) hipFree(ctx->plan_dev);
    ctx->plan_host = nullptr;
    ctx->plan_dev = nullptr;
    size_t cap = std::max<size_t>(n * 2, 1 << 20);
    HIPCHK(ctx, hipHostMalloc((void**)&ctx->plan_host, cap, hipHostMallocDefault));
    HIPCHK(ctx, hipMalloc((void**)&ctx->plan_dev, cap));
    ctx->plan_cap = cap;
  } else {
    HIPCHK(ctx, hipEventSynchronize(ctx->plan_evt));  // previous upload finished reading plan_host
  }
  std::memcpy(ctx->plan_host, pb.bytes.data(), n);
  HIPCHK(ctx, hipMemcpyAsync(ctx->plan_dev, ctx->plan_host, n, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipEventRecord(ctx->plan_evt, s));
  ctx->plan_last = pb.bytes;
  ctx->plan_last_id = plan_id;
  return 0;
}

int ensure_ws(dctae_ctx* ctx, size_t ws_bytes, size_t stage_bytes) {
  if (ws_bytes > ctx->ws_bytes) {
    HIPCHK(ctx, hipDeviceSynchronize());
    if (ctx->ws) hipFree(ctx->ws);
    ctx->ws = nullptr;
    ctx->ws_bytes = 0;
    if (hipMalloc((void**)&ctx->ws, ws_bytes) != hipSuccess)
      return fail(ctx, DCTAE_ENOMEM, "workspace allocation of " + std::to_string(ws_bytes) + " bytes failed");
    ctx->ws_bytes = ws_bytes;
  }
  if (stage_bytes > ctx->stage_bytes) {
    HIPCHK(ctx, hipDeviceSynchronize());
    if (ctx->stage) hipFree(ctx->stage);
    ctx->stage = nullptr;
    ctx->stage_bytes = 0;
    if (hipMalloc((void**)&ctx->stage, stage_bytes) != hipSuccess)
      return fail(ctx, DCTAE_ENOMEM, "staging allocation of " + std::to_string(stage_bytes) + " bytes failed");
    ctx->stage_bytes = stage_bytes;
  }
  if (ctx->ws_poison) {   // a request of <= 256 bytes leaves that buffer alone (a call's second ensure_ws)
    HIPCHK(ctx, hipDeviceSynchronize());
    if (ws_bytes > 256) HIPCHK(ctx, hipMemset(ctx->ws, 0xff, ctx->ws_bytes));
    if (stage_bytes > 256) HIPCHK(ctx, hipMemset(ctx->stage, 0xff, ctx->stage_bytes));
    HIPCHK(ctx, hipDeviceSynchronize());
  }
  return 0;
}

// orthonormal DCT-II matrix rows [0, rows) of size N, fp64 -> fp32.
// parity 0 / 1: the even / odd rows k = 2i (+1) restricted to the columns
// n < ceil(N/2) / floor(N/2), the operand of the folded transform
// X[k] = sum_n C[k][n] (x[n] +- x[N-1-n]) (C[k][N-1-n] = (-1)^k C[k][n]).
int dct_matrix(dctae_ctx* ctx, int N, int rows, const float** out, int parity = -1) {
  auto key = std::make_pair(N, rows * 4 + parity + 1);
  auto it = ctx->dct.find(key);
  if (it != ctx->dct.end()) {
    *out = it->second;
    return 0;
  }
  const int R = parity < 0 ? rows : (parity == 0 ? (rows + 1) / 2 : rows / 2);
  const int Nc = parity < 0 ? N : (parity == 0 ? (N + 1) / 2 : N / 2);
  std::vector<float> h((size_t)std::max(R, 1) * std::max(Nc, 1));
  const double pi = 3.14159265358979323846;
  for (int i = 0; i < R; ++i) {
    const int k = parity < 0 ? i : 2 * i + parity;
    double sk = (k == 0) ? std::sqrt(1.0 / N) : std::sqrt(2.0 / N);
    for (int n = 0; n < Nc; ++n) {
      // reduce the angle exactly: cos(pi*(2n+1)k/(2N)) with (2n+1)k mod 4N
      long long a = ((long long)(2 * n + 1) * k) % (4ll * N);
      h[(size_t)i * Nc + n] = (float)(sk * std::cos(pi * (double)a / (2.0 * N)));
    }
  }
  float* d = nullptr;
  HIPCHK(ctx, hipMalloc((void**)&d, h.size() * sizeof(float)));
  HIPCHK(ctx, hipMemcpy(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  ctx->dct[key] = d;
  {
    std::vector<uint16_t> x;
    dctae_ctx::X3Mat xm{nullptr, R, Nc, 0, 0, nullptr, 0};
    split_matrix_x3(h.data(), R, Nc, x, &xm.Rp, &xm.Kp);
    HIPCHK(ctx, hipMalloc((void**)&xm.d, x.size() * sizeof(uint16_t)));
    HIPCHK(ctx, hipMemcpy(xm.d, x.data(), x.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    int rp, kp;
    split_matrix_h2(h.data(), R, Nc, x, &rp, &kp, &xm.hexp);
    HIPCHK(ctx, hipMalloc((void**)&xm.dh, x.size() * sizeof(uint16_t)));
    HIPCHK(ctx, hipMemcpy(xm.dh, x.data(), x.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    ctx->dct_x3[d] = xm;
  }
  *out = d;
  return 0;
}

// grow-only scratch for the LFQ projections' pre-split weight (N x K)
int proj_scratch(dctae_ctx* ctx, int N, int K) {
  const size_t need = lfq_proj_scratch_bytes(N, K);
  if (need <= ctx->proj_bytes) return 0;
  HIPCHK(ctx, hipDeviceSynchronize());
  if (ctx->proj_ws) hipFree(ctx->proj_ws);
  ctx->proj_ws = nullptr;
  ctx->proj_bytes = 0;
  if (hipMalloc((void**)&ctx->proj_ws, need) != hipSuccess)
    return fail(ctx, DCTAE_ENOMEM, "LFQ projection scratch allocation failed");
  ctx->proj_bytes = need;
  return 0;
}

// point a GEMM's shared DCT-matrix operand at its pre-split planes (used by
// k_gemm_x3 only): the operand must be a whole cached matrix read row-major
// with k contiguous
void attach_x3(const dctae_ctx* ctx, GemmProblem& g) {
  const int sh = gemm_share(g);
  if (ctx->gemm_x3) {
    // k_gemm_x3's tiles: 128 wide along the shared operand (launch_gemm_x3)
    if (sh == 1) g.tile_n = 128;
    if (sh == 2) g.tile_m = 128;
    g.tiles_n = (g.N + g.tile_n - 1) / g.tile_n;
  }
  const float* m = sh == 1 ? g.B : sh == 2 ? g.A : nullptr;
  if (!m) return;
  auto it = ctx->dct_x3.find(m);
  if (it == ctx->dct_x3.end()) return;
  const auto& x = it->second;
  const int64_t sr = sh == 1 ? g.sBn : g.sAm, sk = sh == 1 ? g.sBk : g.sAk;
  const int rows = sh == 1 ? g.N : g.M;
  if (sk != 1 || sr != x.K || g.K > x.K || rows > x.R) return;
  g.Xs = x.d;
  g.xs_ld = x.Kp;
  g.xs_plane = (int64_t)x.Rp * x.Kp;
  g.Xh = x.dh;
  g.xh_exp = x.hexp;
}

int check_cfg(dctae_ctx* ctx, const dctae_fe_cfg* cfg) {
  if (!cfg) return fail(ctx, DCTAE_EINVAL, "cfg is NULL");
  if (cfg->channels != 3) return fail(ctx, DCTAE_EUNSUP, "channels must be 3 (IPT colour transform)");
  if (cfg->patch_size < 1 || cfg->patch_size > kMaxP)
    return fail(ctx, DCTAE_EUNSUP, "patch_size must be in [1, 16]");
  if (cfg->max_patch_h < 1 || cfg->max_patch_w < 1 || cfg->max_seq_len < 1)
    return fail(ctx, DCTAE_EINVAL, "max_patch_h/w and max_seq_len must be >= 1");
  return 0;
}

int check_lfq(dctae_ctx* ctx, const dctae_lfq* lfq, int PP) {
  if (!lfq) return fail(ctx, DCTAE_EINVAL, "lfq is NULL");
  if (lfq->codebook_dim < 1 || lfq->codebook_dim > 16)
    return fail(ctx, DCTAE_EUNSUP, "codebook_dim must be in [1, 16] (codebook_size <= 65536)");
  if (lfq->codebook_dim * lfq->num_codebooks != PP)
    return fail(ctx, DCTAE_EUNSUP, "LFQ with projections is not fused: codebook_dim*num_codebooks != P*P");
  return 0;
}

// build the per-image descriptor (tokens, crop, kept corner); FE:312-345, 364-399
int describe(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int H, int W, ImgDesc& d) {
  const int P = cfg->patch_size;
  if (H < P || W < P)
    return fail(ctx, DCTAE_EINVAL, "image " + std::to_string(H) + "x" + std::to_string(W) +
                                       " is smaller than patch_size (FE:313-314)");
  std::memset(&d, 0, sizeof(d));
  d.plan_w = d.plan_h = -1;
  d.H = H;
  d.W = W;
  d.ph = std::max(H / P, 1);
  d.pw = std::max(W / P, 1);
  d.qh = std::min(d.ph, cfg->max_patch_h);
  d.qw = std::min(d.pw, cfg->max_patch_w);
  d.Kh = P * d.qh;
  d.Kw = P * d.qw;
  d.T = cfg->channels * d.qh * d.qw;
  return 0;
}

GemmProblem gemm(const float* A, int64_t sAc, int64_t sAm, int64_t sAk, const float* B, int64_t sBc, int64_t sBn,
                 int64_t sBk, float* O, int64_t sOc, int64_t sOm, int64_t sOn, int M, int N, int K, int C) {
  GemmProblem g{};
  g.A = A;
  g.B = B;
  g.O = O;
  g.sAc = sAc, g.sAm = sAm, g.sAk = sAk;
  g.sBc = sBc, g.sBn = sBn, g.sBk = sBk;
  g.sOc = sOc, g.sOm = sOm, g.sOn = sOn;
  g.M = M, g.N = N, g.K = K, g.C = C;
  g.tile_m = g.tile_n = 64;
  g.tiles_n = (N + 63) / 64;
  return g;
}

// XCD-aware order of a GEMM tile list (speed only; any order is correct).
// Workgroup b runs on XCD b % 8, so the tiles that read the same per-channel
// operand panel -- (problem, tile row) when B is the shared matrix (share 1),
// (problem, tile column) when A is (share 2) -- are dealt to one XCD as
// consecutive b / 8: the panel is then fetched into that XCD's L2 once instead
// of once per XCD.  Groups go to the least-loaded XCD; the lanes are padded to
// equal length with empty tiles (problem -1, the kernels return at once) so
// the b % 8 affinity holds to the end of the launch.
void xcd_deal_tiles(std::vector<TileRef>& t, const GemmProblem* probs, int share) {
  if (t.size() < 16 || share == 0) return;
  // with many problems (>= 64, e.g. a batch of images), all tiles of a problem
  // on one XCD: its shared operand (a DCT matrix of up to ~1 MB pre-split) is
  // fetched into one L2 instead of all eight, and the per-channel rows re-read
  // by its N tiles hit there too; with few, the tiles sharing the per-channel
  // operand's rows (or columns) as the unit, so every XCD gets work
  int n_prob = 0;
  {
    std::vector<int> seen;
    for (const TileRef& r : t) seen.push_back(r.problem);
    std::sort(seen.begin(), seen.end());
    n_prob = (int)(std::unique(seen.begin(), seen.end()) - seen.begin());
  }
  const bool per_problem = n_prob >= 64;
  std::vector<std::vector<TileRef>> groups;
  std::map<std::pair<int, int>, size_t> gi;
  for (const TileRef& r : t) {
    const int tn = probs[r.problem].tiles_n;
    const std::pair<int, int> key{r.problem, per_problem ? 0 : (share == 1 ? r.tile / tn : r.tile % tn)};
    auto it = gi.find(key);
    if (it == gi.end()) {
      gi[key] = groups.size();
      groups.push_back({r});
    } else {
      groups[it->second].push_back(r);
    }
  }
  std::vector<std::vector<TileRef>> lanes(8);
  for (auto& g : groups) {
    size_t best = 0;
    for (size_t x = 1; x < 8; ++x)
      if (lanes[x].size() < lanes[best].size()) best = x;
    lanes[best].insert(lanes[best].end(), g.begin(), g.end());
  }
  size_t maxlen = 0;
  for (auto& l : lanes) maxlen = std::max(maxlen, l.size());
  std::vector<TileRef> out;
  out.reserve(8 * maxlen);
  for (size_t q = 0; q < maxlen; ++q)
    for (int x = 0; x < 8; ++x) out.push_back(q < lanes[x].size() ? lanes[x][q] : TileRef{-1, 0});
  t.swap(out);
}

void add_tiles(std::vector<TileRef>& t, int prob, const GemmProblem& g) {
  int tm = (g.M + g.tile_m - 1) / g.tile_m;
  for (int i = 0; i < tm * g.tiles_n; ++i) t.push_back({prob, i});
}

const float* norm_thr(const dctae_norm* norm) { return norm ? norm->thr_dev : nullptr; }

EncParams enc_params(const dctae_fe_cfg* cfg, const dctae_norm* norm, const dctae_lfq* lfq) {
  EncParams ep{};
  ep.P = cfg->patch_size;
  ep.C = cfg->channels;
  ep.maxph = cfg->max_patch_h;
  ep.maxpw = cfg->max_patch_w;
  ep.S = cfg->max_seq_len;
  for (int i = 0; i < 3; ++i) ep.ci[i] = cfg->channel_importances[i];
  ep.mw = cfg->magnitude_weight;
  if (norm) {
    ep.median = norm->median_dev;
    ep.b = norm->b_dev;
    ep.eps = norm->eps;
    ep.min_val = norm->min_val;
    ep.max_val = norm->max_val;
  }
  if (lfq) {
    ep.cb_dim = lfq->codebook_dim;
    ep.ncb = lfq->num_codebooks;
    ep.scale = lfq->codebook_scale;
    uint64_t pos, neg;
    lfq_index_masks(ep.scale, ep.cb_dim, &pos, &neg);
    ep.code_pos = (uint32_t)pos;
    ep.code_neg = (uint32_t)neg;
  }
  return ep;
}

int next_pow2(int x) {
  int p = 1;
  while (p < x) p <<= 1;
  return p;
}

// Room for `need` more float2 in the FFT table buffer; grows it (the offsets
// stay valid) after draining the device, since launches in flight may read it.
int tab_reserve(dctae_ctx* ctx, int64_t need) {
  if (ctx->fft_tab_used + need <= ctx->fft_tab_cap) return 0;
  const int64_t cap = std::max(2 * ctx->fft_tab_cap, ctx->fft_tab_used + need);
  float2* t = nullptr;
  if (hipMalloc((void**)&t, cap * sizeof(float2)) != hipSuccess) return -1;
  if (hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(t, ctx->fft_tab, ctx->fft_tab_used * sizeof(float2), hipMemcpyDeviceToDevice) != hipSuccess) {
    hipFree(t);
    return -1;
  }
  hipFree(ctx->fft_tab);
  ctx->fft_tab = t;
  ctx->fft_tab_cap = cap;
  return 0;
}

int64_t tab_put(dctae_ctx* ctx, const std::vector<float2>& h) {
  if (tab_reserve(ctx, (int64_t)h.size())) return -1;
  if (hipMemcpy(ctx->fft_tab + ctx->fft_tab_used, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice) !=
      hipSuccess)
    return -1;
  const int64_t o = ctx->fft_tab_used;
  ctx->fft_tab_used += (int64_t)h.size();
  return o;
}

// in-place radix-2 FFT in float64 (host tables only), e^{-2 pi i nk / L}
void fft_f64(std::vector<std::complex<double>>& a) {
  const int L = (int)a.size();
  for (int i = 1, j = 0; i < L; ++i) {
    int bit = L >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(a[i], a[j]);
  }
  const double pi = 3.14159265358979323846;
  for (int len = 2; len <= L; len <<= 1)
    for (int i = 0; i < L; i += len)
      for (int k = 0; k < len / 2; ++k) {
        const std::complex<double> w = std::polar(1.0, -2.0 * pi * k / len);
        const std::complex<double> u = a[i + k], v = a[i + k + len / 2] * w;
        a[i + k] = u + v;
        a[i + k + len / 2] = u - v;
      }
}

// Bluestein plan for length N (dctae_bluestein.hip): tables in float64 -> fp32;
// -1 outside N in [32, 1024] or with the option off
int bs_plan_for(dctae_ctx* ctx, int N, FftPlan* out) {
  if (!ctx->fft_enabled || !ctx->bluestein || N < 32 || N > 1024) return -1;
  auto it = ctx->bs_plans.find(N);
  if (it != ctx->bs_plans.end()) {
    *out = it->second;
    return it->second.kind == 1 ? 0 : -1;
  }
  FftPlan p{};
  p.N = N;
  p.M = N / 2;
  int L = 256;
  while (L < 2 * N - 1) L <<= 1;
  const double pi = 3.14159265358979323846;
  auto bad = [&]() {
    ctx->bs_plans[N] = p;  // kind 0: no Bluestein plan for N
    return -1;
  };
  auto tw_it = ctx->bs_tw.find(L);
  if (tw_it == ctx->bs_tw.end()) {
    std::vector<float2> tw(L);
    for (int m = 0; m < L; ++m) {
      const double a = -2.0 * pi * m / L;
      tw[m] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    const int64_t o = tab_put(ctx, tw);
    if (o < 0) return bad();
    tw_it = ctx->bs_tw.emplace(L, o).first;
  }
  std::vector<std::complex<double>> c(N), b(L, 0.0);
  for (int n = 0; n < N; ++n) c[n] = std::polar(1.0, -pi * (double)(((int64_t)n * n) % (2 * N)) / N);
  for (int m = 0; m < N; ++m) {
    b[m] = std::conj(c[m]);
    if (m) b[L - m] = std::conj(c[m]);
  }
  fft_f64(b);
  std::vector<float2> h(2 * N + L);
  for (int n = 0; n < N; ++n) h[n] = make_float2((float)c[n].real(), (float)c[n].imag());
  for (int m = 0; m < L; ++m) h[N + m] = make_float2((float)(b[m].real() / L), (float)(b[m].imag() / L));
  for (int k = 0; k < N; ++k) {
    const double sk = (k == 0) ? std::sqrt(1.0 / N) : std::sqrt(2.0 / N);
    const std::complex<double> e = std::polar(0.5 * sk, -pi * k / (2.0 * N));
    h[N + L + k] = make_float2((float)e.real(), (float)e.imag());
  }
  const int64_t o = tab_put(ctx, h);
  if (o < 0) return bad();
  p.kind = 1;
  p.bs_L = L;
  p.npass = 1;
  p.bs_tw_off = tw_it->second;
  p.bs_chirp_off = o;
  p.bs_bhat_off = o + N;
  p.bs_post_off = o + N + L;
  ctx->bs_plans[N] = p;
  *out = p;
  return 0;
}

int bs_lidx(int L) { return L == 256 ? 0 : L == 512 ? 1 : L == 1024 ? 2 : 3; }
constexpr int kBsL[4] = {256, 512, 1024, 2048};

// FFT plan for length N (Makhoul: M = N/2 point complex FFT); -1 if N has no plan
int fft_plan_for(dctae_ctx* ctx, int N, int P, FftPlan* out) {
  // even N: Makhoul on the N / 2 point complex FFT of z[m] = v[2m] + i v[2m + 1];
  // odd N (ctx->fft_odd): the N point complex FFT of v (the real-FFT form)
  const bool odd = (N & 1) != 0;
  const int Mc = odd ? N : N / 2;
  if (!ctx->fft_enabled || N < 4 || (odd && (!ctx->fft_odd || N < 15)) || Mc > 512) return -1;
  if ((size_t)16 * Mc * kMaxP > ctx->lds_limit) return -1;
  auto it = ctx->fft_plans.find(N);
  if (it != ctx->fft_plans.end()) {
    *out = it->second;
    out->spec = ctx->fft_spec_enabled ? fft_spec_id(N, out->radix, out->npass, P) : 0;
    if (out->spec) out->rows_per_block = fft_spec_rows_per_block(out->spec);
    if (!out->spec && !ctx->fft_generic) return -1;   // the GEMM DCT (see dctae_ctx::fft_generic)
    return it->second.npass > 0 ? 0 : -1;
  }
  FftPlan p{};
  p.N = N;
  p.M = Mc;
  p.odd = odd ? 1 : 0;
  int m = p.M, np = 0;
  const int rads[7] = {16, 8, 4, 2, 7, 5, 3};
  while (m > 1 && np < 8) {
    bool ok = false;
    for (int r : rads)
      if (m % r == 0) {
        p.radix[np++] = r;
        m /= r;
        ok = true;
        break;
      }
    if (!ok) break;
  }
  if (m != 1) {
    p.npass = 0;
    ctx->fft_plans[N] = p;
    return -1;
  }
  p.npass = np;
  // rows per block of k_fft_rows: 2 (ping-pong) x rows x 3 jobs x (2M+1) floats <= 52 KiB
  p.rows_per_block = std::max(1, std::min(8, (int)(53248 / (24 * (2 * p.M + 1)))));
  const int64_t need = p.M + 2ll * (p.M + 1) + 2ll * p.M;
  if (tab_reserve(ctx, need)) {
    p.npass = 0;
    ctx->fft_plans[N] = p;
    return -1;
  }
  std::vector<float2> h(need);
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < p.M; ++k) {
    double a = -2.0 * pi * k / p.M;
    h[k] = make_float2((float)std::cos(a), (float)std::sin(a));
  }
  for (int k = 0; odd && k <= p.M; ++k) {
    // X_k = Re(w_k V_k), w_k = s_k e^{-i pi k / (2N)} (Makhoul's reordering holds for odd N)
    const double sk = (k == 0) ? std::sqrt(1.0 / N) : std::sqrt(2.0 / N);
    const double t1 = -pi * k / (2.0 * N);
    h[p.M + 2 * k] = make_float2((float)(std::cos(t1) * sk), (float)(std::sin(t1) * sk));
    h[p.M + 2 * k + 1] = make_float2(0.0f, 0.0f);
  }
  for (int k = 0; !odd && k <= p.M; ++k) {
    // W = alpha (A + B) + beta (A - B), A = Z[k], B = conj Z[M-k]
    //   alpha = a/2 * s, beta = -i * a * e^{-2 pi i k / N} / 2 * s, a = e^{-i pi k / (2N)}
    const double sk = (k == 0) ? std::sqrt(1.0 / N) : std::sqrt(2.0 / N);
    const double t1 = -pi * k / (2.0 * N), t2 = t1 - 2.0 * pi * k / N;
    const double ar = std::cos(t1) * 0.5 * sk, ai = std::sin(t1) * 0.5 * sk;
    const double br = std::cos(t2) * 0.5 * sk, bi = std::sin(t2) * 0.5 * sk;
    h[p.M + 2 * k] = make_float2((float)ar, (float)ai);
    h[p.M + 2 * k + 1] = make_float2((float)bi, (float)-br);  // -i * (br + i bi) = bi - i br
  }
  for (int k = 0; odd && k < p.M; ++k) {   // no DCT-III on odd plans (the FFT decode is 512 only)
    h[p.M + 2 * (p.M + 1) + 2 * k] = make_float2(0.0f, 0.0f);
    h[p.M + 2 * (p.M + 1) + 2 * k + 1] = make_float2(0.0f, 0.0f);
  }
  for (int k = 0; !odd && k < p.M; ++k) {
    // DCT-III pre-processing (dctae_idct.hip): Z_k = a_k A_k + b_k B_k; stored conjugated
    const double g = std::sqrt(N / 2.0) / p.M;
    const double e = 2.0 * pi * k / N;                       // i e^{i e} = (-sin e, cos e)
    const double t1 = pi * k / (2.0 * N), t2 = pi * (k + p.M) / (2.0 * N);
    const double pr = 1.0 - std::sin(e), pi_ = std::cos(e);  // 1 + i e^{i e}
    const double qr = 1.0 + std::sin(e), qi = -std::cos(e);  // 1 - i e^{i e}
    const double ar = 0.5 * g * (pr * std::cos(t1) - pi_ * std::sin(t1)), ai = 0.5 * g * (pr * std::sin(t1) + pi_ * std::cos(t1));
    const double br = 0.5 * g * (qr * std::cos(t2) - qi * std::sin(t2)), bi = 0.5 * g * (qr * std::sin(t2) + qi * std::cos(t2));
    h[p.M + 2 * (p.M + 1) + 2 * k] = make_float2((float)ar, (float)-ai);
    h[p.M + 2 * (p.M + 1) + 2 * k + 1] = make_float2((float)br, (float)-bi);
  }
  if (hipMemcpy(ctx->fft_tab + ctx->fft_tab_used, h.data(), need * sizeof(float2), hipMemcpyHostToDevice) !=
      hipSuccess) {
    p.npass = 0;
    ctx->fft_plans[N] = p;
    return -1;
  }
  p.tw_off = ctx->fft_tab_used;
  p.post_off = ctx->fft_tab_used + p.M;
  p.ipre_off = ctx->fft_tab_used + p.M + 2ll * (p.M + 1);
  ctx->fft_tab_used += need;
  ctx->fft_plans[N] = p;
  *out = p;
  out->spec = ctx->fft_spec_enabled ? fft_spec_id(N, out->radix, out->npass, P) : 0;
  if (out->spec) out->rows_per_block = fft_spec_rows_per_block(out->spec);
  if (!out->spec && !ctx->fft_generic) return -1;   // the GEMM DCT (see dctae_ctx::fft_generic)
  return 0;
}

}  // namespace

// Encode plan: everything the launch sequence needs, cached on the inputs.
constexpr int kVariants = 3;  // 0 = generic FFT kernels, 1.. = dctae_fft2.hip specialisations

struct ChunkJob {
  int i0, i1;
  size_t desc_off, gp_off, rows_t_off, cols_t_off;
  size_t fr_off[kVariants], fc_off[kVariants];
  int n_fr[kVariants], n_fc[kVariants];
  int64_t tw_off[kVariants], post_off_r[kVariants], tw_off_c[kVariants], post_off_c[kVariants];
  int n_rows_tiles, n_cols_tiles;
  size_t pc_off;      // k_fft_cols7 list: the spec-1 images of the job (one tile-column count qw)
  int n_pc, pc_qw;
  size_t pb_off;      // k_cols512b list: the band-layout images of the job
  int n_pb;
  int max_T, any_gemm_rows, any_gemm_cols, fold_t, any_bs_cols;
  size_t ipt_off;            // k_rgb_to_ipt blocks (local image, first group)
  int n_ipt;
  size_t fold_off;           // local indices of the images whose T k_fold_t folds
  int n_fold;
  int64_t fold_max_hw;
  size_t br_off[4], bc_off[4];   // Bluestein row / column blocks per L = 256 .. 2048
  int n_br[4], n_bc[4];
  int64_t max_hw;
  size_t lds_rows, lds_cols;
  int64_t amax_off;   // k_gemm_h2: |max| bits per image (IPT, T) in the workspace, floats
  int h2;             // the job's GEMMs on k_gemm_h2
  size_t epi_off;     // k_tile_epilogue_p blocks (local image, 3 h + c) of the images with Y in the workspace
  int n_epi;
  size_t fused_t_off;  // k_rows_fused tiles (row problem, row-pair block)
  int n_fused_tiles, any_fused;
};

struct EncPlan {
  uint64_t id = 0;
  PlanBuf pb;
  std::vector<ChunkJob> jobs;
  size_t all_desc_off = 0;   // every image, global token offsets (sort_pack)
  int n_img = 0, max_T = 1;
  int64_t n_tok = 0;
  size_t rowlen_off = 0, plans_off = 0;
  size_t ws_need = 0, st_need = 0;
  int ncb = 0;
  bool any_pad = true;   // some packed row shorter than max_seq_len
  bool uniform = false;  // every image of the call has the same (H, W)
};

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" {

int dctae_abi_version(void) { return DCTAE_ABI_VERSION; }

int dctae_ctx_create(int device, dctae_ctx** out) {
  if (!out) return DCTAE_EINVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    g_err = "no HIP device";
    return DCTAE_EHIP;
  }
  if (device < 0 || device >= n) {
    g_err = "bad device index";
    return DCTAE_EINVAL;
  }
  if (hipSetDevice(device) != hipSuccess) {
    g_err = "hipSetDevice failed";
    return DCTAE_EHIP;
  }
  dctae_ctx* c = new dctae_ctx();
  c->device = device;
  default_colors(c->cm);
  if (hipEventCreateWithFlags(&c->plan_evt, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->done_evt, kDoneEvtFlags) != hipSuccess ||
      hipMalloc((void**)&c->err_dev, sizeof(int)) != hipSuccess || hipMemset(c->err_dev, 0, sizeof(int)) != hipSuccess) {
    g_err = "context allocation failed";
    delete c;
    return DCTAE_EHIP;
  }
  c->fft_tab_cap = 1 << 20;
  {
    const char* e = getenv("DCTAE_WS_POISON");
    c->ws_poison = e && e[0] == '1';
  }
  if (hipMalloc((void**)&c->fft_tab, c->fft_tab_cap * sizeof(float2)) != hipSuccess) {
    g_err = "FFT table allocation failed";
    delete c;
    return DCTAE_EHIP;
  }
  c->lds_limit = fft_kernel_setup(device);
  {
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0) c->n_cu = cu;
    hipGetLastError();
  }
  hipEventRecord(c->plan_evt, 0);
  *out = c;
  return 0;
}

int dctae_ctx_destroy(dctae_ctx* ctx) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  hipDeviceSynchronize();
  for (auto& kv : ctx->dct) hipFree(kv.second);
  for (auto& kv : ctx->dct_x3) {
    hipFree(kv.second.d);
    hipFree(kv.second.dh);
  }
  if (ctx->ws) hipFree(ctx->ws);
  if (ctx->stage) hipFree(ctx->stage);
  if (ctx->plan_host) hipHostFree(ctx->plan_host);
  if (ctx->plan_dev) hipFree(ctx->plan_dev);
  if (ctx->err_dev) hipFree(ctx->err_dev);
  if (ctx->fft_tab) hipFree(ctx->fft_tab);
  if (ctx->st_ws) hipFree(ctx->st_ws);
  if (ctx->vq_ws) hipFree(ctx->vq_ws);
  if (ctx->proj_ws) hipFree(ctx->proj_ws);
  delete ctx->enc_plan;
  for (auto& p : ctx->pending) {
    hipEventDestroy(p.a);
    hipEventDestroy(p.b);
  }
  for (auto e : ctx->evt_pool) hipEventDestroy(e);
  hipEventDestroy(ctx->plan_evt);
  hipEventDestroy(ctx->done_evt);
  if (ctx->side) {
    hipStreamDestroy(ctx->side);
    hipEventDestroy(ctx->side_in);
    hipEventDestroy(ctx->side_out);
  }
  delete ctx;
  return 0;
}

const char* dctae_last_error(dctae_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

// Python passes the reference's exact fp32 colour matrices (util.py:40-41, 91)
int dctae_set_color_matrices(dctae_ctx* ctx, const float* rgb2lms, const float* lms2ipt, const float* ipt2lms,
                             const float* lms2rgb) {
  if (!ctx) return DCTAE_EINVAL;
  std::memcpy(ctx->cm.rgb2lms, rgb2lms, 36);
  std::memcpy(ctx->cm.lms2ipt, lms2ipt, 36);
  std::memcpy(ctx->cm.ipt2lms, ipt2lms, 36);
  std::memcpy(ctx->cm.lms2rgb, lms2rgb, 36);
  return 0;
}

int dctae_set_workspace_limit(dctae_ctx* ctx, int64_t bytes) {
  if (!ctx || bytes < (1 << 20)) return DCTAE_EINVAL;
  ctx->ws_limit = bytes;
  return 0;
}

int dctae_set_fft(dctae_ctx* ctx, int enable) {
  if (!ctx) return DCTAE_EINVAL;
  ctx->fft_enabled = enable != 0;
  return 0;
}

int dctae_set_chunk_bytes(dctae_ctx* ctx, int64_t bytes) {
  if (!ctx || bytes < (1 << 20)) return DCTAE_EINVAL;
  ctx->chunk_bytes = bytes;
  return 0;
}

int dctae_set_option(dctae_ctx* ctx, const char* key, int64_t value) {
  if (!ctx || !key) return DCTAE_EINVAL;
  const std::string k(key);
  if (k == "fft") ctx->fft_enabled = value != 0;
  else if (k == "fft_spec") ctx->fft_spec_enabled = value != 0;
  else if (k == "bluestein") ctx->bluestein = value != 0;
  else if (k == "chunk_bytes" && value >= (1 << 20)) ctx->chunk_bytes = value;
  else if (k == "xcd_order") ctx->xcd_order = value != 0;
  else if (k == "workspace_limit" && value >= (1 << 20)) ctx->ws_limit = value;
#ifdef DCTAE_PROFILING
  // profiling switches: they make dctae_encode write WRONG outputs (shared T
  // slots, skipped loads / stores) and exist only in a profiling build
  // (`make PROFILING=1`, a separate library), never in the shipped one
  else if (k == "t_alias" && value >= 0) ctx->t_alias = (int)value;
  else if (k == "bs_ablate" && value >= 0 && value <= 7) ctx->bs_ablate = (int)value;
  else if (k == "gate" && value >= 0 && value <= 6) ctx->gate = (int)value;
#else
  else if (k == "t_alias" || k == "bs_ablate" || k == "gate")
    return fail(ctx, DCTAE_EUNSUP, "option " + k + " exists only in a profiling build (make PROFILING=1)");
#endif
  else if (k == "rows_kernel" && (value == 2 || value == 4)) ctx->rows_kernel = (int)value;
  else if (k == "cols512b") ctx->cols512b = value != 0;
  else if (k == "cols_wide") ctx->cols_wide = value != 0;
  else if (k == "sort_overlap") ctx->sort_overlap = value != 0;
  else if (k == "halves") ctx->halves = value != 0;
  else if (k == "fft_decode") ctx->fft_decode = value != 0;
  else if (k == "dec_rows_kernel" && (value == 2 || value == 3)) ctx->dec_rows_kernel = (int)value;
  else if (k == "dec_cols_kernel" && (value == 1 || value == 2)) ctx->dec_cols_kernel = (int)value;
  else if (k == "sort_kernel" && (value == 1 || value == 2)) ctx->sort_kernel = (int)value;
  else if (k == "gemm_x3") ctx->gemm_x3 = value != 0;
  else if (k == "gemm_h2") ctx->gemm_h2 = value != 0;
  else if (k == "gemm_dma") ctx->gemm_dma = value != 0;
  else if (k == "rows_fused") ctx->rows_fused = value != 0;
  else if (k == "cols_dma") ctx->cols_dma = value != 0;
  else if (k == "lfq_ws") ctx->lfq_ws = value != 0;
  else if (k == "fft_odd") ctx->fft_odd = value != 0;   // checked before the plan cache (fft_plan_for)
  else if (k == "fft_generic") ctx->fft_generic = value != 0;
  else if (k == "tperm") ctx->tperm = value != 0;
  else if (k == "ws_poison") ctx->ws_poison = value != 0;
  else return fail(ctx, DCTAE_EINVAL, "unknown option or bad value: " + k);
  return 0;
}

int dctae_norm_thresholds(dctae_ctx* ctx, const dctae_norm* norm, int64_t n, float* thr_dev, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!norm || !norm->median_dev || !norm->b_dev || !thr_dev || n < 0)
    return fail(ctx, DCTAE_EINVAL, "bad threshold arguments");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipMemsetAsync(ctx->err_dev, 0, sizeof(int), s));
  launch_norm_thresholds(norm->median_dev, norm->b_dev, n, norm->eps, norm->min_val, norm->max_val, thr_dev,
                         ctx->err_dev, s);
  HIPCHK(ctx, hipGetLastError());
  int h = 0;
  HIPCHK(ctx, hipMemcpyAsync(&h, ctx->err_dev, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  HIPCHK(ctx, hipMemsetAsync(ctx->err_dev, 0, sizeof(int), s));
  if (h) return fail(ctx, DCTAE_EUNSUP, "negative PatchNorm std: thresholds undefined (use thr_dev = NULL)");
  return 0;
}

int dctae_set_timing(dctae_ctx* ctx, int enable) {
  if (!ctx) return DCTAE_EINVAL;
  ctx->timing = enable != 0;
  return 0;
}

int dctae_timing_collect(dctae_ctx* ctx) {
  if (!ctx) return DCTAE_EINVAL;
  for (auto& p : ctx->pending) {
    float ms = 0;
    HIPCHK(ctx, hipEventSynchronize(p.b));
    HIPCHK(ctx, hipEventElapsedTime(&ms, p.a, p.b));
    TimingEntry* e = nullptr;
    for (auto& t : ctx->totals)
      if (t.name == p.name) e = &t;
    if (!e) {
      ctx->totals.push_back({p.name, 0.0, 0});
      e = &ctx->totals.back();
    }
    e->ms += ms;
    e->launches += 1;
    ctx->evt_pool.push_back(p.a);
    ctx->evt_pool.push_back(p.b);
  }
  ctx->pending.clear();
  return 0;
}

int dctae_timing_get(dctae_ctx* ctx, int idx, const char** name, double* total_ms, int64_t* launches) {
  if (!ctx || idx < 0 || idx >= (int)ctx->totals.size()) return DCTAE_EINVAL;
  if (name) *name = ctx->totals[idx].name.c_str();
  if (total_ms) *total_ms = ctx->totals[idx].ms;
  if (launches) *launches = ctx->totals[idx].launches;
  return 0;
}

int dctae_timing_reset(dctae_ctx* ctx) {
  if (!ctx) return DCTAE_EINVAL;
  dctae_timing_collect(ctx);
  ctx->totals.clear();
  return 0;
}

int dctae_check_device_errors(dctae_ctx* ctx, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  int h = 0;
  HIPCHK(ctx, hipMemcpyAsync(&h, ctx->err_dev, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  HIPCHK(ctx, hipMemsetAsync(ctx->err_dev, 0, sizeof(int), s));
  if (h & 1) return fail(ctx, DCTAE_EINVAL, "channel/position index out of range of the PatchNorm tables");
  if (h & 2) return fail(ctx, DCTAE_EINVAL, "batched_image_ids entry has no image (patch_sizes mismatch)");
  if (h & 4) return fail(ctx, DCTAE_EINVAL, "token position outside its image's patch grid");
  if (h & 16) return fail(ctx, DCTAE_EINVAL, "VectorQuantize index out of range of the codebook");
  return 0;
}

int dctae_synth_images(dctae_ctx* ctx, uint64_t seed, int64_t first_index, int32_t n_img, int32_t H, int32_t W,
                       float* rgb_dev, void* stream) {
  if (!ctx || !rgb_dev || n_img < 0 || H < 1 || W < 1) return fail(ctx, DCTAE_EINVAL, "bad synth args");
  if (n_img == 0) return 0;
  Timer t(ctx, (hipStream_t)stream, "synth");
  launch_synth(seed, first_index, n_img, H, W, rgb_dev, (hipStream_t)stream);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

// The encode engine.  Full mode (pack != NULL): packed DCTPatches outputs.
// Token mode (pack == NULL): spectrum tokens in flat order (tokens_dev /
// scores_dev at tok_off).  Per image the row DCT (length W) and the column
// DCT (length H) each run on the FFT kernels when the length has a plan, else
// on the MFMA GEMM; the intermediate T[c][y][kx] (3, H, Kw) is shared.
static int build_encode_plan(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images* imgs,
                             const dctae_packing* pack, bool full, int ncb, bool want_raw, bool want_norm,
                             const int64_t* tok_off_user, EncPlan& E) {
  const int n = imgs->n_img;
  const int P = cfg->patch_size, PP = P * P, S = cfg->max_seq_len;
  int rc;
  std::vector<ImgDesc> D(n);
  std::vector<FftPlan> plans;
  std::map<int, int> plan_idx;
  auto plan_of = [&](int N) -> int {
    auto it = plan_idx.find(N);
    if (it != plan_idx.end()) return it->second;
    FftPlan p;
    int idx = -1;
    if (fft_plan_for(ctx, N, P, &p) == 0 || bs_plan_for(ctx, N, &p) == 0) {
      idx = (int)plans.size();
      plans.push_back(p);
    }
    plan_idx[N] = idx;
    return idx;
  };
  for (int i = 0; i < n; ++i) {
    if ((rc = describe(ctx, cfg, imgs->hw[2 * i], imgs->hw[2 * i + 1], D[i]))) return rc;
    D[i].rgb_off = imgs->img_off[i];
    if (full) {
      D[i].row = pack->row[i];
      D[i].col = pack->col[i];
      D[i].k = pack->k[i];
      D[i].local_id = pack->local_id[i];
      if (D[i].k < 1 || D[i].k > D[i].T || D[i].k > S)
        return fail(ctx, DCTAE_EINVAL, "image " + std::to_string(i) + ": k out of range (FE:429-435)");
      if (D[i].row < 0 || D[i].row >= pack->n_rows || D[i].col < 0 || D[i].col + D[i].k > S)
        return fail(ctx, DCTAE_EINVAL, "image " + std::to_string(i) + ": packed span outside (rows, S)");
    }
    D[i].plan_w = plan_of(D[i].W);
    D[i].plan_h = plan_of(D[i].H);
    D[i].bs = (D[i].plan_w >= 0 && plans[D[i].plan_w].kind == 1 ? 1 : 0) |
              (D[i].plan_h >= 0 && plans[D[i].plan_h].kind == 1 ? 2 : 0);
    D[i].tperm = ctx->tperm && D[i].plan_w < 0 && D[i].plan_h < 0;
    // band layout: rows on k_rows512pk (Kw = 448) and columns on k_cols512b (Kh = 448)
    D[i].tband = ctx->cols512b && ctx->rows_kernel == 4 && cfg->max_patch_w == 32 && cfg->max_patch_h == 32 &&
                 D[i].H == 512 && D[i].W == 512 && D[i].Kh == 448 && D[i].Kw == 448 && D[i].bs == 0 && D[i].plan_w >= 0 &&
                 plans[D[i].plan_w].spec == 1 && D[i].plan_h >= 0 && plans[D[i].plan_h].spec == 1;
    // packed encodes of band images: item-major token staging (stage_pos; the
    // staging is internal there, while dctae_spectrum_tokens hands it out in flat order)
    if (full && D[i].tband) D[i].tband |= 2;
  }
  if (full)
    for (int r = 0; r < pack->n_rows; ++r)
      if (pack->row_len[r] < 0 || pack->row_len[r] > S) return fail(ctx, DCTAE_EINVAL, "row_len out of range");
  // chunks: FFT images are grouped so the intermediate T of a chunk stays in
  // the 256 MiB Infinity Cache between the row and column kernels
  auto ws_of = [&](const ImgDesc& d) {
    int64_t w = 3ll * d.Kw * d.H + 64;
    if (d.plan_w < 0) w += 3ll * d.H * d.W + 64;
    if (d.plan_h < 0 || (d.bs & 2)) w += 3ll * d.Kh * d.Kw + 64;
    return w * 4;
  };
  auto st_of = [&](const ImgDesc& d) {
    return (int64_t)d.T * (4 + 2 * ncb + (want_raw && full ? 4 * PP : 0) + (want_norm ? 4 * PP : 0));
  };
  for (int i = 0; i < n;) {
    ChunkJob j{};
    j.i0 = i;
    int64_t wsb = 0;
    while (i < n) {
      const int64_t w = ws_of(D[i]);
      const bool fft = D[i].plan_w >= 0 && D[i].plan_h >= 0;
      const int64_t cap = fft ? std::min<int64_t>(ctx->chunk_bytes, ctx->ws_limit) : ctx->ws_limit;
      if (i > j.i0 && wsb + w > cap) break;
      wsb += w;
      ++i;
    }
    j.i1 = i;
    E.jobs.push_back(j);
  }
  const int rows_cap = P * std::max(cfg->max_patch_h, cfg->max_patch_w);
  std::vector<GemmProblem> probs;
  int64_t tok = 0;
  for (auto& j : E.jobs) {
    int64_t wsf = 0;
    j.max_T = 1;
    j.max_hw = 1;
    auto up = [](int64_t v) { return (v + 63) & ~63ll; };  // 256-byte aligned regions (float4 strip loads)
    for (int i = j.i0; i < j.i1; ++i) {
      ImgDesc& d = D[i];
      if (ctx->t_alias > 0 && i - j.i0 >= ctx->t_alias) {   // profiling: T slots shared (wrong output)
        d.ws_t = D[j.i0 + (i - j.i0) % ctx->t_alias].ws_t;
        d.ws_p = d.ws_y = wsf;
        d.tok_off = full ? tok : tok_off_user[i];
        tok += d.T;
        j.max_T = std::max(j.max_T, d.T);
        j.max_hw = std::max<int64_t>(j.max_hw, (int64_t)d.H * d.W);
        continue;
      }
      d.ws_t = wsf;
      wsf += up(3ll * d.Kw * d.H);
      d.ws_p = wsf;
      if (d.plan_w < 0) wsf += up(3ll * d.H * d.W);
      d.ws_y = wsf;
      if (d.plan_h < 0 || (d.bs & 2)) wsf += up(3ll * d.Kh * d.Kw);
      d.tok_off = full ? tok : tok_off_user[i];
      tok += d.T;
      j.max_T = std::max(j.max_T, d.T);
      j.max_hw = std::max<int64_t>(j.max_hw, (int64_t)d.H * d.W);
    }
    j.amax_off = wsf;
    wsf += up(3ll * (j.i1 - j.i0) + 9);   // |max| pairs, then k_rows_fused's per-image flags, "any" word, 8 tile counters
    E.ws_need = std::max<size_t>(E.ws_need, (size_t)wsf * 4);
    E.max_T = std::max(E.max_T, j.max_T);
  }
  E.n_tok = tok;
  E.n_img = n;
  E.uniform = true;
  for (int i = 1; i < n; ++i) E.uniform = E.uniform && D[i].H == D[0].H && D[i].W == D[0].W;
  {
    int64_t st = 0;
    for (int i = 0; i < n; ++i) st += st_of(D[i]);
    E.st_need = (size_t)st + 4096;
  }
  if ((rc = ensure_ws(ctx, std::max<size_t>(E.ws_need, 256), std::max<size_t>(E.st_need, 256)))) return rc;
  float* ws = ctx->ws;
  for (auto& j : E.jobs) {
    j.desc_off = E.pb.add(D.data() + j.i0, j.i1 - j.i0);
    const size_t p0 = probs.size();
    std::vector<TileRef> rt, ct, ft;
    std::vector<int2> fr[kVariants];
    std::vector<int4> fc[kVariants];
    std::vector<int2> br[4];
    std::vector<int4> bc[4];
    std::vector<int32_t> fold;
    std::vector<int2> ipt;
    std::vector<int32_t> pc, pb;
    std::vector<int2> epi;
    int pc_qw = 0;
    bool pc_ok = cfg->max_patch_h <= 32;   // k_fft_cols7 keeps Kh <= 448 rows
    j.lds_rows = j.lds_cols = 0;
    for (int i = j.i0; i < j.i1; ++i) {
      const ImgDesc& d = D[i];
      const int li = i - j.i0;
      if (d.plan_w < 0) {
        // T[c][y][kx] = sum_x CW[kx][x] * IPT[c][y][x], folded: even kx over
        // IPT[x] + IPT[W-1-x], odd kx over IPT[x] - IPT[W-1-x] (half the flops)
        const size_t q0 = probs.size();
        for (int par = 0; par < 2; ++par) {
          const int M = par ? d.Kw / 2 : (d.Kw + 1) / 2, K = par ? d.W / 2 : (d.W + 1) / 2;
          if (M == 0) continue;
          const float* CW;
          if ((rc = dct_matrix(ctx, d.W, std::min(d.W, rows_cap), &CW, par))) return rc;
          // A: the folded IPT (k_rgb_to_ipt), u at x < ceil(W/2), v after it; B:
          // the half DCT matrix (shared by the channels).  T rows y are the GEMM
          // rows, so a wave's stores run along kx (the accumulator's lane-fast
          // dimension; with the roles swapped they strided by Kw floats)
          // parity-planar T (tperm: the columns are GEMMs too): each parity's
          // outputs are contiguous runs (interleaved stores made every line
          // twice-written: 4.4 GB of writes for 2.7 GB of T on config 4)
          GemmProblem g = d.tperm ? gemm(ws + d.ws_p + (par ? (d.W + 1) / 2 : 0), (int64_t)d.H * d.W, d.W, 1, CW, 0,
                                         K, 1, ws + d.ws_t + (par ? (d.Kw + 1) / 2 : 0), (int64_t)d.Kw * d.H, d.Kw,
                                         1, d.H, M, K, 3)
                                  : gemm(ws + d.ws_p + (par ? (d.W + 1) / 2 : 0), (int64_t)d.H * d.W, d.W, 1, CW, 0,
                                         K, 1, ws + d.ws_t + par, (int64_t)d.Kw * d.H, d.Kw, 2, d.H, M, K, 3);
          attach_x3(ctx, g);
          uint32_t* am = reinterpret_cast<uint32_t*>(ws + j.amax_off) + 2 * li;
          g.amax = am;                               // k_rgb_to_ipt's |max| of the folded IPT
          g.omax = d.plan_h < 0 ? am + 1 : nullptr;  // T's |max| for the column GEMM
          g.pad2 = li;                               // k_rows_fused: the image and the parity
          g.pad3 = par;
          probs.push_back(g);
        }
        // k_rows_fused (colour transform + folds + row GEMM in one pass) for the
        // tperm images whose parity matrices are cached pre-split (both forms:
        // the fix-up runs the bf16 one) and fit its 256 output columns
        bool fz = ctx->rows_fused && d.tperm && probs.size() == q0 + 2;   // both parities, consecutive
        for (size_t q = q0; q < probs.size(); ++q) fz = fz && probs[q].Xh && probs[q].N <= fused_max_n();
        if (fz)
          for (int rb = 0; rb * fused_pairs_per_block() < (d.H + 1) / 2; ++rb) ft.push_back(TileRef{(int)(q0 - p0), rb});
        else
          for (size_t q = q0; q < probs.size(); ++q) add_tiles(rt, (int)(q - p0), probs[q]);
        if (fz) {
          j.any_fused = 1;
        } else {
          j.any_gemm_rows = 1;
          // k_rgb_to_ipt's (x, y)-mirrored pixel groups of this image
          const int64_t ng = (int64_t)(d.plan_h < 0 ? (d.H + 1) / 2 : d.H) * ((d.W + 1) / 2);
          for (int64_t g0 = 0; g0 < ng; g0 += rgb_to_ipt_groups_per_block()) ipt.push_back(make_int2(li, (int)g0));
        }
      } else if (d.bs & 1) {
        const int L = plans[d.plan_w].bs_L, rpb = bs_rows_per_block(L);
        for (int y0 = 0; y0 < d.H; y0 += rpb) br[bs_lidx(L)].push_back(make_int2(li, y0));
      } else {
        const FftPlan& p = plans[d.plan_w];
        for (int y0 = 0; y0 < d.H; y0 += p.rows_per_block) fr[p.spec].push_back(make_int2(li, y0));
        if (p.spec) {
          j.tw_off[p.spec] = p.tw_off;
          j.post_off_r[p.spec] = p.post_off;
        } else {
          j.lds_rows = std::max<size_t>(j.lds_rows, (size_t)2 * p.rows_per_block * 3 * (2 * p.M + 1) * 4);
        }
      }
      if (d.plan_h < 0 || (d.bs & 2))   // Y in the workspace: the tile epilogue's (tile row, channel) blocks
        for (int h = 0; h < d.qh; ++h)
          for (int c = 0; c < 3; ++c) epi.push_back(make_int2(li, 3 * h + c));
      if (d.plan_h < 0) {
        // Y[c][ky][kx] = sum_y CH[ky][y] * T[c][y][kx], folded along y as the rows
        for (int par = 0; par < 2; ++par) {
          const int M = par ? d.Kh / 2 : (d.Kh + 1) / 2, K = par ? d.H / 2 : (d.H + 1) / 2;
          if (M == 0) continue;
          const float* CH;
          if ((rc = dct_matrix(ctx, d.H, std::min(d.H, rows_cap), &CH, par))) return rc;
          // B: T folded along y (by the row GEMM of the y-folded IPT, or in place by
          // k_fold_t after FFT rows): u in rows m < ceil(H/2), v[m] in row H-1-m
          GemmProblem g = gemm(CH, 0, K, 1, ws + d.ws_t + (par ? (int64_t)(d.H - 1) * d.Kw : 0),
                               (int64_t)d.Kw * d.H, 1, par ? -(int64_t)d.Kw : d.Kw,
                               ws + d.ws_y + (int64_t)par * d.Kw, (int64_t)d.Kh * d.Kw, 2 * (int64_t)d.Kw, 1, M,
                               d.Kw, K, 3);
          attach_x3(ctx, g);
          g.amax = reinterpret_cast<uint32_t*>(ws + j.amax_off) + 2 * li + 1;   // T's |max| (row GEMM / k_fold_t)
          add_tiles(ct, (int)(probs.size() - p0), g);
          probs.push_back(g);
        }
        j.any_gemm_cols = 1;
        if (d.plan_w >= 0) {
          j.fold_t = 1;
          fold.push_back(li);
          j.fold_max_hw = std::max<int64_t>(j.fold_max_hw, (int64_t)d.H * d.W);
        }
      } else if (d.bs & 2) {
        const int L = plans[d.plan_h].bs_L, cpb = bs_cols_per_block(L);
        for (int c = 0; c < 3; ++c)
          for (int kx0 = 0; kx0 < d.Kw; kx0 += cpb) bc[bs_lidx(L)].push_back(make_int4(li, c, kx0, 0));
        j.any_bs_cols = 1;
      } else if (d.tband) {
        pb.push_back(li);
        j.tw_off_c[1] = plans[d.plan_h].tw_off;
        j.post_off_c[1] = plans[d.plan_h].post_off;
      } else {
        const FftPlan& p = plans[d.plan_h];
        // generic kernel: one tile column per block; specialised: groups of
        // up to 16 adjacent tile columns walked by one block
        const int G = 1;
        for (int c = 0; c < 3; ++c)
          for (int w = 0; w < d.qw; w += G) fc[p.spec].push_back(make_int4(li, c, w, std::min(G, d.qw - w)));
        if (p.spec == 1) {
          pc_ok = pc_ok && (pc.empty() || d.qw == pc_qw);
          pc_qw = d.qw;
          pc.push_back(li);
        }
        if (p.spec) {
          j.tw_off_c[p.spec] = p.tw_off;
          j.post_off_c[p.spec] = p.post_off;
        } else {
          j.lds_cols = std::max<size_t>(j.lds_cols, (size_t)2 * 2 * p.M * P * 4);
        }
      }
    }
    // k_gemm_h2 when every GEMM of the job has its shared matrix pre-split
    j.h2 = ctx->gemm_x3 && ctx->gemm_h2 && probs.size() > p0;
    for (size_t q = p0; q < probs.size(); ++q) j.h2 = j.h2 && probs[q].Xh != nullptr;
    j.gp_off = E.pb.add(probs.data() + p0, probs.size() - p0);
    if (ctx->xcd_order) {
      xcd_deal_tiles(rt, probs.data() + p0, 1);
      xcd_deal_tiles(ct, probs.data() + p0, 2);
      xcd_deal_tiles(ft, probs.data() + p0, 1);   // an image's blocks on one XCD: its two matrices in one L2
    }
    j.rows_t_off = E.pb.add(rt.data(), rt.size());
    j.fused_t_off = E.pb.add(ft.data(), ft.size());
    j.n_fused_tiles = (int)ft.size();
    j.cols_t_off = E.pb.add(ct.data(), ct.size());
    // XCD-aware order of the column blocks (speed only; any order is correct):
    // blocks b and b+8 are dealt to the same XCD, so give all the blocks of
    // one (image, channel) the same b % 8 and consecutive b / 8 — the 56-byte
    // row slices of neighbouring tile columns then share that XCD's L2 lines.
    if (ctx->xcd_order) {
      for (int v = 1; v < kVariants; ++v) {
        std::vector<int4>& L = fc[v];
        if (L.size() < 16) continue;
        // units = runs of blocks with the same (image, channel), in list order
        std::vector<std::pair<size_t, size_t>> units;
        for (size_t a0 = 0; a0 < L.size();) {
          size_t a1 = a0 + 1;
          while (a1 < L.size() && L[a1].x == L[a0].x && L[a1].y == L[a0].y) ++a1;
          units.push_back({a0, a1});
          a0 = a1;
        }
        std::vector<std::vector<int4>> lanes(8);
        for (size_t u = 0; u < units.size(); ++u)
          for (size_t a = units[u].first; a < units[u].second; ++a) lanes[u % 8].push_back(L[a]);
        std::vector<int4> out;
        out.reserve(L.size());
        size_t maxlen = 0;
        for (auto& l : lanes) maxlen = std::max(maxlen, l.size());
        for (size_t q = 0; q < maxlen; ++q)
          for (int x = 0; x < 8; ++x)
            if (q < lanes[x].size()) out.push_back(lanes[x][q]);
        L.swap(out);
      }
    }
    for (int v = 0; v < kVariants; ++v) {
      j.fr_off[v] = E.pb.add(fr[v].data(), fr[v].size());
      j.fc_off[v] = E.pb.add(fc[v].data(), fc[v].size());
      j.n_fr[v] = (int)fr[v].size();
      j.n_fc[v] = (int)fc[v].size();
    }
    j.ipt_off = E.pb.add(ipt.data(), ipt.size());
    j.n_ipt = (int)ipt.size();
    j.fold_off = E.pb.add(fold.data(), fold.size());
    j.n_fold = (int)fold.size();
    for (int l = 0; l < 4; ++l) {
      j.br_off[l] = E.pb.add(br[l].data(), br[l].size());
      j.bc_off[l] = E.pb.add(bc[l].data(), bc[l].size());
      j.n_br[l] = (int)br[l].size();
      j.n_bc[l] = (int)bc[l].size();
    }
    j.n_rows_tiles = (int)rt.size();
    j.n_cols_tiles = (int)ct.size();
    // all spec-1 column items of the job in one persistent launch, when their qw agree
    j.n_pc = (pc_ok && (int)pc.size() * 3 * pc_qw == (int)fc[1].size()) ? (int)pc.size() : 0;
    j.pc_qw = pc_qw;
    j.pc_off = E.pb.add(pc.data(), pc.size());
    j.n_pb = (int)pb.size();
    j.pb_off = E.pb.add(pb.data(), pb.size());
    j.n_epi = (int)epi.size();
    j.epi_off = E.pb.add(epi.data(), epi.size());
  }
  E.plans_off = E.pb.add(plans.data(), plans.size());
  E.all_desc_off = E.pb.add(D.data(), D.size());
  if (full && pack->n_rows > 0) E.rowlen_off = E.pb.add(pack->row_len, pack->n_rows);
  E.any_pad = false;
  if (full)
    for (int r = 0; r < pack->n_rows; ++r) E.any_pad = E.any_pad || pack->row_len[r] < S;
  E.ncb = ncb;
  return 0;
}

static int encode_impl(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images* imgs,
                       const dctae_packing* pack, const dctae_norm* norm, const dctae_lfq* lfq,
                       const dctae_packed_out* out, const int64_t* tok_off_user, float* tokens_dev,
                       float* scores_dev, hipStream_t s, const float* proj_w = nullptr,
                       const float* proj_b = nullptr) {
  int rc = check_cfg(ctx, cfg);
  if (rc) return rc;
  if (!imgs || imgs->n_img < 0 || (imgs->n_img > 0 && (!imgs->rgb_dev || !imgs->img_off || !imgs->hw)))
    return fail(ctx, DCTAE_EINVAL, "bad image descriptor");
  const bool full = (pack != nullptr);
  const int n = imgs->n_img;
  const int P = cfg->patch_size, PP = P * P;
  const bool want_codes = full && out && out->codes_dev;
  if (full) {
    if (!out || !out->positions_dev || !out->channels_dev || !out->image_ids_dev || !out->key_pad_dev)
      return fail(ctx, DCTAE_EINVAL, "packed outputs positions/channels/image_ids/key_pad are required");
    if ((want_codes || out->patches_dev) && !norm) return fail(ctx, DCTAE_EINVAL, "codes/patches need PatchNorm tables");
    if (want_codes && !proj_w && (rc = check_lfq(ctx, lfq, PP))) return rc;
    if (proj_w && (!want_codes || !lfq || lfq->codebook_dim < 1 || lfq->codebook_dim > 16 ||
                   lfq->num_codebooks < 1 || lfq->num_codebooks > 64 || PP % 4 != 0 ||
                   lfq->codebook_dim * lfq->num_codebooks > 256 || ((uintptr_t)proj_w & 15)))
      return fail(ctx, DCTAE_EUNSUP, "fused LFQ projections: codes output, codebook_dim <= 16, ncb * cd <= 256, "
                                     "P*P % 4 == 0, 16-byte aligned weights");
    if (pack->n_rows < 0 || (n > 0 && (!pack->row || !pack->col || !pack->k || !pack->local_id)) ||
        (pack->n_rows > 0 && !pack->row_len))
      return fail(ctx, DCTAE_EINVAL, "bad packing descriptor");
  }
  if (norm && (!norm->median_dev || !norm->b_dev)) return fail(ctx, DCTAE_EINVAL, "PatchNorm tables are NULL");
  const int ncb = want_codes ? lfq->num_codebooks : 0;
  const bool want_raw = (full && out->raw_patches_dev) || (!full && tokens_dev);
  // LFQ with projections: the column epilogues stage the PatchNorm output,
  // dctae_lfq_project_in turns the staged tokens into staged u16 codes, and the
  // sort / pack gathers those as usual
  const bool want_norm = full && (out->patches_dev || proj_w);

  // ---- plan cache key: every input that shapes the launch sequence
  std::vector<int64_t> key;
  key.reserve(16 + 6ll * n + (full ? pack->n_rows : 0));
  key.insert(key.end(), {(int64_t)full, n, P, cfg->max_patch_h, cfg->max_patch_w, cfg->max_seq_len, ncb,
                         (int64_t)want_raw, (int64_t)want_norm, ctx->chunk_bytes, ctx->ws_limit,
                         (int64_t)ctx->fft_enabled * 2 + (int64_t)ctx->fft_spec_enabled + 4 * ctx->bluestein +
                             64 * ctx->t_alias + 1024 * ctx->xcd_order + 2048 * ctx->gemm_x3 +
                             4096 * ctx->cols512b + 8192 * ctx->rows_kernel + 65536 * ctx->gemm_h2 +
                             131072 * ctx->fft_odd + 262144 * ctx->fft_generic + 524288 * ctx->tperm +
                             1048576 * ctx->rows_fused,
                         (int64_t)(intptr_t)ctx->ws});
  for (int i = 0; i < n; ++i) {
    key.push_back(imgs->img_off[i]);
    key.push_back(((int64_t)imgs->hw[2 * i] << 32) | (uint32_t)imgs->hw[2 * i + 1]);
    if (full) {
      key.push_back(((int64_t)pack->row[i] << 32) | (uint32_t)pack->col[i]);
      key.push_back(((int64_t)pack->k[i] << 32) | (uint32_t)pack->local_id[i]);
    } else {
      key.push_back(tok_off_user[i]);
    }
  }
  if (full) {
    key.push_back(pack->n_rows);
    for (int r = 0; r < pack->n_rows; ++r) key.push_back(pack->row_len[r]);
  }
  if (!ctx->enc_plan || key != ctx->enc_key) {
    EncPlan* E = new EncPlan();
    E->id = ++ctx->plan_counter;
    rc = build_encode_plan(ctx, cfg, imgs, pack, full, ncb, want_raw, want_norm, tok_off_user, *E);
    if (rc) {
      delete E;
      return rc;
    }
    // the workspace may have moved (ensure_ws) -> the ws pointer is part of the key
    key[12] = (int64_t)(intptr_t)ctx->ws;
    delete ctx->enc_plan;
    ctx->enc_plan = E;
    ctx->enc_key = key;
  }
  EncPlan& E = *ctx->enc_plan;
  if (proj_w && E.any_pad)
    return fail(ctx, DCTAE_EUNSUP, "fused LFQ projections need rows without padding (the pad token's codes)");
  order_after_previous(ctx, s);
  if ((rc = upload_plan(ctx, E.pb, s, E.id))) return rc;
  uint8_t* pd = ctx->plan_dev;
  const FftPlan* plans_d = (const FftPlan*)(pd + E.plans_off);

  EncParams ep = enc_params(cfg, norm, want_codes && !proj_w ? lfq : nullptr);
  if (norm && !want_norm) ep.thr = norm_thr(norm);
  PackSinks ps{};
  if (full) {
    ps.codes = out->codes_dev;
    ps.pos = out->positions_dev;
    ps.ch = out->channels_dev;
    ps.ids = out->image_ids_dev;
    ps.patches = out->patches_dev;
    ps.raw = out->raw_patches_dev;
    ps.scores = out->scores_dev;
    ps.key_pad = out->key_pad_dev;
    // rows filled to max_seq_len (e.g. one 512^2 image per row) have no pads:
    // the sort kernel writes their key_pad zeros, no k_pad_fill launch
    if (pack->n_rows > 0 && E.any_pad) {
      Timer t(ctx, s, "pad_fill");
      launch_pad_fill((const int32_t*)(pd + E.rowlen_off), pack->n_rows, ep, out->key_pad_dev, ps, s);
    }
  }
  // token staging for the whole call (flat token order, global offsets)
  TokenSinks sk{};
  if (full) {
    const int64_t nt = E.n_tok;
    uint8_t* st = ctx->stage;
    sk.scores = (float*)st;
    st += ((nt * 4 + 255) & ~255ll);
    if (ncb) {
      sk.codes = (uint16_t*)st;
      st += ((nt * 2 * ncb + 255) & ~255ll);
    }
    if (want_norm) {
      sk.norm = (float*)st;
      st += nt * 4 * PP;
    }
    if (out->raw_patches_dev) {
      sk.raw = (float*)st;
      st += nt * 4 * PP;
    }
  } else {
    sk.scores = scores_dev;
    sk.raw = tokens_dev;
  }
  EncParams epj = ep;
  if (!full) epj.median = nullptr;
  TokenSinks skc = sk;   // the column kernels' sinks (codes come from the projection kernel)
  if (proj_w) skc.codes = nullptr;
  // row half / column half of a chunk job on a stream
  auto gemm = [&](const ChunkJob& j, size_t tiles_off, int n_tiles, hipStream_t st, int share) {
    if (j.h2)
      launch_gemm_h2((const GemmProblem*)(pd + j.gp_off), (const TileRef*)(pd + tiles_off), n_tiles, st, share,
                     ctx->gemm_dma != 0, ctx->cols_dma != 0);
    else
      ctx_gemm(ctx, 3, (const GemmProblem*)(pd + j.gp_off), (const TileRef*)(pd + tiles_off), n_tiles, st, share);
  };
  auto do_rows = [&](const ChunkJob& j, hipStream_t st) {
    const ImgDesc* dd = (const ImgDesc*)(pd + j.desc_off);
    uint32_t* amax = reinterpret_cast<uint32_t*>(ctx->ws + j.amax_off);
    if (j.h2 || j.any_fused) hipMemsetAsync(amax, 0, 12 * (size_t)(j.i1 - j.i0) + 36, st);   // errors surface at hipGetLastError
    if (j.any_fused) {
      int* flags = reinterpret_cast<int*>(amax + 2 * (j.i1 - j.i0));
      {
        Timer t(ctx, st, "rows_fused");
        launch_rows_fused((const GemmProblem*)(pd + j.gp_off), (const TileRef*)(pd + j.fused_t_off), j.n_fused_tiles,
                          dd, imgs->rgb_dev, ctx->cm, amax, flags, j.i1 - j.i0, st, false);
      }
      Timer t(ctx, st, "rows_fixup");
      launch_rows_fused((const GemmProblem*)(pd + j.gp_off), (const TileRef*)(pd + j.fused_t_off), j.n_fused_tiles, dd,
                        imgs->rgb_dev, ctx->cm, amax, flags, j.i1 - j.i0, st, true);
    }
    if (j.any_gemm_rows) {
      {
        Timer t(ctx, st, "rgb_to_ipt");
        launch_rgb_to_ipt(dd, (const int2*)(pd + j.ipt_off), j.n_ipt, imgs->rgb_dev, ctx->ws, ctx->cm,
                          j.h2 ? amax : nullptr, st);
      }
      Timer t(ctx, st, "gemm_rows");
      gemm(j, j.rows_t_off, j.n_rows_tiles, st, 1);
    }
    for (int l = 0; l < 4; ++l)
      if (j.n_br[l]) {
        Timer t(ctx, st, "bs_rows");
        launch_bs_rows(kBsL[l], dd, plans_d, (const int2*)(pd + j.br_off[l]), j.n_br[l], imgs->rgb_dev, ctx->ws,
                       ctx->fft_tab, ctx->cm, st, ctx->bs_ablate);
      }
    if (j.n_fr[0]) {
      Timer t(ctx, st, "fft_rows");
      launch_fft_rows(dd, plans_d, (const int2*)(pd + j.fr_off[0]), j.n_fr[0], j.lds_rows, imgs->rgb_dev, ctx->ws,
                      ctx->fft_tab, ctx->cm, st);
    }
    for (int v = 1; v < kVariants; ++v)
      if (j.n_fr[v]) {
        Timer t(ctx, st, "fft_rows");
        if (v == 1 && ctx->rows_kernel == 4 && cfg->max_patch_w == 32)
          launch_rows512(dd, (const int2*)(pd + j.fr_off[v]), j.n_fr[v], imgs->rgb_dev, ctx->ws,
                         ctx->fft_tab + j.tw_off[v], ctx->fft_tab + j.post_off_r[v], ctx->cm, st);
        else
          launch_fft_rows_spec(v, dd, (const int2*)(pd + j.fr_off[v]), j.n_fr[v], imgs->rgb_dev, ctx->ws,
                               ctx->fft_tab + j.tw_off[v], ctx->fft_tab + j.post_off_r[v], ctx->cm, st);
      }
  };
  auto do_cols = [&](const ChunkJob& j, hipStream_t st) {
    const int nj = j.i1 - j.i0;
    const ImgDesc* dd = (const ImgDesc*)(pd + j.desc_off);
    if (j.any_gemm_cols) {
      if (j.fold_t) {
        Timer t(ctx, st, "fold_t");
        launch_fold_t(dd, (const int32_t*)(pd + j.fold_off), j.n_fold, j.fold_max_hw, ctx->ws,
                      j.h2 ? reinterpret_cast<uint32_t*>(ctx->ws + j.amax_off) : nullptr, st);
      }
      Timer t(ctx, st, "gemm_cols");
      gemm(j, j.cols_t_off, j.n_cols_tiles, st, 2);
    }
    for (int l = 0; l < 4; ++l)
      if (j.n_bc[l]) {
        Timer t(ctx, st, "bs_cols");
        launch_bs_cols(kBsL[l], dd, plans_d, (const int4*)(pd + j.bc_off[l]), j.n_bc[l], ctx->ws, ctx->fft_tab, st,
                       ctx->bs_ablate);
      }
    if (j.any_gemm_cols || j.any_bs_cols) {
      Timer t(ctx, st, "tile_epilogue");
      launch_tile_epilogue(dd, nj, j.max_T, ctx->ws, epj, skc, st, (const int2*)(pd + j.epi_off), j.n_epi);
    }
    if (j.n_fc[0]) {
      Timer t(ctx, st, "fft_cols");
      launch_fft_cols(dd, plans_d, (const int4*)(pd + j.fc_off[0]), j.n_fc[0], j.lds_cols, ctx->ws, ctx->fft_tab,
                      epj, skc, st);
    }
    if (j.n_pb) {
      Timer t(ctx, st, "fft_cols");
      launch_cols512b(dd, (const int*)(pd + j.pb_off), j.n_pb, ctx->ws, ctx->fft_tab + j.tw_off_c[1],
                      ctx->fft_tab + j.post_off_c[1], epj, skc, st, ctx->cols_wide != 0);
    }
    for (int v = 1; v < kVariants; ++v)
      if (j.n_fc[v]) {
        Timer t(ctx, st, "fft_cols");
        launch_fft_cols_spec(v, dd, (const int4*)(pd + j.fc_off[v]), j.n_fc[v], ctx->ws, ctx->fft_tab + j.tw_off_c[v],
                             ctx->fft_tab + j.post_off_c[v], epj, skc, st,
                             v == 1 && j.n_pc ? (const int*)(pd + j.pc_off) : nullptr, v == 1 ? j.n_pc : 0, j.pc_qw);
      }
  };
  // the pack's parameters (the projection kernel stages raw sign bits: the pack maps them, lfq_index_bits)
  EncParams eps = ep;
  if (proj_w) {
    eps.ncb = lfq->num_codebooks;
    eps.cb_dim = lfq->codebook_dim;
    uint64_t pos, neg;
    lfq_index_masks(lfq->codebook_scale, lfq->codebook_dim, &pos, &neg);
    eps.code_pos = (uint32_t)pos;
    eps.code_neg = (uint32_t)neg;
  }
  const ImgDesc* all_d = (const ImgDesc*)(pd + E.all_desc_off);
  // sort_overlap: one job of band images only -> columns in two halves, the
  // first half's sort / pack on the side stream while the second half's
  // columns run (the sort is latency-bound, the column kernel issue-bound)
  int sorted0 = 0;   // images [0, sorted0) packed on the side stream
  // once work is queued on the side stream, the caller's stream waits for it on
  // every exit (error returns included), so the next call's order_after_previous
  // covers it before the workspace is reused
  struct SideJoin {
    hipStream_t s = nullptr, side = nullptr;
    hipEvent_t e = nullptr;
    bool armed = false;
    void join() {
      if (!armed) return;
      armed = false;
      if (hipEventRecord(e, side) != hipSuccess || hipStreamWaitEvent(s, e, 0) != hipSuccess) hipStreamSynchronize(side);
    }
    ~SideJoin() { join(); }
  } side_join;
  const bool split = full && !proj_w && ctx->sort_overlap && E.jobs.size() == 1 && E.n_img >= 64 &&
                     E.jobs[0].n_pb == E.n_img && E.jobs[0].i0 == 0;
  // halves (option): see dctae_ctx::halves; hv = the plan kernel variant
  int hv = 0;
  if (full && !proj_w && ctx->halves && !split && E.jobs.size() == 1 && E.uniform && E.n_img >= 32) {
    const ChunkJob& j = E.jobs[0];
    bool ok = !j.any_gemm_rows && !j.any_gemm_cols && !j.any_bs_cols && j.n_pb == 0 && j.n_pc == 0 && j.n_fr[0] == 0 &&
              j.n_fc[0] == 0;
    for (int l = 0; l < 4; ++l) ok = ok && !j.n_br[l] && !j.n_bc[l];
    int vv = -1;
    for (int v = 1; v < kVariants; ++v)
      if (j.n_fr[v] || j.n_fc[v]) {
        if (vv < 0 && j.n_fr[v] && j.n_fc[v]) vv = v;
        else ok = false;
      }
    if (ok && vv >= 2 && j.n_fr[vv] % E.n_img == 0 && j.n_fc[vv] % E.n_img == 0) hv = vv;
  }
  if ((split || hv) && !ctx->side) {
    if (hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->side_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->side_out, hipEventDisableTiming) != hipSuccess)
      return fail(ctx, DCTAE_EHIP, "side stream allocation failed");
  }
  if (hv) {
    const ChunkJob& j = E.jobs[0];
    const ImgDesc* dd = (const ImgDesc*)(pd + j.desc_off);
    const int n_img = E.n_img, h = n_img / 2;
    const int rpi = j.n_fr[hv] / n_img, cpi = j.n_fc[hv] / n_img;   // blocks / items per image (image-major lists)
    const int2* rl = (const int2*)(pd + j.fr_off[hv]);
    const int4* cl = (const int4*)(pd + j.fc_off[hv]);
    auto rows = [&](int a, int m, hipStream_t st) {
      Timer t(ctx, st, "fft_rows");
      launch_fft_rows_spec(hv, dd, rl + (size_t)a * rpi, m * rpi, imgs->rgb_dev, ctx->ws, ctx->fft_tab + j.tw_off[hv],
                           ctx->fft_tab + j.post_off_r[hv], ctx->cm, st);
    };
    auto cols = [&](int a, int m, hipStream_t st) {
      Timer t(ctx, st, "fft_cols");
      launch_fft_cols_spec(hv, dd, cl + (size_t)a * cpi, m * cpi, ctx->ws, ctx->fft_tab + j.tw_off_c[hv],
                           ctx->fft_tab + j.post_off_c[hv], epj, skc, st, nullptr, 0, 0);
    };
    rows(0, h, s);
    HIPCHK(ctx, hipEventRecord(ctx->side_in, s));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->side, ctx->side_in, 0));
    side_join.s = s;
    side_join.side = ctx->side;
    side_join.e = ctx->side_out;
    side_join.armed = true;
    cols(0, h, ctx->side);
    {
      Timer t(ctx, ctx->side, "sort_pack");
      launch_sort_pack(all_d, h, next_pow2(E.max_T), eps, sk, ps, ctx->side, ctx->sort_kernel, E.max_T);
    }
    rows(h, n_img - h, s);
    cols(h, n_img - h, s);
    sorted0 = h;
  }
  bool gated = false;
#ifdef DCTAE_PROFILING
  if (ctx->gate && full && !proj_w && !hv && !split && E.jobs.size() == 1 && E.n_img >= 2 &&
      E.jobs[0].n_pb == E.n_img && E.jobs[0].n_fr[1] % E.n_img == 0 && ctx->rows_kernel == 4) {
    const ChunkJob& j = E.jobs[0];
    const ImgDesc* dd = (const ImgDesc*)(pd + j.desc_off);
    const int n_img = E.n_img, h = n_img / 2, rpi = j.n_fr[1] / n_img;
    const int2* rl = (const int2*)(pd + j.fr_off[1]);
    const int* cl = (const int*)(pd + j.pb_off);
    auto rows = [&](int a, int m, hipStream_t st) {
      Timer t(ctx, st, "fft_rows");
      launch_rows512(dd, rl + (size_t)a * rpi, m * rpi, imgs->rgb_dev, ctx->ws, ctx->fft_tab + j.tw_off[1],
                     ctx->fft_tab + j.post_off_r[1], ctx->cm, st);
    };
    auto cols = [&](int a, int m, hipStream_t st) {
      Timer t(ctx, st, "fft_cols");
      launch_cols512b(dd, cl + a, m, ctx->ws, ctx->fft_tab + j.tw_off_c[1], ctx->fft_tab + j.post_off_c[1], epj, skc,
                      st, false);
    };
    auto fork = [&]() -> int {
      HIPCHK(ctx, hipEventRecord(ctx->side_in, s));
      HIPCHK(ctx, hipStreamWaitEvent(ctx->side, ctx->side_in, 0));
      side_join.s = s;
      side_join.side = ctx->side;
      side_join.e = ctx->side_out;
      side_join.armed = true;
      return 0;
    };
    if (!ctx->side && (hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking) != hipSuccess ||
                       hipEventCreateWithFlags(&ctx->side_in, hipEventDisableTiming) != hipSuccess ||
                       hipEventCreateWithFlags(&ctx->side_out, hipEventDisableTiming) != hipSuccess))
      return fail(ctx, DCTAE_EHIP, "side stream allocation failed");
    switch (ctx->gate) {
      case 1: rows(0, n_img, s); break;
      case 2: cols(0, n_img, s); break;
      case 3:
      case 4:
        if (ctx->gate == 4) rows(0, h, s);
        if ((rc = fork())) return rc;
        cols(0, h, ctx->side);
        rows(h, n_img - h, s);
        side_join.join();
        if (ctx->gate == 4) cols(h, n_img - h, s);
        break;
      case 5: rows(h, n_img - h, s); break;
      case 6: cols(0, h, s); break;
    }
    gated = true;
    sorted0 = ctx->gate == 4 ? 0 : E.n_img;
  }
#endif
  for (const ChunkJob& j : E.jobs) {
    if (hv || gated) break;
    do_rows(j, s);
    if (!split) {
      do_cols(j, s);
      continue;
    }
    const ImgDesc* dd = (const ImgDesc*)(pd + j.desc_off);
    const int* list = (const int*)(pd + j.pb_off);
    const int h = j.n_pb / 2;
    {
      Timer t(ctx, s, "fft_cols");
      launch_cols512b(dd, list, h, ctx->ws, ctx->fft_tab + j.tw_off_c[1], ctx->fft_tab + j.post_off_c[1], epj, skc, s,
                      ctx->cols_wide != 0);
    }
    HIPCHK(ctx, hipEventRecord(ctx->side_in, s));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->side, ctx->side_in, 0));
    side_join.s = s;
    side_join.side = ctx->side;
    side_join.e = ctx->side_out;
    side_join.armed = true;
    launch_sort_pack(all_d, h, next_pow2(E.max_T), eps, sk, ps, ctx->side, ctx->sort_kernel, E.max_T);
    {
      Timer t(ctx, s, "fft_cols");
      launch_cols512b(dd, list + h, j.n_pb - h, ctx->ws, ctx->fft_tab + j.tw_off_c[1], ctx->fft_tab + j.post_off_c[1],
                      epj, skc, s, ctx->cols_wide != 0);
    }
    sorted0 = h;
  }
  if (proj_w && E.n_tok > 0) {
    Timer t(ctx, s, "lfq_project_in");
    if ((rc = proj_scratch(ctx, lfq->codebook_dim * lfq->num_codebooks, PP))) return rc;
    // the staged tokens are PatchNorm outputs, clamped to [min_val, max_val]
    // (patchnorm.py:163): the fp16 projection's operand bound
    const float xb = ctx->gemm_h2 ? std::max(std::fabs(norm->min_val), std::fabs(norm->max_val)) : 0.0f;
    launch_lfq_project_in16(sk.norm, E.n_tok, PP, proj_w, proj_b, lfq->codebook_dim, lfq->num_codebooks, sk.codes,
                            ctx->proj_ws, s, xb, ctx->lfq_ws != 0);
  }
  if (full && E.n_img > sorted0) {
    Timer t(ctx, s, "sort_pack");
    launch_sort_pack(all_d + sorted0, E.n_img - sorted0, next_pow2(E.max_T), eps, sk, ps, s, ctx->sort_kernel,
                     E.max_T);
  }
  side_join.join();   // every output complete on the caller's stream
  HIPCHK(ctx, hipGetLastError());
  mark_done(ctx, s);
  return 0;
}

int dctae_encode(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images* imgs, const dctae_packing* pack,
                 const dctae_norm* norm, const dctae_lfq* lfq, const dctae_packed_out* out, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!pack) return fail(ctx, DCTAE_EINVAL, "packing descriptor is NULL");
  hipSetDevice(ctx->device);
  return encode_impl(ctx, cfg, imgs, pack, norm, lfq, out, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

int dctae_encode_lfq_proj(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images* imgs,
                          const dctae_packing* pack, const dctae_norm* norm, const dctae_lfq* lfq,
                          const float* w_in_dev, const float* b_in_dev, const dctae_packed_out* out, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!pack) return fail(ctx, DCTAE_EINVAL, "packing descriptor is NULL");
  if (!w_in_dev || !out || !out->codes_dev) return fail(ctx, DCTAE_EINVAL, "project_in weight and codes output required");
  hipSetDevice(ctx->device);
  return encode_impl(ctx, cfg, imgs, pack, norm, lfq, out, nullptr, nullptr, nullptr, (hipStream_t)stream, w_in_dev,
                     b_in_dev);
}

int dctae_spectrum_tokens(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images* imgs, const int64_t* tok_off,
                          float* tokens_dev, float* scores_dev, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!tok_off || !scores_dev) return fail(ctx, DCTAE_EINVAL, "tok_off and scores_dev are required");
  hipSetDevice(ctx->device);
  return encode_impl(ctx, cfg, imgs, nullptr, nullptr, nullptr, nullptr, tok_off, tokens_dev, scores_dev,
                     (hipStream_t)stream);
}

// Full-image orthonormal 2-D DCT (util.py:333-338 on the whole (3, H, W) image)
// with the optional colour transform: FE._transform_image_in / _out
// (FE:129-152) for callers that run (or override) the stages one by one.
// Two MFMA GEMMs per image on the full DCT matrices (no kept-corner crop).
int dctae_dct2(dctae_ctx* ctx, const float* x, int32_t n_img, int32_t H, int32_t W, int32_t direction, int32_t color,
               float* y, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  hipSetDevice(ctx->device);
  if (n_img < 0 || H < 1 || W < 1 || (direction != 0 && direction != 1)) return fail(ctx, DCTAE_EINVAL, "bad dct2 shape");
  if (color < 0 || color > 3 || (color > 1 && direction != 0))
    return fail(ctx, DCTAE_EINVAL, "dct2 color: 0 none, 1 fp32, 2 / 3 fp16 / bf16 arithmetic (forward only)");
  if (n_img == 0) return 0;
  if (!x || !y || x == y) return fail(ctx, DCTAE_EINVAL, "dct2 needs distinct input / output buffers");
  hipStream_t s = (hipStream_t)stream;
  int rc;
  const int64_t hw = (int64_t)H * W, plane = 3 * hw;
  const float *CW, *CH;
  if ((rc = dct_matrix(ctx, W, W, &CW)) || (rc = dct_matrix(ctx, H, H, &CH))) return rc;
  // workspace: IPT (forward with colour) and the intermediate U / T, per image
  if ((rc = ensure_ws(ctx, (size_t)2 * plane * n_img * 4, 256))) return rc;
  float* a = ctx->ws;                        // forward: IPT input; inverse: IPT output
  float* u = ctx->ws + plane * n_img;        // intermediate
  std::vector<GemmProblem> probs;
  std::vector<TileRef> t1, t2;
  for (int i = 0; i < n_img; ++i) {
    const int64_t o = plane * i;
    GemmProblem g1, g2;
    if (direction == 0) {
      const float* src = color ? a + o : x + o;
      // T[c][y][kx] = sum_x src[c][y][x] CW[kx][x];  Y[c][ky][kx] = sum_y CH[ky][y] T[c][y][kx]
      g1 = gemm(src, hw, W, 1, CW, 0, W, 1, u + o, hw, W, 1, H, W, W, 3);
      g2 = gemm(CH, 0, H, 1, u + o, hw, 1, W, y + o, hw, W, 1, H, W, H, 3);
    } else {
      float* dst = color ? a + o : y + o;
      // U[c][y][kx] = sum_ky CH[ky][y] Y[c][ky][kx];  X[c][y][x] = sum_kx U[c][y][kx] CW[kx][x]
      g1 = gemm(CH, 0, 1, H, x + o, hw, 1, W, u + o, hw, W, 1, H, W, H, 3);
      g2 = gemm(u + o, hw, W, 1, CW, 0, 1, W, dst, hw, W, 1, H, W, W, 3);
    }
    attach_x3(ctx, g1);
    attach_x3(ctx, g2);
    const int pr = (int)probs.size();
    probs.push_back(g1);
    probs.push_back(g2);
    add_tiles(t1, pr, g1);
    add_tiles(t2, pr + 1, g2);
  }
  PlanBuf pb;
  const size_t g_off = pb.add(probs.data(), probs.size());
  const size_t t1_off = pb.add(t1.data(), t1.size());
  const size_t t2_off = pb.add(t2.data(), t2.size());
  order_after_previous(ctx, s);
  if ((rc = upload_plan(ctx, pb, s))) return rc;
  uint8_t* pd = ctx->plan_dev;
  if (direction == 0 && color) {
    Timer t(ctx, s, "rgb_to_ipt");
    launch_color(x, a, hw, n_img, color >= 2 ? color : 0, ctx->cm, s);
  }
  {
    Timer t(ctx, s, "dct2_gemm");
    ctx_gemm(ctx, 3, (const GemmProblem*)(pd + g_off), (const TileRef*)(pd + t1_off), (int)t1.size(), s,
                gemm_share(probs[0]));
    ctx_gemm(ctx, 3, (const GemmProblem*)(pd + g_off), (const TileRef*)(pd + t2_off), (int)t2.size(), s,
                gemm_share(probs[1]));
  }
  if (direction == 1 && color) {
    Timer t(ctx, s, "ipt_to_rgb");
    launch_color(a, y, hw, n_img, 1, ctx->cm, s);
  }
  HIPCHK(ctx, hipGetLastError());
  mark_done(ctx, s);
  return 0;
}

// FE._patch_image (FE:364-452) of one cropped spectrum (3, H, W), H and W
// multiples of P: tiles of the kept corner, importance scores, (score desc,
// index asc) order, top k -> patches (k, P*P), positions (k, 2), channels (k).
int dctae_patch_spectrum(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const float* spec, int32_t H, int32_t W, int32_t k,
                         float* patches, int64_t* positions, int64_t* channels, float* scores, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  hipSetDevice(ctx->device);
  int rc = check_cfg(ctx, cfg);
  if (rc) return rc;
  const int P = cfg->patch_size, PP = P * P;
  if (H % P || W % P) return fail(ctx, DCTAE_EINVAL, "_patch_image: h and w must be multiples of patch_size (FE:368-369)");
  ImgDesc d;
  if ((rc = describe(ctx, cfg, H, W, d))) return rc;
  if (k < 1 || k > d.T) return fail(ctx, DCTAE_EINVAL, "_patch_image: k out of range (FE:429-435)");
  if (!spec || !patches || !positions || !channels) return fail(ctx, DCTAE_EINVAL, "NULL _patch_image buffer");
  hipStream_t s = (hipStream_t)stream;
  d.ws_y = 0;
  d.tok_off = 0;
  d.row = 0;
  d.col = 0;
  d.k = k;
  d.local_id = 0;
  const size_t y_bytes = (size_t)3 * d.Kh * d.Kw * 4;
  const size_t st_scores = ((size_t)d.T * 4 + 255) & ~size_t(255), st_raw = (size_t)d.T * PP * 4;
  const size_t st_ids = ((size_t)k * 8 + 255) & ~size_t(255);
  if ((rc = ensure_ws(ctx, y_bytes, st_scores + st_raw + st_ids + 256))) return rc;
  PlanBuf pb;
  const size_t d_off = pb.add(&d, 1);
  order_after_previous(ctx, s);
  if ((rc = upload_plan(ctx, pb, s))) return rc;
  const ImgDesc* dd = (const ImgDesc*)(ctx->plan_dev + d_off);
  for (int c = 0; c < 3; ++c)   // kept corner (3, Kh, Kw) of the (3, H, W) spectrum
    HIPCHK(ctx, hipMemcpy2DAsync(ctx->ws + (size_t)c * d.Kh * d.Kw, (size_t)d.Kw * 4, spec + (size_t)c * H * W,
                                 (size_t)W * 4, (size_t)d.Kw * 4, d.Kh, hipMemcpyDeviceToDevice, s));
  EncParams ep = enc_params(cfg, nullptr, nullptr);
  ep.S = k;
  TokenSinks sk{};
  sk.scores = (float*)ctx->stage;
  sk.raw = (float*)(ctx->stage + st_scores);
  PackSinks ps{};
  ps.pos = positions;
  ps.ch = channels;
  ps.ids = (int64_t*)(ctx->stage + st_scores + st_raw);
  ps.raw = patches;
  ps.scores = scores;
  {
    Timer t(ctx, s, "tile_epilogue");
    launch_tile_epilogue(dd, 1, d.T, ctx->ws, ep, sk, s);
  }
  {
    Timer t(ctx, s, "sort_pack");
    launch_sort_pack(dd, 1, next_pow2(d.T), ep, sk, ps, s, ctx->sort_kernel, d.T);
  }
  HIPCHK(ctx, hipGetLastError());
  mark_done(ctx, s);
  return 0;
}

static int norm_impl(dctae_ctx* ctx, const dctae_norm* norm, int32_t P, int32_t mh, int32_t mw, const float* x,
                     const int64_t* ch, const int64_t* pos, int64_t n, float* y, int inverse, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!norm || !norm->median_dev || !norm->b_dev) return fail(ctx, DCTAE_EINVAL, "PatchNorm tables are NULL");
  if (P < 1 || mh < 1 || mw < 1 || n < 0) return fail(ctx, DCTAE_EINVAL, "bad PatchNorm shape");
  if (n == 0) return 0;
  if (!x || !ch || !pos || !y) return fail(ctx, DCTAE_EINVAL, "NULL tensor");
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, inverse ? "norm_inverse" : "norm_forward");
  launch_norm(x, ch, pos, n, P * P, mh, mw, norm->median_dev, norm->b_dev, norm->eps, norm->min_val, norm->max_val,
              inverse, y, ctx->err_dev, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_norm_forward(dctae_ctx* ctx, const dctae_norm* norm, int32_t P, int32_t mh, int32_t mw, const float* x,
                       const int64_t* ch, const int64_t* pos, int64_t n, float* y, void* stream) {
  return norm_impl(ctx, norm, P, mh, mw, x, ch, pos, n, y, 0, stream);
}

int dctae_norm_inverse(dctae_ctx* ctx, const dctae_norm* norm, int32_t P, int32_t mh, int32_t mw, const float* y,
                       const int64_t* ch, const int64_t* pos, int64_t n, float* x, void* stream) {
  return norm_impl(ctx, norm, P, mh, mw, y, ch, pos, n, x, 1, stream);
}

// ---- PatchNorm training (patchnorm.py:101-155), kernels in dctae_stats.hip ----
namespace {

struct StatsScratch {
  int32_t *cell, *count, *start, *list;
  float* bn;       // (n_cells) batch counts
  float *t0, *t1;  // two (n_cells, PP) tables (batch median / batch b)
};

int stats_scratch(dctae_ctx* ctx, int64_t n_tok, int n_cells, int PP, bool tables, hipStream_t s,
                  StatsScratch* o) {
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t b_tok = al(sizeof(int32_t) * std::max<int64_t>(n_tok, 1));
  const size_t b_cell = al(sizeof(int32_t) * n_cells);
  const size_t b_tab = tables ? al(sizeof(float) * (size_t)n_cells * PP) : 0;
  const size_t need = 2 * b_tok + 3 * b_cell + 2 * b_tab;
  if (need > ctx->st_bytes) {
    if (ctx->st_ws) {
      HIPCHK(ctx, hipStreamSynchronize(s));
      HIPCHK(ctx, hipFree(ctx->st_ws));
      ctx->st_ws = nullptr;
      ctx->st_bytes = 0;
    }
    HIPCHK(ctx, hipMalloc((void**)&ctx->st_ws, need));
    ctx->st_bytes = need;
  }
  uint8_t* p = ctx->st_ws;
  o->cell = (int32_t*)p;
  p += b_tok;
  o->list = (int32_t*)p;
  p += b_tok;
  o->count = (int32_t*)p;
  p += b_cell;
  o->start = (int32_t*)p;
  p += b_cell;
  o->bn = (float*)p;
  p += b_cell;
  o->t0 = tables ? (float*)p : nullptr;
  p += b_tab;
  o->t1 = tables ? (float*)p : nullptr;
  return 0;
}

int stats_check(dctae_ctx* ctx, int32_t P, int32_t C, int32_t mh, int32_t mw, int64_t n_tok, const float* x,
                const int64_t* ch, const int64_t* pos) {
  if (!ctx) return DCTAE_EINVAL;
  if (P < 1 || C < 1 || mh < 1 || mw < 1 || n_tok < 0) return fail(ctx, DCTAE_EINVAL, "bad PatchNorm shape");
  if ((int64_t)C * mh * mw > (1 << 30)) return fail(ctx, DCTAE_EINVAL, "PatchNorm table too large");
  if (n_tok > (int64_t)INT32_MAX) return fail(ctx, DCTAE_EINVAL, "too many tokens for one statistics batch");
  if (n_tok > 0 && (!x || !ch || !pos)) return fail(ctx, DCTAE_EINVAL, "NULL tensor");
  return 0;
}

}  // namespace

int dctae_norm_batch_stats(dctae_ctx* ctx, int32_t P, int32_t C, int32_t mh, int32_t mw, const float* x,
                           const int64_t* ch, const int64_t* pos, const uint8_t* key_pad, int64_t n_tok,
                           float* batch_n, float* batch_median, void* stream) {
  if (int rc = stats_check(ctx, P, C, mh, mw, n_tok, x, ch, pos)) return rc;
  if (!batch_n || !batch_median) return fail(ctx, DCTAE_EINVAL, "NULL output table");
  hipStream_t s = (hipStream_t)stream;
  const int n_cells = C * mh * mw, PP = P * P;
  StatsScratch w;
  if (int rc = stats_scratch(ctx, n_tok, n_cells, PP, false, s, &w)) return rc;
  Timer t(ctx, s, "norm_batch_stats");
  launch_stats_lists(ch, pos, key_pad, n_tok, C, mh, mw, w.cell, w.count, w.start, w.list, ctx->err_dev, s);
  launch_stats_median(x, PP, n_cells, w.start, w.count, w.list, batch_median, batch_n, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_norm_batch_mad(dctae_ctx* ctx, int32_t P, int32_t C, int32_t mh, int32_t mw, const float* x,
                         const int64_t* ch, const int64_t* pos, const uint8_t* key_pad, int64_t n_tok,
                         const float* median, float* batch_b, void* stream) {
  if (int rc = stats_check(ctx, P, C, mh, mw, n_tok, x, ch, pos)) return rc;
  if (!median || !batch_b) return fail(ctx, DCTAE_EINVAL, "NULL table");
  hipStream_t s = (hipStream_t)stream;
  const int n_cells = C * mh * mw, PP = P * P;
  StatsScratch w;
  if (int rc = stats_scratch(ctx, n_tok, n_cells, PP, false, s, &w)) return rc;
  Timer t(ctx, s, "norm_batch_mad");
  launch_stats_lists(ch, pos, key_pad, n_tok, C, mh, mw, w.cell, w.count, w.start, w.list, ctx->err_dev, s);
  launch_stats_batch_b(x, PP, n_cells, w.start, w.count, w.list, median, batch_b, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_norm_merge(dctae_ctx* ctx, int32_t n_cells, int32_t PP, float* table, const float* batch, float* n,
                     const float* batch_n, int32_t n_update, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (n_cells < 0 || PP < 1) return fail(ctx, DCTAE_EINVAL, "bad PatchNorm shape");
  if (n_cells == 0) return 0;
  if (!n || !batch_n || ((!table || !batch) && PP > 0)) return fail(ctx, DCTAE_EINVAL, "NULL table");
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "norm_merge");
  launch_stats_merge(table, batch, n, batch_n, n_cells, PP, s);
  if (n_update) launch_stats_add(n, batch_n, n_cells, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_norm_train_step(dctae_ctx* ctx, const dctae_norm* norm, float* n_dev, int32_t P, int32_t C, int32_t mh,
                          int32_t mw, const float* x, const int64_t* ch, const int64_t* pos, const uint8_t* key_pad,
                          int64_t n_tok, float* y, void* stream) {
  if (int rc = stats_check(ctx, P, C, mh, mw, n_tok, x, ch, pos)) return rc;
  if (!norm || !norm->median_dev || !norm->b_dev || !n_dev) return fail(ctx, DCTAE_EINVAL, "PatchNorm tables are NULL");
  hipStream_t s = (hipStream_t)stream;
  const int n_cells = C * mh * mw, PP = P * P;
  float* median = const_cast<float*>(norm->median_dev);
  float* b = const_cast<float*>(norm->b_dev);
  StatsScratch w;
  if (int rc = stats_scratch(ctx, n_tok, n_cells, PP, true, s, &w)) return rc;
  Timer t(ctx, s, "norm_train_step");
  launch_stats_lists(ch, pos, key_pad, n_tok, C, mh, mw, w.cell, w.count, w.start, w.list, ctx->err_dev, s);
  launch_stats_median(x, PP, n_cells, w.start, w.count, w.list, w.t0, w.bn, s);      // :112-130
  launch_stats_merge(median, w.t0, n_dev, w.bn, n_cells, PP, s);                     // :135-138
  launch_stats_batch_b(x, PP, n_cells, w.start, w.count, w.list, median, w.t1, s);   // :140-144
  launch_stats_merge(b, w.t1, n_dev, w.bn, n_cells, PP, s);                          // :146-148
  launch_stats_add(n_dev, w.bn, n_cells, s);                                         // :150
  if (y && n_tok > 0) {                                                              // :153-155
    if (key_pad) launch_zero_pads(x, key_pad, n_tok, PP, y, s);
    else if (y != x) HIPCHK(ctx, hipMemcpyAsync(y, x, sizeof(float) * n_tok * PP, hipMemcpyDeviceToDevice, s));
  }
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_lfq_forward(dctae_ctx* ctx, const dctae_lfq* lfq, const float* x, int64_t n, float* q, int64_t* idx,
                      void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!lfq || lfq->codebook_dim < 1 || lfq->codebook_dim > 62 || lfq->num_codebooks < 1)
    return fail(ctx, DCTAE_EINVAL, "bad LFQ config");
  if (n < 0 || (n > 0 && (!x || !idx))) return fail(ctx, DCTAE_EINVAL, "bad LFQ tensors");
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "lfq_forward");
  launch_lfq_forward(x, n, lfq->codebook_dim, lfq->num_codebooks, lfq->codebook_scale, q, idx, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_lfq_indices_to_codes(dctae_ctx* ctx, const dctae_lfq* lfq, const int64_t* idx, int64_t n, float* codes,
                               void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!lfq || lfq->codebook_dim < 1 || lfq->codebook_dim > 31 || lfq->num_codebooks < 1)
    return fail(ctx, DCTAE_EINVAL, "bad LFQ config (codebook_dim <= 31: lfq.py:117 casts to int32)");
  if (n < 0 || (n > 0 && (!idx || !codes))) return fail(ctx, DCTAE_EINVAL, "bad LFQ tensors");
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "lfq_codes");
  launch_lfq_codes(idx, n, lfq->codebook_dim, lfq->num_codebooks, lfq->codebook_scale, codes, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

static int lfq_entropy_check(dctae_ctx* ctx, const dctae_lfq* lfq, const void* h, const void* mask, int64_t n_tok,
                             float temperature) {
  if (!lfq || lfq->codebook_dim < 1 || lfq->num_codebooks < 1 || n_tok < 0)
    return fail(ctx, DCTAE_EINVAL, "bad LFQ config");
  if (!lfq_entropy_supported(lfq->codebook_dim, lfq->num_codebooks, n_tok))
    return fail(ctx, DCTAE_EUNSUP, "LFQ entropy loss: codebook_dim <= 16 and num_codebooks <= 32");
  if (n_tok > 0 && (!h || !mask)) return fail(ctx, DCTAE_EINVAL, "bad LFQ tensors");
  if (!(temperature != 0.0f)) return fail(ctx, DCTAE_EINVAL, "temperature must not be 0");
  return 0;
}

int dctae_lfq_entropy_forward(dctae_ctx* ctx, const dctae_lfq* lfq, const float* h, const uint8_t* mask,
                              int64_t n_tok, float temperature, float eps, float* avg_probs, float* scalars,
                              void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  hipSetDevice(ctx->device);
  int rc;
  if ((rc = lfq_entropy_check(ctx, lfq, h, mask, n_tok, temperature))) return rc;
  if (!avg_probs || !scalars) return fail(ctx, DCTAE_EINVAL, "NULL output");
  if ((rc = ensure_ws(ctx, sizeof(float) * lfq_entropy_fwd_ws_floats(n_tok, lfq->num_codebooks, lfq->codebook_dim),
                      256)))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "lfq_entropy_forward");
  launch_lfq_entropy_fwd(h, mask, n_tok, lfq->num_codebooks, lfq->codebook_dim, lfq->codebook_scale, temperature, eps,
                         ctx->ws, avg_probs, scalars, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_lfq_entropy_backward(dctae_ctx* ctx, const dctae_lfq* lfq, const float* h, const uint8_t* mask,
                               int64_t n_tok, float temperature, float eps, const float* avg_probs,
                               const float* scalars, const float* grad, float* dh, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  hipSetDevice(ctx->device);
  int rc;
  if ((rc = lfq_entropy_check(ctx, lfq, h, mask, n_tok, temperature))) return rc;
  if (!avg_probs || !scalars || !grad || (n_tok > 0 && !dh)) return fail(ctx, DCTAE_EINVAL, "NULL tensor");
  if (n_tok == 0) return 0;
  if ((rc = ensure_ws(ctx, sizeof(float) * lfq_entropy_bwd_ws_floats(lfq->codebook_dim), 256))) return rc;
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "lfq_entropy_backward");
  if (launch_lfq_entropy_bwd(h, mask, n_tok, lfq->num_codebooks, lfq->codebook_dim, lfq->codebook_scale, temperature,
                             eps, avg_probs, scalars, grad, ctx->ws, dh, s))
    return fail(ctx, DCTAE_EHIP, "LFQ entropy backward: the kernel's LDS size could not be set");
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_linear_ordered(dctae_ctx* ctx, const float* x, int64_t n, int32_t K, const float* wt, const float* b,
                         int32_t dim, float* out, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  hipSetDevice(ctx->device);
  if (n < 0 || K < 1 || dim < 1 || n / 16 >= (int64_t)INT32_MAX) return fail(ctx, DCTAE_EINVAL, "bad linear shape");
  if (!linear_ordered_supported(K, dim)) return fail(ctx, DCTAE_EUNSUP, "ordered linear: K <= 512");
  if (n == 0) return 0;
  if (!x || !wt || !out) return fail(ctx, DCTAE_EINVAL, "NULL tensor");
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "linear_ordered");
  launch_linear_ordered(x, n, K, wt, b, dim, out, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

static int lfq_proj_check(dctae_ctx* ctx, const dctae_lfq* lfq, int64_t n, int32_t dim, const void* a,
                          const float* w, const void* o, int max_ncb, bool o_vec = false) {
  if (!lfq || lfq->codebook_dim < 1 || lfq->codebook_dim > 31 || lfq->num_codebooks < 1 ||
      lfq->num_codebooks > max_ncb)
    return fail(ctx, DCTAE_EINVAL, "bad LFQ config (codebook_dim <= 31, num_codebooks <= " + std::to_string(max_ncb) + ")");
  const int64_t cdims = (int64_t)lfq->codebook_dim * lfq->num_codebooks;
  if (dim < 4 || dim > 256 || dim % 4 != 0 || cdims > 256 || cdims % 4 != 0)
    return fail(ctx, DCTAE_EINVAL, "LFQ projections: dim and codebook_dim * num_codebooks must be multiples of 4 <= 256");
  if (n < 0 || (n > 0 && (!a || !w || !o))) return fail(ctx, DCTAE_EINVAL, "bad LFQ projection tensors");
  if (((uintptr_t)a | (uintptr_t)w) & 15) return fail(ctx, DCTAE_EINVAL, "LFQ projections need 16-byte aligned tensors");
  // project_out writes its (n, dim) fp32 rows as 16-byte pieces
  if (o_vec && ((uintptr_t)o & 15))
    return fail(ctx, DCTAE_EINVAL, "LFQ project_out needs a 16-byte aligned output tensor");
  return 0;
}

static int lfq_project_in_impl(dctae_ctx* ctx, const dctae_lfq* lfq, const float* x, int64_t n, int32_t dim,
                               const float* w, const float* b, float x_bound, int64_t* idx, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (int rc = lfq_proj_check(ctx, lfq, n, dim, x, w, idx, 64)) return rc;
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = proj_scratch(ctx, lfq->codebook_dim * lfq->num_codebooks, dim)) return rc;
  // ctx->proj_ws (the pre-split weight) is shared with every call of this
  // context: ordered after the previous call, whatever its stream
  order_after_previous(ctx, s);
  {
    Timer t(ctx, s, "lfq_project_in");
    launch_lfq_project_in(x, n, dim, w, b, lfq->codebook_dim, lfq->num_codebooks, lfq->codebook_scale, idx,
                          ctx->proj_ws, s, ctx->gemm_h2 ? x_bound : 0.0f, ctx->lfq_ws != 0);
  }
  HIPCHK(ctx, hipGetLastError());
  mark_done(ctx, s);
  return 0;
}

int dctae_lfq_project_in(dctae_ctx* ctx, const dctae_lfq* lfq, const float* x, int64_t n, int32_t dim,
                         const float* w, const float* b, int64_t* idx, void* stream) {
  return lfq_project_in_impl(ctx, lfq, x, n, dim, w, b, 0.0f, idx, stream);
}

int dctae_lfq_project_in_bounded(dctae_ctx* ctx, const dctae_lfq* lfq, const float* x, int64_t n, int32_t dim,
                                 const float* w, const float* b, float x_bound, int64_t* idx, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!(x_bound > 0.0f) || !std::isfinite(x_bound)) return fail(ctx, DCTAE_EINVAL, "x_bound must be finite and > 0");
  return lfq_project_in_impl(ctx, lfq, x, n, dim, w, b, x_bound, idx, stream);
}

int dctae_lfq_project_out(dctae_ctx* ctx, const dctae_lfq* lfq, const int64_t* idx, int64_t n, int32_t dim,
                          const float* w, const float* b, float* out, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (int rc = lfq_proj_check(ctx, lfq, n, dim, idx, w, out, 32, true)) return rc;
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = proj_scratch(ctx, dim, lfq->codebook_dim * lfq->num_codebooks)) return rc;
  order_after_previous(ctx, s);   // shared ctx->proj_ws
  {
    Timer t(ctx, s, "lfq_project_out");
    launch_lfq_project_out(idx, n, dim, w, b, lfq->codebook_dim, lfq->num_codebooks, lfq->codebook_scale, out,
                           ctx->proj_ws, s, nullptr, nullptr, nullptr, nullptr, 0.f, 0, 0, nullptr, ctx->gemm_h2 != 0,
                           ctx->lfq_ws != 0);
  }
  HIPCHK(ctx, hipGetLastError());
  mark_done(ctx, s);
  return 0;
}

int dctae_lfq_project_out_inverse_norm(dctae_ctx* ctx, const dctae_lfq* lfq, const int64_t* idx, int64_t n,
                                       int32_t dim, const float* w, const float* b, const dctae_norm* norm,
                                       int32_t max_patch_h, int32_t max_patch_w, const int64_t* channels,
                                       const int64_t* positions, float* out, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (int rc = lfq_proj_check(ctx, lfq, n, dim, idx, w, out, 32, true)) return rc;
  if (!norm || !norm->median_dev || !norm->b_dev || max_patch_h < 1 || max_patch_w < 1 ||
      (n > 0 && (!channels || !positions)))
    return fail(ctx, DCTAE_EINVAL, "inverse PatchNorm needs tables, max_patch_h/w and channels / positions");
  // the fused inverse reads the (3, max_patch_h, max_patch_w, dim) tables and
  // writes out as float4 pieces along each token's dim floats
  if (((uintptr_t)norm->median_dev | (uintptr_t)norm->b_dev | (uintptr_t)out) & 15)
    return fail(ctx, DCTAE_EINVAL, "fused inverse PatchNorm needs 16-byte aligned median / b / out");
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = proj_scratch(ctx, dim, lfq->codebook_dim * lfq->num_codebooks)) return rc;
  order_after_previous(ctx, s);   // shared ctx->proj_ws
  {
    Timer t(ctx, s, "lfq_project_out");
    launch_lfq_project_out(idx, n, dim, w, b, lfq->codebook_dim, lfq->num_codebooks, lfq->codebook_scale, out,
                           ctx->proj_ws, s, channels, positions, norm->median_dev, norm->b_dev, norm->eps, max_patch_h,
                           max_patch_w, ctx->err_dev, ctx->gemm_h2 != 0, ctx->lfq_ws != 0);
  }
  HIPCHK(ctx, hipGetLastError());
  mark_done(ctx, s);
  return 0;
}

// ---- VectorQuantize inference (dctae_vq.hip) --------------------------------
static int vq_check(dctae_ctx* ctx, const dctae_vq* vq) {
  if (!vq || vq->codebook_dim != 16 || vq->heads < 1 || vq->codebook_size < 1 || vq->dim < 1 || !vq->embed_dev)
    return fail(ctx, DCTAE_EINVAL, "bad VectorQuantize config (codebook_dim 16, heads >= 1, codebook_size >= 1)");
  const bool proj = vq->dim != vq->heads * vq->codebook_dim;   // vector_quantize.py:725-728
  if (proj && (!vq->w_in_dev || !vq->b_in_dev || !vq->w_out_dev || !vq->b_out_dev))
    return fail(ctx, DCTAE_EINVAL, "VectorQuantize: dim != heads * codebook_dim needs project_in / project_out");
  if (vq->affine && (!vq->codebook_mean_dev || !vq->codebook_variance_dev || !vq->batch_mean_dev ||
                     !vq->batch_variance_dev || !vq->batch_initted_dev))
    return fail(ctx, DCTAE_EINVAL, "VectorQuantize: affine_param needs codebook / batch statistics");
  return 0;
}

static int vq_scratch(dctae_ctx* ctx, size_t need) {
  if (need <= ctx->vq_bytes) return 0;
  HIPCHK(ctx, hipDeviceSynchronize());
  if (ctx->vq_ws) hipFree(ctx->vq_ws);
  ctx->vq_ws = nullptr;
  ctx->vq_bytes = 0;
  if (hipMalloc((void**)&ctx->vq_ws, need) != hipSuccess)
    return fail(ctx, DCTAE_ENOMEM, "VectorQuantize scratch allocation of " + std::to_string(need) + " bytes failed");
  ctx->vq_bytes = need;
  return 0;
}

// O (n, N) = A (n, K) W^T (N, K) + bias, on k_gemm_f32 (plan uploaded through the shared plan buffer)
static int vq_linear(dctae_ctx* ctx, const float* A, int64_t n, int K, const float* W, const float* bias, int N,
                     float* O, const uint8_t* mask, const float* orig, hipStream_t s, const char* name) {
  // k_gemm_x3 addresses each operand through a buffer resource with a 32-bit
  // byte range: the rows go in chunks whose A and O spans stay below 2^31 bytes
  const int64_t rows_max = ((int64_t)1 << 31) / ((int64_t)4 * std::max(K, N)) - 1;
  std::vector<GemmProblem> g;
  std::vector<TileRef> t;
  for (int64_t r0 = 0; r0 < n; r0 += rows_max) {
    const int rows = (int)std::min(rows_max, n - r0);
    g.push_back(gemm(A + r0 * K, 0, K, 1, W, 0, K, 1, O + r0 * N, 0, N, 1, rows, N, K, 1));
    add_tiles(t, (int)g.size() - 1, g.back());
  }
  PlanBuf pb;
  const size_t g_off = pb.add(g.data(), g.size());
  const size_t t_off = pb.add(t.data(), t.size());
  int rc;
  if ((rc = upload_plan(ctx, pb, s))) return rc;
  Timer tm(ctx, s, name);
  ctx_gemm(ctx, 1, (const GemmProblem*)(ctx->plan_dev + g_off), (const TileRef*)(ctx->plan_dev + t_off), (int)t.size(), s);
  launch_vq_bias(O, bias, n, N, mask, orig, s);
  return 0;
}

int dctae_vq_forward(dctae_ctx* ctx, const dctae_vq* vq, const float* x, const uint8_t* mask, int64_t n_tok,
                     float* quantize, int64_t* indices, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  hipSetDevice(ctx->device);
  int rc = vq_check(ctx, vq);
  if (rc) return rc;
  if (n_tok < 0 || (n_tok > 0 && (!x || !indices))) return fail(ctx, DCTAE_EINVAL, "bad VectorQuantize tensors");
  if (n_tok == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int H = vq->heads, D = vq->codebook_dim, C = vq->codebook_size, HD = H * D;
  // element indices of the (n_tok, dim) input and the (n_tok, H*D) vectors are 32-bit in the kernels
  if (n_tok > (int64_t)INT32_MAX / 64 || n_tok * std::max(vq->dim, HD) > (int64_t)INT32_MAX)
    return fail(ctx, DCTAE_EINVAL, "VectorQuantize: too many tokens in one call (n_tok * max(dim, heads * 16) >= 2^31)");
  const bool proj = vq->dim != HD;
  const int64_t nv = n_tok * H;
  // scratch: acc (64 doubles) | et (C*D) | y2 (C) | xp (n*HD, projected only) | xq (n*HD)
  const size_t acc_b = 64 * sizeof(double);
  const size_t et_b = ((size_t)C * D * 4 + 255) & ~size_t(255);
  const size_t y2_b = ((size_t)C * 4 + 255) & ~size_t(255);
  const size_t v_b = ((size_t)nv * D * 4 + 255) & ~size_t(255);
  const bool need_xq = quantize != nullptr;
  if ((rc = vq_scratch(ctx, acc_b + et_b + y2_b + (proj ? v_b : 0) + ((need_xq && (proj || mask)) ? v_b : 0))))
    return rc;
  uint8_t* p = ctx->vq_ws;
  double* acc = (double*)p;
  float* et = (float*)(p + acc_b);
  float* y2 = (float*)(p + acc_b + et_b);
  uint8_t* q = p + acc_b + et_b + y2_b;
  float* xp = proj ? (float*)q : const_cast<float*>(x);
  if (proj) q += v_b;
  // codes: straight into quantize when nothing follows them
  float* xq = need_xq ? ((proj || mask) ? (float*)q : quantize) : nullptr;
  order_after_previous(ctx, s);
  if (proj && (rc = vq_linear(ctx, x, n_tok, vq->dim, vq->w_in_dev, vq->b_in_dev, HD, xp, nullptr, nullptr, s,
                              "vq_project_in")))
    return rc;
  {
    Timer t(ctx, s, "vq_codebook");
    if (vq->affine) {
      HIPCHK(ctx, hipMemsetAsync(acc, 0, acc_b, s));
      launch_vq_stats(xp, mask, n_tok, H, acc, s);
    }
    launch_vq_codebook(acc, vq->batch_mean_dev, vq->batch_variance_dev, vq->batch_initted_dev, vq->affine_decay,
                       vq->affine, vq->embed_dev, vq->codebook_mean_dev, vq->codebook_variance_dev, C, et, y2, s);
  }
  {
    Timer t(ctx, s, "vq_assign");
    launch_vq_assign(xp, nv, H, et, y2, C, xq, indices, s);
  }
  if (need_xq) {
    if (proj) {
      if ((rc = vq_linear(ctx, xq, n_tok, HD, vq->w_out_dev, vq->b_out_dev, vq->dim, quantize, mask, x, s,
                          "vq_project_out")))
        return rc;
    } else if (mask) {
      HIPCHK(ctx, hipMemcpyAsync(quantize, xq, sizeof(float) * nv * D, hipMemcpyDeviceToDevice, s));
      launch_vq_bias(quantize, nullptr, n_tok, HD, mask, x, s);
    }
  }
  HIPCHK(ctx, hipGetLastError());
  mark_done(ctx, s);
  return 0;
}

int dctae_vq_codes_from_indices(dctae_ctx* ctx, const dctae_vq* vq, const int64_t* idx, int64_t n, float* codes,
                                void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  hipSetDevice(ctx->device);
  int rc = vq_check(ctx, vq);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!idx || !codes))) return fail(ctx, DCTAE_EINVAL, "bad VectorQuantize tensors");
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "vq_codes");
  launch_vq_codes(idx, n * vq->heads, vq->embed_dev, vq->codebook_size, codes, ctx->err_dev, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_vq_output_from_indices(dctae_ctx* ctx, const dctae_vq* vq, const int64_t* idx, int64_t n, float* out,
                                 void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  hipSetDevice(ctx->device);
  int rc = vq_check(ctx, vq);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!idx || !out))) return fail(ctx, DCTAE_EINVAL, "bad VectorQuantize tensors");
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int HD = vq->heads * vq->codebook_dim;
  if (vq->dim == HD) return dctae_vq_codes_from_indices(ctx, vq, idx, n, out, stream);
  if ((rc = vq_scratch(ctx, ((size_t)n * HD * 4 + 255) & ~size_t(255)))) return rc;
  float* codes = (float*)ctx->vq_ws;
  order_after_previous(ctx, s);
  {
    Timer t(ctx, s, "vq_codes");
    launch_vq_codes(idx, n * vq->heads, vq->embed_dev, vq->codebook_size, codes, ctx->err_dev, s);
  }
  if ((rc = vq_linear(ctx, codes, n, HD, vq->w_out_dev, vq->b_out_dev, vq->dim, out, nullptr, nullptr, s,
                      "vq_project_out")))
    return rc;
  HIPCHK(ctx, hipGetLastError());
  mark_done(ctx, s);
  return 0;
}

// decode of 512 x 512 images on the FFT path: token map -> column DCT-III
// (tokens expanded in the kernel) -> U -> row DCT-III + IPT -> RGB
static int decode_fft(dctae_ctx* ctx, const dctae_fe_cfg* cfg, std::vector<ImgDesc>& D, const FftPlan& fpl,
                      int32_t n_rows, const int32_t* img_lut, int32_t lut_w, const int64_t* ids,
                      const uint8_t* key_pad, const int64_t* pos, const int64_t* ch, const dctae_norm* norm,
                      const dctae_lfq* lfq, const int64_t* codes, const float* patches, float* rgb, hipStream_t s,
                      bool normed) {
  const int n_img = (int)D.size();
  const int S = cfg->max_seq_len, P = cfg->patch_size;
  int64_t wsf = 0;
  std::vector<int2> rb;
  for (int i = 0; i < n_img; ++i) {
    ImgDesc& d = D[i];
    d.ws_t = wsf;
    wsf += (3ll * d.H * d.Kw + 63) & ~63ll;
    for (int y0 = 0; y0 < d.H; y0 += 16) rb.push_back(make_int2(i, y0));
  }
  const int64_t map_off = wsf;
  const int64_t map_n = (int64_t)n_img * 3 * cfg->max_patch_h * cfg->max_patch_w;
  wsf += map_n;
  int rc;
  if ((rc = ensure_ws(ctx, (size_t)wsf * 4, 256))) return rc;
  PlanBuf pb;
  const size_t d_off = pb.add(D.data(), D.size());
  const size_t rb_off = pb.add(rb.data(), rb.size());
  const size_t lut_off = pb.add(img_lut, (size_t)n_rows * lut_w);
  order_after_previous(ctx, s);
  if ((rc = upload_plan(ctx, pb, s))) return rc;
  uint8_t* pd = ctx->plan_dev;
  const ImgDesc* dd = (const ImgDesc*)(pd + d_off);
  int32_t* map = (int32_t*)(ctx->ws + map_off);
  HIPCHK(ctx, hipMemsetAsync(map, 0xFF, (size_t)map_n * 4, s));
  DecodeArgs a{};
  a.ids = ids;
  a.key_pad = key_pad;
  a.pos = pos;
  a.ch = ch;
  a.codes = codes;
  a.patches = patches;
  a.lut = (const int32_t*)(pd + lut_off);
  a.lut_w = lut_w;
  a.S = S;
  a.P = P;
  a.use_codes = codes ? 1 : (normed ? 2 : 0);
  if (codes) {
    a.cb_dim = lfq->codebook_dim;
    a.ncb = lfq->num_codebooks;
    a.scale = lfq->codebook_scale;
  }
  if (codes || normed) {
    a.median = norm->median_dev;
    a.b = norm->b_dev;
    a.eps = norm->eps;
  }
  a.maxph = cfg->max_patch_h;
  a.maxpw = cfg->max_patch_w;
  a.err = ctx->err_dev;
  const float2* tw = ctx->fft_tab + fpl.tw_off;
  const float4* pre = reinterpret_cast<const float4*>(ctx->fft_tab + fpl.ipre_off);
  {
    Timer t(ctx, s, "dec_map");
    launch_dec_map((int64_t)n_rows * S, dd, a, map, s);
  }
  // 32 kept tile columns on the default row kernel: U in the band layout
  // (k_idct_cols512b); otherwise row-major U (k_idct_cols512)
  const bool rows512 = ctx->dec_rows_kernel == 3 && D[0].qw == 32;
  const bool band = rows512 && ctx->dec_cols_kernel == 2;
  {
    Timer t(ctx, s, "idct_cols");
    if (band)
      launch_idct_cols512b(dd, n_img, ctx->ws, map, tw, pre, a, s);
    else
      launch_idct_cols512(dd, n_img, D[0].qw, ctx->ws, map, tw, pre, a, s);
  }
  {
    Timer t(ctx, s, "idct_rows");
    if (rows512)
      launch_idct_rows512(band, dd, (const int2*)(pd + rb_off), (int)rb.size(), ctx->ws, rgb, tw, pre, ctx->cm, s);
    else
      launch_idct_rows_spec(1, dd, (const int2*)(pd + rb_off), (int)rb.size(), ctx->ws, rgb, tw, pre, ctx->cm, s);
  }
  HIPCHK(ctx, hipGetLastError());
  mark_done(ctx, s);
  return 0;
}

// normed: patches are PatchNorm outputs (before inverse_norm); the FFT path
// applies the inverse in its column kernel (the (c, strip) tables of a block
// are image-independent), other geometries run dctae_norm_inverse's kernel
// into the staging buffer first
static int decode_impl(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut,
                       int32_t lut_w, int32_t n_img, const int32_t* out_hw, const int64_t* out_off,
                       const int32_t* patch_hw, const int64_t* ids, const uint8_t* key_pad, const int64_t* pos,
                       const int64_t* ch, const dctae_norm* norm, const dctae_lfq* lfq, const int64_t* codes,
                       const float* patches, float* rgb, void* stream, bool normed) {
  if (!ctx) return DCTAE_EINVAL;
  hipSetDevice(ctx->device);
  int rc = check_cfg(ctx, cfg);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int P = cfg->patch_size, PP = P * P, S = cfg->max_seq_len;
  if (normed && (!norm || !norm->median_dev || !norm->b_dev || codes))
    return fail(ctx, DCTAE_EINVAL, "decode of PatchNorm-space patches needs the PatchNorm tables (and no codes)");
  if (n_rows < 0 || n_img < 0 || lut_w < 1 || !img_lut || (n_img > 0 && (!out_hw || !out_off || !patch_hw || !rgb)))
    return fail(ctx, DCTAE_EINVAL, "bad decode descriptor");
  if (n_rows > 0 && (!ids || !key_pad || !pos || !ch)) return fail(ctx, DCTAE_EINVAL, "NULL batch tensor");
  if (codes) {
    if (!norm || !norm->median_dev || !norm->b_dev) return fail(ctx, DCTAE_EINVAL, "decode from codes needs PatchNorm");
    if ((rc = check_lfq(ctx, lfq, PP))) return rc;
  } else if (n_rows > 0 && !patches) {
    return fail(ctx, DCTAE_EINVAL, "decode needs codes or patches");
  }
  if (n_img == 0) return 0;
  for (int64_t i = 0; i < (int64_t)n_rows * lut_w; ++i)
    if (img_lut[i] < -1 || img_lut[i] >= n_img) return fail(ctx, DCTAE_EINVAL, "image LUT entry out of range");
  std::vector<ImgDesc> D(n_img);
  int64_t wsf = 0, max_hw = 1;
  for (int i = 0; i < n_img; ++i) {
    ImgDesc& d = D[i];
    std::memset(&d, 0, sizeof(d));
    d.plan_w = d.plan_h = -1;
    d.H = out_hw[2 * i];
    d.W = out_hw[2 * i + 1];
    d.ph = patch_hw[2 * i];
    d.pw = patch_hw[2 * i + 1];
    if (d.ph < 1 || d.pw < 1 || P * d.ph > d.H || P * d.pw > d.W)
      return fail(ctx, DCTAE_EINVAL, "image " + std::to_string(i) + ": patch_sizes do not fit original_sizes (FE:304)");
    d.qh = std::min(d.ph, cfg->max_patch_h);
    d.qw = std::min(d.pw, cfg->max_patch_w);
    d.Kh = P * d.qh;
    d.Kw = P * d.qw;
    d.rgb_off = out_off[i];
    d.ws_y = wsf;
    wsf += 3ll * d.Kh * d.Kw;
    d.ws_t = wsf;
    wsf += 3ll * d.H * d.Kw;
    d.ws_p = wsf;
    wsf += 3ll * d.H * d.W;
    max_hw = std::max<int64_t>(max_hw, (int64_t)d.H * d.W);
  }
  // the GEMM path's slot map (k_dec_map: the later packed slot wins at a duplicate place, FE:639-643)
  const int64_t gmap_off = (wsf + 63) & ~63ll;
  const int64_t gmap_n = (int64_t)n_img * 3 * cfg->max_patch_h * cfg->max_patch_w;
  // FFT path (dctae_idct.hip): every image 512 x 512 on the specialised plan, recommended LFQ
  bool fftdec = ctx->fft_decode && P == 14 && (!codes || (lfq->codebook_dim == 14 && lfq->num_codebooks == 14));
  for (int i = 0; fftdec && i < n_img; ++i)
    fftdec = D[i].H == 512 && D[i].W == 512 && D[i].qh <= 32 && D[i].qw == D[0].qw;
  FftPlan fpl{};
  if (fftdec) fftdec = fft_plan_for(ctx, 512, P, &fpl) == 0 && fpl.spec == 1;
  if (fftdec)
    return decode_fft(ctx, cfg, D, fpl, n_rows, img_lut, lut_w, ids, key_pad, pos, ch, norm, lfq, codes, patches,
                      rgb, s, normed);
  if (normed && n_rows > 0) {
    // other geometries: the inverse over every packed token into the staging
    // buffer (after the previous call, which may still read it), then as patches
    const int64_t n_tok = (int64_t)n_rows * S;
    if ((rc = ensure_ws(ctx, 0, (size_t)n_tok * PP * 4))) return rc;
    order_after_previous(ctx, s);
    float* inv = reinterpret_cast<float*>(ctx->stage);
    {
      Timer t(ctx, s, "norm_inverse");
      launch_norm(patches, ch, pos, n_tok, PP, cfg->max_patch_h, cfg->max_patch_w, norm->median_dev, norm->b_dev,
                  norm->eps, norm->min_val, norm->max_val, 1, inv, ctx->err_dev, s);
    }
    patches = inv;
  }
  if ((rc = ensure_ws(ctx, (size_t)(gmap_off + gmap_n) * 4, 256))) return rc;
  const int rows_cap = P * std::max(cfg->max_patch_h, cfg->max_patch_w);
  std::vector<GemmProblem> probs;
  std::vector<TileRef> t1, t2;
  for (int i = 0; i < n_img; ++i) {
    const ImgDesc& d = D[i];
    const float *CW, *CH;
    if ((rc = dct_matrix(ctx, d.W, std::min(d.W, rows_cap), &CW))) return rc;
    if ((rc = dct_matrix(ctx, d.H, std::min(d.H, rows_cap), &CH))) return rc;
    float* ws = ctx->ws;
    // U[c][y][kx] = sum_ky CH[ky][y] * Ysp[c][ky][kx]
    GemmProblem g1 = gemm(CH, 0, 1, d.H, ws + d.ws_y, (int64_t)d.Kh * d.Kw, 1, d.Kw, ws + d.ws_t,
                          (int64_t)d.H * d.Kw, d.Kw, 1, d.H, d.Kw, d.Kh, 3);
    // X[c][y][x] = sum_kx U[c][y][kx] * CW[kx][x]
    GemmProblem g2 = gemm(ws + d.ws_t, (int64_t)d.H * d.Kw, d.Kw, 1, CW, 0, 1, d.W, ws + d.ws_p,
                          (int64_t)d.H * d.W, d.W, 1, d.H, d.W, d.Kw, 3);
    attach_x3(ctx, g1);
    attach_x3(ctx, g2);
    int pr = (int)probs.size();
    probs.push_back(g1);
    probs.push_back(g2);
    add_tiles(t1, pr, g1);
    add_tiles(t2, pr + 1, g2);
  }
  if (ctx->xcd_order) {   // as the encode's GEMMs (xcd_deal_tiles): speed only
    xcd_deal_tiles(t1, probs.data(), 2);
    xcd_deal_tiles(t2, probs.data(), 1);
  }
  PlanBuf pb;
  size_t d_off = pb.add(D.data(), D.size());
  size_t g_off = pb.add(probs.data(), probs.size());
  size_t t1_off = pb.add(t1.data(), t1.size());
  size_t t2_off = pb.add(t2.data(), t2.size());
  size_t lut_off = pb.add(img_lut, (size_t)n_rows * lut_w);
  order_after_previous(ctx, s);
  if ((rc = upload_plan(ctx, pb, s))) return rc;
  uint8_t* pd = ctx->plan_dev;
  const ImgDesc* dd = (const ImgDesc*)(pd + d_off);
  HIPCHK(ctx, hipMemsetAsync(ctx->ws, 0, (size_t)wsf * 4, s));
  DecodeArgs a{};
  a.ids = ids;
  a.key_pad = key_pad;
  a.pos = pos;
  a.ch = ch;
  a.codes = codes;
  a.patches = patches;
  a.lut = (const int32_t*)(pd + lut_off);
  a.lut_w = lut_w;
  a.S = S;
  a.P = P;
  a.use_codes = codes ? 1 : 0;
  if (codes) {
    a.cb_dim = lfq->codebook_dim;
    a.ncb = lfq->num_codebooks;
    a.scale = lfq->codebook_scale;
    a.median = norm->median_dev;
    a.b = norm->b_dev;
    a.eps = norm->eps;
  }
  a.maxph = cfg->max_patch_h;
  a.maxpw = cfg->max_patch_w;
  a.err = ctx->err_dev;
  int32_t* gmap = (int32_t*)(ctx->ws + gmap_off);
  HIPCHK(ctx, hipMemsetAsync(gmap, 0xFF, (size_t)gmap_n * 4, s));
  {
    Timer t(ctx, s, "dec_map");
    launch_dec_map((int64_t)n_rows * S, dd, a, gmap, s);
  }
  {
    Timer t(ctx, s, "scatter_tokens");
    launch_scatter_tokens((int64_t)n_rows * S, dd, ctx->ws, a, gmap, s);
  }
  {
    Timer t(ctx, s, "idct_cols");
    ctx_gemm(ctx, 3, (const GemmProblem*)(pd + g_off), (const TileRef*)(pd + t1_off), (int)t1.size(), s, 2);
  }
  {
    Timer t(ctx, s, "idct_rows");
    ctx_gemm(ctx, 3, (const GemmProblem*)(pd + g_off), (const TileRef*)(pd + t2_off), (int)t2.size(), s, 1);
  }
  {
    Timer t(ctx, s, "ipt_to_rgb");
    launch_ipt_to_rgb(dd, n_img, max_hw, ctx->ws, rgb, ctx->cm, s);
  }
  HIPCHK(ctx, hipGetLastError());
  mark_done(ctx, s);
  return 0;
}

int dctae_decode(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut, int32_t lut_w,
                 int32_t n_img, const int32_t* out_hw, const int64_t* out_off, const int32_t* patch_hw,
                 const int64_t* ids, const uint8_t* key_pad, const int64_t* pos, const int64_t* ch,
                 const dctae_norm* norm, const dctae_lfq* lfq, const int64_t* codes, const float* patches,
                 float* rgb, void* stream) {
  return decode_impl(ctx, cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos, ch, norm,
                     lfq, codes, patches, rgb, stream, false);
}

int dctae_decode_normed(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut,
                        int32_t lut_w, int32_t n_img, const int32_t* out_hw, const int64_t* out_off,
                        const int32_t* patch_hw, const int64_t* ids, const uint8_t* key_pad, const int64_t* pos,
                        const int64_t* ch, const dctae_norm* norm, const float* normed_patches, float* rgb,
                        void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (n_rows > 0 && !normed_patches) return fail(ctx, DCTAE_EINVAL, "decode needs the PatchNorm-space patches");
  return decode_impl(ctx, cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos, ch, norm,
                     nullptr, nullptr, normed_patches, rgb, stream, true);
}

// ---------------------------------------------------------------------------
// DCTAutoencoder transformer operators (dctae_model.hip)
// ---------------------------------------------------------------------------
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int dctae_model_linear(dctae_ctx* ctx, int64_t M, int32_t N, int32_t K, const uint16_t* x, int64_t ldx,
                       const uint16_t* w, int32_t w_rows, int64_t ldw, const float* bias, int32_t epilogue, void* out,
                       int64_t ldo, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (M < 0 || N <= 0 || K <= 0 || K % 64 || w_rows < N || ldx < K || ldw < K || ldx % 8 || ldw % 8 || ldo < N)
    return fail(ctx, DCTAE_EINVAL, "model_linear: bad shape (K % 64, ld % 8, w_rows >= N, ld >= K / N)");
  if (epilogue < DCTAE_LIN_F32 || epilogue > DCTAE_LIN_F32_RESIDUAL) return fail(ctx, DCTAE_EINVAL, "model_linear: epilogue");
  if (M == 0) return 0;
  if (!x || !w || !out || !al16(x) || !al16(w)) return fail(ctx, DCTAE_EINVAL, "model_linear: null or unaligned tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  LinearArgs a{x, w, bias, out, M, ldx, ldw, ldo, N, w_rows, K};
  Timer t(ctx, s, "model_linear");
  launch_linear(a, epilogue, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_model_attention(dctae_ctx* ctx, int32_t R, int32_t S, int32_t heads, int32_t head_dim, const uint16_t* qkv,
                          const int64_t* ids, const uint8_t* key_pad, uint16_t* out, int64_t ldo, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (head_dim != 64) return fail(ctx, DCTAE_EUNSUP, "model_attention: head_dim must be 64");
  if (R < 0 || S <= 0 || heads <= 0 || ldo < 64ll * heads || ldo % 8)
    return fail(ctx, DCTAE_EINVAL, "model_attention: bad shape");
  if (R == 0) return 0;
  if (!qkv || !ids || !key_pad || !out || !al16(qkv) || !al16(out))
    return fail(ctx, DCTAE_EINVAL, "model_attention: null or unaligned tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  AttnArgs a{qkv, ids, key_pad, out, R, S, heads, (int32_t)ldo, 0.125f};
  Timer t(ctx, s, "model_attention");
  launch_attention(a, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

static int ln_check(dctae_ctx* ctx, int64_t M, int32_t D, const float* x, const float* g, const float* b) {
  if (M < 0 || D <= 0 || D > 4096) return fail(ctx, DCTAE_EINVAL, "model layernorm: bad shape (D <= 4096)");
  if (M > 0 && (!x || !g || !b)) return fail(ctx, DCTAE_EINVAL, "model layernorm: null tensor");
  return 0;
}

int dctae_model_layernorm(dctae_ctx* ctx, int64_t M, int32_t D, const float* x, int64_t ldx, const float* g,
                          const float* b, float eps, uint16_t* out, int64_t ldo, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  int rc = ln_check(ctx, M, D, x, g, b);
  if (rc || M == 0) return rc;
  if (!out) return fail(ctx, DCTAE_EINVAL, "model_layernorm: null output");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  LnArgs a{};
  a.x = x; a.gamma = g; a.beta = b; a.out_bf16 = out; a.M = M; a.ldx = ldx; a.ldo = ldo; a.D = D; a.eps = eps;
  Timer t(ctx, s, "model_layernorm");
  launch_layernorm(a, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_model_embed_norm(dctae_ctx* ctx, int64_t M, int32_t D, const float* x, int64_t ldx, const float* g,
                           const float* b, float eps, const float* ph, const float* pw, const float* pc,
                           const int64_t* ch, const int64_t* pos, float* out, int64_t ldo, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  int rc = ln_check(ctx, M, D, x, g, b);
  if (rc || M == 0) return rc;
  if (!out || !ph || !pw || !pc || !ch || !pos) return fail(ctx, DCTAE_EINVAL, "model_embed_norm: null tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  LnArgs a{};
  a.x = x; a.gamma = g; a.beta = b; a.out_f32 = out; a.pos_h = ph; a.pos_w = pw; a.pos_c = pc; a.ch = ch;
  a.pos = pos; a.M = M; a.ldx = ldx; a.ldo = ldo; a.D = D; a.eps = eps;
  Timer t(ctx, s, "model_embed_norm");
  launch_layernorm(a, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_model_pos_add(dctae_ctx* ctx, int64_t M, int32_t D, float* x, int64_t ldx, const float* ph, const float* pw,
                        const float* pc, const int64_t* ch, const int64_t* pos, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (M < 0 || D <= 0) return fail(ctx, DCTAE_EINVAL, "model_pos_add: bad shape");
  if (M == 0) return 0;
  if (!x || !ph || !pw || !pc || !ch || !pos) return fail(ctx, DCTAE_EINVAL, "model_pos_add: null tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  PosArgs a{x, ph, pw, pc, ch, pos, M, ldx, D};
  Timer t(ctx, s, "model_pos_add");
  launch_pos_add(a, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_model_to_bf16(dctae_ctx* ctx, int64_t M, int32_t K, const float* x, int64_t ldx, int32_t Kp, uint16_t* out,
                        void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (M < 0 || K < 0 || Kp < K || ldx < K) return fail(ctx, DCTAE_EINVAL, "model_to_bf16: bad shape");
  if (M == 0 || Kp == 0) return 0;
  if (!x || !out) return fail(ctx, DCTAE_EINVAL, "model_to_bf16: null tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "model_to_bf16");
  launch_to_bf16(x, ldx, M, K, Kp, out, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_model_lfq(dctae_ctx* ctx, int64_t M, int32_t ncb, int32_t cbd, float scale, const float* x, int64_t ldx,
                    int64_t* codes, uint16_t* q_bf16, float* q_f32, int64_t ldq, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (M < 0 || ncb <= 0 || cbd <= 0 || cbd > 62 || ldx < (int64_t)ncb * cbd || ((q_bf16 || q_f32) && ldq < (int64_t)ncb * cbd))
    return fail(ctx, DCTAE_EINVAL, "model_lfq: bad shape");
  if (M == 0) return 0;
  if (!x || !codes) return fail(ctx, DCTAE_EINVAL, "model_lfq: null tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  LfqArgs a{x, codes, q_bf16, q_f32, M, ldx, ldq, ncb, cbd, scale};
  Timer t(ctx, s, "model_lfq");
  launch_lfq_codes(a, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

}  // extern "C"
