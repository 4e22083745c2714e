// The context behind the C ABI and what its host units share: error
// reporting, per-launch timing, the ordered call scope through which every
// call reaches the context's scratch, and the planning helpers of
// dctae_plan.hip.  Host code only (no kernels).
//   dctae_api.hip      context, options, timing, scratch growth and plan upload
//   dctae_plan.hip     DCT matrices, GEMM problems and tile lists, FFT / Bluestein plans
//   dctae_encode.hip   the encode plan and launch sequence
//   dctae_enc_layout.h the encode plan's routes, workspace regions, chunk cut and staging carve (no HIP calls)
//   dctae_decode.hip   the decode family's planner (DecodeBatch, below) and the one decode launch sequence
//   dctae_dec_layout.h the decode family's path choice and workspace layouts, forward and backward (no HIP calls)
//   dctae_frames.hip   the frame kernels and image_clip; dctae_decode_frames plans through decode_impl
//   dctae_decode_bwd.hip  the decode's backward and the pixel loss (kernels and launch sequence)
//   dctae_api_ops.hip  PatchNorm, LFQ, VectorQuantize and transformer entry points
#pragma once
#include <cmath>
#include <complex>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/dctae.h"
#include "../../include/dctae_frames.h"
#include "dctae_internal.h"
#include "dctae_launch.h"
#include "dctae_options.h"

struct TimedLaunch {
  const char* name;
  hipEvent_t a, b;
};

struct TimingEntry {
  std::string name;
  double ms = 0.0;
  int64_t launches = 0;
};

namespace dctae {

class OrderedCall;

// a grow-only device buffer of the context
struct DevBuf {
  uint8_t* p = nullptr;
  size_t cap = 0;
  // at least `need` bytes; growing waits for the whole device before it frees
  int grow(dctae_ctx* ctx, size_t need, const char* what);
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// the scratch buffers successive calls share (OrderedCall::scratch)
enum Scratch { kWs, kStage, kStats, kVq, kProj, kNumScratch };

}  // namespace dctae

struct dctae_ctx {
  int device = 0;
  std::string err;
  dctae::Options opt;   // the dctae_set_option switches (dctae_options.h)
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
  uint64_t plan_counter = 0;   // ids of cached plans (OrderedCall::upload)
  // the encode's side stream (SideStream in dctae_encode.hip; created on first use)
  hipStream_t side = nullptr;
  hipEvent_t side_in = nullptr, side_out = nullptr;
  int* err_dev = nullptr;
  dctae::ColorMats cm{};
  // FFT-DCT plans: tables (W_M^k, alpha/beta) in one device buffer
  float2* fft_tab = nullptr;
  int64_t fft_tab_cap = 0, fft_tab_used = 0;
  std::map<int, dctae::FftPlan> fft_plans;   // N -> plan (N = 0 entries never stored)
  std::map<int, dctae::FftPlan> bs_plans;    // N -> Bluestein plan (kind 1; kind 0 = none)
  std::map<int, int64_t> bs_tw;              // L -> offset of W_L^m in fft_tab
  size_t lds_limit = 64 * 1024;              // dynamic LDS the FFT kernels may use
  int n_cu = 256;
  // cached encode plan: valid for enc_key (the call's inputs and the
  // plan-shaping options) while the workspace stays where the plan was built (EncPlan::ws)
  std::vector<int64_t> enc_key;
  struct EncPlan* enc_plan = nullptr;
  // timing
  bool timing = false;
  std::vector<TimedLaunch> pending;
  std::vector<hipEvent_t> evt_pool;
  std::vector<TimingEntry> totals;

 private:
  // What successive calls reuse, reachable only through an open OrderedCall:
  // the scratch buffers (workspace; token staging; PatchNorm statistics; the
  // VectorQuantize vectors, codes and codebook; the LFQ projections' pre-split
  // weight), the plan (pinned host and device copies, the last uploaded bytes
  // for caching) and the event that orders one call after the previous one.
  friend class dctae::OrderedCall;
  friend int ::dctae_ctx_create(int, dctae_ctx**);
  friend int ::dctae_ctx_destroy(dctae_ctx*);
  dctae::DevBuf scratch[dctae::kNumScratch], plan;
  uint8_t* plan_host = nullptr;
  std::vector<uint8_t> plan_last;
  uint64_t plan_last_id = 0;
  hipEvent_t plan_evt = nullptr;
  hipEvent_t done_evt = nullptr;
  hipStream_t last_stream = nullptr;
  bool have_done = false;
};

namespace dctae {

// the last error of a call that had no context to keep it (dctae_last_error(NULL))
extern thread_local std::string g_err;

inline int fail(dctae_ctx* ctx, int code, const std::string& msg) {
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
// a list of the plan: where it starts in the buffer, how many T it holds
template <class T>
struct PlanList {
  size_t off = 0;
  int n = 0;
  const T* at(const uint8_t* pd) const { return reinterpret_cast<const T*>(pd + off); }
};

struct PlanBuf {
  std::vector<uint8_t> bytes;
  template <class T>
  size_t add(const T* p, size_t n) {
    size_t off = (bytes.size() + 255) & ~size_t(255);
    bytes.resize(off + n * sizeof(T));
    if (n) std::memcpy(bytes.data() + off, p, n * sizeof(T));
    return off;
  }
  // an empty list is added too: it pads the buffer to the next 256 bytes
  template <class T>
  PlanList<T> add(const std::vector<T>& v) {
    return {add(v.data(), v.size()), (int)v.size()};
  }
};

inline int DevBuf::grow(dctae_ctx* ctx, size_t need, const char* what) {
  if (need <= cap) return 0;
  HIPCHK(ctx, hipDeviceSynchronize());   // the previous user may have run on another stream
  release();
  if (hipMalloc((void**)&p, need) != hipSuccess) {
    p = nullptr;
    return fail(ctx, DCTAE_ENOMEM, std::string(what) + " allocation of " + std::to_string(need) + " bytes failed");
  }
  cap = need;
  return 0;
}

// One call's use of the context's scratch and plan.  The constructor orders
// the call's stream after the context's previous ordered call on another
// stream (on the same stream it does nothing); the destructor records, on
// every exit path, the event the next call waits for.  Declare it before the
// call's Timers and its SideStream: their destructors (the timer's end event,
// the side stream's join) then run before the record.
class OrderedCall {
 public:
  dctae_ctx* const ctx;
  const hipStream_t s;
  OrderedCall(dctae_ctx* c, hipStream_t st) : ctx(c), s(st) {
    if (ctx->have_done && ctx->last_stream != s) hipStreamWaitEvent(s, ctx->done_evt, 0);
  }
  ~OrderedCall() {
    hipEventRecord(ctx->done_evt, s);
    ctx->last_stream = s;
    ctx->have_done = true;
  }
  OrderedCall(const OrderedCall&) = delete;
  // *out = the scratch buffer `which`, grown to at least `bytes` (0: as it is)
  template <class T>
  int scratch(Scratch which, size_t bytes, T** out) {
    uint8_t* p = nullptr;
    const int rc = scratch_bytes(which, bytes, &p);
    *out = reinterpret_cast<T*>(p);
    return rc;
  }
  // *base = the device copy of pb (uploaded on s unless the plan buffer holds
  // these bytes already: the same non-zero plan_id, or equal bytes)
  int upload(const PlanBuf& pb, uint8_t** base, uint64_t plan_id = 0);

 private:
  int scratch_bytes(Scratch which, size_t bytes, uint8_t** out);
  unsigned poisoned = 0;   // Options::ws_poison: the buffers this call has filled, one bit each
};

inline void ctx_gemm(const dctae_ctx* ctx, int nc, const GemmProblem* probs, const TileRef* tiles, int n_tiles,
                     hipStream_t s, int share = 0) {
  if (ctx->opt.gemm_x3)
    launch_gemm_x3(nc, probs, tiles, n_tiles, s, share);
  else
    launch_gemm(nc, probs, tiles, n_tiles, s, share);
}

// ---- dctae_plan.hip ----
int dct_matrix(dctae_ctx* ctx, int N, int rows, const float** out, int parity = -1);
void attach_x3(const dctae_ctx* ctx, GemmProblem& g);
int check_cfg(dctae_ctx* ctx, const dctae_fe_cfg* cfg);
int check_lfq(dctae_ctx* ctx, const dctae_lfq* lfq, int PP);
int describe(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int H, int W, ImgDesc& d);
GemmProblem gemm(const float* A, int64_t sAc, int64_t sAm, int64_t sAk, const float* B, int64_t sBc, int64_t sBn,
                 int64_t sBk, float* O, int64_t sOc, int64_t sOm, int64_t sOn, int M, int N, int K, int C);
void xcd_deal_tiles(std::vector<TileRef>& t, const GemmProblem* probs, int share);
void xcd_deal_col_blocks(std::vector<int4>& L);
void add_tiles(std::vector<TileRef>& t, int prob, const GemmProblem& g);
EncParams enc_params(const dctae_fe_cfg* cfg, const dctae_norm* norm, const dctae_lfq* lfq);
int next_pow2(int x);
int bs_plan_for(dctae_ctx* ctx, int N, FftPlan* out);
int fft_plan_for(dctae_ctx* ctx, int N, int P, FftPlan* out);
// the Bluestein block lists of a chunk job are kept per FFT length L
inline int bs_lidx(int L) { return L == 256 ? 0 : L == 512 ? 1 : L == 1024 ? 2 : 3; }
constexpr int kBsL[4] = {256, 512, 1024, 2048};

// ---- dctae_decode.hip: what the decodes, dctae_decode_frames and dctae_decode_backward share ----
// the packed batch as the entry points take it (include/dctae.h)
struct DecodeBatch {
  const dctae_fe_cfg* cfg;
  int32_t n_rows;
  const int32_t* img_lut;
  int32_t lut_w, n_img;
  const int32_t* out_hw;
  const int64_t* out_off;
  const int32_t* patch_hw;
  const int64_t* ids;
  const uint8_t* key_pad;
  const int64_t *pos, *ch;
  hipStream_t s;
};
inline DecodeBatch decode_batch(const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut, int32_t lut_w,
                                int32_t n_img, const int32_t* out_hw, const int64_t* out_off, const int32_t* patch_hw,
                                const int64_t* ids, const uint8_t* key_pad, const int64_t* pos, const int64_t* ch,
                                void* stream) {
  return {cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos, ch, (hipStream_t)stream};
}
int decode_check(dctae_ctx* ctx, const DecodeBatch& B, const char* own, bool img_bufs, bool tok_bufs);
int decode_geometry(dctae_ctx* ctx, const DecodeBatch& B, std::vector<ImgDesc>& D, int64_t* max_hw);
int decode_gemm_pair(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const ImgDesc& d, float* ws, GemmProblem* g1,
                     GemmProblem* g2, const float** CW, const float** CH);
// the caller's codes with their type as a tag (int64 from dctae.h, int16 from dctae_codes16.h)
struct CodeSrc {
  const void* p = nullptr;
  CodeType type = CodeType::kI64;
  CodeSrc() = default;
  CodeSrc(const int64_t* c) : p(c) {}
  CodeSrc(const int16_t* c) : p(c), type(CodeType::kI16) {}
  explicit operator bool() const { return p != nullptr; }
};
// int16 codes hold codebook_dim <= 15 bits (dctae_codes16.h); 0, or the refusal
int check_codes16(dctae_ctx* ctx, const dctae_lfq* lfq);
DecodeArgs decode_args(const dctae_ctx* ctx, const DecodeBatch& B, const dctae_norm* norm, const dctae_lfq* lfq,
                       const void* codes, const float* patches, const int32_t* lut, bool normed);
// the call body of every decode entry.  fr = NULL: the batch's images into out at B.out_off; else the frames of
// fr into out at fr->out_off (B.out_off unused), with clip the image_clip of each
int decode_impl(dctae_ctx* ctx, const DecodeBatch& B, const dctae_norm* norm, const dctae_lfq* lfq,
                const CodeSrc& codes, const float* patches, void* out, PixelType px, bool normed,
                const dctae_frames* fr = nullptr, bool clip = false);

// ---- dctae_frames.hip ----
int frames_check(dctae_ctx* ctx, const DecodeBatch& B, const dctae_frames* fr);
// descs / mm on the device; two timed stages: clip_minmax, clip_store
int clip_launch(dctae_ctx* ctx, const ClipSpan* descs, int n, int64_t max_n, const float* in, uint32_t* mm, void* out,
                PixelType px, hipStream_t s);

// ---- dctae_encode.hip ----
void drop_encode_plan(dctae_ctx* ctx);   // dctae_ctx_destroy: EncPlan is complete only there

}  // namespace dctae
