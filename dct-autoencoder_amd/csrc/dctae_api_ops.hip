// C ABI entry points of the single operators: PatchNorm and its statistics,
// LFQ (entropy and projections included), VectorQuantize, the transformer
// operators of dctae_model.hip and the fused optimizer step of dctae_optim.hip.
#include "dctae_ctx.h"
#include "dctae_model.h"
#include "../../include/dctae_codes16.h"

using namespace dctae;

extern "C" {

int dctae_norm_thresholds(dctae_ctx* ctx, const dctae_norm* norm, int64_t n, float* thr_dev, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!norm || !norm->median_dev || !norm->b_dev || !thr_dev || n < 0)
    return fail(ctx, DCTAE_EINVAL, "bad threshold arguments");
  hipStream_t s = (hipStream_t)stream;
  OrderedCall oc(ctx, s);   // clears and reads the shared ctx->err_dev
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

// ---- reconstruction losses (main.py:71, 79-83) and inverse PatchNorm's gradient, dctae_rec_loss.hip ----
static int rec_loss_check(dctae_ctx* ctx, const dctae_norm* norm, int32_t P, int32_t mh, int32_t mw, int64_t n) {
  if (!norm || !norm->median_dev || !norm->b_dev) return fail(ctx, DCTAE_EINVAL, "PatchNorm tables are NULL");
  if (P < 1 || P > 1024 || mh < 1 || mw < 1 || n < 0) return fail(ctx, DCTAE_EINVAL, "bad PatchNorm shape");
  if (!rec_loss_supported(n, P * P)) return fail(ctx, DCTAE_EUNSUP, "reconstruction losses: too many tokens in one call");
  return 0;
}

int dctae_norm_inverse_backward(dctae_ctx* ctx, const dctae_norm* norm, int32_t P, int32_t mh, int32_t mw,
                                const float* grad, const int64_t* ch, const int64_t* pos, int64_t n, float* dy,
                                void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  hipSetDevice(ctx->device);
  if (int rc = rec_loss_check(ctx, norm, P, mh, mw, n)) return rc;
  if (n == 0) return 0;
  if (!grad || !ch || !pos || !dy) return fail(ctx, DCTAE_EINVAL, "NULL tensor");
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "norm_inverse_backward");
  launch_rec_loss_bwd(nullptr, nullptr, nullptr, ch, pos, nullptr, n, P * P, mh, mw, norm->median_dev, norm->b_dev,
                      norm->eps, nullptr, nullptr, grad, dy, ctx->err_dev, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_rec_loss_forward(dctae_ctx* ctx, const dctae_norm* norm, int32_t P, int32_t mh, int32_t mw, const float* out,
                           const float* tn, const float* raw, const int64_t* ch, const int64_t* pos,
                           const uint8_t* key_pad, int64_t n, float* unnorm, float* scalars, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  hipSetDevice(ctx->device);
  if (int rc = rec_loss_check(ctx, norm, P, mh, mw, n)) return rc;
  if (!scalars) return fail(ctx, DCTAE_EINVAL, "NULL output");
  if (n > 0 && (!out || !tn || !raw || !ch || !pos || !key_pad)) return fail(ctx, DCTAE_EINVAL, "NULL tensor");
  hipStream_t s = (hipStream_t)stream;
  OrderedCall oc(ctx, s);
  float* ws;   // the block partials
  if (int rc = oc.scratch(kWs, rec_loss_ws_bytes(n, P * P), &ws)) return rc;
  Timer t(ctx, s, "rec_loss_forward");
  launch_rec_loss_fwd(out, tn, raw, ch, pos, key_pad, n, P * P, mh, mw, norm->median_dev, norm->b_dev, norm->eps,
                      unnorm, ws, scalars, ctx->err_dev, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_rec_loss_backward(dctae_ctx* ctx, const dctae_norm* norm, int32_t P, int32_t mh, int32_t mw,
                            const float* out, const float* tn, const float* raw, const int64_t* ch, const int64_t* pos,
                            const uint8_t* key_pad, int64_t n, const float* scalars, const float* grad,
                            const float* grad_unnorm, float* dout, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  hipSetDevice(ctx->device);
  if (int rc = rec_loss_check(ctx, norm, P, mh, mw, n)) return rc;
  if (!scalars || !grad) return fail(ctx, DCTAE_EINVAL, "NULL tensor");
  if (n == 0) return 0;
  if (!out || !tn || !raw || !ch || !pos || !key_pad || !dout) return fail(ctx, DCTAE_EINVAL, "NULL tensor");
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "rec_loss_backward");
  launch_rec_loss_bwd(out, tn, raw, ch, pos, key_pad, n, P * P, mh, mw, norm->median_dev, norm->b_dev, norm->eps,
                      scalars, grad, grad_unnorm, dout, ctx->err_dev, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

// ---- PatchNorm training (patchnorm.py:101-155), kernels in dctae_stats.hip ----
namespace {

struct StatsScratch {
  int32_t *cell, *count, *start, *list;
  float* bn;       // (n_cells) batch counts
  float *t0, *t1;  // two (n_cells, PP) tables (batch median / batch b)
};

int stats_scratch(OrderedCall& oc, int64_t n_tok, int n_cells, int PP, bool tables, StatsScratch* o) {
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t b_tok = al(sizeof(int32_t) * std::max<int64_t>(n_tok, 1));
  const size_t b_cell = al(sizeof(int32_t) * n_cells);
  const size_t b_tab = tables ? al(sizeof(float) * (size_t)n_cells * PP) : 0;
  uint8_t* p;
  if (int rc = oc.scratch(kStats, 2 * b_tok + 3 * b_cell + 2 * b_tab, &p)) return rc;
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
  OrderedCall oc(ctx, s);
  StatsScratch w;
  if (int rc = stats_scratch(oc, n_tok, n_cells, PP, false, &w)) return rc;
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
  OrderedCall oc(ctx, s);
  StatsScratch w;
  if (int rc = stats_scratch(oc, n_tok, n_cells, PP, false, &w)) return rc;
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
  OrderedCall oc(ctx, s);
  StatsScratch w;
  if (int rc = stats_scratch(oc, n_tok, n_cells, PP, true, &w)) return rc;
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
  hipStream_t s = (hipStream_t)stream;
  OrderedCall oc(ctx, s);
  float* ws;   // the partial histograms
  if ((rc = oc.scratch(kWs, sizeof(float) * lfq_entropy_fwd_ws_floats(n_tok, lfq->num_codebooks, lfq->codebook_dim),
                       &ws)))
    return rc;
  Timer t(ctx, s, "lfq_entropy_forward");
  launch_lfq_entropy_fwd(h, mask, n_tok, lfq->num_codebooks, lfq->codebook_dim, lfq->codebook_scale, temperature, eps,
                         ws, avg_probs, scalars, s);
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
  hipStream_t s = (hipStream_t)stream;
  OrderedCall oc(ctx, s);
  float* ws;
  if ((rc = oc.scratch(kWs, sizeof(float) * lfq_entropy_bwd_ws_floats(lfq->codebook_dim), &ws))) return rc;
  Timer t(ctx, s, "lfq_entropy_backward");
  if (launch_lfq_entropy_bwd(h, mask, n_tok, lfq->num_codebooks, lfq->codebook_dim, lfq->codebook_scale, temperature,
                             eps, avg_probs, scalars, grad, ws, dh, s))
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

// idx / ct: the caller's indices and their type (int16: dctae_codes16.h)
static int lfq_project_in_impl(dctae_ctx* ctx, const dctae_lfq* lfq, const float* x, int64_t n, int32_t dim,
                               const float* w, const float* b, float x_bound, void* idx, CodeType ct, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (int rc = lfq_proj_check(ctx, lfq, n, dim, x, w, idx, 64)) return rc;
  if (ct == CodeType::kI16) {
    if (int rc = check_codes16(ctx, lfq)) return rc;
    if ((uintptr_t)idx & 1) return fail(ctx, DCTAE_EINVAL, "int16 indices must be 2-byte aligned");
  }
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  OrderedCall oc(ctx, s);
  uint16_t* wsp;   // the pre-split weight
  if (int rc = oc.scratch(kProj, lfq_proj_scratch_bytes(lfq->codebook_dim * lfq->num_codebooks, dim), &wsp)) return rc;
  Timer t(ctx, s, "lfq_project_in");
  const float xb = ctx->opt.gemm_h2 ? x_bound : 0.0f;
  if (ct == CodeType::kI16)
    launch_lfq_project_in_c16(x, n, dim, w, b, lfq->codebook_dim, lfq->num_codebooks, lfq->codebook_scale,
                              static_cast<int16_t*>(idx), wsp, s, xb, ctx->opt.lfq_ws != 0);
  else
    launch_lfq_project_in(x, n, dim, w, b, lfq->codebook_dim, lfq->num_codebooks, lfq->codebook_scale,
                          static_cast<int64_t*>(idx), wsp, s, xb, ctx->opt.lfq_ws != 0);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_lfq_project_in(dctae_ctx* ctx, const dctae_lfq* lfq, const float* x, int64_t n, int32_t dim,
                         const float* w, const float* b, int64_t* idx, void* stream) {
  return lfq_project_in_impl(ctx, lfq, x, n, dim, w, b, 0.0f, idx, CodeType::kI64, stream);
}

int dctae_lfq_project_in_c16(dctae_ctx* ctx, const dctae_lfq* lfq, const float* x, int64_t n, int32_t dim,
                             const float* w, const float* b, int16_t* idx, void* stream) {
  return lfq_project_in_impl(ctx, lfq, x, n, dim, w, b, 0.0f, idx, CodeType::kI16, stream);
}

int dctae_lfq_project_in_bounded(dctae_ctx* ctx, const dctae_lfq* lfq, const float* x, int64_t n, int32_t dim,
                                 const float* w, const float* b, float x_bound, int64_t* idx, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!(x_bound > 0.0f) || !std::isfinite(x_bound)) return fail(ctx, DCTAE_EINVAL, "x_bound must be finite and > 0");
  return lfq_project_in_impl(ctx, lfq, x, n, dim, w, b, x_bound, idx, CodeType::kI64, stream);
}

// the checks project_out's two forms share; int16 indices (dctae_codes16.h) are
// loaded one by one, so they need 2-byte alignment where int64 ones need 16
static int lfq_project_out_check(dctae_ctx* ctx, const dctae_lfq* lfq, const CodeSrc& idx, int64_t n, int32_t dim,
                                 const float* w, const float* out) {
  const bool c16 = idx.type == CodeType::kI16;
  if (int rc = lfq_proj_check(ctx, lfq, n, dim, c16 ? (const void*)w : idx.p, w, out, 32, true)) return rc;
  if (!c16) return 0;
  if (n > 0 && !idx.p) return fail(ctx, DCTAE_EINVAL, "bad LFQ projection tensors");
  if ((uintptr_t)idx.p & 1) return fail(ctx, DCTAE_EINVAL, "int16 indices must be 2-byte aligned");
  return check_codes16(ctx, lfq);
}

static int lfq_project_out_impl(dctae_ctx* ctx, const dctae_lfq* lfq, const CodeSrc& idx, int64_t n, int32_t dim,
                                const float* w, const float* b, float* out, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (int rc = lfq_project_out_check(ctx, lfq, idx, n, dim, w, out)) return rc;
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  OrderedCall oc(ctx, s);
  uint16_t* wsp;
  if (int rc = oc.scratch(kProj, lfq_proj_scratch_bytes(dim, lfq->codebook_dim * lfq->num_codebooks), &wsp)) return rc;
  Timer t(ctx, s, "lfq_project_out");
  launch_lfq_project_out(idx.p, n, dim, w, b, lfq->codebook_dim, lfq->num_codebooks, lfq->codebook_scale, out, wsp, s,
                         nullptr, nullptr, nullptr, nullptr, 0.f, 0, 0, nullptr, ctx->opt.gemm_h2 != 0,
                         ctx->opt.lfq_ws != 0, idx.type);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_lfq_project_out(dctae_ctx* ctx, const dctae_lfq* lfq, const int64_t* idx, int64_t n, int32_t dim,
                          const float* w, const float* b, float* out, void* stream) {
  return lfq_project_out_impl(ctx, lfq, idx, n, dim, w, b, out, stream);
}

int dctae_lfq_project_in_bounded_c16(dctae_ctx* ctx, const dctae_lfq* lfq, const float* x, int64_t n, int32_t dim,
                                     const float* w, const float* b, float x_bound, int16_t* idx, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!(x_bound > 0.0f) || !std::isfinite(x_bound)) return fail(ctx, DCTAE_EINVAL, "x_bound must be finite and > 0");
  return lfq_project_in_impl(ctx, lfq, x, n, dim, w, b, x_bound, idx, CodeType::kI16, stream);
}

int dctae_lfq_project_out_c16(dctae_ctx* ctx, const dctae_lfq* lfq, const int16_t* idx, int64_t n, int32_t dim,
                              const float* w, const float* b, float* out, void* stream) {
  return lfq_project_out_impl(ctx, lfq, idx, n, dim, w, b, out, stream);
}

static int lfq_project_out_inverse_norm_impl(dctae_ctx* ctx, const dctae_lfq* lfq, const CodeSrc& idx, int64_t n,
                                             int32_t dim, const float* w, const float* b, const dctae_norm* norm,
                                             int32_t max_patch_h, int32_t max_patch_w, const int64_t* channels,
                                             const int64_t* positions, float* out, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (int rc = lfq_project_out_check(ctx, lfq, idx, n, dim, w, out)) return rc;
  if (!norm || !norm->median_dev || !norm->b_dev || max_patch_h < 1 || max_patch_w < 1 ||
      (n > 0 && (!channels || !positions)))
    return fail(ctx, DCTAE_EINVAL, "inverse PatchNorm needs tables, max_patch_h/w and channels / positions");
  // the fused inverse reads the (3, max_patch_h, max_patch_w, dim) tables and
  // writes out as float4 pieces along each token's dim floats
  if (((uintptr_t)norm->median_dev | (uintptr_t)norm->b_dev | (uintptr_t)out) & 15)
    return fail(ctx, DCTAE_EINVAL, "fused inverse PatchNorm needs 16-byte aligned median / b / out");
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  OrderedCall oc(ctx, s);
  uint16_t* wsp;
  if (int rc = oc.scratch(kProj, lfq_proj_scratch_bytes(dim, lfq->codebook_dim * lfq->num_codebooks), &wsp)) return rc;
  Timer t(ctx, s, "lfq_project_out");
  launch_lfq_project_out(idx.p, n, dim, w, b, lfq->codebook_dim, lfq->num_codebooks, lfq->codebook_scale, out, wsp, s,
                         channels, positions, norm->median_dev, norm->b_dev, norm->eps, max_patch_h, max_patch_w,
                         ctx->err_dev, ctx->opt.gemm_h2 != 0, ctx->opt.lfq_ws != 0, idx.type);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_lfq_project_out_inverse_norm(dctae_ctx* ctx, const dctae_lfq* lfq, const int64_t* idx, int64_t n,
                                       int32_t dim, const float* w, const float* b, const dctae_norm* norm,
                                       int32_t max_patch_h, int32_t max_patch_w, const int64_t* channels,
                                       const int64_t* positions, float* out, void* stream) {
  return lfq_project_out_inverse_norm_impl(ctx, lfq, idx, n, dim, w, b, norm, max_patch_h, max_patch_w, channels,
                                           positions, out, stream);
}

int dctae_lfq_project_out_inverse_norm_c16(dctae_ctx* ctx, const dctae_lfq* lfq, const int16_t* idx, int64_t n,
                                           int32_t dim, const float* w, const float* b, const dctae_norm* norm,
                                           int32_t max_patch_h, int32_t max_patch_w, const int64_t* channels,
                                           const int64_t* positions, float* out, void* stream) {
  return lfq_project_out_inverse_norm_impl(ctx, lfq, idx, n, dim, w, b, norm, max_patch_h, max_patch_w, channels,
                                           positions, out, stream);
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

// O (n, N) = A (n, K) W^T (N, K) + bias, on k_gemm_f32 (plan uploaded through the shared plan buffer)
static int vq_linear(OrderedCall& oc, const float* A, int64_t n, int K, const float* W, const float* bias, int N,
                     float* O, const uint8_t* mask, const float* orig, const char* name) {
  dctae_ctx* ctx = oc.ctx;
  const hipStream_t s = oc.s;
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
  uint8_t* pd;
  if (int rc = oc.upload(pb, &pd)) return rc;
  Timer tm(ctx, s, name);
  ctx_gemm(ctx, 1, (const GemmProblem*)(pd + g_off), (const TileRef*)(pd + t_off), (int)t.size(), s);
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
  OrderedCall oc(ctx, s);
  uint8_t* p;
  if ((rc = oc.scratch(kVq, acc_b + et_b + y2_b + (proj ? v_b : 0) + ((need_xq && (proj || mask)) ? v_b : 0), &p)))
    return rc;
  double* acc = (double*)p;
  float* et = (float*)(p + acc_b);
  float* y2 = (float*)(p + acc_b + et_b);
  uint8_t* q = p + acc_b + et_b + y2_b;
  float* xp = proj ? (float*)q : const_cast<float*>(x);
  if (proj) q += v_b;
  // codes: straight into quantize when nothing follows them
  float* xq = need_xq ? ((proj || mask) ? (float*)q : quantize) : nullptr;
  if (proj &&
      (rc = vq_linear(oc, x, n_tok, vq->dim, vq->w_in_dev, vq->b_in_dev, HD, xp, nullptr, nullptr, "vq_project_in")))
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
      if ((rc = vq_linear(oc, xq, n_tok, HD, vq->w_out_dev, vq->b_out_dev, vq->dim, quantize, mask, x, "vq_project_out")))
        return rc;
    } else if (mask) {
      HIPCHK(ctx, hipMemcpyAsync(quantize, xq, sizeof(float) * nv * D, hipMemcpyDeviceToDevice, s));
      launch_vq_bias(quantize, nullptr, n_tok, HD, mask, x, s);
    }
  }
  HIPCHK(ctx, hipGetLastError());
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
  OrderedCall oc(ctx, s);
  float* codes;
  if ((rc = oc.scratch(kVq, ((size_t)n * HD * 4 + 255) & ~size_t(255), &codes))) return rc;
  {
    Timer t(ctx, s, "vq_codes");
    launch_vq_codes(idx, n * vq->heads, vq->embed_dev, vq->codebook_size, codes, ctx->err_dev, s);
  }
  if ((rc = vq_linear(oc, codes, n, HD, vq->w_out_dev, vq->b_out_dev, vq->dim, out, nullptr, nullptr, "vq_project_out")))
    return rc;
  HIPCHK(ctx, hipGetLastError());
  return 0;
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

// ---------------------------------------------------------------------------
// training: the forward's attention with its log-sum-exp, and the backward
// operators (dctae_model_bwd.hip)
// ---------------------------------------------------------------------------
int dctae_model_attention_lse(dctae_ctx* ctx, int32_t R, int32_t S, int32_t heads, int32_t head_dim, const uint16_t* qkv,
                              const int64_t* ids, const uint8_t* key_pad, uint16_t* out, int64_t ldo, float* lse,
                              void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (head_dim != 64) return fail(ctx, DCTAE_EUNSUP, "model_attention_lse: head_dim must be 64");
  if (R < 0 || S <= 0 || heads <= 0 || ldo < 64ll * heads || ldo % 8)
    return fail(ctx, DCTAE_EINVAL, "model_attention_lse: bad shape");
  if (R == 0) return 0;
  if (!qkv || !ids || !key_pad || !out || !lse || !al16(qkv) || !al16(out))
    return fail(ctx, DCTAE_EINVAL, "model_attention_lse: null or unaligned tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  AttnArgs a{qkv, ids, key_pad, out, R, S, heads, (int32_t)ldo, 0.125f, lse};
  Timer t(ctx, s, "model_attention_lse");
  launch_attention(a, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_model_attention_bwd(dctae_ctx* ctx, int32_t R, int32_t S, int32_t heads, int32_t head_dim, const uint16_t* qkv,
                              const int64_t* ids, const uint8_t* key_pad, const uint16_t* out, int64_t ldo,
                              const uint16_t* d_out, int64_t lddo, const float* lse, float* delta_ws, uint16_t* dqkv,
                              void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (head_dim != 64) return fail(ctx, DCTAE_EUNSUP, "model_attention_bwd: head_dim must be 64");
  if (R < 0 || S <= 0 || heads <= 0 || ldo < 64ll * heads || ldo % 8 || lddo < 64ll * heads || lddo % 8)
    return fail(ctx, DCTAE_EINVAL, "model_attention_bwd: bad shape");
  if (R == 0) return 0;
  if (!qkv || !ids || !key_pad || !out || !d_out || !lse || !delta_ws || !dqkv || !al16(qkv) || !al16(out) ||
      !al16(d_out) || !al16(dqkv))
    return fail(ctx, DCTAE_EINVAL, "model_attention_bwd: null or unaligned tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  AttnBwdArgs a{qkv, out, d_out, lse, ids, key_pad, delta_ws, dqkv, R, S, heads, (int32_t)ldo, (int32_t)lddo, 0.125f};
  Timer t(ctx, s, "model_attention_bwd");
  launch_attention_bwd(a, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_model_transpose_pack(dctae_ctx* ctx, int64_t M, int32_t C, const uint16_t* x, int64_t ldx, int64_t Mp,
                               uint16_t* out, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (M < 0 || C < 0 || ldx < C || Mp < M || Mp % 64) return fail(ctx, DCTAE_EINVAL, "model_transpose_pack: bad shape");
  if (Mp == 0 || C == 0) return 0;
  if (!x || !out) return fail(ctx, DCTAE_EINVAL, "model_transpose_pack: null tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "model_transpose_pack");
  launch_transpose_pack(x, ldx, M, C, Mp, out, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_model_colsum(dctae_ctx* ctx, int64_t M, int32_t N, const void* x, int64_t ldx, int32_t is_bf16, float* ws,
                       float* out, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (M < 0 || N < 0 || ldx < N) return fail(ctx, DCTAE_EINVAL, "model_colsum: bad shape");
  if (N == 0) return 0;
  if ((M > 0 && !x) || !out || (M > 256 && !ws)) return fail(ctx, DCTAE_EINVAL, "model_colsum: null tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "model_colsum");
  launch_colsum(x, ldx, M, N, is_bf16 != 0, ws, out, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_model_layernorm_bwd(dctae_ctx* ctx, int64_t M, int32_t D, const float* x, int64_t ldx, const float* g,
                              float eps, const float* dy, int64_t lddy, float* dx, int64_t lddx, int32_t accumulate,
                              float* part_g, float* part_b, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (M < 0 || D <= 0 || D > 2048 || ldx < D || lddy < D || lddx < D)
    return fail(ctx, DCTAE_EINVAL, "model_layernorm_bwd: bad shape (D <= 2048)");
  if (M == 0) return 0;
  if (!x || !g || !dy || !dx || !part_g || !part_b) return fail(ctx, DCTAE_EINVAL, "model_layernorm_bwd: null tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  LnBwdArgs a{x, g, dy, dx, part_g, part_b, M, ldx, lddy, lddx, D, accumulate, eps};
  Timer t(ctx, s, "model_layernorm_bwd");
  launch_layernorm_bwd(a, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_model_qgelu(dctae_ctx* ctx, int64_t M, int32_t N, const uint16_t* pre, int64_t ldp, uint16_t* out,
                      int64_t ldo, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (M < 0 || N < 0 || ldp < N || ldo < N) return fail(ctx, DCTAE_EINVAL, "model_qgelu: bad shape");
  if (M == 0 || N == 0) return 0;
  if (!pre || !out) return fail(ctx, DCTAE_EINVAL, "model_qgelu: null tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "model_qgelu");
  launch_qgelu(pre, ldp, M, N, out, ldo, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_model_qgelu_bwd(dctae_ctx* ctx, int64_t M, int32_t N, const uint16_t* df, int64_t lddf, const uint16_t* pre,
                          int64_t ldp, uint16_t* dpre, int64_t lddp, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (M < 0 || N < 0 || lddf < N || ldp < N || lddp < N) return fail(ctx, DCTAE_EINVAL, "model_qgelu_bwd: bad shape");
  if (M == 0 || N == 0) return 0;
  if (!df || !pre || !dpre) return fail(ctx, DCTAE_EINVAL, "model_qgelu_bwd: null tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "model_qgelu_bwd");
  launch_qgelu_bwd(df, lddf, pre, ldp, M, N, dpre, lddp, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_model_pos_grad(dctae_ctx* ctx, int64_t M, int32_t D, const float* g, int64_t ldg, const int64_t* idx,
                         int64_t idx_stride, int32_t rows, float* out, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (M < 0 || D <= 0 || ldg < D || rows < 0 || idx_stride <= 0) return fail(ctx, DCTAE_EINVAL, "model_pos_grad: bad shape");
  if (rows == 0) return 0;
  if ((M > 0 && (!g || !idx)) || !out) return fail(ctx, DCTAE_EINVAL, "model_pos_grad: null tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "model_pos_grad");
  launch_pos_grad(g, ldg, M, D, idx, idx_stride, rows, out, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// fused optimizer step (dctae_optim.hip)
// ---------------------------------------------------------------------------
static int optim_fail(dctae_ctx* ctx, int code, const char* msg) { return ctx ? fail(ctx, code, msg) : code; }

int dctae_optim_plan(dctae_ctx* ctx, dctae_optim_seg* segs, int32_t count, int64_t* n_norm_blocks, int64_t* n_work) {
  if (count < 0 || (count > 0 && !segs) || !n_norm_blocks || !n_work)
    return optim_fail(ctx, DCTAE_EINVAL, "optim_plan: bad arguments");
  int64_t nb = 0, nw = 0;
  for (int32_t i = 0; i < count; ++i) {
    dctae_optim_seg& s = segs[i];
    if (s.rows < 0 || s.cols < 0 || (s.cols > 0 && s.rows > INT64_MAX / s.cols))
      return optim_fail(ctx, DCTAE_EINVAL, "optim_plan: bad segment shape");
    const int64_t n = s.rows * s.cols;
    if (n > 0 && (!s.p || !s.exp_avg || !s.exp_avg_sq)) return optim_fail(ctx, DCTAE_EINVAL, "optim_plan: null tensor");
    if (s.group < 0 || s.group >= DCTAE_OPTIM_MAX_GROUPS) return optim_fail(ctx, DCTAE_EINVAL, "optim_plan: bad group");
    const bool packed = s.w_dst || s.wt_dst;
    if (packed && s.copy_dst) return optim_fail(ctx, DCTAE_EINVAL, "optim_plan: copy_dst on a packed segment");
    if ((s.w_dst && (s.ldw < s.cols || s.w_row_off < 0)) || (s.wt_dst && (s.wt_col_off < 0 || s.ldwt < s.wt_col_off + s.rows)))
      return optim_fail(ctx, DCTAE_EINVAL, "optim_plan: pack destination smaller than the segment");
    s.norm0 = nb;
    s.work0 = nw;
    nb += (n + OPT_NORM_CHUNK - 1) / OPT_NORM_CHUNK;
    nw += packed ? ((s.rows + OPT_TILE - 1) / OPT_TILE) * ((s.cols + OPT_TILE - 1) / OPT_TILE)
                 : (n + OPT_FLAT_CHUNK - 1) / OPT_FLAT_CHUNK;
  }
  if (nb > INT32_MAX) return optim_fail(ctx, DCTAE_EUNSUP, "optim_plan: too many gradient elements for one launch");
  *n_norm_blocks = nb;
  *n_work = nw;
  return 0;
}

int dctae_optim_gradnorm(dctae_ctx* ctx, const dctae_optim_seg* segs, int32_t count, int64_t n_norm_blocks,
                         float max_norm, double* ws, float* stats, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (count < 0 || n_norm_blocks < 0 || n_norm_blocks > INT32_MAX) return fail(ctx, DCTAE_EINVAL, "optim_gradnorm: bad size");
  if (!stats || (n_norm_blocks > 0 && (!segs || !ws || count == 0)))
    return fail(ctx, DCTAE_EINVAL, "optim_gradnorm: null tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "optim_gradnorm");
  launch_gradnorm(segs, count, n_norm_blocks, max_norm, ws, stats, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_optim_adamw_pack(dctae_ctx* ctx, const dctae_optim_seg* segs, int32_t count, int64_t n_work,
                           const dctae_optim_group* groups, int32_t n_groups, const float* stats, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (count < 0 || n_work < 0) return fail(ctx, DCTAE_EINVAL, "optim_adamw_pack: bad size");
  if (n_groups < 1 || n_groups > DCTAE_OPTIM_MAX_GROUPS || !groups)
    return fail(ctx, DCTAE_EUNSUP, "optim_adamw_pack: 1 .. DCTAE_OPTIM_MAX_GROUPS hyper-parameter groups");
  if (n_work == 0) return 0;
  if (!segs || count == 0) return fail(ctx, DCTAE_EINVAL, "optim_adamw_pack: null table");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  Timer t(ctx, s, "optim_adamw_pack");
  launch_adamw_pack(segs, count, n_work, groups, n_groups, stats, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

}  // extern "C"
