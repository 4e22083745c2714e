// The decode engine: dctae_decode and dctae_decode_normed, and their byte-output
// forms dctae_decode_u8 and dctae_decode_normed_u8 (include/dctae_u8_out.h), and
// the int16-code forms dctae_decode_c16 and dctae_decode_u8_c16 (include/dctae_codes16.h).
#include "dctae_ctx.h"
#include "../../include/dctae_u8_out.h"
#include "../../include/dctae_codes16.h"

using namespace dctae;

namespace dctae {

// cfg, the descriptor's pointers and the batch tensors.  own: the caller's own
// refusal that ranks before the descriptor's (or NULL); img_bufs / tok_bufs:
// the caller's per-image / per-token buffers are there
int decode_check(dctae_ctx* ctx, const DecodeBatch& B, const char* own, bool img_bufs, bool tok_bufs) {
  const int rc = check_cfg(ctx, B.cfg);
  if (rc) return rc;
  if (own) return fail(ctx, DCTAE_EINVAL, own);
  if (B.n_rows < 0 || B.n_img < 0 || B.lut_w < 1 || !B.img_lut ||
      (B.n_img > 0 && (!B.out_hw || !B.out_off || !B.patch_hw || !img_bufs)))
    return fail(ctx, DCTAE_EINVAL, "bad decode descriptor");
  if (B.n_rows > 0 && (!B.ids || !B.key_pad || !B.pos || !B.ch || !tok_bufs))
    return fail(ctx, DCTAE_EINVAL, "NULL batch tensor");
  return 0;
}

// the LUT's range, then D[i] = the geometry of image i (no workspace offsets:
// every caller lays out its own) and *max_hw = the largest H W (at least 1)
int decode_geometry(dctae_ctx* ctx, const DecodeBatch& B, std::vector<ImgDesc>& D, int64_t* max_hw) {
  const dctae_fe_cfg* cfg = B.cfg;
  const int P = cfg->patch_size, n_img = B.n_img;
  for (int64_t i = 0; i < (int64_t)B.n_rows * B.lut_w; ++i)
    if (B.img_lut[i] < -1 || B.img_lut[i] >= n_img) return fail(ctx, DCTAE_EINVAL, "image LUT entry out of range");
  D.resize(n_img);
  *max_hw = 1;
  for (int i = 0; i < n_img; ++i) {
    ImgDesc& d = D[i];
    std::memset(&d, 0, sizeof(d));
    d.plan_w = d.plan_h = -1;
    d.H = B.out_hw[2 * i];
    d.W = B.out_hw[2 * i + 1];
    d.ph = B.patch_hw[2 * i];
    d.pw = B.patch_hw[2 * i + 1];
    if (d.ph < 1 || d.pw < 1 || P * d.ph > d.H || P * d.pw > d.W)
      return fail(ctx, DCTAE_EINVAL, "image " + std::to_string(i) + ": patch_sizes do not fit original_sizes (FE:304)");
    if (B.out_off[i] < 0) return fail(ctx, DCTAE_EINVAL, "negative image offset");
    d.qh = std::min(d.ph, cfg->max_patch_h);
    d.qw = std::min(d.pw, cfg->max_patch_w);
    d.Kh = P * d.qh;
    d.Kw = P * d.qw;
    d.rgb_off = B.out_off[i];
    *max_hw = std::max<int64_t>(*max_hw, (int64_t)d.H * d.W);
  }
  return 0;
}

// the decode's GEMM pair of image d on the workspace ws, with their split
// matrices attached, and the two DCT matrices they share with the adjoint pair
int decode_gemm_pair(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const ImgDesc& d, float* ws, GemmProblem* g1,
                     GemmProblem* g2, const float** CW, const float** CH) {
  const int rows_cap = cfg->patch_size * std::max(cfg->max_patch_h, cfg->max_patch_w);
  int rc;
  if ((rc = dct_matrix(ctx, d.W, std::min(d.W, rows_cap), CW))) return rc;
  if ((rc = dct_matrix(ctx, d.H, std::min(d.H, rows_cap), CH))) return rc;
  // U[c][y][kx] = sum_ky CH[ky][y] * Ysp[c][ky][kx]
  *g1 = gemm(*CH, 0, 1, d.H, ws + d.ws_y, (int64_t)d.Kh * d.Kw, 1, d.Kw, ws + d.ws_t, (int64_t)d.H * d.Kw, d.Kw, 1,
             d.H, d.Kw, d.Kh, 3);
  // X[c][y][x] = sum_kx U[c][y][kx] * CW[kx][x]
  *g2 = gemm(ws + d.ws_t, (int64_t)d.H * d.Kw, d.Kw, 1, *CW, 0, 1, d.W, ws + d.ws_p, (int64_t)d.H * d.W, d.W, 1, d.H,
             d.W, d.Kw, 3);
  attach_x3(ctx, *g1);
  attach_x3(ctx, *g2);
  return 0;
}

// the token-side arguments of the decode kernels; lut: the plan's copy of
// B.img_lut; normed: `patches` are PatchNorm outputs that the kernel inverts
// (the FFT path's column kernel)
DecodeArgs decode_args(const dctae_ctx* ctx, const DecodeBatch& B, const dctae_norm* norm, const dctae_lfq* lfq,
                       const void* codes, const float* patches, const int32_t* lut, bool normed) {
  DecodeArgs a{};
  a.ids = B.ids;
  a.key_pad = B.key_pad;
  a.pos = B.pos;
  a.ch = B.ch;
  a.codes = codes;
  a.patches = patches;
  a.lut = lut;
  a.lut_w = B.lut_w;
  a.S = B.cfg->max_seq_len;
  a.P = B.cfg->patch_size;
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
  a.maxph = B.cfg->max_patch_h;
  a.maxpw = B.cfg->max_patch_w;
  a.err = ctx->err_dev;
  return a;
}

int check_codes16(dctae_ctx* ctx, const dctae_lfq* lfq) {
  if (lfq && lfq->codebook_dim > 15)
    return fail(ctx, DCTAE_EINVAL, "int16 codes hold codebook_dim <= 15 bits, got codebook_dim = " +
                                       std::to_string(lfq->codebook_dim));
  return 0;
}

}  // namespace dctae

// decode of 512 x 512 images on the FFT path: token map -> column DCT-III
// (tokens expanded in the kernel) -> U -> row DCT-III + IPT -> RGB.
// rgb / px: the caller's images and their pixel type (ImgDesc::rgb_off in pixels)
static int decode_fft(OrderedCall& oc, const DecodeBatch& B, std::vector<ImgDesc>& D, const FftPlan& fpl,
                      const dctae_norm* norm, const dctae_lfq* lfq, const CodeSrc& codes, const float* patches,
                      void* rgb, PixelType px, bool normed) {
  dctae_ctx* ctx = oc.ctx;
  const hipStream_t s = oc.s;
  const dctae_fe_cfg* cfg = B.cfg;
  const int n_img = B.n_img;
  // 32 kept tile columns on the default row kernel: U in the band layout
  // (k_idct_cols512b); otherwise row-major U (k_idct_cols512)
  const bool rows512 = ctx->opt.dec_rows_kernel == 3 && D[0].qw == 32;
  const bool band = rows512 && ctx->opt.dec_cols_kernel == 2;
  // k_idct_rows512 stores four byte pixels at once (dctae_u8_out.h): refused before any launch
  for (int i = 0; px == PixelType::kU8 && rows512 && i < n_img; ++i)
    if (((uintptr_t)rgb + (uintptr_t)D[i].rgb_off) % 4)
      return fail(ctx, DCTAE_EINVAL, "image " + std::to_string(i) + ": a 512 x 512 byte image on the 512-wide row "
                  "kernel must start 4-byte aligned (rgb_dev + out_off[i])");
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
  float* ws;
  if ((rc = oc.scratch(kWs, (size_t)wsf * 4, &ws))) return rc;
  PlanBuf pb;
  const size_t d_off = pb.add(D.data(), D.size());
  const size_t rb_off = pb.add(rb.data(), rb.size());
  const size_t lut_off = pb.add(B.img_lut, (size_t)B.n_rows * B.lut_w);
  uint8_t* pd;
  if ((rc = oc.upload(pb, &pd))) return rc;
  const ImgDesc* dd = (const ImgDesc*)(pd + d_off);
  int32_t* map = (int32_t*)(ws + map_off);
  HIPCHK(ctx, hipMemsetAsync(map, 0xFF, (size_t)map_n * 4, s));
  const DecodeArgs a = decode_args(ctx, B, norm, lfq, codes.p, patches, (const int32_t*)(pd + lut_off), normed);
  const float2* tw = ctx->fft_tab + fpl.tw_off;
  const float4* pre = reinterpret_cast<const float4*>(ctx->fft_tab + fpl.ipre_off);
  {
    Timer t(ctx, s, "dec_map");
    launch_dec_map((int64_t)B.n_rows * cfg->max_seq_len, dd, a, map, s);
  }
  {
    Timer t(ctx, s, "idct_cols");
    if (band)
      launch_idct_cols512b(dd, n_img, ws, map, tw, pre, a, s, codes.type);
    else
      launch_idct_cols512(dd, n_img, D[0].qw, ws, map, tw, pre, a, s, codes.type);
  }
  {
    Timer t(ctx, s, "idct_rows");
    if (rows512)
      launch_idct_rows512(band, dd, (const int2*)(pd + rb_off), (int)rb.size(), ws, rgb, px, tw, pre, ctx->cm, s);
    else
      launch_idct_rows_spec(1, dd, (const int2*)(pd + rb_off), (int)rb.size(), ws, rgb, px, tw, pre, ctx->cm, s);
  }
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

// normed: patches are PatchNorm outputs (before inverse_norm); the FFT path
// applies the inverse in its column kernel (the (c, strip) tables of a block
// are image-independent), other geometries run dctae_norm_inverse's kernel
// into the staging buffer first.  px: the pixel type of the caller's images
// (B.out_off in pixels); the tag rides to the kernels that write them, every
// workspace request, plan entry and launch before them is the same.  codes:
// the caller's codes with their type, a tag that rides to the kernels that
// load them (the column kernels of the FFT path, k_scatter_tokens) in the same way
static int decode_impl(dctae_ctx* ctx, const DecodeBatch& B, const dctae_norm* norm, const dctae_lfq* lfq,
                       const CodeSrc& codes, const float* patches, void* rgb, PixelType px, bool normed) {
  hipSetDevice(ctx->device);
  const dctae_fe_cfg* cfg = B.cfg;
  const hipStream_t s = B.s;
  const int n_rows = B.n_rows, n_img = B.n_img;
  const char* own = nullptr;
  if (normed && (!norm || !norm->median_dev || !norm->b_dev || codes))
    own = "decode of PatchNorm-space patches needs the PatchNorm tables (and no codes)";
  int rc = decode_check(ctx, B, own, rgb != nullptr, true);
  if (rc) return rc;
  const int P = cfg->patch_size, PP = P * P, S = cfg->max_seq_len;
  if (codes) {
    if (!norm || !norm->median_dev || !norm->b_dev) return fail(ctx, DCTAE_EINVAL, "decode from codes needs PatchNorm");
    if ((rc = check_lfq(ctx, lfq, PP))) return rc;
    if (codes.type == CodeType::kI16 && (rc = check_codes16(ctx, lfq))) return rc;
  } else if (n_rows > 0 && !patches) {
    return fail(ctx, DCTAE_EINVAL, "decode needs codes or patches");
  }
  if (n_img == 0) return 0;
  std::vector<ImgDesc> D;
  int64_t wsf = 0, max_hw;
  if ((rc = decode_geometry(ctx, B, D, &max_hw))) return rc;
  for (ImgDesc& d : D) {   // the GEMM path's workspace: Y, U and the ipt image, image by image
    d.ws_y = wsf;
    wsf += 3ll * d.Kh * d.Kw;
    d.ws_t = wsf;
    wsf += 3ll * d.H * d.Kw;
    d.ws_p = wsf;
    wsf += 3ll * d.H * d.W;
  }
  // the GEMM path's slot map (k_dec_map: the later packed slot wins at a duplicate place, FE:639-643)
  const int64_t gmap_off = (wsf + 63) & ~63ll;
  const int64_t gmap_n = (int64_t)n_img * 3 * cfg->max_patch_h * cfg->max_patch_w;
  // FFT path (dctae_idct.hip): every image 512 x 512 on the specialised plan, recommended LFQ
  bool fftdec = ctx->opt.fft_decode && P == 14 && (!codes || (lfq->codebook_dim == 14 && lfq->num_codebooks == 14));
  for (int i = 0; fftdec && i < n_img; ++i)
    fftdec = D[i].H == 512 && D[i].W == 512 && D[i].qh <= 32 && D[i].qw == D[0].qw;
  FftPlan fpl{};
  if (fftdec) fftdec = fft_plan_for(ctx, 512, P, &fpl) == 0 && fpl.spec == 1;
  OrderedCall oc(ctx, s);
  if (fftdec)
    return decode_fft(oc, B, D, fpl, norm, lfq, codes, patches, rgb, px, normed);
  if (normed && n_rows > 0) {
    // other geometries: the inverse over every packed token into the staging buffer, then as patches
    const int64_t n_tok = (int64_t)n_rows * S;
    float* inv;
    if ((rc = oc.scratch(kStage, (size_t)n_tok * PP * 4, &inv))) return rc;
    Timer t(ctx, s, "norm_inverse");
    launch_norm(patches, B.ch, B.pos, n_tok, PP, cfg->max_patch_h, cfg->max_patch_w, norm->median_dev, norm->b_dev,
                norm->eps, norm->min_val, norm->max_val, 1, inv, ctx->err_dev, s);
    patches = inv;
  }
  float* ws;
  if ((rc = oc.scratch(kWs, (size_t)(gmap_off + gmap_n) * 4, &ws))) return rc;
  std::vector<GemmProblem> probs;
  std::vector<TileRef> t1, t2;
  for (const ImgDesc& d : D) {
    GemmProblem g1, g2;
    const float *CW, *CH;
    if ((rc = decode_gemm_pair(ctx, cfg, d, ws, &g1, &g2, &CW, &CH))) return rc;
    int pr = (int)probs.size();
    probs.push_back(g1);
    probs.push_back(g2);
    add_tiles(t1, pr, g1);
    add_tiles(t2, pr + 1, g2);
  }
  if (ctx->opt.xcd_order) {   // as the encode's GEMMs (xcd_deal_tiles): speed only
    xcd_deal_tiles(t1, probs.data(), 2);
    xcd_deal_tiles(t2, probs.data(), 1);
  }
  PlanBuf pb;
  size_t d_off = pb.add(D.data(), D.size());
  size_t g_off = pb.add(probs.data(), probs.size());
  size_t t1_off = pb.add(t1.data(), t1.size());
  size_t t2_off = pb.add(t2.data(), t2.size());
  size_t lut_off = pb.add(B.img_lut, (size_t)n_rows * B.lut_w);
  uint8_t* pd;
  if ((rc = oc.upload(pb, &pd))) return rc;
  const ImgDesc* dd = (const ImgDesc*)(pd + d_off);
  HIPCHK(ctx, hipMemsetAsync(ws, 0, (size_t)wsf * 4, s));
  // PatchNorm-space patches were inverted into the staging buffer above: plain patches here
  const DecodeArgs a = decode_args(ctx, B, norm, lfq, codes.p, patches, (const int32_t*)(pd + lut_off), false);
  int32_t* gmap = (int32_t*)(ws + gmap_off);
  HIPCHK(ctx, hipMemsetAsync(gmap, 0xFF, (size_t)gmap_n * 4, s));
  {
    Timer t(ctx, s, "dec_map");
    launch_dec_map((int64_t)n_rows * S, dd, a, gmap, s);
  }
  {
    Timer t(ctx, s, "scatter_tokens");
    launch_scatter_tokens((int64_t)n_rows * S, dd, ws, a, gmap, s, codes.type);
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
    launch_ipt_to_rgb(dd, n_img, max_hw, ws, rgb, px, ctx->cm, s);
  }
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

extern "C" {

int dctae_decode(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut, int32_t lut_w,
                 int32_t n_img, const int32_t* out_hw, const int64_t* out_off, const int32_t* patch_hw,
                 const int64_t* ids, const uint8_t* key_pad, const int64_t* pos, const int64_t* ch,
                 const dctae_norm* norm, const dctae_lfq* lfq, const int64_t* codes, const float* patches,
                 float* rgb, void* stream) {
  const DecodeBatch B{cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos, ch,
                      (hipStream_t)stream};
  if (!ctx) return DCTAE_EINVAL;
  return decode_impl(ctx, B, norm, lfq, codes, patches, rgb, PixelType::kF32, false);
}

int dctae_decode_u8(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut, int32_t lut_w,
                    int32_t n_img, const int32_t* out_hw, const int64_t* out_off, const int32_t* patch_hw,
                    const int64_t* ids, const uint8_t* key_pad, const int64_t* pos, const int64_t* ch,
                    const dctae_norm* norm, const dctae_lfq* lfq, const int64_t* codes, const float* patches,
                    uint8_t* rgb, void* stream) {
  const DecodeBatch B{cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos, ch,
                      (hipStream_t)stream};
  if (!ctx) return DCTAE_EINVAL;
  return decode_impl(ctx, B, norm, lfq, codes, patches, rgb, PixelType::kU8, false);
}

int dctae_decode_normed(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut,
                        int32_t lut_w, int32_t n_img, const int32_t* out_hw, const int64_t* out_off,
                        const int32_t* patch_hw, const int64_t* ids, const uint8_t* key_pad, const int64_t* pos,
                        const int64_t* ch, const dctae_norm* norm, const float* normed_patches, float* rgb,
                        void* stream) {
  const DecodeBatch B{cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos, ch,
                      (hipStream_t)stream};
  if (!ctx) return DCTAE_EINVAL;
  if (n_rows > 0 && !normed_patches) return fail(ctx, DCTAE_EINVAL, "decode needs the PatchNorm-space patches");
  return decode_impl(ctx, B, norm, nullptr, CodeSrc(), normed_patches, rgb, PixelType::kF32, true);
}

int dctae_decode_normed_u8(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut,
                           int32_t lut_w, int32_t n_img, const int32_t* out_hw, const int64_t* out_off,
                           const int32_t* patch_hw, const int64_t* ids, const uint8_t* key_pad, const int64_t* pos,
                           const int64_t* ch, const dctae_norm* norm, const float* normed_patches, uint8_t* rgb,
                           void* stream) {
  const DecodeBatch B{cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos, ch,
                      (hipStream_t)stream};
  if (!ctx) return DCTAE_EINVAL;
  if (n_rows > 0 && !normed_patches) return fail(ctx, DCTAE_EINVAL, "decode needs the PatchNorm-space patches");
  return decode_impl(ctx, B, norm, nullptr, CodeSrc(), normed_patches, rgb, PixelType::kU8, true);
}

// the int16-code entries (include/dctae_codes16.h): the same calls, the code type apart
int dctae_decode_c16(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut, int32_t lut_w,
                     int32_t n_img, const int32_t* out_hw, const int64_t* out_off, const int32_t* patch_hw,
                     const int64_t* ids, const uint8_t* key_pad, const int64_t* pos, const int64_t* ch,
                     const dctae_norm* norm, const dctae_lfq* lfq, const int16_t* codes, const float* patches,
                     float* rgb, void* stream) {
  const DecodeBatch B{cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos, ch,
                      (hipStream_t)stream};
  if (!ctx) return DCTAE_EINVAL;
  return decode_impl(ctx, B, norm, lfq, codes, patches, rgb, PixelType::kF32, false);
}

int dctae_decode_u8_c16(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut,
                        int32_t lut_w, int32_t n_img, const int32_t* out_hw, const int64_t* out_off,
                        const int32_t* patch_hw, const int64_t* ids, const uint8_t* key_pad, const int64_t* pos,
                        const int64_t* ch, const dctae_norm* norm, const dctae_lfq* lfq, const int16_t* codes,
                        const float* patches, uint8_t* rgb, void* stream) {
  const DecodeBatch B{cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos, ch,
                      (hipStream_t)stream};
  if (!ctx) return DCTAE_EINVAL;
  return decode_impl(ctx, B, norm, lfq, codes, patches, rgb, PixelType::kU8, false);
}

}  // extern "C"
