// The decode engine: dctae_decode and dctae_decode_normed, and their byte-output
// forms dctae_decode_u8 and dctae_decode_normed_u8 (include/dctae_u8_out.h), and
// the int16-code forms dctae_decode_c16 and dctae_decode_u8_c16 (include/dctae_codes16.h).
// dctae_decode_frames (dctae_frames.hip) plans and launches through the same decode_impl.
#include "dctae_ctx.h"
#include "dctae_dec_layout.h"
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

// The planner and launch sequence of every decode entry: token map -> spectrum
// -> column DCT-III -> row DCT-III -> RGB, for a list of targets.  A plain
// decode's targets are the batch's images (out at B.out_off); a frames call's
// are its frames sorted by source image, one ImgDesc each with the source's
// geometry and its own workspace and output offsets (dctae_frames.hip), which
// the same kernels take as images: only the two token-driven kernels have a
// frame form.  FFT path (every image 512 x 512): the column kernel expands
// the tokens and, for PatchNorm-space patches (normed), inverts them; other
// geometries scatter the tokens into Y for the GEMM pair, after
// dctae_norm_inverse's kernel into the staging buffer.  px / codes.type: the
// caller's pixel and code types, tags that ride to the kernels that write /
// load them; every workspace request, plan entry and launch is the same.
// clip to bytes ("staged"): the kernels write fp32 targets into the workspace
// and k_clip_store writes the bytes.
int decode_impl(dctae_ctx* ctx, const DecodeBatch& B, const dctae_norm* norm, const dctae_lfq* lfq,
                const CodeSrc& codes, const float* patches, void* out, PixelType px, bool normed,
                const dctae_frames* fr, bool clip) {
  hipSetDevice(ctx->device);
  const dctae_fe_cfg* cfg = B.cfg;
  const hipStream_t s = B.s;
  const int n_rows = B.n_rows, n_img = B.n_img;
  const char* own = nullptr;
  if (normed && (!norm || !norm->median_dev || !norm->b_dev || codes))
    own = "decode of PatchNorm-space patches needs the PatchNorm tables (and no codes)";
  int rc = decode_check(ctx, B, own, out != nullptr || (fr && fr->n_frames == 0), true);
  if (rc) return rc;
  const int P = cfg->patch_size, PP = P * P;
  const int64_t n_tok = (int64_t)n_rows * cfg->max_seq_len;
  if (codes) {
    if (!norm || !norm->median_dev || !norm->b_dev) return fail(ctx, DCTAE_EINVAL, "decode from codes needs PatchNorm");
    if ((rc = check_lfq(ctx, lfq, PP))) return rc;
    if (codes.type == CodeType::kI16 && (rc = check_codes16(ctx, lfq))) return rc;
  } else if (n_rows > 0 && !patches) {
    return fail(ctx, DCTAE_EINVAL, "decode needs codes or patches");
  }
  if (!fr && n_img == 0) return 0;
  std::vector<ImgDesc> D, F;   // the batch's images; the frames sorted by image (stable)
  int64_t max_hw;
  if ((rc = decode_geometry(ctx, B, D, &max_hw))) return rc;
  std::vector<int> order;    // sorted frame g is the caller's frame order[g]
  std::vector<int2> range;   // image im owns the sorted frames [range[im].x, range[im].y)
  std::vector<int32_t> cut;
  if (fr) {
    if ((rc = frames_check(ctx, B, fr))) return rc;
    if (fr->n_frames == 0) return 0;
    if (!out) return fail(ctx, DCTAE_EINVAL, "bad decode descriptor");
    for (int f = 0; f < fr->n_frames; ++f) order.push_back(f);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return fr->img[x] < fr->img[y]; });
    range.assign(n_img, make_int2(0, 0));
    max_hw = 1;
    for (int g = 0; g < fr->n_frames; ++g) {
      const int im = fr->img[order[g]];
      if (g == 0 || fr->img[order[g - 1]] != im) range[im].x = g;
      range[im].y = g + 1;
      cut.push_back(fr->cut[order[g]]);
      F.push_back(D[im]);
      F[g].rgb_off = fr->out_off[order[g]];
      max_hw = std::max<int64_t>(max_hw, (int64_t)D[im].H * D[im].W);
    }
  }
  std::vector<ImgDesc>& T = fr ? F : D;   // the targets
  const int n_tg = (int)T.size();
  // where the kernels write a target: the caller's buffer, or fp32 staging in the workspace
  const bool staged = clip && px == PixelType::kU8;
  const PixelType wpx = staged ? PixelType::kF32 : px;

  // The path (decode_path, dctae_dec_layout.h), then the specialised plan of its side.  Per image the predicate
  // asks what the FFT kernels are compiled for, fftdec = D[i].H == 512 && D[i].W == 512 (kFftDecSide) at
  // qh <= 32 and one qw; tests/test_pixel_loss_shapes_host.py reads the side out of this line for its cases
  static_assert(kFftDecSide == 512, "the comment above quotes the side");
  DecPath path = decode_path(ctx->opt, P, (bool)codes, codes ? lfq->codebook_dim : 0, codes ? lfq->num_codebooks : 0,
                             D.data(), n_img);
  FftPlan fpl{};
  if (path.fft && !(fft_plan_for(ctx, kFftDecSide, P, &fpl) == 0 && fpl.spec == 1)) path = DecPath{};
  // k_idct_rows512 stores four byte pixels at once (dctae_u8_out.h): refused before any launch
  for (int g = 0; wpx == PixelType::kU8 && path.rows512 && g < n_tg; ++g)
    if (((uintptr_t)out + (uintptr_t)T[g].rgb_off) % 4) {
      const std::string what = fr ? "frame" : "image";
      return fail(ctx, DCTAE_EINVAL, what + " " + std::to_string(fr ? order[g] : g) + ": a 512 x 512 byte " + what +
                  " on the 512-wide row kernel must start 4-byte aligned (" +
                  (fr ? "out_dev + out_off[f])" : "rgb_dev + out_off[i])"));
    }
  const DecLayout L = decode_layout(T.data(), n_tg, path.fft, cfg->max_patch_h, cfg->max_patch_w, clip, staged);
  std::vector<ClipSpan> cd;   // clip (frames only): from where the kernels wrote frame g to the caller's frame
  for (int g = 0; clip && g < n_tg; ++g) cd.push_back({T[g].rgb_off, fr->out_off[order[g]], 3ll * T[g].H * T[g].W});

  OrderedCall oc(ctx, s);
  if (!path.fft && normed && n_rows > 0) {
    // PatchNorm-space patches on the GEMM path: inverted once over every packed token into the staging buffer
    float* inv;
    if ((rc = oc.scratch(kStage, (size_t)n_tok * PP * 4, &inv))) return rc;
    Timer t(ctx, s, "norm_inverse");
    launch_norm(patches, B.ch, B.pos, n_tok, PP, cfg->max_patch_h, cfg->max_patch_w, norm->median_dev, norm->b_dev,
                norm->eps, norm->min_val, norm->max_val, 1, inv, ctx->err_dev, s);
    patches = inv;
  }
  float* ws;
  if ((rc = oc.scratch(kWs, (size_t)L.total * 4, &ws))) return rc;
  std::vector<GemmProblem> probs;
  std::vector<TileRef> t1, t2;
  for (int g = 0; !path.fft && g < n_tg; ++g) {
    GemmProblem g1, g2;
    const float *CW, *CH;
    if ((rc = decode_gemm_pair(ctx, cfg, T[g], ws, &g1, &g2, &CW, &CH))) return rc;
    add_tiles(t1, 2 * g, g1);
    add_tiles(t2, 2 * g + 1, g2);
    probs.push_back(g1);
    probs.push_back(g2);
  }
  if (!path.fft && ctx->opt.xcd_order) {   // as the encode's GEMMs (xcd_deal_tiles): speed only
    xcd_deal_tiles(t1, probs.data(), 2);
    xcd_deal_tiles(t2, probs.data(), 1);
  }
  // the plan: an empty list adds nothing, so a plain decode's carries no frame lists and each path only its own
  PlanBuf pb;
  const PlanList<ImgDesc> pl_d = pb.add(D), pl_f = pb.add(F);
  const PlanList<int2> pl_range = pb.add(range);
  const PlanList<int32_t> pl_cut = pb.add(cut);
  const PlanList<int2> pl_rb = pb.add(L.row_blocks);
  const PlanList<GemmProblem> pl_g = pb.add(probs);
  const PlanList<TileRef> pl_t1 = pb.add(t1), pl_t2 = pb.add(t2);
  const PlanList<ClipSpan> pl_cd = pb.add(cd);
  const size_t lut_off = pb.add(B.img_lut, (size_t)n_rows * B.lut_w);
  uint8_t* pd;
  if ((rc = oc.upload(pb, &pd))) return rc;
  const ImgDesc* dd = pl_d.at(pd);
  const ImgDesc* td = fr ? pl_f.at(pd) : dd;
  int32_t* map = (int32_t*)(ws + L.map_off);
  void* wout = staged ? (void*)ws : out;
  if (!path.fft) HIPCHK(ctx, hipMemsetAsync(ws, 0, (size_t)L.wsf * 4, s));
  // normed: the FFT path's column kernel inverts; the GEMM path's patches were inverted above
  const DecodeArgs a = decode_args(ctx, B, norm, lfq, codes.p, patches, (const int32_t*)(pd + lut_off),
                                   path.fft && normed);
  HIPCHK(ctx, hipMemsetAsync(map, 0xFF, (size_t)L.map_n * 4, s));
  {
    Timer t(ctx, s, "dec_map");
    if (fr)
      launch_frames_map(n_tok, dd, a, pl_range.at(pd), pl_cut.at(pd), map, s);
    else
      launch_dec_map(n_tok, dd, a, map, s);
  }
  if (path.fft) {
    const float2* tw = ctx->fft_tab + fpl.tw_off;
    const float4* pre = reinterpret_cast<const float4*>(ctx->fft_tab + fpl.ipre_off);
    {
      Timer t(ctx, s, "idct_cols");
      if (path.band)
        launch_idct_cols512b(td, n_tg, ws, map, tw, pre, a, s, codes.type);
      else
        launch_idct_cols512(td, n_tg, D[0].qw, ws, map, tw, pre, a, s, codes.type);
    }
    Timer t(ctx, s, "idct_rows");
    if (path.rows512)
      launch_idct_rows512(path.band, td, pl_rb.at(pd), pl_rb.n, ws, wout, wpx, tw, pre, ctx->cm, s);
    else
      launch_idct_rows_spec(1, td, pl_rb.at(pd), pl_rb.n, ws, wout, wpx, tw, pre, ctx->cm, s);
  } else {
    {
      Timer t(ctx, s, "scatter_tokens");
      if (fr)
        launch_scatter_frames(n_tok, dd, td, ws, a, pl_range.at(pd), pl_cut.at(pd), map, s, codes.type);
      else
        launch_scatter_tokens(n_tok, dd, ws, a, map, s, codes.type);
    }
    {
      Timer t(ctx, s, "idct_cols");
      ctx_gemm(ctx, 3, pl_g.at(pd), pl_t1.at(pd), pl_t1.n, s, 2);
    }
    {
      Timer t(ctx, s, "idct_rows");
      ctx_gemm(ctx, 3, pl_g.at(pd), pl_t2.at(pd), pl_t2.n, s, 1);
    }
    Timer t(ctx, s, "ipt_to_rgb");
    launch_ipt_to_rgb(td, n_tg, max_hw, ws, wout, wpx, ctx->cm, s);
  }
  if (clip && (rc = clip_launch(ctx, pl_cd.at(pd), n_tg, 3 * max_hw, (const float*)wout, (uint32_t*)(ws + L.mm_off),
                                out, px, s)))
    return rc;
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

}  // namespace dctae

extern "C" {

int dctae_decode(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut, int32_t lut_w,
                 int32_t n_img, const int32_t* out_hw, const int64_t* out_off, const int32_t* patch_hw,
                 const int64_t* ids, const uint8_t* key_pad, const int64_t* pos, const int64_t* ch,
                 const dctae_norm* norm, const dctae_lfq* lfq, const int64_t* codes, const float* patches,
                 float* rgb, void* stream) {
  const DecodeBatch B = decode_batch(cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos,
                                     ch, stream);
  if (!ctx) return DCTAE_EINVAL;
  return decode_impl(ctx, B, norm, lfq, codes, patches, rgb, PixelType::kF32, false);
}

int dctae_decode_u8(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut, int32_t lut_w,
                    int32_t n_img, const int32_t* out_hw, const int64_t* out_off, const int32_t* patch_hw,
                    const int64_t* ids, const uint8_t* key_pad, const int64_t* pos, const int64_t* ch,
                    const dctae_norm* norm, const dctae_lfq* lfq, const int64_t* codes, const float* patches,
                    uint8_t* rgb, void* stream) {
  const DecodeBatch B = decode_batch(cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos,
                                     ch, stream);
  if (!ctx) return DCTAE_EINVAL;
  return decode_impl(ctx, B, norm, lfq, codes, patches, rgb, PixelType::kU8, false);
}

int dctae_decode_normed(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut,
                        int32_t lut_w, int32_t n_img, const int32_t* out_hw, const int64_t* out_off,
                        const int32_t* patch_hw, const int64_t* ids, const uint8_t* key_pad, const int64_t* pos,
                        const int64_t* ch, const dctae_norm* norm, const float* normed_patches, float* rgb,
                        void* stream) {
  const DecodeBatch B = decode_batch(cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos,
                                     ch, stream);
  if (!ctx) return DCTAE_EINVAL;
  if (n_rows > 0 && !normed_patches) return fail(ctx, DCTAE_EINVAL, "decode needs the PatchNorm-space patches");
  return decode_impl(ctx, B, norm, nullptr, CodeSrc(), normed_patches, rgb, PixelType::kF32, true);
}

int dctae_decode_normed_u8(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut,
                           int32_t lut_w, int32_t n_img, const int32_t* out_hw, const int64_t* out_off,
                           const int32_t* patch_hw, const int64_t* ids, const uint8_t* key_pad, const int64_t* pos,
                           const int64_t* ch, const dctae_norm* norm, const float* normed_patches, uint8_t* rgb,
                           void* stream) {
  const DecodeBatch B = decode_batch(cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos,
                                     ch, stream);
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
  const DecodeBatch B = decode_batch(cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos,
                                     ch, stream);
  if (!ctx) return DCTAE_EINVAL;
  return decode_impl(ctx, B, norm, lfq, codes, patches, rgb, PixelType::kF32, false);
}

int dctae_decode_u8_c16(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut,
                        int32_t lut_w, int32_t n_img, const int32_t* out_hw, const int64_t* out_off,
                        const int32_t* patch_hw, const int64_t* ids, const uint8_t* key_pad, const int64_t* pos,
                        const int64_t* ch, const dctae_norm* norm, const dctae_lfq* lfq, const int16_t* codes,
                        const float* patches, uint8_t* rgb, void* stream) {
  const DecodeBatch B = decode_batch(cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos,
                                     ch, stream);
  if (!ctx) return DCTAE_EINVAL;
  return decode_impl(ctx, B, norm, lfq, codes, patches, rgb, PixelType::kU8, false);
}

}  // extern "C"
