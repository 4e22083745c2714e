// The encode engine: plan, plan cache and launch sequence of dctae_encode,
// dctae_spectrum_tokens, dctae_dct2 and dctae_patch_spectrum.
#include "dctae_ctx.h"
#include "dctae_enc_layout.h"
#include "../../include/dctae_u8.h"
#include "../../include/dctae_codes16.h"

using namespace dctae;

// Encode plan: everything the launch sequence needs, cached on the inputs.
constexpr int kVariants = 3;  // 0 = generic FFT kernels, 1.. = dctae_fft2.hip specialisations

struct FftTables {
  int64_t tw_off, post_off;   // a compile-time plan kernel's tables in the context's FFT table buffer (FftPlan)
};

struct ChunkJob {
  int i0, i1;
  PlanList<ImgDesc> desc;
  PlanList<GemmProblem> gp;
  PlanList<TileRef> rows_t, cols_t;   // the GEMMs' tiles
  PlanList<TileRef> fused_t;          // k_rows_fused tiles (row problem, row-pair block)
  PlanList<int2> fr[kVariants];       // FFT row blocks (local image, first row) per kernel variant
  PlanList<int4> fc[kVariants];       // FFT column blocks (local image, channel, tile column, count)
  FftTables row_tab[kVariants], col_tab[kVariants];
  PlanList<int32_t> pc;   // k_fft_cols7 list: the spec-1 images of the job (one tile-column count qw)
  int n_pc, pc_qw;        // n_pc = pc.n when one persistent launch serves all of them, else 0
  PlanList<int32_t> pb;   // k_cols512b list: the band-layout images of the job
  int max_T;
  PlanList<int2> ipt;       // k_rgb_to_ipt blocks (local image, first group)
  PlanList<int32_t> fold;   // local indices of the images whose T k_fold_t folds
  int64_t fold_max_hw;
  PlanList<int2> br[4];   // Bluestein row / column blocks per L = 256 .. 2048
  PlanList<int4> bc[4];
  size_t lds_rows, lds_cols;
  int64_t amax_off;     // k_gemm_h2: |max| bits per image (IPT, T) in the workspace, floats
  int h2;               // the job's GEMMs on k_gemm_h2
  PlanList<int2> epi;   // k_tile_epilogue_p blocks (local image, 3 h + c) of the images with Y in the workspace
};

struct EncPlan {
  uint64_t id = 0;
  PlanBuf pb;
  std::vector<ChunkJob> jobs;
  PlanList<ImgDesc> all_desc;   // every image, global token offsets (sort_pack)
  PlanList<int32_t> rowlen;
  PlanList<FftPlan> plans;
  int n_img = 0, max_T = 1;
  int64_t n_tok = 0;
  size_t ws_need = 0;
  StageLayout stage;     // the token staging: its scratch request and token_sinks' carve
  float* ws = nullptr;   // the workspace its GEMM problems point into: the plan drops when the workspace moves
  bool any_pad = true;   // some packed row shorter than max_seq_len
  bool uniform = false;  // every image of the call has the same (H, W)
};

// The images of a call: dctae_images or dctae_images_u8, with the pixel type
// as a tag (img_off counts pixels of that type).  ok = false: the caller's
// descriptor pointer was NULL.
struct ImageSet {
  bool ok = false;
  const void* rgb = nullptr;
  const int64_t* img_off = nullptr;
  const int32_t* hw = nullptr;
  int32_t n_img = 0;
  PixelType px = PixelType::kF32;
  ImageSet() = default;
  explicit ImageSet(const dctae_images* d) {
    if (d) ok = true, rgb = d->rgb_dev, img_off = d->img_off, hw = d->hw, n_img = d->n_img;
  }
  explicit ImageSet(const dctae_images_u8* d) : px(PixelType::kU8) {
    if (d) ok = true, rgb = d->rgb_dev, img_off = d->img_off, hw = d->hw, n_img = d->n_img;
  }
};

// The packed outputs of a call: dctae_packed_out or dctae_packed_out16, with
// the code type as a tag.  ok = false: the caller's pointer was NULL.
struct PackedOut {
  bool ok = false;
  void* codes_dev = nullptr;
  int64_t *positions_dev = nullptr, *channels_dev = nullptr, *image_ids_dev = nullptr;
  uint8_t* key_pad_dev = nullptr;
  float *patches_dev = nullptr, *raw_patches_dev = nullptr, *scores_dev = nullptr;
  CodeType ct = CodeType::kI64;
  PackedOut() = default;
  template <typename T>
  void take(const T* o) {
    if (!o) return;
    ok = true, codes_dev = o->codes_dev, positions_dev = o->positions_dev, channels_dev = o->channels_dev;
    image_ids_dev = o->image_ids_dev, key_pad_dev = o->key_pad_dev, patches_dev = o->patches_dev;
    raw_patches_dev = o->raw_patches_dev, scores_dev = o->scores_dev;
  }
  explicit PackedOut(const dctae_packed_out* o) { take(o); }
  explicit PackedOut(const dctae_packed_out16* o) : ct(CodeType::kI16) { take(o); }
};

// One encode call: its arguments and what they ask for.
struct EncCall {
  const dctae_fe_cfg* cfg;
  ImageSet imgs;
  const dctae_packing* pack;   // NULL: token mode
  const dctae_norm* norm;
  const dctae_lfq* lfq;
  PackedOut out;
  const int64_t* tok_off_user;   // token mode: the caller's token offsets
  float *tokens_dev, *scores_dev;
  const float *proj_w, *proj_b;   // fused LFQ projections (dctae_encode_lfq_proj)
  // set by check()
  bool full, want_codes, want_raw, want_norm;
  int ncb;
  int check(dctae_ctx* ctx);
  std::vector<int64_t> plan_key(const Options& opt) const;
};

int EncCall::check(dctae_ctx* ctx) {
  int rc = check_cfg(ctx, cfg);
  if (rc) return rc;
  if (!imgs.ok || imgs.n_img < 0 || (imgs.n_img > 0 && (!imgs.rgb || !imgs.img_off || !imgs.hw)))
    return fail(ctx, DCTAE_EINVAL, "bad image descriptor");
  full = (pack != nullptr);
  const int n = imgs.n_img;
  const int P = cfg->patch_size, PP = P * P;
  want_codes = full && out.ok && out.codes_dev;
  if (full) {
    if (!out.ok || !out.positions_dev || !out.channels_dev || !out.image_ids_dev || !out.key_pad_dev)
      return fail(ctx, DCTAE_EINVAL, "packed outputs positions/channels/image_ids/key_pad are required");
    if ((want_codes || out.patches_dev) && !norm) return fail(ctx, DCTAE_EINVAL, "codes/patches need PatchNorm tables");
    if (want_codes && !proj_w && (rc = check_lfq(ctx, lfq, PP))) return rc;
    if (want_codes && out.ct == CodeType::kI16) {   // dctae_codes16.h: the limit and the alignment rule
      if ((rc = check_codes16(ctx, lfq))) return rc;
      // k_sort_pack2's ncb == 14 branch stores two codes (4 bytes) at once; every other store is one code
      const uintptr_t al = lfq && lfq->num_codebooks == 14 ? 4 : 2;
      if ((uintptr_t)out.codes_dev % al)
        return fail(ctx, DCTAE_EINVAL, "int16 codes_dev must be " + std::to_string(al) + "-byte aligned" +
                                           (al == 4 ? " at num_codebooks = 14 (two codes per store)" : ""));
    }
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
  ncb = want_codes ? lfq->num_codebooks : 0;
  want_raw = (full && out.raw_patches_dev) || (!full && tokens_dev);
  // LFQ with projections: the column epilogues stage the PatchNorm output,
  // dctae_lfq_project_in turns the staged tokens into staged u16 codes, and the
  // sort / pack gathers those as usual
  want_norm = full && (out.patches_dev || proj_w);
  return 0;
}

// plan cache key: every input that shapes the launch sequence (the workspace
// pointer is compared beside it: EncPlan::ws)
std::vector<int64_t> EncCall::plan_key(const Options& opt) const {
  const int n = imgs.n_img;
  std::vector<int64_t> key;
  key.reserve(32 + 6ll * n + (full ? pack->n_rows : 0));
  // byte images: the base's alignment is part of the key, since describe_images' refusal of a misaligned
  // 512-wide image (dctae_u8.h) depends on rgb_dev + img_off and must not be skipped by a plan cached
  // for the same offsets at another base
  const int64_t px_key = imgs.px == PixelType::kU8 ? 1 + (int64_t)(((uintptr_t)imgs.rgb & 3) << 1) : 0;
  key.insert(key.end(), {(int64_t)full, n, cfg->patch_size, cfg->max_patch_h, cfg->max_patch_w, cfg->max_seq_len, ncb,
                         (int64_t)want_raw, (int64_t)want_norm, px_key});
  push_plan_options(opt, key);
  for (int i = 0; i < n; ++i) {
    key.push_back(imgs.img_off[i]);
    key.push_back(((int64_t)imgs.hw[2 * i] << 32) | (uint32_t)imgs.hw[2 * i + 1]);
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
  return key;
}

// spec-1 (512-wide) rows run on k_rows512pk, else on k_fft_rows2<512, 16, 16>
static bool rows512_kernel(const dctae_ctx* ctx, const dctae_fe_cfg* cfg) {
  return ctx->opt.rows_kernel == 4 && cfg->max_patch_w == 32;
}

// the images of a call with their routes, and the FFT plans plan_w / plan_h index
struct EncImages {
  std::vector<ImgDesc> D;
  std::vector<FftPlan> plans;
};

// planner stage 1: describe and validate the images (geometry, packing, routes, tperm, tband)
static int describe_images(dctae_ctx* ctx, const EncCall& c, EncImages& im) {
  const dctae_fe_cfg* cfg = c.cfg;
  const dctae_packing* pack = c.pack;
  const int n = c.imgs.n_img, P = cfg->patch_size, S = cfg->max_seq_len;
  int rc;
  std::vector<ImgDesc>& D = im.D;
  std::vector<FftPlan>& plans = im.plans;
  D.resize(n);
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
    ImgDesc& d = D[i];
    if ((rc = describe(ctx, cfg, c.imgs.hw[2 * i], c.imgs.hw[2 * i + 1], d))) return rc;
    d.rgb_off = c.imgs.img_off[i];
    if (c.full) {
      d.row = pack->row[i];
      d.col = pack->col[i];
      d.k = pack->k[i];
      d.local_id = pack->local_id[i];
      if (d.k < 1 || d.k > d.T || d.k > S)
        return fail(ctx, DCTAE_EINVAL, "image " + std::to_string(i) + ": k out of range (FE:429-435)");
      if (d.row < 0 || d.row >= pack->n_rows || d.col < 0 || d.col + d.k > S)
        return fail(ctx, DCTAE_EINVAL, "image " + std::to_string(i) + ": packed span outside (rows, S)");
    }
    d.plan_w = plan_of(d.W);
    d.plan_h = plan_of(d.H);
    d.bs = (d.plan_w >= 0 && plans[d.plan_w].kind == 1 ? 1 : 0) | (d.plan_h >= 0 && plans[d.plan_h].kind == 1 ? 2 : 0);
    d.tperm = ctx->opt.tperm && row_route(d) == Route::kGemm && col_route(d) == Route::kGemm;
    // band layout: rows on k_rows512pk (Kw = 448) and columns on k_cols512b (Kh = 448)
    d.tband = ctx->opt.cols512b && ctx->opt.rows_kernel == 4 && cfg->max_patch_w == 32 && cfg->max_patch_h == 32 &&
              d.H == 512 && d.W == 512 && d.Kh == 448 && d.Kw == 448 && row_route(d) == Route::kFft &&
              col_route(d) == Route::kFft && plans[d.plan_w].spec == 1 && plans[d.plan_h].spec == 1;
    // packed encodes of band images: item-major token staging (stage_pos; the
    // staging is internal there, while dctae_spectrum_tokens hands it out in flat order)
    if (c.full && d.tband) d.tband |= 2;
    // k_rows512pk loads four byte pixels as one dword (dctae_u8.h: the alignment rule)
    if (c.imgs.px == PixelType::kU8 && rows512_kernel(ctx, cfg) && row_route(d) == Route::kFft &&
        plans[d.plan_w].spec == 1 && (((uintptr_t)c.imgs.rgb + (uint64_t)d.rgb_off) & 3))
      return fail(ctx, DCTAE_EINVAL, "image " + std::to_string(i) + ": a 512-wide byte image on k_rows512pk must "
                                     "start at a 4-byte aligned address (rgb_dev + img_off[i])");
  }
  if (c.full)
    for (int r = 0; r < pack->n_rows; ++r)
      if (pack->row_len[r] < 0 || pack->row_len[r] > S) return fail(ctx, DCTAE_EINVAL, "row_len out of range");
  return 0;
}

// planner stage 4: the lists of one chunk job, an image's row pass and column
// pass at a time, then commit() serialises them
struct JobLists {
  dctae_ctx* ctx;
  const dctae_fe_cfg* cfg;
  const std::vector<FftPlan>& plans;
  float* ws;
  ChunkJob& j;
  std::vector<GemmProblem>& probs;   // the call's; the job's start at p0
  const size_t p0;
  const int rows_cap = cfg->patch_size * std::max(cfg->max_patch_h, cfg->max_patch_w);
  std::vector<TileRef> rt, ct, ft;
  std::vector<int2> fr[kVariants], br[4], ipt, epi;
  std::vector<int4> fc[kVariants], bc[4];
  std::vector<int32_t> fold, pc, pb;
  int pc_qw = 0;
  bool pc_ok = cfg->max_patch_h <= 32;   // k_fft_cols7 keeps Kh <= 448 rows

  uint32_t* amax(int li) const { return reinterpret_cast<uint32_t*>(ws + j.amax_off) + 2 * li; }

  // the row pass of image d (local index li): T from the RGB image
  int rows(const ImgDesc& d, int li) {
    const Route route = row_route(d);
    if (route == Route::kBluestein) {
      const int L = plans[d.plan_w].bs_L, rpb = bs_rows_per_block(L);
      for (int y0 = 0; y0 < d.H; y0 += rpb) br[bs_lidx(L)].push_back(make_int2(li, y0));
      return 0;
    }
    if (route == Route::kFft) {
      const FftPlan& p = plans[d.plan_w];
      for (int y0 = 0; y0 < d.H; y0 += p.rows_per_block) fr[p.spec].push_back(make_int2(li, y0));
      if (p.spec)
        j.row_tab[p.spec] = {p.tw_off, p.post_off};
      else
        j.lds_rows = std::max<size_t>(j.lds_rows, (size_t)2 * p.rows_per_block * 3 * (2 * p.M + 1) * 4);
      return 0;
    }
    // T[c][y][kx] = sum_x CW[kx][x] * IPT[c][y][x], folded: even kx over
    // IPT[x] + IPT[W-1-x], odd kx over IPT[x] - IPT[W-1-x] (half the flops)
    const bool gemm_cols = col_route(d) == Route::kGemm;
    const size_t q0 = probs.size();
    for (int par = 0; par < 2; ++par) {
      const int M = par ? d.Kw / 2 : (d.Kw + 1) / 2, K = par ? d.W / 2 : (d.W + 1) / 2;
      if (M == 0) continue;
      const float* CW;
      if (int rc = dct_matrix(ctx, d.W, std::min(d.W, rows_cap), &CW, par)) return rc;
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
      g.amax = amax(li);                              // k_rgb_to_ipt's |max| of the folded IPT
      g.omax = gemm_cols ? amax(li) + 1 : nullptr;    // T's |max| for the column GEMM
      g.pad2 = li;                                    // k_rows_fused: the image and the parity
      g.pad3 = par;
      probs.push_back(g);
    }
    // k_rows_fused (colour transform + folds + row GEMM in one pass) for the
    // tperm images whose parity matrices are cached pre-split (both forms:
    // the fix-up runs the bf16 one) and fit its 256 output columns
    bool fz = ctx->opt.rows_fused && d.tperm && probs.size() == q0 + 2;   // both parities, consecutive
    for (size_t q = q0; q < probs.size(); ++q) fz = fz && probs[q].Xh && probs[q].N <= fused_max_n();
    if (fz) {
      for (int rb = 0; rb * fused_pairs_per_block() < (d.H + 1) / 2; ++rb) ft.push_back(TileRef{(int)(q0 - p0), rb});
      return 0;
    }
    for (size_t q = q0; q < probs.size(); ++q) add_tiles(rt, (int)(q - p0), probs[q]);
    // k_rgb_to_ipt's (x, y)-mirrored pixel groups of this image
    const int64_t ng = (int64_t)(gemm_cols ? (d.H + 1) / 2 : d.H) * ((d.W + 1) / 2);
    for (int64_t g0 = 0; g0 < ng; g0 += rgb_to_ipt_groups_per_block()) ipt.push_back(make_int2(li, (int)g0));
    return 0;
  }

  // the column pass of image d: tokens from T (through Y and the tile epilogue on the GEMM and Bluestein routes)
  int cols(const ImgDesc& d, int li) {
    if (regions_of(d).y)   // Y in the workspace: the tile epilogue's (tile row, channel) blocks
      for (int h = 0; h < d.qh; ++h)
        for (int c = 0; c < 3; ++c) epi.push_back(make_int2(li, 3 * h + c));
    const Route route = col_route(d);
    if (route == Route::kBluestein) {
      const int L = plans[d.plan_h].bs_L, cpb = bs_cols_per_block(L);
      for (int c = 0; c < 3; ++c)
        for (int kx0 = 0; kx0 < d.Kw; kx0 += cpb) bc[bs_lidx(L)].push_back(make_int4(li, c, kx0, 0));
    } else if (route == Route::kBand) {
      pb.push_back(li);
      j.col_tab[1] = {plans[d.plan_h].tw_off, plans[d.plan_h].post_off};
    } else if (route == Route::kFft) {
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
      if (p.spec)
        j.col_tab[p.spec] = {p.tw_off, p.post_off};
      else
        j.lds_cols = std::max<size_t>(j.lds_cols, (size_t)2 * 2 * p.M * cfg->patch_size * 4);
    } else {
      // Y[c][ky][kx] = sum_y CH[ky][y] * T[c][y][kx], folded along y as the rows
      for (int par = 0; par < 2; ++par) {
        const int M = par ? d.Kh / 2 : (d.Kh + 1) / 2, K = par ? d.H / 2 : (d.H + 1) / 2;
        if (M == 0) continue;
        const float* CH;
        if (int rc = dct_matrix(ctx, d.H, std::min(d.H, rows_cap), &CH, par)) return rc;
        // B: T folded along y (by the row GEMM of the y-folded IPT, or in place by
        // k_fold_t after FFT rows): u in rows m < ceil(H/2), v[m] in row H-1-m
        GemmProblem g = gemm(CH, 0, K, 1, ws + d.ws_t + (par ? (int64_t)(d.H - 1) * d.Kw : 0),
                             (int64_t)d.Kw * d.H, 1, par ? -(int64_t)d.Kw : d.Kw,
                             ws + d.ws_y + (int64_t)par * d.Kw, (int64_t)d.Kh * d.Kw, 2 * (int64_t)d.Kw, 1, M,
                             d.Kw, K, 3);
        attach_x3(ctx, g);
        g.amax = amax(li) + 1;   // T's |max| (row GEMM / k_fold_t)
        add_tiles(ct, (int)(probs.size() - p0), g);
        probs.push_back(g);
      }
      if (row_route(d) != Route::kGemm) {
        fold.push_back(li);
        j.fold_max_hw = std::max<int64_t>(j.fold_max_hw, (int64_t)d.H * d.W);
      }
    }
    return 0;
  }

  // the job's lists into the plan; the order of the adds is the order of the plan's bytes
  void commit(PlanBuf& out, const ImgDesc* D) {
    const GemmProblem* gp = probs.data() + p0;
    const int n_gp = (int)(probs.size() - p0);
    j.desc = {out.add(D, j.i1 - j.i0), j.i1 - j.i0};
    // k_gemm_h2 when every GEMM of the job has its shared matrix pre-split
    j.h2 = ctx->opt.gemm_x3 && ctx->opt.gemm_h2 && n_gp > 0;
    for (int q = 0; q < n_gp; ++q) j.h2 = j.h2 && gp[q].Xh != nullptr;
    j.gp = {out.add(gp, n_gp), n_gp};
    if (ctx->opt.xcd_order) {
      xcd_deal_tiles(rt, gp, 1);
      xcd_deal_tiles(ct, gp, 2);
      xcd_deal_tiles(ft, gp, 1);   // an image's blocks on one XCD: its two matrices in one L2
      for (int v = 1; v < kVariants; ++v) xcd_deal_col_blocks(fc[v]);
    }
    j.rows_t = out.add(rt);
    j.fused_t = out.add(ft);
    j.cols_t = out.add(ct);
    for (int v = 0; v < kVariants; ++v) {
      j.fr[v] = out.add(fr[v]);
      j.fc[v] = out.add(fc[v]);
    }
    j.ipt = out.add(ipt);
    j.fold = out.add(fold);
    for (int l = 0; l < 4; ++l) {
      j.br[l] = out.add(br[l]);
      j.bc[l] = out.add(bc[l]);
    }
    // all spec-1 column items of the job in one persistent launch, when their qw agree
    j.n_pc = (pc_ok && (int)pc.size() * 3 * pc_qw == (int)fc[1].size()) ? (int)pc.size() : 0;
    j.pc_qw = pc_qw;
    j.pc = out.add(pc);
    j.pb = out.add(pb);
    j.epi = out.add(epi);
  }
};

// The encode engine.  Full mode (pack != NULL): packed DCTPatches outputs.
// Token mode (pack == NULL): spectrum tokens in flat order (tokens_dev /
// scores_dev at tok_off).  Per image the row DCT (length W) and the column
// DCT (length H) each run on the FFT kernels when the length has a plan, else
// on the MFMA GEMM; the intermediate T[c][y][kx] (3, H, Kw) is shared.
static int build_encode_plan(OrderedCall& oc, const EncCall& c, EncPlan& E) {
  dctae_ctx* ctx = oc.ctx;
  int rc;
  // 1. describe and validate the images
  EncImages im;
  if ((rc = describe_images(ctx, c, im))) return rc;
  std::vector<ImgDesc>& D = im.D;
  const int n = (int)D.size();
  // 2. cut chunks and lay out the workspace (dctae_enc_layout.h); tokens in image order
  const WsLayout wl = lay_out_workspace(D.data(), n, ctx->opt);
  E.ws_need = wl.ws_need;
  for (const JobRange& r : wl.jobs) {
    ChunkJob j{};
    j.i0 = r.i0, j.i1 = r.i1, j.amax_off = r.amax_off, j.max_T = 1;
    for (int i = j.i0; i < j.i1; ++i) {
      D[i].tok_off = c.full ? E.n_tok : c.tok_off_user[i];
      E.n_tok += D[i].T;
      j.max_T = std::max(j.max_T, D[i].T);
    }
    E.max_T = std::max(E.max_T, j.max_T);
    E.jobs.push_back(j);
  }
  E.n_img = n;
  E.uniform = true;
  for (int i = 1; i < n; ++i) E.uniform = E.uniform && D[i].H == D[0].H && D[i].W == D[0].W;
  // 3. size the scratch: both buffers where the plan is built (token_sinks carves the staging)
  E.stage = StageLayout(E.n_tok, c.ncb, c.cfg->patch_size * c.cfg->patch_size, c.want_norm, c.want_raw && c.full);
  uint8_t* st;
  if ((rc = oc.scratch(kWs, std::max<size_t>(E.ws_need, 256), &E.ws)) ||
      (rc = oc.scratch(kStage, std::max<size_t>(E.stage.need, 256), &st)))
    return rc;
  // 4. build each job's lists
  std::vector<GemmProblem> probs;
  for (ChunkJob& j : E.jobs) {
    JobLists b{ctx, c.cfg, im.plans, E.ws, j, probs, probs.size()};
    for (int i = j.i0; i < j.i1; ++i)
      if ((rc = b.rows(D[i], i - j.i0)) || (rc = b.cols(D[i], i - j.i0))) return rc;
    b.commit(E.pb, D.data() + j.i0);
  }
  // 5. serialise what the jobs share
  E.plans = E.pb.add(im.plans);
  E.all_desc = E.pb.add(D);
  E.any_pad = false;
  if (c.full) {
    if (c.pack->n_rows > 0) E.rowlen = {E.pb.add(c.pack->row_len, c.pack->n_rows), c.pack->n_rows};
    for (int r = 0; r < c.pack->n_rows; ++r) E.any_pad = E.any_pad || c.pack->row_len[r] < c.cfg->max_seq_len;
  }
  return 0;
}

// the call's plan: the cached one, or a new one that replaces it
static int encode_plan(OrderedCall& oc, const EncCall& c, EncPlan** out) {
  dctae_ctx* ctx = oc.ctx;
  std::vector<int64_t> key = c.plan_key(ctx->opt);
  float* ws;   // as it is now: another call may have moved it since the plan was built
  int rc = oc.scratch(kWs, 0, &ws);
  if (rc) return rc;
  if (!ctx->enc_plan || ctx->enc_plan->ws != ws || key != ctx->enc_key) {
    EncPlan* E = new EncPlan();
    E->id = ++ctx->plan_counter;
    rc = build_encode_plan(oc, c, *E);
    if (rc) {
      delete E;
      return rc;
    }
    delete ctx->enc_plan;
    ctx->enc_plan = E;
    ctx->enc_key = std::move(key);
  }
  *out = ctx->enc_plan;
  return 0;
}

void dctae::drop_encode_plan(dctae_ctx* ctx) {
  delete ctx->enc_plan;
  ctx->enc_plan = nullptr;
}

static PackSinks pack_sinks(const PackedOut& out) {
  return PackSinks{out.codes_dev,   out.positions_dev,   out.channels_dev, out.image_ids_dev,
                   out.patches_dev, out.raw_patches_dev, out.scores_dev,   out.key_pad_dev};
}

// token staging for the whole call (flat token order, global offsets)
static int token_sinks(OrderedCall& oc, const EncCall& c, const EncPlan& E, TokenSinks& sk) {
  sk = TokenSinks{};
  if (!c.full) {
    sk.scores = c.scores_dev;
    sk.raw = c.tokens_dev;
    return 0;
  }
  uint8_t* st;
  if (int rc = oc.scratch(kStage, std::max<size_t>(E.stage.need, 256), &st)) return rc;
  sk.scores = (float*)(st + E.stage.scores);
  if (c.ncb) sk.codes = (uint16_t*)(st + E.stage.codes);
  if (c.want_norm) sk.norm = (float*)(st + E.stage.norm);
  if (c.want_raw) sk.raw = (float*)(st + E.stage.raw);
  return 0;
}

// The context's side stream for the length of one call.  fork(s) lets the side
// stream start after what `s` holds so far; once forked, `s` waits for the side
// stream at join() and on every exit (error returns included), so the call's
// OrderedCall, declared before it, records the side stream's work too.
struct SideStream {
  dctae_ctx* ctx;
  hipStream_t s = nullptr;
  bool armed = false;
  explicit SideStream(dctae_ctx* c) : ctx(c) {}
  int ensure() {
    if (ctx->side) return 0;
    if (hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->side_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->side_out, hipEventDisableTiming) != hipSuccess)
      return fail(ctx, DCTAE_EHIP, "side stream allocation failed");
    return 0;
  }
  int fork(hipStream_t from) {
    HIPCHK(ctx, hipEventRecord(ctx->side_in, from));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->side, ctx->side_in, 0));
    s = from;
    armed = true;
    return 0;
  }
  void join() {
    if (!armed) return;
    armed = false;
    if (hipEventRecord(ctx->side_out, ctx->side) != hipSuccess || hipStreamWaitEvent(s, ctx->side_out, 0) != hipSuccess)
      hipStreamSynchronize(ctx->side);
  }
  ~SideStream() { join(); }
};

// What the launches of one call share, and the pieces of its launch sequence.
struct EncLaunch {
  dctae_ctx* ctx;
  const dctae_fe_cfg* cfg;
  const ImageSet& imgs;
  const EncPlan& E;
  hipStream_t s;             // the caller's stream
  uint8_t* pd;               // the uploaded plan
  const FftPlan* plans_d;
  const ImgDesc* all_d;      // every image of the call (sort / pack)
  EncParams epj;             // the column epilogues' parameters
  TokenSinks sk, skc;        // the call's staging; the column kernels' sinks
  EncParams eps;             // the pack's parameters
  PackSinks ps;
  CodeType ct;               // the type behind ps.codes

  void gemm(const ChunkJob& j, const PlanList<TileRef>& tiles, hipStream_t st, int share) const {
    if (j.h2)
      launch_gemm_h2(j.gp.at(pd), tiles.at(pd), tiles.n, st, share, ctx->opt.gemm_dma != 0, ctx->opt.cols_dma != 0);
    else
      ctx_gemm(ctx, 3, j.gp.at(pd), tiles.at(pd), tiles.n, st, share);
  }

  // The FFT kernel families that are launched on part of a list too: blocks /
  // items [a, a + m) of the job's list on a stream, one spelling each.
  void rows_spec(const ChunkJob& j, int v, int a, int m, hipStream_t st) const {
    Timer t(ctx, st, "fft_rows");
    launch_fft_rows_spec(v, j.desc.at(pd), j.fr[v].at(pd) + a, m, imgs.rgb, imgs.px, E.ws,
                         ctx->fft_tab + j.row_tab[v].tw_off, ctx->fft_tab + j.row_tab[v].post_off, ctx->cm, st);
  }
  void rows512(const ChunkJob& j, int a, int m, hipStream_t st) const {
    Timer t(ctx, st, "fft_rows");
    launch_rows512(j.desc.at(pd), j.fr[1].at(pd) + a, m, imgs.rgb, imgs.px, E.ws, ctx->fft_tab + j.row_tab[1].tw_off,
                   ctx->fft_tab + j.row_tab[1].post_off, ctx->cm, st);
  }
  void cols_band(const ChunkJob& j, int a, int m, hipStream_t st, bool allow_wide = true) const {
    Timer t(ctx, st, "fft_cols");
    launch_cols512b(j.desc.at(pd), j.pb.at(pd) + a, m, E.ws, ctx->fft_tab + j.col_tab[1].tw_off,
                    ctx->fft_tab + j.col_tab[1].post_off, epj, skc, st, allow_wide && ctx->opt.cols_wide != 0);
  }
  // (k_fft_cols7's persistent list serves the whole spec-1 list: a job that has one is never split)
  void cols_spec(const ChunkJob& j, int v, int a, int m, hipStream_t st) const {
    Timer t(ctx, st, "fft_cols");
    launch_fft_cols_spec(v, j.desc.at(pd), j.fc[v].at(pd) + a, m, E.ws, ctx->fft_tab + j.col_tab[v].tw_off,
                         ctx->fft_tab + j.col_tab[v].post_off, epj, skc, st,
                         v == 1 && j.n_pc ? j.pc.at(pd) : nullptr, v == 1 ? j.n_pc : 0, j.pc_qw);
  }

  // row half of a chunk job on a stream
  void do_rows(const ChunkJob& j, hipStream_t st) const {
    const ImgDesc* dd = j.desc.at(pd);
    const int nj = j.i1 - j.i0;
    uint32_t* amax = reinterpret_cast<uint32_t*>(E.ws + j.amax_off);
    if (j.h2 || j.fused_t.n) hipMemsetAsync(amax, 0, 12 * (size_t)nj + 36, st);   // errors surface at hipGetLastError
    if (j.fused_t.n) {
      int* flags = reinterpret_cast<int*>(amax + 2 * nj);
      for (int fixup = 0; fixup < 2; ++fixup) {
        Timer t(ctx, st, fixup ? "rows_fixup" : "rows_fused");
        launch_rows_fused(j.gp.at(pd), j.fused_t.at(pd), j.fused_t.n, dd, imgs.rgb, imgs.px, ctx->cm, amax, flags, nj,
                          st, fixup != 0);
      }
    }
    if (j.rows_t.n) {
      {
        Timer t(ctx, st, "rgb_to_ipt");
        launch_rgb_to_ipt(dd, j.ipt.at(pd), j.ipt.n, imgs.rgb, imgs.px, E.ws, ctx->cm, j.h2 ? amax : nullptr, st);
      }
      Timer t(ctx, st, "gemm_rows");
      gemm(j, j.rows_t, st, 1);
    }
    for (int l = 0; l < 4; ++l)
      if (j.br[l].n) {
        Timer t(ctx, st, "bs_rows");
        launch_bs_rows(kBsL[l], dd, plans_d, j.br[l].at(pd), j.br[l].n, imgs.rgb, imgs.px, E.ws, ctx->fft_tab, ctx->cm,
                       st, ctx->opt.bs_ablate);
      }
    if (j.fr[0].n) {
      Timer t(ctx, st, "fft_rows");
      launch_fft_rows(dd, plans_d, j.fr[0].at(pd), j.fr[0].n, j.lds_rows, imgs.rgb, imgs.px, E.ws, ctx->fft_tab,
                      ctx->cm, st);
    }
    for (int v = 1; v < kVariants; ++v)
      if (j.fr[v].n) {
        if (v == 1 && rows512_kernel(ctx, cfg))
          rows512(j, 0, j.fr[v].n, st);
        else
          rows_spec(j, v, 0, j.fr[v].n, st);
      }
  }

  // column half of a chunk job on a stream
  void do_cols(const ChunkJob& j, hipStream_t st) const {
    const ImgDesc* dd = j.desc.at(pd);
    if (j.cols_t.n) {
      if (j.fold.n) {
        Timer t(ctx, st, "fold_t");
        launch_fold_t(dd, j.fold.at(pd), j.fold.n, j.fold_max_hw, E.ws,
                      j.h2 ? reinterpret_cast<uint32_t*>(E.ws + j.amax_off) : nullptr, st);
      }
      Timer t(ctx, st, "gemm_cols");
      gemm(j, j.cols_t, st, 2);
    }
    for (int l = 0; l < 4; ++l)
      if (j.bc[l].n) {
        Timer t(ctx, st, "bs_cols");
        launch_bs_cols(kBsL[l], dd, plans_d, j.bc[l].at(pd), j.bc[l].n, E.ws, ctx->fft_tab, st, ctx->opt.bs_ablate);
      }
    if (j.epi.n) {   // the images with Y in the workspace: columns on the GEMM or Bluestein
      Timer t(ctx, st, "tile_epilogue");
      launch_tile_epilogue(dd, j.i1 - j.i0, j.max_T, E.ws, epj, skc, st, j.epi.at(pd), j.epi.n);
    }
    if (j.fc[0].n) {
      Timer t(ctx, st, "fft_cols");
      launch_fft_cols(dd, plans_d, j.fc[0].at(pd), j.fc[0].n, j.lds_cols, E.ws, ctx->fft_tab, epj, skc, st);
    }
    if (j.pb.n) cols_band(j, 0, j.pb.n, st);
    for (int v = 1; v < kVariants; ++v)
      if (j.fc[v].n) cols_spec(j, v, 0, j.fc[v].n, st);
  }

  // sort / pack of images [a, a + m) on a stream
  void sort_pack(int a, int m, hipStream_t st) const {
    launch_sort_pack(all_d + a, m, next_pow2(E.max_T), eps, sk, ps, st, ctx->opt.sort_kernel, E.max_T, ct);
  }

  // halves (option): see Options::halves.  The plan kernel variant (>= 2) of
  // a call that qualifies, else 0.
  int halves_variant() const {
    if (E.jobs.size() != 1 || !E.uniform || E.n_img < 32) return 0;
    const ChunkJob& j = E.jobs[0];
    bool ok = !j.rows_t.n && !j.cols_t.n && j.pb.n == 0 && j.n_pc == 0 && j.fr[0].n == 0 && j.fc[0].n == 0;
    for (int l = 0; l < 4; ++l) ok = ok && !j.br[l].n && !j.bc[l].n;
    int vv = -1;
    for (int v = 1; v < kVariants; ++v)
      if (j.fr[v].n || j.fc[v].n) {
        if (vv < 0 && j.fr[v].n && j.fc[v].n) vv = v;
        else ok = false;
      }
    return ok && vv >= 2 && j.fr[vv].n % E.n_img == 0 && j.fc[vv].n % E.n_img == 0 ? vv : 0;
  }

  // the halves schedule on plan kernel variant hv; *sorted0 = the images it packed
  int run_halves(int hv, SideStream& side, int* sorted0) const {
    const ChunkJob& j = E.jobs[0];
    const int n_img = E.n_img, h = n_img / 2;
    const int rpi = j.fr[hv].n / n_img, cpi = j.fc[hv].n / n_img;   // blocks / items per image (image-major lists)
    rows_spec(j, hv, 0, h * rpi, s);
    if (int rc = side.fork(s)) return rc;
    cols_spec(j, hv, 0, h * cpi, ctx->side);
    {
      Timer t(ctx, ctx->side, "sort_pack");
      sort_pack(0, h, ctx->side);
    }
    rows_spec(j, hv, h * rpi, (n_img - h) * rpi, s);
    cols_spec(j, hv, h * cpi, (n_img - h) * cpi, s);
    *sorted0 = h;
    return 0;
  }

  // sort_overlap: one job of band images only -> columns in two halves, the
  // first half's sort / pack on the side stream while the second half's
  // columns run (the sort is latency-bound, the column kernel issue-bound)
  int run_split_cols(const ChunkJob& j, SideStream& side, int* sorted0) const {
    const int h = j.pb.n / 2;
    cols_band(j, 0, h, s);
    if (int rc = side.fork(s)) return rc;
    sort_pack(0, h, ctx->side);
    cols_band(j, h, j.pb.n - h, s);
    *sorted0 = h;
    return 0;
  }

#ifdef DCTAE_PROFILING
  bool gate_applies() const {
    return ctx->opt.gate && E.jobs.size() == 1 && E.n_img >= 2 && E.jobs[0].pb.n == E.n_img &&
           E.jobs[0].fr[1].n % E.n_img == 0 && ctx->opt.rows_kernel == 4;
  }

  // the profiling gate (Options::gate): part of the band path; *sorted0 = the images to leave unpacked
  int run_gate(SideStream& side, int* sorted0) const {
    const ChunkJob& j = E.jobs[0];
    const int n_img = E.n_img, h = n_img / 2, rpi = j.fr[1].n / n_img;
    auto rows = [&](int a, int m, hipStream_t st) { rows512(j, a * rpi, m * rpi, st); };
    auto cols = [&](int a, int m, hipStream_t st) { cols_band(j, a, m, st, false); };
    const int64_t gate = ctx->opt.gate;
    if (int rc = side.ensure()) return rc;
    switch (gate) {
      case 1: rows(0, n_img, s); break;
      case 2: cols(0, n_img, s); break;
      case 3:
      case 4:
        if (gate == 4) rows(0, h, s);
        if (int rc = side.fork(s)) return rc;
        cols(0, h, ctx->side);
        rows(h, n_img - h, s);
        side.join();
        if (gate == 4) cols(h, n_img - h, s);
        break;
      case 5: rows(h, n_img - h, s); break;
      case 6: cols(0, h, s); break;
    }
    *sorted0 = gate == 4 ? 0 : E.n_img;
    return 0;
  }
#endif
};

// one encode call on stream s: c holds the entry point's arguments
static int encode_call(dctae_ctx* ctx, EncCall& c, hipStream_t s) {
  int rc = c.check(ctx);
  if (rc) return rc;
  const dctae_fe_cfg* cfg = c.cfg;
  const dctae_norm* norm = c.norm;
  const dctae_lfq* lfq = c.lfq;
  const float* proj_w = c.proj_w;
  const bool full = c.full;
  OrderedCall oc(ctx, s);   // before the plan: building it sizes the workspace
  EncPlan* plan;
  if ((rc = encode_plan(oc, c, &plan))) return rc;
  const EncPlan& E = *plan;
  if (proj_w && E.any_pad)
    return fail(ctx, DCTAE_EUNSUP, "fused LFQ projections need rows without padding (the pad token's codes)");
  uint8_t* pd;
  if ((rc = oc.upload(E.pb, &pd, E.id))) return rc;

  EncParams ep = enc_params(cfg, norm, c.want_codes && !proj_w ? lfq : nullptr);
  if (norm && !c.want_norm) ep.thr = norm->thr_dev;
  EncLaunch L{ctx, cfg, c.imgs, E, s, pd, E.plans.at(pd), E.all_desc.at(pd)};
  L.epj = ep;
  if (!full) L.epj.median = nullptr;
  // the pack's parameters (the projection kernel stages raw sign bits: the pack maps them, lfq_index_bits)
  L.eps = ep;
  if (proj_w) {
    L.eps.ncb = lfq->num_codebooks;
    L.eps.cb_dim = lfq->codebook_dim;
    uint64_t pos, neg;
    lfq_index_masks(lfq->codebook_scale, lfq->codebook_dim, &pos, &neg);
    L.eps.code_pos = (uint32_t)pos;
    L.eps.code_neg = (uint32_t)neg;
  }
  if (full) {
    L.ps = pack_sinks(c.out);
    L.ct = c.out.ct;
    // rows filled to max_seq_len (e.g. one 512^2 image per row) have no pads:
    // the sort kernel writes their key_pad zeros, no k_pad_fill launch
    if (c.pack->n_rows > 0 && E.any_pad) {
      Timer t(ctx, s, "pad_fill");
      launch_pad_fill(E.rowlen.at(pd), c.pack->n_rows, ep, c.out.key_pad_dev, L.ps, s, L.ct);
    }
  }
  if ((rc = token_sinks(oc, c, E, L.sk))) return rc;
  L.skc = L.sk;   // the column kernels' sinks (codes come from the projection kernel)
  if (proj_w) L.skc.codes = nullptr;

  // the two-stream schedules apply to packed encodes without fused projections
  SideStream side(ctx);
  const bool two = full && !proj_w;
  const bool split = two && ctx->opt.sort_overlap && E.jobs.size() == 1 && E.n_img >= 64 &&
                     E.jobs[0].pb.n == E.n_img && E.jobs[0].i0 == 0;
  const int hv = two && ctx->opt.halves && !split ? L.halves_variant() : 0;
  if ((split || hv) && (rc = side.ensure())) return rc;
  int sorted0 = 0;   // images [0, sorted0) need no sort / pack on the caller's stream
  bool whole = false;   // the call's rows and columns are launched
  if (hv) {
    if ((rc = L.run_halves(hv, side, &sorted0))) return rc;
    whole = true;
  }
#ifdef DCTAE_PROFILING
  if (two && !hv && !split && L.gate_applies()) {
    if ((rc = L.run_gate(side, &sorted0))) return rc;
    whole = true;
  }
#endif
  for (const ChunkJob& j : E.jobs) {
    if (whole) break;
    L.do_rows(j, s);
    if (!split)
      L.do_cols(j, s);
    else if ((rc = L.run_split_cols(j, side, &sorted0)))
      return rc;
  }
  if (proj_w && E.n_tok > 0) {
    Timer t(ctx, s, "lfq_project_in");
    const int PP = cfg->patch_size * cfg->patch_size;
    uint16_t* wsp;
    if ((rc = oc.scratch(kProj, lfq_proj_scratch_bytes(lfq->codebook_dim * lfq->num_codebooks, PP), &wsp))) return rc;
    // the staged tokens are PatchNorm outputs, clamped to [min_val, max_val]
    // (patchnorm.py:163): the fp16 projection's operand bound
    const float xb = ctx->opt.gemm_h2 ? std::max(std::fabs(norm->min_val), std::fabs(norm->max_val)) : 0.0f;
    launch_lfq_project_in16(L.sk.norm, E.n_tok, PP, proj_w, c.proj_b, lfq->codebook_dim, lfq->num_codebooks,
                            L.sk.codes, wsp, s, xb, ctx->opt.lfq_ws != 0);
  }
  if (full && E.n_img > sorted0) {
    Timer t(ctx, s, "sort_pack");
    L.sort_pack(sorted0, E.n_img - sorted0, s);
  }
  side.join();   // every output complete on the caller's stream
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

// the three encode entries for either image descriptor and either code type
// (the pixel type rides in the ImageSet, the code type in the PackedOut)
static int encode_packed(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const ImageSet& imgs, const dctae_packing* pack,
                         const dctae_norm* norm, const dctae_lfq* lfq, const PackedOut& out, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!pack) return fail(ctx, DCTAE_EINVAL, "packing descriptor is NULL");
  hipSetDevice(ctx->device);
  EncCall c{};
  c.cfg = cfg, c.imgs = imgs, c.pack = pack, c.norm = norm, c.lfq = lfq, c.out = out;
  return encode_call(ctx, c, (hipStream_t)stream);
}

static int encode_packed_proj(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const ImageSet& imgs, const dctae_packing* pack,
                              const dctae_norm* norm, const dctae_lfq* lfq, const float* w_in_dev,
                              const float* b_in_dev, const PackedOut& out, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!pack) return fail(ctx, DCTAE_EINVAL, "packing descriptor is NULL");
  if (!w_in_dev || !out.ok || !out.codes_dev) return fail(ctx, DCTAE_EINVAL, "project_in weight and codes output required");
  hipSetDevice(ctx->device);
  EncCall c{};
  c.cfg = cfg, c.imgs = imgs, c.pack = pack, c.norm = norm, c.lfq = lfq, c.out = out;
  c.proj_w = w_in_dev, c.proj_b = b_in_dev;
  return encode_call(ctx, c, (hipStream_t)stream);
}

static int encode_tokens(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const ImageSet& imgs, const int64_t* tok_off,
                         float* tokens_dev, float* scores_dev, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!tok_off || !scores_dev) return fail(ctx, DCTAE_EINVAL, "tok_off and scores_dev are required");
  hipSetDevice(ctx->device);
  EncCall c{};
  c.cfg = cfg, c.imgs = imgs, c.tok_off_user = tok_off, c.tokens_dev = tokens_dev, c.scores_dev = scores_dev;
  return encode_call(ctx, c, (hipStream_t)stream);
}

extern "C" {

int dctae_encode(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images* imgs, const dctae_packing* pack,
                 const dctae_norm* norm, const dctae_lfq* lfq, const dctae_packed_out* out, void* stream) {
  return encode_packed(ctx, cfg, ImageSet(imgs), pack, norm, lfq, PackedOut(out), stream);
}

int dctae_encode_lfq_proj(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images* imgs,
                          const dctae_packing* pack, const dctae_norm* norm, const dctae_lfq* lfq,
                          const float* w_in_dev, const float* b_in_dev, const dctae_packed_out* out, void* stream) {
  return encode_packed_proj(ctx, cfg, ImageSet(imgs), pack, norm, lfq, w_in_dev, b_in_dev, PackedOut(out), stream);
}

int dctae_spectrum_tokens(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images* imgs, const int64_t* tok_off,
                          float* tokens_dev, float* scores_dev, void* stream) {
  return encode_tokens(ctx, cfg, ImageSet(imgs), tok_off, tokens_dev, scores_dev, stream);
}

// the byte-image entries (include/dctae_u8.h): the same calls, the pixel type apart
int dctae_encode_u8(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images_u8* imgs, const dctae_packing* pack,
                    const dctae_norm* norm, const dctae_lfq* lfq, const dctae_packed_out* out, void* stream) {
  return encode_packed(ctx, cfg, ImageSet(imgs), pack, norm, lfq, PackedOut(out), stream);
}

int dctae_encode_lfq_proj_u8(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images_u8* imgs,
                             const dctae_packing* pack, const dctae_norm* norm, const dctae_lfq* lfq,
                             const float* w_in_dev, const float* b_in_dev, const dctae_packed_out* out, void* stream) {
  return encode_packed_proj(ctx, cfg, ImageSet(imgs), pack, norm, lfq, w_in_dev, b_in_dev, PackedOut(out), stream);
}

int dctae_spectrum_tokens_u8(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images_u8* imgs,
                             const int64_t* tok_off, float* tokens_dev, float* scores_dev, void* stream) {
  return encode_tokens(ctx, cfg, ImageSet(imgs), tok_off, tokens_dev, scores_dev, stream);
}

// the int16-code entries (include/dctae_codes16.h): the same calls, the code type apart
int dctae_encode_c16(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images* imgs, const dctae_packing* pack,
                     const dctae_norm* norm, const dctae_lfq* lfq, const dctae_packed_out16* out, void* stream) {
  return encode_packed(ctx, cfg, ImageSet(imgs), pack, norm, lfq, PackedOut(out), stream);
}

int dctae_encode_u8_c16(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images_u8* imgs,
                        const dctae_packing* pack, const dctae_norm* norm, const dctae_lfq* lfq,
                        const dctae_packed_out16* out, void* stream) {
  return encode_packed(ctx, cfg, ImageSet(imgs), pack, norm, lfq, PackedOut(out), stream);
}

int dctae_encode_lfq_proj_c16(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images* imgs,
                              const dctae_packing* pack, const dctae_norm* norm, const dctae_lfq* lfq,
                              const float* w_in_dev, const float* b_in_dev, const dctae_packed_out16* out,
                              void* stream) {
  return encode_packed_proj(ctx, cfg, ImageSet(imgs), pack, norm, lfq, w_in_dev, b_in_dev, PackedOut(out), stream);
}

int dctae_encode_lfq_proj_u8_c16(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images_u8* imgs,
                                 const dctae_packing* pack, const dctae_norm* norm, const dctae_lfq* lfq,
                                 const float* w_in_dev, const float* b_in_dev, const dctae_packed_out16* out,
                                 void* stream) {
  return encode_packed_proj(ctx, cfg, ImageSet(imgs), pack, norm, lfq, w_in_dev, b_in_dev, PackedOut(out), stream);
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
  OrderedCall oc(ctx, s);
  float* a;                                  // forward: IPT input; inverse: IPT output
  if ((rc = oc.scratch(kWs, (size_t)2 * plane * n_img * 4, &a))) return rc;
  float* u = a + plane * n_img;              // intermediate
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
  uint8_t* pd;
  if ((rc = oc.upload(pb, &pd))) return rc;
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
  OrderedCall oc(ctx, s);
  float* ws;
  uint8_t *stage, *pd;
  if ((rc = oc.scratch(kWs, y_bytes, &ws)) || (rc = oc.scratch(kStage, st_scores + st_raw + st_ids + 256, &stage)))
    return rc;
  PlanBuf pb;
  const size_t d_off = pb.add(&d, 1);
  if ((rc = oc.upload(pb, &pd))) return rc;
  const ImgDesc* dd = (const ImgDesc*)(pd + d_off);
  for (int c = 0; c < 3; ++c)   // kept corner (3, Kh, Kw) of the (3, H, W) spectrum
    HIPCHK(ctx, hipMemcpy2DAsync(ws + (size_t)c * d.Kh * d.Kw, (size_t)d.Kw * 4, spec + (size_t)c * H * W,
                                 (size_t)W * 4, (size_t)d.Kw * 4, d.Kh, hipMemcpyDeviceToDevice, s));
  EncParams ep = enc_params(cfg, nullptr, nullptr);
  ep.S = k;
  TokenSinks sk{};
  sk.scores = (float*)stage;
  sk.raw = (float*)(stage + st_scores);
  PackSinks ps{};
  ps.pos = positions;
  ps.ch = channels;
  ps.ids = (int64_t*)(stage + st_scores + st_raw);
  ps.raw = patches;
  ps.scores = scores;
  {
    Timer t(ctx, s, "tile_epilogue");
    launch_tile_epilogue(dd, 1, d.T, ws, ep, sk, s);
  }
  {
    Timer t(ctx, s, "sort_pack");
    launch_sort_pack(dd, 1, next_pow2(d.T), ep, sk, ps, s, ctx->opt.sort_kernel, d.T);
  }
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

}  // extern "C"
