// Host-side planning shared by the encode and decode units: DCT matrices,
// GEMM problems and tile lists, FFT and Bluestein plans.
#include "dctae_ctx.h"

namespace dctae {

// orthonormal DCT-II matrix rows [0, rows) of size N, fp64 -> fp32.
// parity 0 / 1: the even / odd rows k = 2i (+1) restricted to the columns
// n < ceil(N/2) / floor(N/2), the operand of the folded transform
// X[k] = sum_n C[k][n] (x[n] +- x[N-1-n]) (C[k][N-1-n] = (-1)^k C[k][n]).
int dct_matrix(dctae_ctx* ctx, int N, int rows, const float** out, int parity) {
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

// point a GEMM's shared DCT-matrix operand at its pre-split planes (used by
// k_gemm_x3 only): the operand must be a whole cached matrix read row-major
// with k contiguous
void attach_x3(const dctae_ctx* ctx, GemmProblem& g) {
  const int sh = gemm_share(g);
  if (ctx->opt.gemm_x3) {
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

// XCD-aware order of the column blocks (image, channel, tile column, count) of a
// compile-time plan kernel (speed only; any order is correct): blocks b and
// b+8 are dealt to the same XCD, so give all the blocks of one (image, channel)
// the same b % 8 and consecutive b / 8 — the 56-byte row slices of
// neighbouring tile columns then share that XCD's L2 lines.
void xcd_deal_col_blocks(std::vector<int4>& L) {
  if (L.size() < 16) return;
  // units = runs of blocks with the same (image, channel), in list order
  std::vector<std::vector<int4>> lanes(8);
  size_t u = 0;
  for (size_t a0 = 0; a0 < L.size(); ++u) {
    size_t a1 = a0 + 1;
    while (a1 < L.size() && L[a1].x == L[a0].x && L[a1].y == L[a0].y) ++a1;
    lanes[u % 8].insert(lanes[u % 8].end(), L.begin() + a0, L.begin() + a1);
    a0 = a1;
  }
  std::vector<int4> out;
  out.reserve(L.size());
  size_t maxlen = 0;
  for (auto& l : lanes) maxlen = std::max(maxlen, l.size());
  for (size_t q = 0; q < maxlen; ++q)
    for (int x = 0; x < 8; ++x)
      if (q < lanes[x].size()) out.push_back(lanes[x][q]);
  L.swap(out);
}

void add_tiles(std::vector<TileRef>& t, int prob, const GemmProblem& g) {
  int tm = (g.M + g.tile_m - 1) / g.tile_m;
  for (int i = 0; i < tm * g.tiles_n; ++i) t.push_back({prob, i});
}


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
  if (!ctx->opt.fft_enabled || !ctx->opt.bluestein || N < 32 || N > 1024) return -1;
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


// FFT plan for length N (Makhoul: M = N/2 point complex FFT); -1 if N has no plan
int fft_plan_for(dctae_ctx* ctx, int N, int P, FftPlan* out) {
  // even N: Makhoul on the N / 2 point complex FFT of z[m] = v[2m] + i v[2m + 1];
  // odd N (ctx->opt.fft_odd): the N point complex FFT of v (the real-FFT form)
  const bool odd = (N & 1) != 0;
  const int Mc = odd ? N : N / 2;
  if (!ctx->opt.fft_enabled || N < 4 || (odd && (!ctx->opt.fft_odd || N < 15)) || Mc > 512) return -1;
  if ((size_t)16 * Mc * kMaxP > ctx->lds_limit) return -1;
  auto it = ctx->fft_plans.find(N);
  if (it != ctx->fft_plans.end()) {
    *out = it->second;
    out->spec = ctx->opt.fft_spec_enabled ? fft_spec_id(N, out->radix, out->npass, P) : 0;
    if (out->spec) out->rows_per_block = fft_spec_rows_per_block(out->spec);
    if (!out->spec && !ctx->opt.fft_generic) return -1;   // the GEMM DCT (see Options::fft_generic)
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
  out->spec = ctx->opt.fft_spec_enabled ? fft_spec_id(N, out->radix, out->npass, P) : 0;
  if (out->spec) out->rows_per_block = fft_spec_rows_per_block(out->spec);
  if (!out->spec && !ctx->opt.fft_generic) return -1;   // the GEMM DCT (see Options::fft_generic)
  return 0;
}

}  // namespace dctae
