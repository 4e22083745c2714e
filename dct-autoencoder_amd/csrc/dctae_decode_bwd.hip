// Backward of the decode (FE.postprocess, FE:289-310, as dctae_decode computes
// it) and the fused pixel loss of the reference's step_autoencoder
// (main.py:95-110): dctae_decode_backward, dctae_pixel_loss_forward.
//
//   forward   tokens -> Y (kept corner, zero elsewhere) -> U = CH^T Y -> ipt = U CW -> rgb
//   backward  G (3,H,W) -> g_ipt (colour adjoint, k_color_bwd)
//               -> T = g_ipt CW^T (H x Kw) -> dY = CH T (Kh x Kw)      (k_gemm_x3)
//               -> dpatches[row, s, :] = the token's P x P tile of dY  (k_gather_tokens)
//
// The colour adjoint needs the pre-colour image ipt at every pixel.  It is
// recomputed from the patches by the colour-less GEMM inverse (dec_map,
// scatter_tokens and the decode's two GEMMs) at the head of the backward:
// the forward kernels -- the 512 x 512 FFT path included, whose row kernel
// fuses the colour transform and never stores ipt -- stay exactly as they are.
// The workspace regions of the recompute (Y, U, ipt) are reused in place by
// the adjoint (dY, T, g_ipt).  The recompute takes the DC coefficient of every
// channel out of Y before the GEMMs (k_take_dc) and the colour kernel adds its
// constant Y00 / sqrt(H W) back: a GEMM's error is relative to the largest
// term it accumulates, which for an image is the DC term, some 50 x the rest.
// Measured on a 61 x 47 image against float64: ipt to 2.7e-8 rms instead of
// 8.2e-8, and the derivative |l|^(1/gamma - 1) taken at it moves the gradient
// by 1.2e-6 instead of 6.1e-6 of a largest element of 30.
//
// The unit is built with -ffp-contract=off like the rest of the library; powf
// is the precise one.  Nothing here uses floating-point atomics: the loss is
// block partials (double) in the workspace, added in a fixed order by one block.
#include "dctae_ctx.h"
#include "dctae_dec_layout.h"
#include "dctae_device.h"

using namespace dctae;

namespace {

constexpr int kThreads = 256;
constexpr int kLossBlocks = 64;    // blocks per image of the pixel loss (grid.x)

__device__ __forceinline__ float qnan() { return __int_as_float(0x7fc00000); }

template <class T>
__device__ inline T block_sum(T v, T* red, int tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = red[tid] + red[tid + o];
    __syncthreads();
  }
  return red[0];
}

struct PixImg {
  int64_t off;   // element offset of the (3,H,W) image in both RGB buffers
  int64_t n;     // 3 H W
};

// ---- (d) pixel loss ----------------------------------------------------------
// grid (gx, n_img): block (b, i) takes the units [b upb, (b + 1) upb) of image i
// (a unit = W floats); part[i gx + b] = its sum of (x_hat - x)^2
template <int W>
__device__ __forceinline__ void pixel_sq_block(const float* __restrict__ a, const float* __restrict__ b, int64_t units,
                                               float& acc) {
  const int64_t per = (units + gridDim.x - 1) / gridDim.x;
  const int64_t u0 = (int64_t)blockIdx.x * per, u1 = min(units, u0 + per);
  for (int64_t u = u0 + threadIdx.x; u < u1; u += kThreads) {
    if constexpr (W == 4) {
      const float4 p = reinterpret_cast<const float4*>(a)[u], q = reinterpret_cast<const float4*>(b)[u];
      const float d0 = p.x - q.x, d1 = p.y - q.y, d2 = p.z - q.z, d3 = p.w - q.w;
      acc += d0 * d0;
      acc += d1 * d1;
      acc += d2 * d2;
      acc += d3 * d3;
    } else {
      const float d = a[u] - b[u];
      acc += d * d;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_pixel_loss_fwd(const PixImg* __restrict__ imgs,
                                                             const float* __restrict__ xh,
                                                             const float* __restrict__ x, int vec_bases,
                                                             double* __restrict__ part) {
  __shared__ double redd[kThreads];
  const PixImg d = imgs[blockIdx.y];
  const float *a = xh + d.off, *b = x + d.off;
  float acc = 0.0f;   // a thread's terms in fp32, threads and blocks in double
  if (vec_bases && (d.off & 3) == 0 && (d.n & 3) == 0)
    pixel_sq_block<4>(a, b, d.n >> 2, acc);
  else
    pixel_sq_block<1>(a, b, d.n, acc);
  const double t = block_sum((double)acc, redd, threadIdx.x);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// sc[0] = pixel_loss = mean_i mse_i, sc[1 + i] = mse_i (one block): thread t
// adds the gx partials of the images t, t + 256, ... in order, then the tree
__global__ __launch_bounds__(kThreads) void k_pixel_loss_finish(const PixImg* __restrict__ imgs,
                                                                const double* __restrict__ part, int gx, int n_img,
                                                                float* __restrict__ sc) {
  __shared__ double redd[kThreads];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < n_img; i += kThreads) {
    double m = 0.0;
    for (int b = 0; b < gx; ++b) m += part[(int64_t)i * gx + b];
    m /= (double)imgs[i].n;
    sc[1 + i] = (float)m;
    s += m;
  }
  const double t = block_sum(s, redd, tid);
  if (tid == 0) sc[0] = (float)(t / (double)n_img);   // n_img = 0: 0 / 0 = NaN
}

// dc[3 i + c] = Y[c][0][0] of image i, which is then zeroed (one block per image)
__global__ void k_take_dc(const ImgDesc* __restrict__ imgs, float* __restrict__ ws, float* __restrict__ dc) {
  const int c = threadIdx.x;
  if (c >= 3) return;
  const ImgDesc d = imgs[blockIdx.x];
  float* y = ws + d.ws_y + (int64_t)c * d.Kh * d.Kw;
  dc[3 * blockIdx.x + c] = *y;
  *y = 0.0f;
}

// ---- (a) colour adjoint --------------------------------------------------------
// in place on the workspace image: ipt -> g_ipt.  With l = ipt2lms ipt,
// rgb = lms2rgb (sign(l) |l|^(1/gamma)):
//   g_ipt = ipt2lms^T ((1/gamma) |l|^(1/gamma - 1) (lms2rgb^T G))      (0 at l = 0)
// G = grad (the generic vjp), or g[0] 2 (x_hat - x) / (3 H W n_img) formed here
// (the pixel loss's own gradient image is never stored).
template <int W>
__device__ __forceinline__ void color_bwd_px(const ColorMats& cm, float* __restrict__ p, int64_t hw,
                                             const float* __restrict__ grad, const float* __restrict__ xh,
                                             const float* __restrict__ x, float k, const float (&dc)[3],
                                             int64_t u) {
  const float inv_gamma = 2.3255813121795654296875f;  // fp32(1/0.43), as the forward
  const float e1 = inv_gamma - 1.0f;
  float ipt[3][W], G[3][W];
  for (int c = 0; c < 3; ++c) {
    const int64_t e = c * hw + u * W;
    if constexpr (W == 4) {
      const float4 v = *reinterpret_cast<const float4*>(p + e);
      ipt[c][0] = v.x, ipt[c][1] = v.y, ipt[c][2] = v.z, ipt[c][3] = v.w;
      if (grad) {
        const float4 g = *reinterpret_cast<const float4*>(grad + e);
        G[c][0] = g.x, G[c][1] = g.y, G[c][2] = g.z, G[c][3] = g.w;
      } else {
        const float4 a = *reinterpret_cast<const float4*>(xh + e), b = *reinterpret_cast<const float4*>(x + e);
        G[c][0] = k * (a.x - b.x), G[c][1] = k * (a.y - b.y), G[c][2] = k * (a.z - b.z), G[c][3] = k * (a.w - b.w);
      }
    } else {
      ipt[c][0] = p[e];
      G[c][0] = grad ? grad[e] : k * (xh[e] - x[e]);
    }
  }
  float o[3][W];
#pragma unroll
  for (int i = 0; i < W; ++i) {
    float gm[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float l = mat3_row(cm.ipt2lms, j, ipt[0][i] + dc[0], ipt[1][i] + dc[1], ipt[2][i] + dc[2]);
      // lms2rgb^T G: column j of lms2rgb
      const float up = fmaf(cm.lms2rgb[6 + j], G[2][i], fmaf(cm.lms2rgb[3 + j], G[1][i], cm.lms2rgb[j] * G[0][i]));
      const float al = fabsf(l);
      const float dl = al > 0.0f ? inv_gamma * powf(al, e1) : (l == l ? 0.0f : l);
      gm[j] = dl * up;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      o[c][i] = fmaf(cm.ipt2lms[6 + c], gm[2], fmaf(cm.ipt2lms[3 + c], gm[1], cm.ipt2lms[c] * gm[0]));
  }
  for (int c = 0; c < 3; ++c) {
    const int64_t e = c * hw + u * W;
    if constexpr (W == 4)
      *reinterpret_cast<float4*>(p + e) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
    else
      p[e] = o[c][0];
  }
}

// grid (gx, n_img), grid-stride inside the image
__global__ __launch_bounds__(kThreads) void k_color_bwd(const ImgDesc* __restrict__ imgs, float* __restrict__ ws,
                                                        const float* __restrict__ grad,
                                                        const float* __restrict__ xh, const float* __restrict__ x,
                                                        const float* __restrict__ g,
                                                        const float* __restrict__ dcs, int n_img, int vec_bases,
                                                        ColorMats cm) {
  const ImgDesc d = imgs[blockIdx.y];
  const int64_t hw = (int64_t)d.H * d.W;
  float k = 0.0f;
  if (!grad) k = (g[0] / (float)n_img) * (2.0f / (float)(3 * hw));
  // the DC coefficients' constant image Y00 / sqrt(H W) (k_take_dc)
  const float idc = (float)(1.0 / sqrt((double)hw));
  const float dc[3] = {dcs[3 * blockIdx.y] * idc, dcs[3 * blockIdx.y + 1] * idc, dcs[3 * blockIdx.y + 2] * idc};
  float* p = ws + d.ws_p;
  const float* gr = grad ? grad + d.rgb_off : nullptr;
  const float* a = grad ? nullptr : xh + d.rgb_off;
  const float* b = grad ? nullptr : x + d.rgb_off;
  const int64_t first = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
  // ws_p is a multiple of 4 floats (decode_bwd_layout)
  if (vec_bases && (hw & 3) == 0 && (d.rgb_off & 3) == 0) {
    for (int64_t u = first; u < (hw >> 2); u += step) color_bwd_px<4>(cm, p, hw, gr, a, b, k, dc, u);
  } else {
    for (int64_t u = first; u < hw; u += step) color_bwd_px<1>(cm, p, hw, gr, a, b, k, dc, u);
  }
}

// ---- (c) adjoint of revert_patching ---------------------------------------------
// every element of dpatches is written: the P x P tile of dY at the token's
// place where the token owns it in the forward's slot map (k_dec_map: the later
// packed slot of a duplicate place wins, FE:639-643), exact zeros at padding
// and at an overwritten duplicate, NaN (and the context's index error, set by
// k_dec_map's identical checks) at a token the forward flags.
// A unit = W consecutive floats of a token.
template <int W>
__global__ __launch_bounds__(kThreads) void k_gather_tokens(int64_t units, const ImgDesc* __restrict__ imgs,
                                                            const float* __restrict__ ws, DecodeArgs a,
                                                            const int32_t* __restrict__ map,
                                                            float* __restrict__ dp) {
  const int P = a.P, PP = P * P, U = PP / W;
  const int64_t first = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
  int64_t t = first / U;
  int q = (int)(first - t * U);
  const int64_t dt = step / U;
  const int dq = (int)(step % U);
  for (int64_t u = first; u < units; u += step) {
    const int64_t e = t * PP + (int64_t)q * W;
    float r[W];
#pragma unroll
    for (int i = 0; i < W; ++i) r[i] = 0.0f;
    if (!a.key_pad[t]) {
      const int64_t row = t / a.S, id = a.ids[t];
      const int im = (id < 0 || id >= a.lut_w) ? -1 : a.lut[row * a.lut_w + id];
      bool bad = im < 0;
      if (!bad) {
        const ImgDesc d = imgs[im];
        const int64_t c = a.ch[t], h = a.pos[2 * t], w = a.pos[2 * t + 1];
        bad = c < 0 || c >= 3 || h < 0 || h >= d.qh || w < 0 || w >= d.qw;
        if (!bad && map[(((int64_t)im * 3 + c) * a.maxpw + w) * a.maxph + h] == (int32_t)t) {
          const float* y = ws + d.ws_y + (c * d.Kh + (int64_t)P * h) * d.Kw + (int64_t)P * w;
#pragma unroll
          for (int i = 0; i < W; ++i) {
            const int qq = q * W + i, p1 = qq / P, p2 = qq - p1 * P;
            r[i] = y[(int64_t)p1 * d.Kw + p2];
          }
        }
      }
      if (bad) {   // k_dec_map made the same checks and set the context's index error
#pragma unroll
        for (int i = 0; i < W; ++i) r[i] = qnan();
      }
    }
    if constexpr (W == 4)
      *reinterpret_cast<float4*>(dp + e) = make_float4(r[0], r[1], r[2], r[3]);
    else
      dp[e] = r[0];
    t += dt;
    q += dq;
    if (q >= U) {
      q -= U;
      t += 1;
    }
  }
}

bool aligned16(std::initializer_list<const void*> ps) {
  uintptr_t bits = 0;
  for (const void* p : ps) bits |= (uintptr_t)p;
  return (bits & 15) == 0;
}

}  // namespace

extern "C" {

int dctae_pixel_loss_forward(dctae_ctx* ctx, int32_t n_img, const int32_t* out_hw, const int64_t* out_off,
                             const float* rgb_hat_dev, const float* rgb_dev, float* scalars_dev, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  hipSetDevice(ctx->device);
  if (n_img < 0 || !scalars_dev || (n_img > 0 && (!out_hw || !out_off || !rgb_hat_dev || !rgb_dev)))
    return fail(ctx, DCTAE_EINVAL, "bad pixel loss arguments");
  if (n_img > 65535) return fail(ctx, DCTAE_EUNSUP, "pixel loss: more than 65535 images in one call");
  hipStream_t s = (hipStream_t)stream;
  std::vector<PixImg> D(std::max(n_img, 1));
  int64_t max_n = 1;
  for (int i = 0; i < n_img; ++i) {
    const int64_t H = out_hw[2 * i], W = out_hw[2 * i + 1];
    if (H < 1 || W < 1 || out_off[i] < 0) return fail(ctx, DCTAE_EINVAL, "bad pixel loss image descriptor");
    D[i].off = out_off[i];
    D[i].n = 3 * H * W;
    max_n = std::max(max_n, D[i].n);
  }
  // at least four float4 per thread and block; at most kLossBlocks blocks per image
  const int gx = (int)std::min<int64_t>(kLossBlocks, (max_n + 16 * kThreads - 1) / (16 * kThreads));
  int rc;
  OrderedCall oc(ctx, s);
  double* part;
  if ((rc = oc.scratch(kWs, std::max<size_t>((size_t)n_img * gx * sizeof(double), 512), &part))) return rc;
  PlanBuf pb;
  const size_t d_off = pb.add(D.data(), D.size());
  uint8_t* pd;
  if ((rc = oc.upload(pb, &pd))) return rc;
  const PixImg* dd = (const PixImg*)(pd + d_off);
  Timer t(ctx, s, "pixel_loss_forward");
  if (n_img > 0)
    k_pixel_loss_fwd<<<dim3(gx, n_img), kThreads, 0, s>>>(dd, rgb_hat_dev, rgb_dev,
                                                          aligned16({rgb_hat_dev, rgb_dev}) ? 1 : 0, part);
  k_pixel_loss_finish<<<1, kThreads, 0, s>>>(dd, part, gx, n_img, scalars_dev);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_decode_backward(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut,
                          int32_t lut_w, int32_t n_img, const int32_t* out_hw, const int64_t* out_off,
                          const int32_t* patch_hw, const int64_t* ids, const uint8_t* key_pad, const int64_t* pos,
                          const int64_t* ch, const float* patches, const float* grad_rgb, const float* rgb_hat,
                          const float* rgb, const float* g, float* dpatches, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  const DecodeBatch B{cfg, n_rows, img_lut, lut_w, n_img, out_hw, out_off, patch_hw, ids, key_pad, pos, ch, s};
  if (!ctx) return DCTAE_EINVAL;
  hipSetDevice(ctx->device);
  int rc = decode_check(ctx, B, nullptr, true, patches && dpatches);
  if (rc) return rc;
  const int PP = cfg->patch_size * cfg->patch_size;
  if (n_img > 0 && !grad_rgb && (!rgb_hat || !rgb || !g))
    return fail(ctx, DCTAE_EINVAL, "decode backward needs grad_rgb, or rgb_hat, rgb and the upstream scalar");
  if (n_img > 65535) return fail(ctx, DCTAE_EUNSUP, "decode backward: more than 65535 images in one call");
  if (n_rows == 0) return 0;
  const int64_t n_tok = (int64_t)n_rows * cfg->max_seq_len;
  if (n_tok > ((int64_t)1 << 31) - 1) return fail(ctx, DCTAE_EUNSUP, "decode backward: too many tokens in one call");
  std::vector<ImgDesc> D;
  int64_t max_hw;
  if ((rc = decode_geometry(ctx, B, D, &max_hw))) return rc;
  // workspace: every Y first (one memset), then U / T and ipt / g_ipt per image, the slot map, the DC coefficients
  const DecBwdLayout L = decode_bwd_layout(D.data(), n_img, cfg->max_patch_h, cfg->max_patch_w);
  D.resize(std::max(n_img, 1));   // the plan holds a descriptor even without images
  const int64_t y_floats = L.y_floats, gmap_off = L.map_off, gmap_n = L.map_n, dc_off = L.dc_off;
  OrderedCall oc(ctx, s);
  float* ws;
  if ((rc = oc.scratch(kWs, L.request, &ws))) return rc;
  std::vector<GemmProblem> probs;
  std::vector<TileRef> t1, t2, t3, t4;
  for (int i = 0; i < n_img; ++i) {
    const ImgDesc& d = D[i];
    const float *CW, *CH;
    GemmProblem gs[4];
    // the decode's pair: U[c][y][kx] = sum_ky CH[ky][y] Y[c][ky][kx];  ipt[c][y][x] = sum_kx U[c][y][kx] CW[kx][x]
    if ((rc = decode_gemm_pair(ctx, cfg, d, ws, &gs[0], &gs[1], &CW, &CH))) return rc;
    // its adjoint, truncated to the kept corner:
    // T[c][y][kx] = sum_x g_ipt[c][y][x] CW[kx][x];  dY[c][ky][kx] = sum_y CH[ky][y] T[c][y][kx]
    gs[2] = gemm(ws + d.ws_p, (int64_t)d.H * d.W, d.W, 1, CW, 0, d.W, 1, ws + d.ws_t, (int64_t)d.H * d.Kw, d.Kw, 1,
                 d.H, d.Kw, d.W, 3);
    gs[3] = gemm(CH, 0, d.H, 1, ws + d.ws_t, (int64_t)d.H * d.Kw, 1, d.Kw, ws + d.ws_y, (int64_t)d.Kh * d.Kw, d.Kw, 1,
                 d.Kh, d.Kw, d.H, 3);
    attach_x3(ctx, gs[2]);
    attach_x3(ctx, gs[3]);
    std::vector<TileRef>* ts[4] = {&t1, &t2, &t3, &t4};
    for (int k = 0; k < 4; ++k) {
      add_tiles(*ts[k], (int)probs.size(), gs[k]);
      probs.push_back(gs[k]);
    }
  }
  if (ctx->opt.xcd_order) {   // speed only
    xcd_deal_tiles(t1, probs.data(), 2);
    xcd_deal_tiles(t2, probs.data(), 1);
    xcd_deal_tiles(t3, probs.data(), 1);
    xcd_deal_tiles(t4, probs.data(), 2);
  }
  PlanBuf pb;
  const size_t d_off = pb.add(D.data(), D.size());
  const size_t g_off = pb.add(probs.data(), probs.size());
  const size_t t1_off = pb.add(t1.data(), t1.size());
  const size_t t2_off = pb.add(t2.data(), t2.size());
  const size_t t3_off = pb.add(t3.data(), t3.size());
  const size_t t4_off = pb.add(t4.data(), t4.size());
  const size_t lut_off = pb.add(img_lut, (size_t)n_rows * lut_w);
  uint8_t* pd;
  if ((rc = oc.upload(pb, &pd))) return rc;
  const ImgDesc* dd = (const ImgDesc*)(pd + d_off);
  const GemmProblem* gp = (const GemmProblem*)(pd + g_off);
  const DecodeArgs a = decode_args(ctx, B, nullptr, nullptr, nullptr, patches, (const int32_t*)(pd + lut_off), false);
  int32_t* gmap = (int32_t*)(ws + gmap_off);
  if (n_img > 0) {
    HIPCHK(ctx, hipMemsetAsync(ws, 0, (size_t)y_floats * 4, s));
    HIPCHK(ctx, hipMemsetAsync(gmap, 0xFF, (size_t)gmap_n * 4, s));
  }
  {
    Timer t(ctx, s, "dec_map");
    launch_dec_map(n_tok, dd, a, gmap, s);
  }
  if (n_img > 0) {
    {
      Timer t(ctx, s, "bwd_recompute_ipt");
      launch_scatter_tokens(n_tok, dd, ws, a, gmap, s);
      k_take_dc<<<n_img, 64, 0, s>>>(dd, ws, ws + dc_off);
      ctx_gemm(ctx, 3, gp, (const TileRef*)(pd + t1_off), (int)t1.size(), s, 2);
      ctx_gemm(ctx, 3, gp, (const TileRef*)(pd + t2_off), (int)t2.size(), s, 1);
    }
    {
      Timer t(ctx, s, "color_bwd");
      const int gx = (int)std::min<int64_t>((max_hw + 4 * kThreads - 1) / (4 * kThreads), 256);
      const bool vb = grad_rgb ? aligned16({grad_rgb}) : aligned16({rgb_hat, rgb});
      k_color_bwd<<<dim3(gx, n_img), kThreads, 0, s>>>(dd, ws, grad_rgb, rgb_hat, rgb, g, ws + dc_off, n_img,
                                                       vb ? 1 : 0, ctx->cm);
    }
    {
      Timer t(ctx, s, "dct_rows_bwd");
      ctx_gemm(ctx, 3, gp, (const TileRef*)(pd + t3_off), (int)t3.size(), s, 1);
    }
    {
      Timer t(ctx, s, "dct_cols_bwd");
      ctx_gemm(ctx, 3, gp, (const TileRef*)(pd + t4_off), (int)t4.size(), s, 2);
    }
  }
  {
    Timer t(ctx, s, "gather_tokens");
    const bool vec = PP % 4 == 0 && aligned16({dpatches});
    const int64_t units = n_tok * (vec ? PP / 4 : PP);
    const int nb = (int)std::min<int64_t>((units + kThreads - 1) / kThreads, 16384);
    if (vec)
      k_gather_tokens<4><<<nb, kThreads, 0, s>>>(units, dd, ws, a, gmap, dpatches);
    else
      k_gather_tokens<1><<<nb, kThreads, 0, s>>>(units, dd, ws, a, gmap, dpatches);
  }
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

}  // extern "C"
