// Progressive decode (include/dctae_frames.h): the token-prefix frames of the
// images of a packed batch in one launch sequence, and image_clip.
//
// A frame is (source image, slot cut): the decode of the image's tokens at row
// slots j < cut.  The slot map of every frame is built in one pass over the
// tokens (k_frames_map: k_dec_map's layout, one slab per frame); from there on
// a frame is an image: one ImgDesc per frame with its source's geometry and its
// own workspace and output offsets, handed to the decode's own kernels
// (launch_idct_cols512(b), launch_idct_rows512 / _spec, the DCT GEMMs,
// launch_ipt_to_rgb), which read tokens only through the map.  The GEMM path's
// token scatter is the one kernel that is token-driven and so needs a frame
// form (k_scatter_frames).  The frame tables travel in arguments of their own:
// DecodeArgs, ImgDesc and every existing kernel are as they were.  The planner
// and the launch sequence are the decode's own (decode_impl, dctae_decode.hip),
// which branches to the two launchers here where a frames call differs.
#include "dctae_ctx.h"
#include "dctae_device.h"
#include "../../include/dctae_frames.h"

using namespace dctae;

namespace dctae {

namespace {

// the frames sorted by source image: image im owns the sorted frames
// [range[im].x, range[im].y), sorted frame g cuts its image's row at cut[g]
struct FrameTabs {
  const int2* range;
  const int32_t* cut;
};

// one image of dctae_image_clip / one clipped frame as the kernels take it: ClipSpan's fields
struct ClipDesc {
  int64_t in_off, out_off, n;
};
static_assert(sizeof(ClipDesc) == sizeof(ClipSpan) && alignof(ClipDesc) == alignof(ClipSpan), "clip_launch casts");

// ---------------------------------------------------------------------------
// slot map per frame: map[frame][c][w][h] = packed slot of the token (or -1),
// one slab of k_dec_map's layout per sorted frame.  A token of image im at row
// slot j goes, by atomicMax (the later slot wins, FE:639-643), into every frame
// of im with j < cut.  k_dec_map's argument checks and error flags.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void frames_map_token(int64_t t, int64_t id, int64_t c, int64_t h, int64_t w,
                                                 const ImgDesc* __restrict__ imgs, const DecodeArgs& a,
                                                 const FrameTabs& ft, int32_t* __restrict__ map) {
  const int64_t r = t / a.S;
  const int j = (int)(t - r * a.S);
  if (id < 0 || id >= a.lut_w) {
    atomicOr(a.err, 2);
    return;
  }
  const int im = a.lut[r * a.lut_w + id];
  if (im < 0) {
    atomicOr(a.err, 2);
    return;
  }
  const int qh = imgs[im].qh, qw = imgs[im].qw;
  if (c < 0 || c >= 3 || h < 0 || h >= qh || w < 0 || w >= qw) {
    atomicOr(a.err, 4);
    return;
  }
  const int2 fr = ft.range[im];
  const int64_t place = (c * a.maxpw + w) * a.maxph + h;
  const int64_t slab = (int64_t)3 * a.maxpw * a.maxph;
  for (int g = fr.x; g < fr.y; ++g)
    if (j < ft.cut[g]) atomicMax(map + g * slab + place, (int32_t)t);
}

// k_dec_map's two loops: four consecutive tokens per thread through 16-byte
// loads for the first 4 n4 tokens (n4 = 0 unless the tensors are 16-byte
// aligned), the rest token by token
__global__ void k_frames_map(int64_t n_tok, int64_t n4, const ImgDesc* __restrict__ imgs, DecodeArgs a, FrameTabs ft,
                             int32_t* __restrict__ map) {
  typedef long long i64x2 __attribute__((ext_vector_type(2)));
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t0 = 4 * q;
    const uint32_t kp = *reinterpret_cast<const uint32_t*>(a.key_pad + t0);
    if (kp == 0x01010101u) continue;
    const i64x2* ip = reinterpret_cast<const i64x2*>(a.ids + t0);
    const i64x2* cp = reinterpret_cast<const i64x2*>(a.ch + t0);
    const i64x2* pp = reinterpret_cast<const i64x2*>(a.pos + 2 * t0);
    const i64x2 i01 = ip[0], i23 = ip[1], c01 = cp[0], c23 = cp[1];
    const i64x2 p0 = pp[0], p1 = pp[1], p2 = pp[2], p3 = pp[3];
    if (!(kp & 0xffu)) frames_map_token(t0, i01.x, c01.x, p0.x, p0.y, imgs, a, ft, map);
    if (!(kp & 0xff00u)) frames_map_token(t0 + 1, i01.y, c01.y, p1.x, p1.y, imgs, a, ft, map);
    if (!(kp & 0xff0000u)) frames_map_token(t0 + 2, i23.x, c23.x, p2.x, p2.y, imgs, a, ft, map);
    if (!(kp & 0xff000000u)) frames_map_token(t0 + 3, i23.y, c23.y, p3.x, p3.y, imgs, a, ft, map);
  }
  for (int64_t t = 4 * n4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_tok;
       t += (int64_t)gridDim.x * blockDim.x)
    if (!a.key_pad[t]) frames_map_token(t, a.ids[t], a.ch[t], a.pos[2 * t], a.pos[2 * t + 1], imgs, a, ft, map);
}

}  // namespace

void launch_frames_map(int64_t n_tok, const ImgDesc* imgs, const DecodeArgs& a, const int2* range, const int32_t* cut,
                       int32_t* map, hipStream_t s) {
  const FrameTabs ft{range, cut};
  const bool al = ((uintptr_t)a.ids | (uintptr_t)a.ch | (uintptr_t)a.pos) % 16 == 0 && (uintptr_t)a.key_pad % 4 == 0;
  const int64_t n4 = al ? n_tok / 4 : 0;
  const int gx = (int)std::min<int64_t>((std::max<int64_t>(n4, n_tok - 4 * n4) + 255) / 256, 8192);
  if (gx > 0) hipLaunchKernelGGL(k_frames_map, dim3(gx), dim3(256), 0, s, n_tok, n4, imgs, a, ft, map);
}

namespace {

// ---------------------------------------------------------------------------
// GEMM path: k_scatter_tokens for frames.  Token-driven like it (one element of
// one token per thread and step, the same dequantisation); the element goes
// into the spectrum corner of every frame of the token's image whose map names
// the token.  The map has made ownership unique per frame: plain stores.
// imgs: the batch's images (argument checks, corner geometry); frames: one
// descriptor per sorted frame (ws_y).
// ---------------------------------------------------------------------------
template <typename Code>
__global__ void k_scatter_frames(int64_t n_tok, const ImgDesc* __restrict__ imgs, const ImgDesc* __restrict__ frames,
                                 float* __restrict__ ws, DecodeArgs a, FrameTabs ft, const int32_t* __restrict__ map) {
  const int PP = a.P * a.P;
  const int64_t total = n_tok * PP;
  const int64_t slab = (int64_t)3 * a.maxpw * a.maxph;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = e / PP;
    const int q = (int)(e % PP);
    if (a.key_pad[t]) continue;
    const int64_t r = t / a.S;
    const int64_t id = a.ids[t];
    if (id < 0 || id >= a.lut_w) { atomicOr(a.err, 2); continue; }
    const int im = a.lut[r * a.lut_w + id];
    if (im < 0) { atomicOr(a.err, 2); continue; }
    const ImgDesc d = imgs[im];
    const int64_t c = a.ch[t], h = a.pos[2 * t], w = a.pos[2 * t + 1];
    if (c < 0 || c >= 3 || h < 0 || h >= d.qh || w < 0 || w >= d.qw) { atomicOr(a.err, 4); continue; }
    const int2 fr = ft.range[im];
    const int64_t place = (c * a.maxpw + w) * a.maxph + h;
    const int p1 = q / a.P, p2 = q % a.P;
    const int64_t at = (c * d.Kh + (int64_t)a.P * h + p1) * d.Kw + (int64_t)a.P * w + p2;
    float v = 0.0f;
    bool have = false;
    for (int g = fr.x; g < fr.y; ++g) {
      if (map[g * slab + place] != (int32_t)t) continue;   // beyond the frame's cut, or a later slot wins
      if (!have) {
        have = true;
        if (a.use_codes) {
          const int cbi = q / a.cb_dim, dd = q % a.cb_dim;
          const int32_t code = (int32_t)static_cast<const Code*>(a.codes)[t * a.ncb + cbi];
          const float bit = ((code & (1 << (a.cb_dim - 1 - dd))) != 0) ? 1.0f : 0.0f;
          const float y = __fsub_rn(__fmul_rn(bit, a.scale * 2.0f), a.scale);
          const int64_t tab = ((c * a.maxph + h) * a.maxpw + w) * PP + q;
          v = pn_inverse(y, a.median[tab], a.b[tab], a.eps);
        } else {
          v = a.patches[e];
        }
      }
      ws[frames[g].ws_y + at] = v;
    }
  }
}

}  // namespace

void launch_scatter_frames(int64_t n_tok, const ImgDesc* imgs, const ImgDesc* frames, float* ws, const DecodeArgs& a,
                           const int2* range, const int32_t* cut, const int32_t* map, hipStream_t s, CodeType ct) {
  const FrameTabs ft{range, cut};
  const int64_t total = n_tok * a.P * a.P;
  const int gx = (int)std::min<int64_t>((total + 255) / 256, 16384);
  if (gx <= 0) return;
  if (ct == CodeType::kI16)
    hipLaunchKernelGGL(k_scatter_frames<int16_t>, dim3(gx), dim3(256), 0, s, n_tok, imgs, frames, ws, a, ft, map);
  else
    hipLaunchKernelGGL(k_scatter_frames<int64_t>, dim3(gx), dim3(256), 0, s, n_tok, imgs, frames, ws, a, ft, map);
}

namespace {

// ---------------------------------------------------------------------------
// image_clip (util.py:143-147): y = (x - min) / (max - min) per image.
// k_clip_minmax: mm[2 i] = max of ~key(x), mm[2 i + 1] = max of key(x) over
// image i, key = float_key (order-preserving for finite values, every key and
// its complement above 0, the cleared slot): integer atomicMax, so min and
// max are exact and the same on every run.  k_clip_store: the two fp32
// operations, each rounded on its own, through store_px.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float key_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// Both kernels: four values per thread and step through 16-byte loads where
// the image starts 16-byte aligned (and, in k_clip_store, its result at four
// elements' alignment), the remaining n % 4 values (or all of them) one by one.
__global__ __launch_bounds__(256) void k_clip_minmax(const ClipDesc* __restrict__ descs, const float* __restrict__ in,
                                                     uint32_t* __restrict__ mm) {
  const ClipDesc d = descs[blockIdx.y];
  const float* x = in + d.in_off;
  const int64_t n4 = (uintptr_t)x % 16 == 0 ? d.n / 4 : 0;
  const int64_t first = (int64_t)blockIdx.x * 256, step = (int64_t)gridDim.x * 256;
  const int64_t rest = d.n - 4 * n4;
  if (first >= (n4 > rest ? n4 : rest)) return;   // block-uniform: nothing of this image left for the block
  uint32_t lo = 0, hi = 0;
#pragma unroll 2
  for (int64_t q = first + threadIdx.x; q < n4; q += step) {
    const float4 v = reinterpret_cast<const float4*>(x)[q];
    const uint32_t k0 = float_key(v.x), k1 = float_key(v.y), k2 = float_key(v.z), k3 = float_key(v.w);
    lo = max(max(lo, ~k0), max(max(~k1, ~k2), ~k3));
    hi = max(max(hi, k0), max(max(k1, k2), k3));
  }
  for (int64_t i = 4 * n4 + first + threadIdx.x; i < d.n; i += step) {
    const uint32_t k = float_key(x[i]);
    lo = max(lo, ~k);
    hi = max(hi, k);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    lo = max(lo, (uint32_t)__shfl_xor((int)lo, m));
    hi = max(hi, (uint32_t)__shfl_xor((int)hi, m));
  }
  // one pair of atomics per block: every block of an image hits the same two words
  __shared__ uint32_t part[2][4];
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = lo;
    part[1][threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const uint32_t* p = part[threadIdx.x];
    atomicMax(mm + 2 * blockIdx.y + threadIdx.x, max(max(p[0], p[1]), max(p[2], p[3])));
  }
}

template <typename Out>
__global__ __launch_bounds__(256) void k_clip_store(const ClipDesc* __restrict__ descs, const float* in,
                                                    const uint32_t* __restrict__ mm, Out* out) {
  const ClipDesc d = descs[blockIdx.y];
  const float lo = key_float(~mm[2 * blockIdx.y]), hi = key_float(mm[2 * blockIdx.y + 1]);
  const float span = __fsub_rn(hi, lo);
  const float* x = in + d.in_off;
  Out* y = out + d.out_off;
  const int64_t n4 = (uintptr_t)x % 16 == 0 && (uintptr_t)y % (4 * sizeof(Out)) == 0 ? d.n / 4 : 0;
  const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
#pragma unroll 2
  for (int64_t q = first; q < n4; q += step) {
    const float4 v = reinterpret_cast<const float4*>(x)[q];
    const float r[4] = {__fdiv_rn(__fsub_rn(v.x, lo), span), __fdiv_rn(__fsub_rn(v.y, lo), span),
                        __fdiv_rn(__fsub_rn(v.z, lo), span), __fdiv_rn(__fsub_rn(v.w, lo), span)};
    if constexpr (sizeof(Out) == 4)
      reinterpret_cast<float4*>(y)[q] = make_float4(r[0], r[1], r[2], r[3]);
    else
      reinterpret_cast<uint32_t*>(y)[q] = dword_from_units(r);
  }
  for (int64_t i = 4 * n4 + first; i < d.n; i += step) y[i] = store_px<Out>(__fdiv_rn(__fsub_rn(x[i], lo), span));
}

}  // namespace

// descs / mm on the device; mm is cleared here.  fp32 results may overwrite their inputs.
// Two timed stages: clip_minmax, clip_store
int clip_launch(dctae_ctx* ctx, const ClipSpan* spans, int n, int64_t max_n, const float* in, uint32_t* mm, void* out,
                PixelType px, hipStream_t s) {
  const ClipDesc* descs = reinterpret_cast<const ClipDesc*>(spans);
  HIPCHK(ctx, hipMemsetAsync(mm, 0, (size_t)n * 8, s));
  // k_clip_store: two values' worth of 16-byte steps per thread; k_clip_minmax: eight, so that few blocks
  // of an image meet at its two words (one block per 2048 values ran at 0.18 TB/s, bound by the atomics)
  const int gx = (int)std::min<int64_t>((max_n + 2047) / 2048, 512);
  const int gm = (int)std::min<int64_t>((max_n + 8191) / 8192, 512);
  if (gx <= 0) return 0;
  {
    Timer t(ctx, s, "clip_minmax");
    hipLaunchKernelGGL(k_clip_minmax, dim3(gm, n), dim3(256), 0, s, descs, in, mm);
  }
  Timer t(ctx, s, "clip_store");
  if (px == PixelType::kU8)
    hipLaunchKernelGGL(k_clip_store<uint8_t>, dim3(gx, n), dim3(256), 0, s, descs, in, mm, (uint8_t*)out);
  else
    hipLaunchKernelGGL(k_clip_store<float>, dim3(gx, n), dim3(256), 0, s, descs, in, mm, (float*)out);
  return 0;
}

constexpr int kMaxFrames = 65535;   // a frame is a grid row of the colour and clip kernels

// the frame tables' refusals (the batch's own have been made)
int frames_check(dctae_ctx* ctx, const DecodeBatch& B, const dctae_frames* fr) {
  if (fr->n_frames < 0 || fr->n_frames > kMaxFrames)
    return fail(ctx, DCTAE_EINVAL, "n_frames outside [0, 65535], got " + std::to_string(fr->n_frames));
  if (fr->n_frames > 0 && (!fr->img || !fr->cut || !fr->out_off)) return fail(ctx, DCTAE_EINVAL, "NULL frame array");
  for (int f = 0; f < fr->n_frames; ++f) {
    if (fr->img[f] < 0 || fr->img[f] >= B.n_img)
      return fail(ctx, DCTAE_EINVAL, "frame " + std::to_string(f) + ": image " + std::to_string(fr->img[f]) +
                                         " out of range (n_img = " + std::to_string(B.n_img) + ")");
    if (fr->cut[f] < 0 || fr->cut[f] > B.cfg->max_seq_len)
      return fail(ctx, DCTAE_EINVAL, "frame " + std::to_string(f) + ": cut " + std::to_string(fr->cut[f]) +
                                         " outside [0, max_seq_len]");
    if (fr->out_off[f] < 0) return fail(ctx, DCTAE_EINVAL, "frame " + std::to_string(f) + ": negative frame offset");
  }
  return 0;
}

}  // namespace dctae

extern "C" {

int dctae_decode_frames(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut,
                        int32_t lut_w, int32_t n_img, const int32_t* out_hw, const int32_t* patch_hw,
                        const int64_t* ids, const uint8_t* key_pad, const int64_t* pos, const int64_t* ch,
                        const dctae_frames* frames, const dctae_norm* norm, const dctae_lfq* lfq, const void* codes,
                        int32_t codes_type, const float* patches, int32_t normed, int32_t clip, void* out,
                        int32_t out_type, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (!frames) return fail(ctx, DCTAE_EINVAL, "NULL frame table");
  if (out_type != DCTAE_PIXEL_F32 && out_type != DCTAE_PIXEL_U8)
    return fail(ctx, DCTAE_EINVAL, "out_type: DCTAE_PIXEL_F32 or DCTAE_PIXEL_U8, got " + std::to_string(out_type));
  if (codes_type != DCTAE_CODES_I64 && codes_type != DCTAE_CODES_I16)
    return fail(ctx, DCTAE_EINVAL, "codes_type: DCTAE_CODES_I64 or DCTAE_CODES_I16, got " + std::to_string(codes_type));
  if (clip != DCTAE_CLIP_NONE && clip != DCTAE_CLIP_MINMAX)
    return fail(ctx, DCTAE_EINVAL, "clip: DCTAE_CLIP_NONE or DCTAE_CLIP_MINMAX, got " + std::to_string(clip));
  if (normed != 0 && normed != 1) return fail(ctx, DCTAE_EINVAL, "normed: 0 or 1, got " + std::to_string(normed));
  // the batch's images have no offsets of their own here: the frames carry them
  const std::vector<int64_t> zero((size_t)std::max(n_img, 1), 0);
  const DecodeBatch B = decode_batch(cfg, n_rows, img_lut, lut_w, n_img, out_hw, zero.data(), patch_hw, ids, key_pad,
                                     pos, ch, stream);
  CodeSrc cs;
  if (codes) cs = codes_type == DCTAE_CODES_I16 ? CodeSrc((const int16_t*)codes) : CodeSrc((const int64_t*)codes);
  if (normed && n_rows > 0 && !patches) return fail(ctx, DCTAE_EINVAL, "decode needs the PatchNorm-space patches");
  return decode_impl(ctx, B, norm, lfq, cs, patches, out, out_type == DCTAE_PIXEL_U8 ? PixelType::kU8 : PixelType::kF32,
                     normed != 0, frames, clip == DCTAE_CLIP_MINMAX);
}

int dctae_image_clip(dctae_ctx* ctx, int32_t n_img, const int32_t* hw, const int64_t* in_off, const float* in,
                     const int64_t* out_off, void* out, int32_t out_type, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (out_type != DCTAE_PIXEL_F32 && out_type != DCTAE_PIXEL_U8)
    return fail(ctx, DCTAE_EINVAL, "out_type: DCTAE_PIXEL_F32 or DCTAE_PIXEL_U8, got " + std::to_string(out_type));
  if (n_img < 0 || n_img > kMaxFrames)
    return fail(ctx, DCTAE_EINVAL, "image_clip: n_img outside [0, 65535], got " + std::to_string(n_img));
  if (n_img > 0 && (!hw || !in_off || !out_off || !in || !out))
    return fail(ctx, DCTAE_EINVAL, "image_clip: NULL array or buffer");
  std::vector<ClipSpan> cd((size_t)n_img);
  int64_t max_n = 1;
  for (int i = 0; i < n_img; ++i) {
    if (hw[2 * i] < 1 || hw[2 * i + 1] < 1)
      return fail(ctx, DCTAE_EINVAL, "image_clip: image " + std::to_string(i) + " has a side < 1");
    if (in_off[i] < 0 || out_off[i] < 0)
      return fail(ctx, DCTAE_EINVAL, "image_clip: image " + std::to_string(i) + ": negative image offset");
    cd[i] = {in_off[i], out_off[i], 3ll * hw[2 * i] * hw[2 * i + 1]};
    max_n = std::max(max_n, cd[i].n);
  }
  if (n_img == 0) return 0;
  hipSetDevice(ctx->device);
  const hipStream_t s = (hipStream_t)stream;
  OrderedCall oc(ctx, s);
  int rc;
  uint32_t* mm;
  if ((rc = oc.scratch(kWs, (size_t)n_img * 8, &mm))) return rc;
  PlanBuf pb;
  const size_t cd_off = pb.add(cd.data(), cd.size());
  uint8_t* pd;
  if ((rc = oc.upload(pb, &pd))) return rc;
  if ((rc = clip_launch(ctx, (const ClipSpan*)(pd + cd_off), n_img, max_n, in, mm, out,
                        out_type == DCTAE_PIXEL_U8 ? PixelType::kU8 : PixelType::kF32, s)))
    return rc;
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

}  // extern "C"
