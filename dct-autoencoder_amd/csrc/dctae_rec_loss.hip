// Reconstruction losses of a training step (the reference's main.py:71, 79-83)
// over packed tokens of PP = patch_size^2 floats, and the gradient of
// PatchNorm.inverse_norm (patchnorm.py:167-177):
//   rec_loss              = mean over real tokens of |out - tn|
//   rec_loss_unnormalized = mean over real tokens of |inverse_norm(out) - raw|
// One read of the three tensors in the forward (plus the optional write of
// inverse_norm(out)), one in the backward; signs are recomputed from the
// inputs, nothing is saved per element.  The unit is built with
// -ffp-contract=off and d1 / d2 are the reference's separately rounded fp32
// operations (pn_inverse), so sign(d2) is the reference's.
//
// Determinism: every block owns a fixed contiguous range of the elements, its
// partial sums (double) and token count go to the workspace, and one block adds
// them in a fixed order; no floating-point atomics.  tn / raw of padded tokens
// are never read; out is read there only to write unnorm.
#include "dctae_device.h"
#include "dctae_launch.h"

namespace dctae {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;   // partials in the workspace: 8 blocks per CU

struct Tok {          // one thread's position in the token stream, advanced without a division
  int64_t t;          // token
  int q;              // unit inside the token (a float, or a float4 in the vector form)
};

__device__ __forceinline__ void advance(Tok& k, int dt, int dq, int U) {
  k.t += dt;
  k.q += dq;
  if (k.q >= U) {
    k.q -= U;
    k.t += 1;
  }
}

template <int W>
struct Vec;
template <>
struct Vec<1> {
  float v[1];
  static __device__ __forceinline__ Vec ld(const float* p) { return Vec{{*p}}; }
  __device__ __forceinline__ void st(float* p) const { *p = v[0]; }
};
template <>
struct Vec<4> {
  float v[4];
  static __device__ __forceinline__ Vec ld(const float* p) {
    const float4 f = *reinterpret_cast<const float4*>(p);
    return Vec{{f.x, f.y, f.z, f.w}};
  }
  __device__ __forceinline__ void st(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

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

__device__ __forceinline__ float qnan() { return __int_as_float(0x7fc00000); }

// torch.sign: 0 at 0, NaN at NaN
__device__ __forceinline__ float sgn(float d) { return d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : d == d ? 0.0f : d; }

__device__ __forceinline__ bool bad_index(int64_t c, int64_t h, int64_t w, int maxph, int maxpw) {
  return c < 0 || c >= 3 || h < 0 || h >= maxph || w < 0 || w >= maxpw;
}

// ---- forward ---------------------------------------------------------------
// block b takes the units [b upb, (b + 1) upb); a unit is W floats of a token.
// part[2 b], part[2 b + 1] = the block's sums of |d1|, |d2|; cnt[b] = its real tokens
template <int W>
__global__ __launch_bounds__(kThreads) void k_rec_loss_fwd(
    const float* __restrict__ out, const float* __restrict__ tn, const float* __restrict__ raw,
    const int64_t* __restrict__ ch, const int64_t* __restrict__ pos, const uint8_t* __restrict__ key_pad,
    int64_t units, int64_t upb, int PP, int maxph, int maxpw, const float* __restrict__ med,
    const float* __restrict__ b, float eps, float* __restrict__ unnorm, double* __restrict__ part,
    int* __restrict__ cnt, int* __restrict__ err) {
  __shared__ double redd[kThreads];
  __shared__ int redi[kThreads];
  const int tid = threadIdx.x, U = PP / W;
  const int64_t u0 = (int64_t)blockIdx.x * upb, u1 = min(units, u0 + upb);
  double s1 = 0.0, s2 = 0.0;
  int m = 0;
  Tok k;
  k.t = (u0 + tid) / U;
  k.q = (int)((u0 + tid) - k.t * U);
  const int dt = kThreads / U, dq = kThreads % U;
  for (int64_t u = u0 + tid; u < u1; u += kThreads, advance(k, dt, dq, U)) {
    const bool real = key_pad[k.t] == 0;
    if (!real && !unnorm) continue;
    const int64_t e = k.t * PP + k.q * W;
    const int64_t c = ch[k.t], h = pos[2 * k.t], w = pos[2 * k.t + 1];
    if (real && k.q == 0) m += 1;
    if (bad_index(c, h, w, maxph, maxpw)) {
      // the reference raises IndexError on out-of-range table indices
      atomicOr(err, 1);
      if (real) s1 = s2 = qnan();
      if (unnorm)
        for (int i = 0; i < W; ++i) unnorm[e + i] = qnan();
      continue;
    }
    const int64_t tab = ((c * maxph + h) * maxpw + w) * PP + k.q * W;
    const Vec<W> o = Vec<W>::ld(out + e), mv = Vec<W>::ld(med + tab), bv = Vec<W>::ld(b + tab);
    Vec<W> inv;
#pragma unroll
    for (int i = 0; i < W; ++i) inv.v[i] = pn_inverse(o.v[i], mv.v[i], bv.v[i], eps);
    if (unnorm) inv.st(unnorm + e);
    if (real) {
      const Vec<W> a = Vec<W>::ld(tn + e), r = Vec<W>::ld(raw + e);
      float a1 = 0.0f, a2 = 0.0f;   // a unit's four terms in fp32, units in double
#pragma unroll
      for (int i = 0; i < W; ++i) {
        a1 += fabsf(o.v[i] - a.v[i]);
        a2 += fabsf(inv.v[i] - r.v[i]);
      }
      s1 += (double)a1;
      s2 += (double)a2;
    }
  }
  const double t1 = block_sum(s1, redd, tid);
  const double t2 = block_sum(s2, redd, tid);
  const int ms = block_sum(m, redi, tid);
  if (tid == 0) {
    part[2 * blockIdx.x] = t1;
    part[2 * blockIdx.x + 1] = t2;
    cnt[blockIdx.x] = ms;
  }
}

// sc[0] = rec_loss, sc[1] = rec_loss_unnormalized, sc[2] = M (one block):
// thread t adds the partials t, t + 256, ... in order, then the tree
__global__ __launch_bounds__(kThreads) void k_rec_loss_finish(const double* __restrict__ part,
                                                              const int* __restrict__ cnt, int nb, int PP,
                                                              float* __restrict__ sc) {
  __shared__ double redd[kThreads];
  const int tid = threadIdx.x;
  double s1 = 0.0, s2 = 0.0, m = 0.0;
  for (int i = tid; i < nb; i += kThreads) {
    s1 += part[2 * i];
    s2 += part[2 * i + 1];
    m += (double)cnt[i];
  }
  const double t1 = block_sum(s1, redd, tid);
  const double t2 = block_sum(s2, redd, tid);
  const double M = block_sum(m, redd, tid);
  if (tid == 0) {
    const double N = M * (double)PP;   // M = 0: 0 / 0 = NaN, as F.l1_loss of an empty selection
    sc[0] = (float)(t1 / N);
    sc[1] = (float)(t2 / N);
    sc[2] = (float)M;
  }
}

// ---- backward --------------------------------------------------------------
// LOSS: dout = g0 sign(d1) / (M PP) + (gU + g1 sign(d2) / (M PP)) std at real
// tokens, gU std at padded ones (exact zeros without gU) -- the order in which
// autograd forms it: the gradient of inverse_norm's output first, then times
// std.  !LOSS: dout = gU std at every token (inverse_norm's own backward).
template <int W, bool LOSS>
__global__ __launch_bounds__(kThreads) void k_rec_loss_bwd(
    const float* __restrict__ out, const float* __restrict__ tn, const float* __restrict__ raw,
    const int64_t* __restrict__ ch, const int64_t* __restrict__ pos, const uint8_t* __restrict__ key_pad,
    int64_t units, int PP, int maxph, int maxpw, const float* __restrict__ med, const float* __restrict__ b,
    float eps, const float* __restrict__ sc, const float* __restrict__ g, const float* __restrict__ gu,
    float* __restrict__ dout, int* __restrict__ err) {
  const int U = PP / W;
  float k1 = 0.0f, k2 = 0.0f;
  if (LOSS) {
    const float N = sc[2] * (float)PP;
    k1 = g[0] / N;
    k2 = g[1] / N;
  }
  const int64_t first = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
  Tok k;
  k.t = first / U;
  k.q = (int)(first - k.t * U);
  const int dt = (int)(step / U), dq = (int)(step % U);
  for (int64_t u = first; u < units; u += step, advance(k, dt, dq, U)) {
    const int64_t e = k.t * PP + k.q * W;
    const bool real = LOSS && key_pad[k.t] == 0;
    Vec<W> r;
    if (!real && !gu) {
#pragma unroll
      for (int i = 0; i < W; ++i) r.v[i] = 0.0f;
      r.st(dout + e);
      continue;
    }
    const int64_t c = ch[k.t], h = pos[2 * k.t], w = pos[2 * k.t + 1];
    if (bad_index(c, h, w, maxph, maxpw)) {
      atomicOr(err, 1);
#pragma unroll
      for (int i = 0; i < W; ++i) r.v[i] = qnan();
      r.st(dout + e);
      continue;
    }
    const int64_t tab = ((c * maxph + h) * maxpw + w) * PP + k.q * W;
    const Vec<W> bv = Vec<W>::ld(b + tab);
    Vec<W> up;
    if (gu) up = Vec<W>::ld(gu + e);
    if (real) {
      const Vec<W> o = Vec<W>::ld(out + e), a = Vec<W>::ld(tn + e), x = Vec<W>::ld(raw + e),
                   mv = Vec<W>::ld(med + tab);
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const float sd = __fadd_rn(__fmul_rn(bv.v[i], 1.41421353816986083984375f), eps);   // pn_inverse's std
        const float d1 = o.v[i] - a.v[i];
        const float d2 = pn_inverse(o.v[i], mv.v[i], bv.v[i], eps) - x.v[i];
        float gi = k2 * sgn(d2);
        if (gu) gi = up.v[i] + gi;
        r.v[i] = gi * sd + k1 * sgn(d1);
      }
    } else {
#pragma unroll
      for (int i = 0; i < W; ++i)
        r.v[i] = up.v[i] * __fadd_rn(__fmul_rn(bv.v[i], 1.41421353816986083984375f), eps);
    }
    r.st(dout + e);
  }
}

// float4 form: whole float4 pieces per token and every base on a 16-byte boundary
bool vec_ok(int PP, std::initializer_list<const void*> ps) {
  uintptr_t bits = 0;
  for (const void* p : ps) bits |= (uintptr_t)p;
  return PP % 4 == 0 && (bits & 15) == 0;
}

int fwd_blocks(int64_t units, int64_t* upb) {
  // at least one unit per thread; past kMaxBlocks blocks the blocks grow
  int64_t per = std::max<int64_t>(kThreads, (units + kMaxBlocks - 1) / kMaxBlocks);
  per = (per + kThreads - 1) / kThreads * kThreads;
  *upb = per;
  return (int)((units + per - 1) / per);
}

}  // namespace

bool rec_loss_supported(int64_t n_tok, int PP) {
  return n_tok >= 0 && PP >= 1 && PP <= (1 << 20) && n_tok <= ((int64_t)1 << 40) / PP;
}

size_t rec_loss_ws_bytes(int64_t n_tok, int PP) {
  // sized for the scalar form (the larger grid); 16 bytes of doubles + 4 of count per block
  int64_t upb;
  const int nb = fwd_blocks(std::max<int64_t>(1, n_tok * PP), &upb);
  return (size_t)nb * (2 * sizeof(double) + sizeof(int));
}

void launch_rec_loss_fwd(const float* out, const float* tn, const float* raw, const int64_t* ch, const int64_t* pos,
                         const uint8_t* key_pad, int64_t n_tok, int PP, int maxph, int maxpw, const float* med,
                         const float* b, float eps, float* unnorm, void* ws, float* scalars, int* err,
                         hipStream_t st) {
  const bool vec = vec_ok(PP, {out, tn, raw, med, b, unnorm});
  const int64_t units = n_tok * (vec ? PP / 4 : PP);
  int64_t upb = kThreads;
  const int nb = units > 0 ? fwd_blocks(units, &upb) : 0;
  double* part = reinterpret_cast<double*>(ws);   // nb <= the scalar form's grid (rec_loss_ws_bytes)
  int* cnt = reinterpret_cast<int*>(part + 2 * (size_t)nb);
  if (nb > 0) {
    if (vec)
      k_rec_loss_fwd<4><<<nb, kThreads, 0, st>>>(out, tn, raw, ch, pos, key_pad, units, upb, PP, maxph, maxpw, med, b,
                                                 eps, unnorm, part, cnt, err);
    else
      k_rec_loss_fwd<1><<<nb, kThreads, 0, st>>>(out, tn, raw, ch, pos, key_pad, units, upb, PP, maxph, maxpw, med, b,
                                                 eps, unnorm, part, cnt, err);
  }
  k_rec_loss_finish<<<1, kThreads, 0, st>>>(part, cnt, nb, PP, scalars);
}

// out / tn / raw / key_pad / scalars / g NULL: dout = gu std (inverse_norm's backward)
void launch_rec_loss_bwd(const float* out, const float* tn, const float* raw, const int64_t* ch, const int64_t* pos,
                         const uint8_t* key_pad, int64_t n_tok, int PP, int maxph, int maxpw, const float* med,
                         const float* b, float eps, const float* scalars, const float* g, const float* gu,
                         float* dout, int* err, hipStream_t st) {
  if (n_tok <= 0) return;
  const bool loss = out != nullptr;
  const bool vec = vec_ok(PP, {out, tn, raw, med, b, gu, dout});
  const int64_t units = n_tok * (vec ? PP / 4 : PP);
  const int nb = (int)std::min<int64_t>((units + kThreads - 1) / kThreads, 4 * kMaxBlocks);
#define DCTAE_REC_BWD(W, L)                                                                                         \
  k_rec_loss_bwd<W, L><<<nb, kThreads, 0, st>>>(out, tn, raw, ch, pos, key_pad, units, PP, maxph, maxpw, med, b, eps, \
                                                scalars, g, gu, dout, err)
  if (vec) {
    if (loss) DCTAE_REC_BWD(4, true);
    else DCTAE_REC_BWD(4, false);
  } else {
    if (loss) DCTAE_REC_BWD(1, true);
    else DCTAE_REC_BWD(1, false);
  }
#undef DCTAE_REC_BWD
}

}  // namespace dctae
