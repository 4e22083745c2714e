// Fused optimizer step: gradient-norm clip, AdamW and the bf16
// weight packs of k_linear in one pass over a device-resident segment table
// (dctae_optim_seg, include/dctae.h), one entry per parameter tensor.
//
//   k_gradnorm_partial  one block per OPT_NORM_CHUNK gradient elements of one
//                       segment: squares (exact in fp64) summed in fp64, each
//                       thread over a fixed set of elements, then a fixed
//                       shuffle / LDS tree; one partial per block
//   k_gradnorm_final    one block: every thread sums a contiguous run of the
//                       partials in index order, then the same tree; writes
//                       the norm and torch's clip_grad_norm_ coefficient
//   k_adamw_pack        persistent blocks stride over the work items of the
//                       table.  Flat segment: OPT_FLAT_CHUNK elements, 16-byte
//                       loads / stores where the segment's pointers allow
//                       (the gradient's alignment is checked on its own: it
//                       may be a view).  Packed segment: a 64 x 64 tile of a
//                       2-D weight: p / m / v updated in fp32, the rounded
//                       bf16 tile stored row-major into w_dst and, through a
//                       transposed LDS tile, in 16-byte rows into wt_dst.
//                       Elements outside the tensor are never written, so the
//                       packs' zero padding stays zero.
//
// Arithmetic per element (torch.optim.AdamW, single-tensor path; fp32, every
// operation rounded on its own: the unit is built with -ffp-contract=off):
//   g' = g * coef;  p = p * decay;  m = lerp(m, g', w1);
//   v = v * beta2 + (w2 * g') * g';  p = p - (step_size * m) / (sqrt(v) / bc2_sqrt + eps)
// No floating-point atomics anywhere: a step repeats bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dctae_model.h"

namespace dctae {

namespace {

typedef dctae_optim_seg Seg;
typedef dctae_optim_group Group;

struct GroupsArg {
  Group g[DCTAE_OPTIM_MAX_GROUPS];
};

__device__ __forceinline__ uint16_t f2bf(float f) {   // round to nearest even, as Tensor.to(torch.bfloat16)
  const __bf16 h = (__bf16)f;
  return __builtin_bit_cast(uint16_t, h);
}

__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the segment that owns item idx of a prefix (norm0 or work0): the last one whose first item is <= idx
template <bool NORM>
__device__ __forceinline__ int find_seg(const Seg* segs, int count, int64_t idx) {
  int lo = 0, hi = count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    const int64_t first = NORM ? segs[mid].norm0 : segs[mid].work0;
    if (first <= idx) lo = mid; else hi = mid;
  }
  return lo;
}

// sum of acc over the block's 256 threads in a fixed order; valid in thread 0
__device__ __forceinline__ double block_sum(double acc, double* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ double sq(float x) {
  const double d = (double)x;
  return d * d;
}

__global__ __launch_bounds__(256) void k_gradnorm_partial(const Seg* __restrict__ segs, int count,
                                                          double* __restrict__ partial) {
  __shared__ double red[4];
  const int64_t b = blockIdx.x;
  const Seg& sg = segs[find_seg<true>(segs, count, b)];
  const int64_t n = sg.rows * sg.cols;
  const int64_t start = (b - sg.norm0) * OPT_NORM_CHUNK;
  const int64_t len = min(n - start, OPT_NORM_CHUNK);
  const float* g = sg.g + start;
  const bool vec = al16(g);
  double acc = 0.0;
#pragma unroll 4
  for (int k = 0; k < (int)(OPT_NORM_CHUNK / 1024); ++k) {
    const int64_t i = ((int64_t)k * 256 + threadIdx.x) * 4;
    if (i + 3 < len) {
      float4 v;
      if (vec) v = *reinterpret_cast<const float4*>(g + i);
      else v = make_float4(g[i], g[i + 1], g[i + 2], g[i + 3]);
      acc += sq(v.x);
      acc += sq(v.y);
      acc += sq(v.z);
      acc += sq(v.w);
    } else {
      for (int j = 0; j < 4; ++j)
        if (i + j < len) acc += sq(g[i + j]);
    }
  }
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) partial[b] = tot;
}

__global__ __launch_bounds__(256) void k_gradnorm_final(const double* __restrict__ partial, int64_t n, float max_norm,
                                                        float* __restrict__ stats) {
  __shared__ double red[4];
  const int64_t per = (n + 255) / 256;
  const int64_t lo = min(n, per * threadIdx.x), hi = min(n, lo + per);
  double acc = 0.0;
  for (int64_t i = lo; i < hi; ++i) acc += partial[i];
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(tot);
    const float c = max_norm / (norm + 1e-6f);
    stats[0] = norm;
    stats[1] = c > 1.f ? 1.f : c;   // a NaN stays a NaN, as torch.clamp(max=1)
  }
}

__device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, const Group& h, float coef) {
  g = g * coef;
  p = p * h.decay;
  const float d = g - m;
  m = h.w1 < 0.5f ? m + h.w1 * d : g - d * (1.f - h.w1);   // torch's lerp
  v = v * h.beta2 + (h.w2 * g) * g;
  const float denom = __fdiv_rn(__fsqrt_rn(v), h.bc2_sqrt) + h.eps;
  p = p - __fdiv_rn(h.step_size * m, denom);
}

__device__ __forceinline__ void adamw4(float4& p, const float4& g, float4& m, float4& v, const Group& h, float coef) {
  adamw1(p.x, g.x, m.x, v.x, h, coef);
  adamw1(p.y, g.y, m.y, v.y, h, coef);
  adamw1(p.z, g.z, m.z, v.z, h, coef);
  adamw1(p.w, g.w, m.w, v.w, h, coef);
}

__device__ __forceinline__ float4 load_g4(const float* g, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(g);
  return make_float4(g[0], g[1], g[2], g[3]);
}

// OPT_FLAT_CHUNK elements of a flat segment starting at element `start`
__device__ __forceinline__ void flat_item(const Seg& sg, const Group& h, float coef, int64_t start) {
  const int64_t n = sg.rows * sg.cols;
  const int64_t len = min(n - start, OPT_FLAT_CHUNK);
  float* p = sg.p + start;
  float* m = sg.exp_avg + start;
  float* v = sg.exp_avg_sq + start;
  const float* g = sg.g + start;
  float* cp = sg.copy_dst ? sg.copy_dst + start : nullptr;
  const bool vec = al16(p) && al16(m) && al16(v) && (!cp || al16(cp));
  const bool gvec = al16(g);
#pragma unroll
  for (int k = 0; k < (int)(OPT_FLAT_CHUNK / 1024); ++k) {
    const int64_t i = ((int64_t)k * 256 + threadIdx.x) * 4;
    if (vec && i + 3 < len) {
      float4 p4 = *reinterpret_cast<const float4*>(p + i);
      float4 m4 = *reinterpret_cast<const float4*>(m + i);
      float4 v4 = *reinterpret_cast<const float4*>(v + i);
      const float4 g4 = load_g4(g + i, gvec);
      adamw4(p4, g4, m4, v4, h, coef);
      *reinterpret_cast<float4*>(p + i) = p4;
      *reinterpret_cast<float4*>(m + i) = m4;
      *reinterpret_cast<float4*>(v + i) = v4;
      if (cp) *reinterpret_cast<float4*>(cp + i) = p4;
    } else {
      for (int j = 0; j < 4; ++j) {
        const int64_t e = i + j;
        if (e < len) {
          float pe = p[e], me = m[e], ve = v[e];
          adamw1(pe, g[e], me, ve, h, coef);
          p[e] = pe;
          m[e] = me;
          v[e] = ve;
          if (cp) cp[e] = pe;
        }
      }
    }
  }
}

constexpr int TSTR = OPT_TILE + 2;   // halfwords per row of the transposed LDS tile: 33 dwords, an odd bank stride

// tile `t` (row-major over the segment's tile grid) of a packed segment
__device__ __forceinline__ void tile_item(const Seg& sg, const Group& h, float coef, int64_t t,
                                          uint16_t (*T)[TSTR]) {
  const int64_t rows = sg.rows, cols = sg.cols;
  const int64_t tcn = (cols + OPT_TILE - 1) / OPT_TILE;
  const int64_t r_base = (t / tcn) * OPT_TILE, c_base = (t % tcn) * OPT_TILE;
  const bool vec = (cols & 3) == 0 && al16(sg.p) && al16(sg.exp_avg) && al16(sg.exp_avg_sq);
  const bool gvec = (cols & 3) == 0 && al16(sg.g);
  const bool wvec = sg.w_dst && (sg.ldw & 3) == 0 && ((uintptr_t)sg.w_dst & 7) == 0;
  const int c4 = (threadIdx.x & 15) * 4, rr = threadIdx.x >> 4;
  const int64_t C = c_base + c4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = rr + 16 * k;
    const int64_t R = r_base + r;
    if (R >= rows || C >= cols) continue;
    const int64_t idx = R * cols + C;
    uint16_t bf[4];
    int nv;   // valid elements of this thread's four
    if (vec && C + 3 < cols) {
      float4 p4 = *reinterpret_cast<const float4*>(sg.p + idx);
      float4 m4 = *reinterpret_cast<const float4*>(sg.exp_avg + idx);
      float4 v4 = *reinterpret_cast<const float4*>(sg.exp_avg_sq + idx);
      const float4 g4 = load_g4(sg.g + idx, gvec);
      adamw4(p4, g4, m4, v4, h, coef);
      *reinterpret_cast<float4*>(sg.p + idx) = p4;
      *reinterpret_cast<float4*>(sg.exp_avg + idx) = m4;
      *reinterpret_cast<float4*>(sg.exp_avg_sq + idx) = v4;
      bf[0] = f2bf(p4.x); bf[1] = f2bf(p4.y); bf[2] = f2bf(p4.z); bf[3] = f2bf(p4.w);
      nv = 4;
    } else {
      nv = (int)min((int64_t)4, cols - C);
      for (int j = 0; j < 4; ++j) {
        bf[j] = 0;
        if (j < nv) {
          float pe = sg.p[idx + j], me = sg.exp_avg[idx + j], ve = sg.exp_avg_sq[idx + j];
          adamw1(pe, sg.g[idx + j], me, ve, h, coef);
          sg.p[idx + j] = pe;
          sg.exp_avg[idx + j] = me;
          sg.exp_avg_sq[idx + j] = ve;
          bf[j] = f2bf(pe);
        }
      }
    }
    if (sg.w_dst) {
      uint16_t* dst = sg.w_dst + (sg.w_row_off + R) * sg.ldw + C;
      if (wvec && nv == 4) {
        uint2 pk;
        pk.x = (uint32_t)bf[0] | ((uint32_t)bf[1] << 16);
        pk.y = (uint32_t)bf[2] | ((uint32_t)bf[3] << 16);
        *reinterpret_cast<uint2*>(dst) = pk;
      } else {
        for (int j = 0; j < nv; ++j) dst[j] = bf[j];
      }
    }
    if (sg.wt_dst) {
#pragma unroll
      for (int j = 0; j < 4; ++j) T[c4 + j][r] = bf[j];
    }
  }
  if (!sg.wt_dst) return;   // uniform over the block
  __syncthreads();
  const bool tvec = (sg.ldwt & 7) == 0 && (sg.wt_col_off & 7) == 0 && al16(sg.wt_dst);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int q = threadIdx.x + 256 * k;
    const int c = q >> 3, r0 = (q & 7) * 8;
    const int64_t Cq = c_base + c, R0 = r_base + r0;
    if (Cq >= cols || R0 >= rows) continue;
    uint16_t* dst = sg.wt_dst + Cq * sg.ldwt + sg.wt_col_off + R0;
    if (tvec && R0 + 8 <= rows) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(&T[c][r0]);
      *reinterpret_cast<uint4*>(dst) = make_uint4(src[0], src[1], src[2], src[3]);
    } else {
      const int nr = (int)min((int64_t)8, rows - R0);
      for (int j = 0; j < nr; ++j) dst[j] = T[c][r0 + j];
    }
  }
  __syncthreads();   // T is free for the block's next tile
}

__global__ __launch_bounds__(256) void k_adamw_pack(const Seg* __restrict__ segs, int count, int64_t n_work,
                                                    GroupsArg hp, const float* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) uint16_t T[OPT_TILE][TSTR];
  const float coef = stats ? stats[1] : 1.f;
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const Seg sg = segs[find_seg<false>(segs, count, w)];
    const Group h = hp.g[sg.group];
    const int64_t item = w - sg.work0;
    if (sg.w_dst || sg.wt_dst) tile_item(sg, h, coef, item, T);
    else flat_item(sg, h, coef, item * OPT_FLAT_CHUNK);
  }
}

}  // namespace

void launch_gradnorm(const dctae_optim_seg* segs, int count, int64_t n_blocks, float max_norm, double* ws, float* stats,
                     hipStream_t s) {
  if (n_blocks > 0)
    hipLaunchKernelGGL(k_gradnorm_partial, dim3((unsigned)n_blocks), dim3(256), 0, s, segs, count, ws);
  hipLaunchKernelGGL(k_gradnorm_final, dim3(1), dim3(256), 0, s, ws, n_blocks, max_norm, stats);
}

void launch_adamw_pack(const dctae_optim_seg* segs, int count, int64_t n_work, const dctae_optim_group* groups,
                       int n_groups, const float* stats, hipStream_t s) {
  if (n_work <= 0) return;
  GroupsArg hp{};
  for (int i = 0; i < n_groups; ++i) hp.g[i] = groups[i];
  const unsigned grid = (unsigned)std::min<int64_t>(n_work, 2048);
  hipLaunchKernelGGL(k_adamw_pack, dim3(grid), dim3(256), 0, s, segs, count, n_work, hp, stats);
}

}  // namespace dctae
