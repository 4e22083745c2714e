// What the split-operand MFMA GEMM units (dctae_gemm_x3.hip, dctae_gemm_dma.hip,
// dctae_rows_fused.hip) share, each rule stated once: the k chunk and the LDS
// swizzle, the fp16 operand exponents, the piece fragments and their products,
// the in-register two-piece split, the |max| reduction, the 32 x 32 C/D-map
// epilogue and the lane layout of the pre-split matrix planes for LDS DMA.
// The first part is plain C++17 that a host compiler builds
// alone (tests/test_mfma_tile_host.py does); the rest is device code.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define DCTAE_HD __host__ __device__ __attribute__((always_inline))
#else
#define DCTAE_HD
#endif

namespace dctae {

constexpr int XK = 32;        // k chunk

// LDS image of one operand tile: three bf16 pieces of ROWS x 32 k, rows of
// 64 bytes, the 16-byte k group kq of row r at slot kq ^ swz(r).  With this
// swizzle the 16-lane groups of a ds_read_b128 fragment read, the 8-lane
// groups of the staging ds_write_b128 (two rows x four k groups, or eight rows
// x one k group) all hit distinct banks (exhaustive check over the lane
// groups of MI355X_MICROARCH.md §LDS).
DCTAE_HD inline int swz(int r) { return ((r >> 1) ^ (r >> 2)) & 3; }
DCTAE_HD inline int lds_off(int r, int kq) { return r * XK + 8 * (kq ^ swz(r)); }

// The fp16 operand exponents, from the bits of an operand's |max| (uint order:
// NaN above Inf above finite).  The matrix side (split_matrix_h2, k_split_w_h2):
// max in [2^(e-1), 2^e) scaled by 2^(14 - e) lies in [2^13, 2^14), fp16 range
// with headroom; a zero or non-finite max leaves the operand unscaled.
DCTAE_HD inline int h2_matrix_exp(uint32_t max_bits) {
  int e = 0;
  if (max_bits != 0u && max_bits < 0x7f800000u) {
    float mx;
    __builtin_memcpy(&mx, &max_bits, 4);
    frexpf(mx, &e);   // max in [2^(e-1), 2^e)
    e = 14 - e;
  }
  return e;
}
// The per-channel operand of k_gemm_h2 and its kin: the same, clamped so that
// 2^ea and the output's 2^-(ea + xh_exp) stay exact powers of two in fp32
DCTAE_HD inline int h2_operand_exp(uint32_t max_bits) {
  const int e = h2_matrix_exp(max_bits);
  return e < -100 ? -100 : e > 100 ? 100 : e;
}

}  // namespace dctae

#if defined(__HIPCC__)
#include "dctae_device.h"

namespace dctae {

constexpr int kOob = 0x7ffffff0;   // a lane offset past every buffer range: the load returns 0, the store is dropped

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bfv8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 hv8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void_t;

template <int ROWS, int NP = 3>
struct Pieces {
  uint16_t p[NP][ROWS * XK];
};

template <int ROWS, int NP>
__device__ __forceinline__ void read_frag(bf16x8 (&f)[NP], const Pieces<ROWS, NP>& L, int r, int kq) {
  const int o = lds_off(r, kq);
#pragma unroll
  for (int q = 0; q < NP; ++q) f[q] = *reinterpret_cast<const bf16x8*>(&L.p[q][o]);
}

// k_gemm_h2: the three fp16 products of piece order <= 1, small terms first
__device__ __forceinline__ void mfma_pieces(floatx16& acc, const bf16x8 (&a)[2], const bf16x8 (&b)[2]) {
  const hv8 a0 = __builtin_bit_cast(hv8, a[0]), a1 = __builtin_bit_cast(hv8, a[1]);
  const hv8 b0 = __builtin_bit_cast(hv8, b[0]), b1 = __builtin_bit_cast(hv8, b[1]);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc, 0, 0, 0);
}

// six split products, small terms first
__device__ __forceinline__ void mfma_pieces(floatx16& acc, const bf16x8 (&a)[3], const bf16x8 (&b)[3]) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
}

// The two-piece fp16 split of k_gemm_h2, on one 8-deep fragment in registers:
// v (this lane's k = kb .. kb + 7; k past K zeroed in the last chunk, `last`
// uniform) scaled by the exact 2^ea (h2_operand_exp: |max| < 2^14), then
// out[0] = fp16(vs), out[1] = fp16(vs - out[0]).  v_ldexp_f32: exact as the
// multiply, and beside MFMAs a packed f32 multiply costs ~5x its issue slot
// (MI355X_MICROARCH.md).  split_store<ROWS, 2> (dctae_gemm_x3.hip) and fold of
// k_rows_fused are other instruction forms of the same arithmetic.
__device__ __forceinline__ void split_h2(f32x8 v, int ea, int kb, int K, bool last, bf16x8 (&out)[2]) {
  if (last) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = kb + e < K ? v[e] : 0.0f;
  }
  f32x8 vs;
#pragma unroll
  for (int e = 0; e < 8; ++e) vs[e] = ldexpf(v[e], ea);
  const hv8 h0 = __builtin_convertvector(vs, hv8);
  // the residual vs - h0 (exact) as one mixed-precision FMA per value
  // (written out: the compiler forms cvt + sub, then packs the subs)
  const u32x4 hw = __builtin_bit_cast(u32x4, h0);
  f32x8 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r[2 * e]) : "v"(hw[e]), "v"(vs[2 * e]));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r[2 * e + 1]) : "v"(hw[e]), "v"(vs[2 * e + 1]));
  }
  out[0] = __builtin_bit_cast(bf16x8, h0);
  out[1] = __builtin_bit_cast(bf16x8, __builtin_convertvector(r, hv8));
}

// the n 32 x 32 accumulators of a wave
__device__ __forceinline__ void zero_acc(floatx16* acc, int n) {
#pragma unroll
  for (int b = 0; b < n; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.0f;
}

// k_gemm_h2: the outputs unscaled by the exact 2^-(ea + xh_exp), one multiply per
// value, before their |max| is taken and before they are stored
__device__ __forceinline__ void scale_acc(floatx16* acc, int n, float unscale) {
#pragma unroll
  for (int b = 0; b < n; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] *= unscale;
}
// |max| in uint order (padded rows / columns accumulate zeros: no mask needed)
__device__ __forceinline__ uint32_t absmax_acc(const floatx16* acc, int n) {
  uint32_t mx = 0;
#pragma unroll
  for (int b = 0; b < n; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = max(mx, __float_as_uint(acc[b][r]) & 0x7fffffffu);
  return mx;
}

// The |max| of a 256-thread block into p.omax (T's |max| for the column GEMM):
// one atomic per block; part: 4 words of LDS nobody else uses from here on
__device__ __forceinline__ void block_absmax(const GemmProblem& p, uint32_t mx, uint32_t* part) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(p.omax, max(max(part[0], part[1]), max(part[2], part[3])));
}

// The epilogue.  Row-major outputs (a row's extent within the row stride) go
// through buffer stores on the channel's output range [0, ext): one 32-bit
// lane offset per 32 x 32 block plus a uniform row step; rows past M land past
// the range and columns past N get the offset kOob, so no per-store predicate
// or 64-bit address math.  Other outputs take predicated plain stores.
__device__ __forceinline__ int64_t out_extent(const GemmProblem& p) {   // elements of one channel's output
  return (int64_t)(p.M - 1) * p.sOm + (int64_t)(p.N - 1) * p.sOn + 1;
}
// row-major, and every offset of a tile (rows past M included) below kOob
__device__ __forceinline__ bool out_row_major(const GemmProblem& p, int64_t ext) {
  return p.sOm > 0 && p.sOn > 0 && p.sOm >= (int64_t)(p.N - 1) * p.sOn + 1 && (ext + 160 * p.sOm) * 4 < kOob;
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t out_rsrc(const GemmProblem& p, int64_t ext, int c) {
  return __builtin_amdgcn_make_buffer_rsrc(p.O + (int64_t)c * p.sOc, 0, (int)(ext * 4), 0x00020000);
}
// One 32 x 32 block of channel c: this lane's 16 values at column gn and rows
// gm + (r & 3) + 8 (r >> 2) (C/D map: col = lane & 31, row = (r & 3) +
// 8 (r >> 2) + 4 (lane >> 5); the caller adds 4 (lane >> 5) to gm and lane & 31
// to gn).  ROWS: the buffer-store path (out_row_major holds), else the
// predicated fallback; a kernel tests out_row_major once and runs its blocks
// through one form.
template <bool ROWS>
__device__ __forceinline__ void store_acc_32x32(const GemmProblem& p, int64_t ext, int c, int gm, int gn,
                                                const floatx16& acc) {
  if constexpr (ROWS) {
    const int sOm4 = (int)(p.sOm * 4);
    const auto rsrc = out_rsrc(p, ext, c);
    const int vo = gn < p.N ? gm * sOm4 + (int)(gn * p.sOn * 4) : kOob;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[r]), rsrc, vo + ((r & 3) + 8 * (r >> 2)) * sOm4, 0, 0);
  } else {
    float* O = p.O + (int64_t)c * p.sOc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = gm + (r & 3) + 8 * (r >> 2);
      if (m < p.M && gn < p.N) O[(int64_t)m * p.sOm + (int64_t)gn * p.sOn] = acc[r];
    }
  }
}

// The pre-split fp16 matrix planes (GemmProblem::Xh: 2 planes, padded to Rp rows
// of xs_ld k, so every load of a tile is in range) as LDS DMA streams them:
// one wave-instruction moves 16 rows x 64 bytes (1 KB) of one plane -- row
// group rg = rows 16 rg + lane / 4 from matrix row r0, LDS slot lane % 4 = k
// quad (lane % 4) ^ swz(row), the layout lds_off reads.  A chunk's offset adds
// k0 * 2 bytes and the plane's xs_plane * 2.
__device__ __forceinline__ int xh_bytes(const GemmProblem& p) { return (int)(2 * p.xs_plane * 2); }
__device__ __forceinline__ __amdgpu_buffer_rsrc_t xh_rsrc(const GemmProblem& p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(p.Xh), 0, xh_bytes(p), 0x00020000);
}
__device__ __forceinline__ int xh_lane_off(const GemmProblem& p, int r0, int rg) {
  const int lane = threadIdx.x & 63;
  const int row = 16 * rg + (lane >> 2), kq = (lane & 3) ^ swz(row);
  return ((r0 + row) * p.xs_ld + 8 * kq) * 2;
}

// Workgroup barrier for LDS hand-offs only: this wave's LDS writes done, then
// s_barrier.  __syncthreads() is a release fence as well, which on gfx9
// (loads and stores share vmcnt) waits for EVERY outstanding vector memory
// operation -- the prefetched loads in flight included -- so with it no load
// or LDS-DMA chunk could stay in flight across a chunk's barriers.  Users wait
// for their own LDS-DMA chunks (wait_vm) before it.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// s_waitcnt vmcnt(n) (gfx9 encoding: vmcnt in bits 3:0 and 15:14, expcnt and lgkmcnt left at their maxima)
template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt");
  __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}

}  // namespace dctae
#endif
