// k_gemm_h2r / k_gemm_h2c: k_gemm_h2<3, 1> (the encode's row GEMM: A = the
// folded IPT of the three channels, k contiguous; B = the pre-split half DCT
// matrix) and k_gemm_h2<3, 2> (the column GEMM: A = the pre-split half DCT
// matrix of H; B = T per channel, n = kx contiguous, k = y strided by +-Kw)
// with both operands streamed global -> LDS by buffer_load ... lds: no staging
// registers and no store phase.  A two-stage LDS ring of [matrix fp16 2 planes
// x 128 x 32 | fp32 operand 3 x 64 x 32] (40 KB per stage: two blocks per CU),
// the next chunk in flight during the current one's MFMAs, one barrier per
// chunk; the fp32 operand's fragments are scaled and split into the two fp16
// pieces in registers (split_h2; k past K zeroed there).  Products and their
// order are k_gemm_h2's (bit-identical, options gemm_dma / cols_dma).  The
// ablations of k_gemm_h2 put ~0.75 ms of config 4's 2.3 ms row
// GEMM in its register-staged A loads.
// One body serves both; what depends on which operand is the fp32 one -- its
// descriptors, lane offsets, LDS slots and the fragment read -- is a policy
// (OwnRows, OwnCols).  A policy's wave-instruction h of channel c fills the
// 1 KB at (wave + 4 h) * 1024 of the channel's 8 KB.
#include <type_traits>

#include "dctae_launch.h"
#include "dctae_mfma_tile.h"

namespace dctae {

namespace {

template <int SH>
struct DmaShape {
  static constexpr int NC = 3, TM = SH == 2 ? 128 : 64, TN = SH == 1 ? 128 : 64;
  static constexpr int X_PL = 128 * XK * 2;                 // 8 KB per matrix plane
  static constexpr int X_BYTES = 2 * X_PL;                  // 16 KB
  static constexpr int F_CH = 64 * XK * 4;                  // 8 KB per channel of the fp32 operand
  static constexpr int STAGE = X_BYTES + NC * F_CH;         // 40 KB
};

// SH = 1, the fp32 operand is A: 64 rows x 32 k per channel, a row 8 slots of
// 4 floats, slot s of row r at s ^ ((r >> 1) & 7) (the 16 rows of a 16-lane
// ds_read_b128 group then cover the 16 slot positions of the 256-byte bank
// window: with s ^ (r & 7) rows r and r + 8 collided, PMC 37 % of the kernel's
// LDS cycles in bank conflicts).  Channel c's element range is
// [0, (M - 1) sAm + K - 1] (sAk = 1, sAm > 0); wave-instruction h: rows
// 8 (wave + 4 h) + lane / 8, LDS slot lane % 8; rows past M get an offset past
// the range (the load returns 0, no access).
struct OwnRows {
  // (with a template-dependent size this array made the host pass drop the
  // kernel's launch stub without a diagnostic: undefined symbol at load time)
  __amdgpu_buffer_rsrc_t rsrc[3];
  int off[2];
  int row;   // this lane's row in the tile
  __device__ __forceinline__ OwnRows(const GemmProblem& p, int m0, int, int wave, int lane, int own) : row(own) {
    const int64_t ext = (int64_t)(p.M - 1) * p.sAm + p.K;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      rsrc[c] = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A + (int64_t)c * p.sAc), 0, (int)(ext * 4),
                                                  0x00020000);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = 8 * (wave + 4 * h) + (lane >> 3), s8 = (lane & 7) ^ ((r >> 1) & 7);
      off[h] = m0 + r < p.M ? (int)(((int64_t)(m0 + r) * p.sAm + 4 * s8) * 4) : kOob;
    }
  }
  __device__ __forceinline__ int voff(int h, int k0) const { return (int)((uint32_t)off[h] + (uint32_t)k0 * 4u); }
  // k = 8 kq .. 8 kq + 7 of this lane's row
  __device__ __forceinline__ f32x8 frag(const float* ch, int kq, int) const {
    const float* ar = ch + row * XK;
    const f32x4 lo = *reinterpret_cast<const f32x4*>(ar + 4 * ((2 * kq) ^ ((row >> 1) & 7)));
    const f32x4 hi = *reinterpret_cast<const f32x4*>(ar + 4 * ((2 * kq + 1) ^ ((row >> 1) & 7)));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  }
};

// SH = 2, the fp32 operand is B = T: 32 k-rows x 64 columns per channel, four
// rows per 1 KB wave-instruction.  The MFMA fragment (8 consecutive k of one
// column) is 8 ds_read_b32 down a column; the 16-byte column groups of rows
// with (k >> 3) odd are swapped by 8 slots, so the two half-waves (k groups 8
// apart) read disjoint banks.  Channel c's element range is [lo, hi] (sBn = 1,
// sBk = +-Kw) plus 64 floats, so a 16-byte piece straddling its end is read
// whole (it stays inside the workspace's padded regions); wave-instruction h:
// rows 4 (wave + 4 h) + lane / 16, LDS slot lane % 16 = column group
// (lane % 16) ^ (8 ((row >> 3) & 1)).
struct OwnCols {
  __amdgpu_buffer_rsrc_t rsrc[3];
  int off[2];
  int step;   // bytes per k row (negative for the odd parity's descending rows)
  int col;    // this lane's column in the tile
  __device__ __forceinline__ OwnCols(const GemmProblem& p, int, int n0, int wave, int lane, int own) : col(own) {
    const int64_t lo = p.sBk < 0 ? (int64_t)(p.K - 1) * p.sBk : 0;
    const int64_t hi = (int64_t)(p.N - 1) + (p.sBk > 0 ? (int64_t)(p.K - 1) * p.sBk : 0);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      rsrc[c] = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.B + (int64_t)c * p.sBc + lo), 0,
                                                  (int)((hi - lo + 1 + 64) * 4), 0x00020000);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = 4 * (wave + 4 * h) + (lane >> 4), q = (lane & 15) ^ (8 * ((r >> 3) & 1));
      off[h] = (int)(((int64_t)r * p.sBk + n0 + 4 * q - lo) * 4);
    }
    step = (int)(p.sBk * 4);
  }
  __device__ __forceinline__ int voff(int h, int k0) const { return off[h] + k0 * step; }
  // k = 8 kq .. 8 kq + 7 of this lane's column (kq = 2 ks + half: rows 8 kq + e have (k >> 3) & 1 = half)
  __device__ __forceinline__ f32x8 frag(const float* ch, int kq, int half) const {
    const float* bc = ch + (8 * kq) * 64 + 4 * ((col >> 2) ^ (8 * half)) + (col & 3);
    f32x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = bc[e * 64];
    return v;
  }
};

template <int SH>
__device__ __forceinline__ void gemm_h2_dma_body(const GemmProblem* __restrict__ probs,
                                                 const TileRef* __restrict__ tiles) {
  using S = DmaShape<SH>;
  using Own = typename std::conditional<SH == 1, OwnRows, OwnCols>::type;
  constexpr int NC = S::NC, STAGE = S::STAGE;
  __shared__ __attribute__((aligned(16))) uint8_t ring[2 * STAGE];
  const TileRef tr = tiles[blockIdx.x];
  if (tr.problem < 0) return;   // padding of an XCD-dealt list
  const GemmProblem p = probs[tr.problem];
  const int tm = tr.tile / p.tiles_n, tn = tr.tile % p.tiles_n;
  const int m0 = tm * S::TM, n0 = tn * S::TN;
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l32 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int wx = SH == 1 ? wn : wm, wo = SH == 1 ? wm : wn;   // this wave's 64 matrix rows, its 32 of the fp32 operand
  // the fp32 operand scaled by 2^ea (|max| < 2^14), the output unscaled (gemm_x3_body)
  const int ea = h2_operand_exp(*p.amax);
  const float unscale = ldexpf(1.0f, -(ea + p.xh_exp));
  const auto xrsrc = xh_rsrc(p);
  const int xoff[2] = {xh_lane_off(p, SH == 1 ? n0 : m0, wave), xh_lane_off(p, SH == 1 ? n0 : m0, wave + 4)};
  const int xsp2 = (int)(p.xs_plane * 2);
  const Own own(p, m0, n0, wave, lane, wo * 32 + l32);
  auto dma = [&](int st, int k0) {
    uint8_t* base = ring + st * STAGE;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int pl = j >> 1, h = j & 1;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, (lds_void_t*)(base + pl * S::X_PL + (wave + 4 * h) * 1024), 16,
                                               xoff[h] + k0 * 2 + pl * xsp2, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 2 * NC; ++j) {
      const int c = j >> 1, h = j & 1;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(own.rsrc[c],
                                               (lds_void_t*)(base + S::X_BYTES + c * S::F_CH + (wave + 4 * h) * 1024), 16,
                                               own.voff(h, k0), 0, 0, 0);
    }
  };
  constexpr int BM = S::TM / 64, BN = S::TN / 64;   // 32 x 32 blocks per wave: 1 x 2 or 2 x 1
  floatx16 acc[NC][BM][BN];
  zero_acc(&acc[0][0][0], NC * 2);
  auto compute = [&](int st, int k0) {
    const uint8_t* base = ring + st * STAGE;
    const uint16_t* Xp = reinterpret_cast<const uint16_t*>(base);
    const float* Ff = reinterpret_cast<const float*>(base + S::X_BYTES);
#pragma unroll
    for (int ks = 0; ks < XK / 16; ++ks) {
      const int kq = 2 * ks + half;
      bf16x8 x[2][2];
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
          x[b][pl] = *reinterpret_cast<const bf16x8*>(Xp + pl * (S::X_PL / 2) + lds_off(wx * 64 + 32 * b + l32, kq));
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        bf16x8 f[2];
        split_h2(own.frag(Ff + c * (S::F_CH / 4), kq, half), ea, k0 + 8 * kq, p.K, k0 + XK > p.K, f);
#pragma unroll
        for (int b = 0; b < 2; ++b) {   // the products in k_gemm_h2's order: (A, B)
          if constexpr (SH == 1) mfma_pieces(acc[c][0][b], f, x[b]);
          else mfma_pieces(acc[c][b][0], x[b], f);
        }
      }
    }
  };
  // chunk i lands in stage i % 2.  At the top of iteration i this wave's
  // chunk-i loads are done; the barrier makes that every wave's and frees
  // stage (i + 1) % 2 (chunk i - 1's MFMAs done) for chunk i + 1
  const int nk = (p.K + XK - 1) / XK;
  dma(0, 0);
  for (int i = 0; i < nk; ++i) {
    wait_vm<0>();
    __syncthreads();
    if (i + 1 < nk) dma((i + 1) & 1, (i + 1) * XK);
    compute(i & 1, i * XK);
  }
  scale_acc(&acc[0][0][0], NC * 2, unscale);
  if (p.omax) {
    __syncthreads();   // every wave past its last LDS read: the partials alias the ring
    block_absmax(p, absmax_acc(&acc[0][0][0], NC * 2), reinterpret_cast<uint32_t*>(ring));
  }
  const int64_t ext = out_extent(p);
  const int gm = m0 + wm * (S::TM / 2) + 4 * half, gn = n0 + wn * (S::TN / 2) + l32;
  if (out_row_major(p, ext)) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int i = 0; i < BM; ++i)
#pragma unroll
        for (int j = 0; j < BN; ++j) store_acc_32x32<true>(p, ext, c, gm + 32 * i, gn + 32 * j, acc[c][i][j]);
    return;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int i = 0; i < BM; ++i)
#pragma unroll
      for (int j = 0; j < BN; ++j) store_acc_32x32<false>(p, ext, c, gm + 32 * i, gn + 32 * j, acc[c][i][j]);
}

}  // namespace

__global__ __launch_bounds__(256, 2) void k_gemm_h2r(const GemmProblem* __restrict__ probs,
                                                    const TileRef* __restrict__ tiles) {
  gemm_h2_dma_body<1>(probs, tiles);
}

__global__ __launch_bounds__(256, 2) void k_gemm_h2c(const GemmProblem* __restrict__ probs,
                                                    const TileRef* __restrict__ tiles) {
  gemm_h2_dma_body<2>(probs, tiles);
}

void launch_gemm_h2_dma(const GemmProblem* probs, const TileRef* tiles, int n_tiles, hipStream_t s, int share) {
  if (share == 1)
    hipLaunchKernelGGL(k_gemm_h2r, dim3(n_tiles), dim3(256), 0, s, probs, tiles);
  else
    hipLaunchKernelGGL(k_gemm_h2c, dim3(n_tiles), dim3(256), 0, s, probs, tiles);
}

}  // namespace dctae
