// k_rows_fused: colour transform, (x, y) folds and row GEMM of both parities
// in one pass, for the images whose rows and columns both run on the GEMM DCT
// (ImgDesc::tperm; reference util.py:70-82 then util.py:333).  The separate
// path writes the folded IPT (k_rgb_to_ipt, 3.4 GB on config 4) and reads it
// back in the row GEMM.  Here a block owns 16 row pairs (y, H-1-y) -- 32
// folded rows: 16 sums, 16 differences -- and every output column of both
// parities (N <= 256 each: Kw <= 512).  Per 32-deep k chunk each of its 512
// threads loads the 4 pixels (y, k), (y, W-1-k), (H-1-y, k), (H-1-y, W-1-k),
// computes their IPT and the folds of both parities in registers
// (k_rgb_to_ipt's arithmetic, value for value: every pixel is transformed
// once), and writes the fp16 pieces to LDS; waves 0-3 run the even-kx
// columns against the even half DCT matrix, waves 4-7 the odd ones (64
// columns of 32 rows and 3 channels each, 96 accumulator VGPRs).  The
// matrices stream through a two-stage LDS ring (LDS DMA), the pixels two
// chunks ahead in registers.
// Scale: the image's |max| (k_gemm_h2's operand scale) is unknown before the
// transform, so the first pass splits at a fixed 2^kFusedSE and records
// the |max| of the folded values; an image with a value outside the safe fp16
// range (|v| 2^SE >= 2^15, or not finite) is flagged, and the fix-up launch
// (fix = 1, flagged images only, grid-stride) redoes it at the scale k_gemm_h2
// derives from that |max| -- the old path's arithmetic for those images.
// The form that interleaved chunk i + 1's colour transform with chunk i's
// MFMAs encoded the config-4 batch non-deterministically and was removed.
#include <algorithm>

#include "dctae_launch.h"
#include "dctae_mfma_tile.h"

namespace dctae {

namespace {

// One 16-byte-per-lane buffer_load ... lds (lane i -> lds + 16 i), written
// out so the compiler does not see an LDS DMA in flight: it otherwise waits
// for every outstanding vector load (vmcnt(0)) before the next LDS read it
// cannot prove disjoint, prefetched register loads included.  The caller
// waits for the chunk (wait_vm) before its barrier.  rsrc: the raw buffer
// descriptor words (base, num_records, 0x00020000).
// The s_nop: nothing inside an asm string gets the wait states hipcc adds to
// its own instructions (cdna_hip_programming.md, "What hipcc does not do" 2):
// an LDS DMA needs one after the s_mov to M0, and a descriptor or soffset SGPR
// written by VALU (readfirstlane) needs five before a buffer instruction reads
// it.  Without them a piece could land at the previous M0 -- seen as rare
// run-to-run differences of a few tokens on the config-4 batch.
__device__ __forceinline__ void dma_lds16(u32x4 rsrc, const void* lds, int voff) {
  const uint32_t m0 = (uint32_t)(uintptr_t)lds;
  asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voff), "s"(rsrc), "{m0}"(m0) : "memory");
}
__device__ __forceinline__ u32x4 rsrc_words(const void* base, uint32_t bytes) {
  const uint64_t a = (uint64_t)(uintptr_t)base;
  u32x4 r;
  r[0] = (uint32_t)a;
  r[1] = (uint32_t)(a >> 32) & 0xffffu;   // stride 0
  r[2] = bytes;
  r[3] = 0x00020000u;
  return r;
}

}  // namespace

constexpr int kFusedSE = 11;       // the first pass's operand scale 2^kFusedSE
constexpr int kFusedPairs = 16;    // row pairs per block
constexpr int kFusedTN = 256;      // output columns per parity

// PxT: the caller's pixels, float or uint8_t (dctae_pixel.h): one buffer load
// per pixel either way (a dword or a byte, the descriptor's range in bytes)
template <typename PxT>
__global__ __launch_bounds__(512, 1) void k_rows_fused(const GemmProblem* __restrict__ probs,
                                                      const TileRef* __restrict__ tiles, int n_tiles,
                                                      const ImgDesc* __restrict__ imgs, const PxT* __restrict__ rgb,
                                                      ColorMats cm, uint32_t* __restrict__ amax, int* __restrict__ flags,
                                                      int n_img, int fix) {
  constexpr int TN = kFusedTN, NPR = kFusedPairs;
  constexpr int B_PL = TN * XK * 2;          // 16 KB: one plane of one parity's matrix chunk
  constexpr int B_ST = 4 * B_PL;             // 64 KB: 2 parities x 2 planes
  constexpr int A_CQ = 2 * NPR * XK;         // halves per (parity, channel, piece): 32 rows x 32 k
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * B_ST + 12 * A_CQ * 2];   // 152 KB
  uint16_t* As = reinterpret_cast<uint16_t*>(lds + 2 * B_ST);
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l32 = lane & 31;
  // the wave index as a uniform value: the parity's matrix descriptor and the
  // column-range tests stay scalar (from tid they were per-lane: a waterfall
  // loop around every matrix load and a divergent branch around every MFMA)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pw = wave >> 2, wc = wave & 3;   // this wave's parity and 64-column slice
  const float gam = 0.430000007152557373046875f;
  if (fix && flags[n_img] == 0) return;      // fix-up: no image of the job flagged
  // The first pass: a persistent grid taking tiles from
  // per-XCD counters (flags[n_img + 1 + x]): block b runs on XCD b % 8 and
  // takes the dealt list's positions x + 8 k of its XCD lane in counter order,
  // so the image-per-XCD dealing holds without a static split's imbalance, and
  // the next tile's counter value is fetched while this tile runs
  const bool dyn = !fix;
  const int xl = (int)(blockIdx.x & 7);
  int* ctr = flags + n_img + 1 + xl;
  for (int t = blockIdx.x; t < n_tiles;) {
    int t_next = 0;   // (dyn, thread 0) the next position of this XCD lane
    if (dyn && tid == 0) t_next = xl + 8 * ((int)(gridDim.x >> 3) + atomicAdd(ctr, 1));
    const TileRef tr = tiles[t];
    const GemmProblem pu = probs[max(tr.problem, 0)], pv = probs[max(tr.problem, 0) + 1];   // even and odd parity
    const int li = pu.pad2;
    // padding of an XCD-dealt list, or (fix-up) an image not flagged: the next tile
    if (tr.problem < 0 || (fix && flags[li] == 0)) {
      if (dyn) {
        uint32_t* part = reinterpret_cast<uint32_t*>(lds);
        __syncthreads();
        if (tid == 0) part[24] = (uint32_t)t_next;
        __syncthreads();
        t = __builtin_amdgcn_readfirstlane((int)part[24]);   // uniform: the descriptors stay scalar
        __syncthreads();
      } else {
        t += (int)gridDim.x;
      }
      continue;
    }
    const ImgDesc d = imgs[li];
    const int H = d.H, W = d.W, Hh = (H + 1) >> 1, Ku = pu.K, Kv = pv.K;
    const int j0 = tr.tile * NPR;
    // operand scale 2^se: fixed in the first pass, k_gemm_h2's rule on the recorded |max| in the fix-up
    const int se = fix ? h2_operand_exp(amax[2 * li]) : kFusedSE;
    // the matrices: wave-instruction j: parity j / 4, plane (j / 2) % 2, row
    // group rg = wave + 8 (j % 2) of the plane layout of xh_lane_off
    const u32x4 brs[2] = {rsrc_words(pu.Xh, (uint32_t)xh_bytes(pu)), rsrc_words(pv.Xh, (uint32_t)xh_bytes(pv))};
    int boff[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      boff[0][h] = xh_lane_off(pu, 0, wave + 8 * h);
      boff[1][h] = xh_lane_off(pv, 0, wave + 8 * h);
    }
    const int xsp2[2] = {(int)(pu.xs_plane * 2), (int)(pv.xs_plane * 2)};
    const int nrow[2] = {(pu.N + 31) & ~31, (pv.N + 31) & ~31};   // matrix rows the MFMAs read
    auto dma_b = [&](int st, int k0) {
#if defined(DCTAE_PROFILING) && defined(DCTAE_FUSED_ABL) && (DCTAE_FUSED_ABL & 8)
      return;   // profiling ablation: no matrix loads (wrong output)
#endif
      uint8_t* base = lds + st * B_ST;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int par = j >> 2, pl = (j >> 1) & 1, h = j & 1;
        if (16 * (wave + 8 * h) < nrow[par])   // rows past the parity's N (rounded to the MFMA blocks) are never read
          dma_lds16(brs[par], base + (2 * par + pl) * B_PL + (wave + 8 * h) * 1024,
                    boff[par][h] + k0 * 2 + pl * xsp2[par]);
      }
    };
    // the pixels: row pair pr = tid / 32 (y = j0 + pr, y2 = H-1-y), column k = k0 + tid % 32 and W-1-k
    const int pr = tid >> 5, kk0 = tid & 31;
    const int y = j0 + pr;
    const bool vy = y < Hh;
    const int yy = vy ? y : 0, y2 = H - 1 - yy;
    const bool yp = y2 != yy;
    const int hw = H * W;
    const auto rrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<PxT*>(rgb + d.rgb_off), 0,
                                                         3 * hw * (int)sizeof(PxT), 0x00020000);
    typedef float Px[4][3];
    Px pxa, pxb;
    auto load_rgb = [&](Px& px, int k0) {
#if defined(DCTAE_PROFILING) && defined(DCTAE_FUSED_ABL) && (DCTAE_FUSED_ABL & 4)
#pragma unroll
      for (int q = 0; q < 4; ++q)   // profiling ablation: no pixel loads (wrong output)
#pragma unroll
        for (int c = 0; c < 3; ++c) px[q][c] = 0.001f * (float)(k0 + q + c + kk0);
      return;
#endif
      const int k = k0 + kk0, kk = k < Ku ? k : 0, x2 = W - 1 - kk;
      const int o[4] = {yy * W + kk, yy * W + x2, y2 * W + kk, y2 * W + x2};
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          // as loaded: the fp32 value, or the byte zero-extended (px_value in pix(), after the wait)
          if constexpr (sizeof(PxT) == 4)
            px[q][c] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, (c * hw + o[q]) * 4, 0, 0));
          else
            px[q][c] = __uint_as_float((uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rrsrc, c * hw + o[q], 0, 0));
    };
    bool bad = false;
    uint32_t fmx = 0;   // |max| of the folded values (the fix-up's scale)
    float pi[4][3];     // the IPT of the chunk position's 4 pixels
    // the colour transform of pixel q (util.py:70-82, k_rgb_to_ipt's arithmetic)
    auto pix = [&](const Px& px, int q) {
      const float r = px_value<PxT>(px[q][0]), g = px_value<PxT>(px[q][1]), b = px_value<PxT>(px[q][2]);
      const float l0 = signed_pow_fast(mat3_row(cm.rgb2lms, 0, r, g, b), gam);
      const float l1 = signed_pow_fast(mat3_row(cm.rgb2lms, 1, r, g, b), gam);
      const float l2 = signed_pow_fast(mat3_row(cm.rgb2lms, 2, r, g, b), gam);
#pragma unroll
      for (int c = 0; c < 3; ++c) pi[q][c] = mat3_row(cm.lms2ipt, c, l0, l1, l2);
    };
    // k_rgb_to_ipt's folds of channel c: row y (sum) and row H-1-y (difference)
    // of both parities, split into fp16 pieces into Ab (the split stated at
    // split_h2, dctae_mfma_tile.h, one value at a time)
    auto fold = [&](int k0, int c, uint16_t* Ab) {
      const int k = k0 + kk0;
      const int kk = k < Ku ? k : 0;
      const bool xp = W - 1 - kk != kk;
      const bool oku = vy && k < Ku, okv = vy && k < Kv;
      const int kq = (k & 31) >> 3, kw = k & 7;
      const float pb = xp ? pi[1][c] : 0.0f, pd = xp ? pi[3][c] : 0.0f;
      const float a = yp ? pi[0][c] + pi[2][c] : pi[0][c];
      const float bb = yp ? pb + pd : pb;
      const float c2 = pi[0][c] - pi[2][c], d2 = pb - pd;
      const float v[2][2] = {{oku ? (xp ? a + bb : a) : 0.0f, oku && yp ? (xp ? c2 + d2 : c2) : 0.0f},
                             {okv ? a - bb : 0.0f, okv && yp ? c2 - d2 : 0.0f}};
#pragma unroll
      for (int par = 0; par < 2; ++par)
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          const float vv = v[par][rr];
          fmx = max(fmx, __float_as_uint(vv) & 0x7fffffffu);
          const float vsc = ldexpf(vv, se);
          bad |= !(fabsf(vsc) < 32768.0f);
          const _Float16 h0 = (_Float16)vsc;
          const _Float16 h1 = (_Float16)(vsc - (float)h0);
          const int row = pr + NPR * rr;
          const int o = lds_off(row, kq) + kw;
          Ab[((par * 3 + c) * 2 + 0) * A_CQ + o] = __builtin_bit_cast(uint16_t, h0);
          Ab[((par * 3 + c) * 2 + 1) * A_CQ + o] = __builtin_bit_cast(uint16_t, h1);
        }
    };
    auto transform = [&](const Px& px, int k0, uint16_t* Ab) {
#if defined(DCTAE_PROFILING) && defined(DCTAE_FUSED_ABL) && (DCTAE_FUSED_ABL & 1)
      // profiling ablation: no colour transform / folds / split (wrong output)
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int pq = 0; pq < 8; ++pq) {
          const int row = pr + NPR * (pq & 1);
          const int o = row * XK + 8 * (((kk0 >> 3)) ^ swz(row)) + (kk0 & 7);
          Ab[((pq >> 2) * 3 + c) * 2 * A_CQ + ((pq >> 1) & 1) * A_CQ + o] =
              (uint16_t)(__float_as_uint(px[pq & 3][c]) & 0x3bffu);
        }
      return;
#endif
#pragma unroll
      for (int q = 0; q < 4; ++q) pix(px, q);
#pragma unroll
      for (int c = 0; c < 3; ++c) fold(k0, c, Ab);
    };
    floatx16 acc[3][2];
    zero_acc(&acc[0][0], 6);
    const int nw = pw ? pv.N : pu.N;   // this wave's parity's output columns
    // the MFMAs of k step ks and channel c of one chunk (stage st, pieces Ab)
    auto mfma_unit = [&](int st, const uint16_t* Ab, int ks, int c) {
#if defined(DCTAE_PROFILING) && defined(DCTAE_FUSED_ABL) && (DCTAE_FUSED_ABL & 2)
      return;   // profiling ablation: no MFMAs (wrong output)
#endif
      const uint16_t* Bp = reinterpret_cast<const uint16_t*>(lds + st * B_ST + 2 * pw * B_PL);
      const int kq = 2 * ks + half;
      bf16x8 a[2];
#pragma unroll
      for (int q = 0; q < 2; ++q)
        a[q] = *reinterpret_cast<const bf16x8*>(Ab + ((pw * 3 + c) * 2 + q) * A_CQ + lds_off(l32, kq));
#pragma unroll
      for (int x = 0; x < 2; ++x)
        if (wc * 64 + 32 * x < nw) {   // (wave-uniform) columns past N: none
          const int rb = wc * 64 + 32 * x + l32;
          bf16x8 b[2];
#pragma unroll
          for (int pl = 0; pl < 2; ++pl)
            b[pl] = *reinterpret_cast<const bf16x8*>(Bp + pl * (B_PL / 2) + lds_off(rb, kq));
          mfma_pieces(acc[c][x], a, b);
        }
    };
    const int nk = (Ku + XK - 1) / XK;
    // Pixels two chunks ahead (pxa: even chunks, pxb: odd), the matrices one;
    // issue order per step i: [matrices i + 1] [pixels i + 2], so at its top at
    // most pixels i + 1's 12 loads may be outstanding.  Every step issues the
    // same loads (past the last chunk: clamped pixels, matrix offsets reading
    // zeros), and the loop body is unconditional, so the compiler's own waits
    // on the pixel registers count exactly.
    auto step = [&](int i, Px& cur) {
      wait_vm<12>();      // this wave's pixels and matrix chunk i
      lds_barrier();      // every wave's; chunk i - 1's MFMAs done (the pieces and stage (i + 1) % 2 free)
      dma_b((i + 1) & 1, (i + 1) * XK);
      transform(cur, i * XK, As);
      load_rgb(cur, (i + 2) * XK);
      lds_barrier();      // the pieces of chunk i
#pragma unroll
      for (int ks = 0; ks < XK / 16; ++ks)
#pragma unroll
        for (int c = 0; c < 3; ++c) mfma_unit(i & 1, As, ks, c);
    };
    load_rgb(pxa, 0);
    dma_b(0, 0);
    load_rgb(pxb, XK);
    int i = 0;
    for (; i + 1 < nk; i += 2) {
      step(i, pxa);
      step(i + 1, pxb);
    }
    if (i < nk) step(i, pxa);
    wait_vm<0>();   // no LDS DMA may outlive the loop (the LDS is reused, and released at exit)
    const GemmProblem& p = pw ? pv : pu;
    const int N = p.N;
    const float unscale = ldexpf(1.0f, -(se + p.xh_exp));
    // C/D map: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5):
    // rows < 16 are the sums (T row j0 + row), the rest the differences (T row
    // H - 1 - (j0 + row - 16)); the middle row of an odd H has no difference
    uint32_t mx = 0;
    int trow[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rr = (r & 3) + 8 * (r >> 2) + 4 * half;
      const int j = j0 + (rr & (NPR - 1));
      const int ty = rr < NPR ? j : H - 1 - j;
      trow[r] = (j < Hh && (rr < NPR || ty != j)) ? ty : -1;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        const bool vn = wc * 64 + 32 * x + l32 < N;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          acc[c][x][r] *= unscale;
          if (vn && trow[r] >= 0) mx = max(mx, __float_as_uint(acc[c][x][r]) & 0x7fffffffu);
        }
      }
    // block reductions: flag, |max| of the folded values, |max| of T
    uint32_t* part = reinterpret_cast<uint32_t*>(lds);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
      fmx = max(fmx, (uint32_t)__shfl_xor((int)fmx, o));
    }
    const bool wbad = __ballot(bad) != 0;   // (__syncthreads_or brings 256 bytes of LDS of its own)
    __syncthreads();   // every wave past its last LDS read: the partials alias the ring
    if (lane == 0) {
      part[wave] = mx;
      part[8 + wave] = fmx;
      part[16 + wave] = wbad ? 1u : 0u;
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t m = 0, f = 0, any_bad = 0;
      for (int w = 0; w < 8; ++w) {
        m = max(m, part[w]);
        f = max(f, part[8 + w]);
        any_bad |= part[16 + w];
      }
      if (!fix) {
        if (f) atomicMax(amax + 2 * li, f);
        if (any_bad) {
          flags[li] = 1;
          flags[n_img] = 1;   // the job's "any" word, read first by the fix-up
        }
      }
      // T's |max| for the column GEMM; a flagged block leaves it to the fix-up
      if (pu.omax && (fix || !any_bad)) atomicMax(pu.omax, m);
    }
    // T is row-major: the buffer stores of store_acc_32x32 (range, kOob), on this kernel's row map
    const int64_t ext = out_extent(p);
    const int sOm4 = (int)(p.sOm * 4);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const auto rsrc = out_rsrc(p, ext, c);
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        const int n = wc * 64 + 32 * x + l32;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int vo = (n < N && trow[r] >= 0) ? trow[r] * sOm4 + n * 4 : kOob;
#if defined(DCTAE_PROFILING) && defined(DCTAE_FUSED_ABL) && (DCTAE_FUSED_ABL & 16)
          if (acc[c][x][r] == 1.2345f)   // profiling ablation: (almost) no T stores (wrong output)
#endif
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[c][x][r]), rsrc, vo, 0, 0);
        }
      }
    }
    if (dyn) {
      uint32_t* part = reinterpret_cast<uint32_t*>(lds);
      if (tid == 0) part[24] = (uint32_t)t_next;
      __syncthreads();
      t = __builtin_amdgcn_readfirstlane((int)part[24]);   // uniform: the descriptors stay scalar
    } else {
      t += (int)gridDim.x;
    }
    __syncthreads();   // the partials / LDS reused by the next tile
  }
}

int fused_pairs_per_block() { return kFusedPairs; }
int fused_max_n() { return kFusedTN; }

void launch_rows_fused(const GemmProblem* probs, const TileRef* tiles, int n_tiles, const ImgDesc* imgs,
                       const void* rgb, PixelType px, const ColorMats& cm, uint32_t* amax, int* flags, int n_img,
                       hipStream_t s, bool fixup) {
  if (n_tiles <= 0) return;
  // the persistent first pass, or the fix-up's short grid-stride launch (every
  // block exits at once when no image is flagged)
  const int g = std::min((n_tiles + 7) & ~7, 256);
  if (px == PixelType::kU8)
    hipLaunchKernelGGL(k_rows_fused<uint8_t>, dim3(g), dim3(512), 0, s, probs, tiles, n_tiles, imgs,
                       (const uint8_t*)rgb, cm, amax, flags, n_img, fixup ? 1 : 0);
  else
    hipLaunchKernelGGL(k_rows_fused<float>, dim3(g), dim3(512), 0, s, probs, tiles, n_tiles, imgs, (const float*)rgb,
                       cm, amax, flags, n_img, fixup ? 1 : 0);
}

}  // namespace dctae
