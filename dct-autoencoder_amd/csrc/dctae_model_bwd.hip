// DCTAutoencoder transformer backward: the kernels under the
// training step of the CLIPEncoder stacks.  bf16 MFMA operands, fp32
// accumulation, and no floating-point atomics: every sum has a fixed order,
// so losses and gradients repeat bit for bit.
//
//   k_attn_bwd_dq   workgroup = 128 queries of one (row, head), sweeps the key
//                   blocks: S^T = K Q^T and dP^T = V dO^T land in the forward's
//                   accumulator layout (query on the lane), so LSE and delta
//                   are per-lane scalars and dS^T is already the B operand of
//                   dQ^T += K^T dS^T (K read transposed like the forward's V).
//                   A first sweep takes delta = sum_j P dP (fp32) and writes
//                   it for the other pass; the second makes dQ.
//   k_attn_bwd_dkv  workgroup = 128 keys, sweeps the query blocks: S = Q K^T
//                   and dP = dO V^T with the key on the lane; P and dS are the
//                   B operands of dV^T += dO^T P and dK^T += Q^T dS, which stay
//                   in accumulators for the whole sweep.
//   k_transpose_pack bf16 (M, C) -> (C, pad64(M)) with a zero tail: the operand
//                   form of dW = dY^T X for the forward's k_linear (the token
//                   sum becomes its K dimension)
//   k_colsum        fixed-order column sums (bias gradients, LayerNorm partials)
//   k_ln_bwd        LayerNorm backward, one wave per row, statistics recomputed
//   k_qgelu / k_qgelu_bwd   quick_gelu on the kept bf16 pre-activation
//   k_pos_grad      position-table gradients, one wave per (table row, 64
//                   columns), tokens in order
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dctae_model.h"
#include "dctae_internal.h"

namespace dctae {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint16_t f2bf(float f) {   // round to nearest even
  const __bf16 h = (__bf16)f;
  return __builtin_bit_cast(uint16_t, h);
}
__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

// ---------------------------------------------------------------------------
// attention backward, d_head = 64.  Block = 128 queries (dQ pass) or 128 keys
// (dK / dV pass), wave = 32 of them; the swept side comes in blocks of 64 rows
// staged in LDS twice: stride 72 for the row-fragment reads (ds_read_b128) and
// stride 96 for the transposed reads (ds_read_b64_tr_b16), the forward's two
// conflict-free layouts.
// ---------------------------------------------------------------------------
constexpr int BR = 128, BS = 64, BD = 64, BSTR = 72, BTS = 96, BTH = 256;
constexpr float LOG2E = 1.4426950408889634f;

// A fragment (d = 32 dt + lane % 32, k step kk) of the transpose of a row-major
// 64 x 64 tile (stride BTS): the forward's V^T read, rows in its key order
__device__ __forceinline__ bf16x8 tr_frag(const uint16_t* T, int dt, int kk, int lane) {
  const int gq = (lane & 15) >> 2, gp = lane & 3, gx = (lane >> 4) & 1;
  const int kb = 32 * (kk >> 1) + 8 * (2 * (kk & 1)) + 4 * (lane >> 5);
  const uint16_t* vr = T + (kb + gq) * BTS + 32 * dt + 16 * gx + 4 * gp;
  const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)vr);
  const s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(vr + 8 * BTS));
  bf16x8 f;
  short* sh = reinterpret_cast<short*>(&f);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    sh[e] = lo[e];
    sh[4 + e] = hi[e];
  }
  return f;
}

__device__ __forceinline__ bf16x8 row_frag(const uint16_t* T, int t, int kk, int lane) {
  return *reinterpret_cast<const bf16x8*>(T + (t * 32 + (lane & 31)) * BSTR + kk * 16 + (lane >> 5) * 8);
}

// stage 64 rows x 64 d of src (row stride ld, rows clamped to S - 1) into both layouts
__device__ __forceinline__ void stage_tile(const uint16_t* src, int64_t ld, int r0, int S, uint16_t* Ts, uint16_t* Tt,
                                           int tid) {
#pragma unroll
  for (int j = 0; j < BS * 8 / BTH; ++j) {
    const int idx = tid + BTH * j, row = idx >> 3, seg = idx & 7;
    const int rg = min(r0 + row, S - 1);
    const uint4 v = *reinterpret_cast<const uint4*>(src + rg * ld + seg * 8);
    if (Ts) *reinterpret_cast<uint4*>(Ts + row * BSTR + seg * 8) = v;
    if (Tt) *reinterpret_cast<uint4*>(Tt + row * BTS + seg * 8) = v;
  }
}

// the wave's (64 d x 32 rows)^T accumulators -> Os[row][d] -> 16-byte row segments of dst
__device__ __forceinline__ void store_rows(const f32x16 (&acc)[2], uint16_t* Os, uint16_t* dst, int64_t ld, int r0, int S,
                                           int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const int rr = wave * 32 + (lane & 31);
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int v = 0; v < 16; ++v) Os[rr * BSTR + 32 * dt + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3)] = f2bf(acc[dt][v]);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < BR * 8 / BTH; ++j) {
    const int idx = tid + BTH * j, r = idx >> 3, seg = idx & 7;
    if (r0 + r < S)
      *reinterpret_cast<uint4*>(dst + (r0 + r) * ld + seg * 8) = *reinterpret_cast<const uint4*>(Os + r * BSTR + seg * 8);
  }
  __syncthreads();
}

__global__ __launch_bounds__(BTH) void k_attn_bwd_dq(AttnBwdArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t Ks[BS * BSTR];
  __shared__ __attribute__((aligned(16))) uint16_t Kt[BS * BTS];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[BS * BSTR];
  __shared__ __attribute__((aligned(16))) int32_t kid[BS];   // key image id, or -1 for a non-pad key (no bias)
  __shared__ __attribute__((aligned(16))) uint16_t Os[BR * BSTR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = a.S, D = a.heads * BD;
  const int q0 = blockIdx.x * BR, h = blockIdx.y, b = blockIdx.z;
  const int64_t rowbase = (int64_t)b * S, ld = 3ll * D;
  const int ql = q0 + wave * 32 + (lane & 31), qc = min(ql, S - 1);
  const int dseg = (lane >> 5) * 8;
  bf16x8 qf[4], dof[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    qf[kk] = *reinterpret_cast<const bf16x8*>(a.qkv + (rowbase + qc) * ld + h * BD + kk * 16 + dseg);
    dof[kk] = *reinterpret_cast<const bf16x8*>(a.dout + (rowbase + qc) * (int64_t)a.lddo + h * BD + kk * 16 + dseg);
  }
  const int64_t stat = ((int64_t)b * a.heads + h) * S;
  const float lse = a.lse[stat + qc];
  const int32_t my_id = (int32_t)a.ids[rowbase + qc];
  const float sc = a.scale * LOG2E;
  f32x16 dq[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) dq[t][v] = 0.0f;
  // Two sweeps over the keys.  The first takes delta = sum_j P dP from the very
  // P and dP (fp32) the second multiplies, so each query's dS sums to zero to
  // fp32 rounding.  rowsum(dO * O) equals it only in exact arithmetic: with the
  // forward's bf16 O the difference is a per-query offset of dS that does not
  // cancel over the keys and lands in dQ, dK and the k_proj bias gradient
  // (analytically zero).
  float dl = 0.0f;
#pragma unroll 1
  for (int sweep = 0; sweep < 2; ++sweep) {
    for (int k0 = 0; k0 < S; k0 += BS) {
      __syncthreads();   // previous block's reads done
      stage_tile(a.qkv + rowbase * ld + h * BD + D, ld, k0, S, Ks, Kt, tid);
      stage_tile(a.qkv + rowbase * ld + h * BD + 2 * D, ld, k0, S, Vs, nullptr, tid);
      if (tid < BS) {
        const int kg = k0 + tid;
        const bool pad = kg < S && a.key_pad[rowbase + kg];
        kid[tid] = pad ? (int32_t)a.ids[rowbase + kg] : -1;
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x16 st, dp;
#pragma unroll
        for (int v = 0; v < 16; ++v) st[v] = dp[v] = 0.0f;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(Ks, t, kk, lane), qf[kk], st, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(Vs, t, kk, lane), dof[kk], dp, 0, 0, 0);
        }
        // dS^T in B-operand order: key step 2 t + (v / 8) holds the lane's values v % 8
        bf16x8 dsf[2];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const int kr = t * 32 + 8 * q4 + 4 * (lane >> 5);
          const int4 ki = *reinterpret_cast<const int4*>(kid + kr);
          const int32_t kis[4] = {ki.x, ki.y, ki.z, ki.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int v = 4 * q4 + e;
            const float s2 = st[v] * sc + (kis[e] == my_id ? LOG2E : 0.0f);
            const float p = k0 + kr + e < S ? __builtin_amdgcn_exp2f(s2 - lse) : 0.0f;
            if (sweep == 0) dl += p * dp[v];
            else dsf[v >> 3][v & 7] = (__bf16)(p * (dp[v] - dl) * a.scale);
          }
        }
        if (sweep == 1) {
#pragma unroll
          for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2)
              dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(Kt, dt, 2 * t + k2, lane), dsf[k2], dq[dt], 0, 0, 0);
        }
      }
    }
    if (sweep == 0) {   // the query's keys are split over lanes l and l ^ 32
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(dl), __float_as_uint(dl), false, false);
      dl = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
      if (lane < 32 && ql < S) a.delta[stat + ql] = dl;
    }
  }
  __syncthreads();
  store_rows(dq, Os, a.dqkv + rowbase * ld + h * BD, ld, q0, S, tid);
}

__global__ __launch_bounds__(BTH) void k_attn_bwd_dkv(AttnBwdArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t Qs[BS * BSTR];
  __shared__ __attribute__((aligned(16))) uint16_t Qt[BS * BTS];
  __shared__ __attribute__((aligned(16))) uint16_t Ds[BS * BSTR];
  __shared__ __attribute__((aligned(16))) uint16_t Dt[BS * BTS];
  __shared__ __attribute__((aligned(16))) int32_t qid[BS];
  __shared__ __attribute__((aligned(16))) float qlse[BS];   // +inf for queries past S: P = 0
  __shared__ __attribute__((aligned(16))) float qdl[BS];
  __shared__ __attribute__((aligned(16))) uint16_t Os[BR * BSTR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = a.S, D = a.heads * BD;
  const int kb0 = blockIdx.x * BR, h = blockIdx.y, b = blockIdx.z;
  const int64_t rowbase = (int64_t)b * S, ld = 3ll * D;
  const int kc = min(kb0 + wave * 32 + (lane & 31), S - 1);
  const int dseg = (lane >> 5) * 8;
  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    kf[kk] = *reinterpret_cast<const bf16x8*>(a.qkv + (rowbase + kc) * ld + D + h * BD + kk * 16 + dseg);
    vf[kk] = *reinterpret_cast<const bf16x8*>(a.qkv + (rowbase + kc) * ld + 2 * D + h * BD + kk * 16 + dseg);
  }
  // the +1.0 bias hits (query, key) when the key is a pad of the query's image
  const int32_t my_id = a.key_pad[rowbase + kc] ? (int32_t)a.ids[rowbase + kc] : -1;
  const int64_t stat = ((int64_t)b * a.heads + h) * S;
  const float sc = a.scale * LOG2E;
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) dk[t][v] = dv[t][v] = 0.0f;
  for (int q0 = 0; q0 < S; q0 += BS) {
    __syncthreads();
    stage_tile(a.qkv + rowbase * ld + h * BD, ld, q0, S, Qs, Qt, tid);
    stage_tile(a.dout + rowbase * a.lddo + h * BD, a.lddo, q0, S, Ds, Dt, tid);
    if (tid < BS) {
      const int qg = q0 + tid, qq = min(qg, S - 1);
      qid[tid] = (int32_t)a.ids[rowbase + qq];
      qlse[tid] = qg < S ? a.lse[stat + qq] : INFINITY;
      qdl[tid] = a.delta[stat + qq];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x16 st, dp;
#pragma unroll
      for (int v = 0; v < 16; ++v) st[v] = dp[v] = 0.0f;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(Qs, t, kk, lane), kf[kk], st, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(Ds, t, kk, lane), vf[kk], dp, 0, 0, 0);
      }
      bf16x8 pf[2], dsf[2];
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int qr = t * 32 + 8 * q4 + 4 * (lane >> 5);
        const int4 qi = *reinterpret_cast<const int4*>(qid + qr);
        const float4 ql = *reinterpret_cast<const float4*>(qlse + qr);
        const float4 qd = *reinterpret_cast<const float4*>(qdl + qr);
        const int32_t qis[4] = {qi.x, qi.y, qi.z, qi.w};
        const float qls[4] = {ql.x, ql.y, ql.z, ql.w};
        const float qds[4] = {qd.x, qd.y, qd.z, qd.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int v = 4 * q4 + e;
          const float s2 = st[v] * sc + (qis[e] == my_id ? LOG2E : 0.0f);
          const float p = __builtin_amdgcn_exp2f(s2 - qls[e]);
          pf[v >> 3][v & 7] = (__bf16)p;
          dsf[v >> 3][v & 7] = (__bf16)(p * (dp[v] - qds[e]) * a.scale);
        }
      }
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(Dt, dt, 2 * t + k2, lane), pf[k2], dv[dt], 0, 0, 0);
          dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(Qt, dt, 2 * t + k2, lane), dsf[k2], dk[dt], 0, 0, 0);
        }
    }
  }
  __syncthreads();
  store_rows(dk, Os, a.dqkv + rowbase * ld + D + h * BD, ld, kb0, S, tid);
  store_rows(dv, Os, a.dqkv + rowbase * ld + 2 * D + h * BD, ld, kb0, S, tid);
}

void launch_attention_bwd(const AttnBwdArgs& a, hipStream_t s) {
  if (a.R <= 0 || a.S <= 0) return;
  const dim3 grid((a.S + BR - 1) / BR, a.heads, a.R);
  hipLaunchKernelGGL(k_attn_bwd_dq, grid, dim3(BTH), 0, s, a);     // writes delta for the second pass
  hipLaunchKernelGGL(k_attn_bwd_dkv, grid, dim3(BTH), 0, s, a);
}

// ---------------------------------------------------------------------------
// bf16 (M, C) -> (C, Mp), columns M .. Mp zero (Mp % 64 == 0)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_transpose_pack(const uint16_t* x, int64_t ldx, int64_t M, int C, int64_t Mp,
                                                        uint16_t* out) {
  __shared__ uint16_t T[64][66];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * 64;
  const int c0 = blockIdx.y * 64;
  for (int r = ty; r < 64; r += 4) {
    const int64_t m = m0 + r;
    const int c = c0 + tx;
    T[r][tx] = (m < M && c < C) ? x[m * ldx + c] : (uint16_t)0;
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int c = c0 + r;
    if (c < C) out[(int64_t)c * Mp + m0 + tx] = T[tx][r];
  }
}

void launch_transpose_pack(const uint16_t* x, int64_t ldx, int64_t M, int C, int64_t Mp, uint16_t* out, hipStream_t s) {
  if (Mp <= 0 || C <= 0) return;
  hipLaunchKernelGGL(k_transpose_pack, dim3((unsigned)(Mp / 64), (unsigned)((C + 63) / 64)), dim3(256), 0, s, x, ldx, M, C,
                     Mp, out);
}

// ---------------------------------------------------------------------------
// column sums in a fixed order: block (64 columns, chunk of `rows` rows), four
// row phases per column added 0 + 1 + 2 + 3
// ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ float ldf(const T* p);
template <>
__device__ __forceinline__ float ldf<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float ldf<uint16_t>(const uint16_t* p) { return bf2f(*p); }

template <typename T>
__global__ __launch_bounds__(256) void k_colsum(const T* x, int64_t ldx, int64_t M, int N, int64_t rows, float* out) {
  __shared__ float red[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx;
  const int64_t r0 = (int64_t)blockIdx.y * rows, r1 = min(M, r0 + rows);
  float acc = 0.0f;
  if (c < N)
    for (int64_t r = r0 + ty; r < r1; r += 4) acc += ldf<T>(x + r * ldx + c);
  red[ty][tx] = acc;
  __syncthreads();
  if (ty == 0 && c < N) out[(int64_t)blockIdx.y * N + c] = ((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx];
}

constexpr int64_t CS_ROWS = 64;   // rows per first-stage block: M = 12288 gives 192 x N / 64 blocks

void launch_colsum(const void* x, int64_t ldx, int64_t M, int N, bool bf16, float* ws, float* out, hipStream_t s) {
  if (N <= 0) return;
  const unsigned gx = (unsigned)((N + 63) / 64);
  const int64_t parts = (M + CS_ROWS - 1) / CS_ROWS;
  const bool two = parts > 4;
  float* o1 = two ? ws : out;
  const int64_t rows = two ? CS_ROWS : (M > 0 ? M : 1);
  const dim3 g1(gx, (unsigned)(two ? parts : 1));
  if (bf16) hipLaunchKernelGGL(k_colsum<uint16_t>, g1, dim3(256), 0, s, (const uint16_t*)x, ldx, M, N, rows, o1);
  else hipLaunchKernelGGL(k_colsum<float>, g1, dim3(256), 0, s, (const float*)x, ldx, M, N, rows, o1);
  if (two) hipLaunchKernelGGL(k_colsum<float>, dim3(gx, 1), dim3(256), 0, s, (const float*)ws, (int64_t)N, parts, N, parts, out);
}

// ---------------------------------------------------------------------------
// LayerNorm backward: one wave per row, LN_RPW consecutive rows per wave.
//   xhat = (x - mean) rstd, g = gamma dy,
//   dx = rstd (g - mean(g) - xhat mean(g xhat))   (added to dx when accumulate)
// Each wave leaves its rows' sums of dy xhat and dy in part_g / part_b row
// (wave index); k_colsum adds those rows in order.
// ---------------------------------------------------------------------------
template <int PER>
__global__ __launch_bounds__(256) void k_ln_bwd(LnBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t r0 = w * LN_RPW;
  if (r0 >= a.M) return;
  const int D = a.D;
  float gam[PER], dg[PER], db[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int c = lane + 64 * i;
    gam[i] = c < D ? a.gamma[c] : 0.0f;
    dg[i] = db[i] = 0.0f;
  }
  const int64_t r1 = min(a.M, r0 + LN_RPW);
  for (int64_t m = r0; m < r1; ++m) {
    const float* x = a.x + m * a.ldx;
    const float* dy = a.dy + m * a.lddy;
    float v[PER], g[PER];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int c = lane + 64 * i;
      v[i] = c < D ? x[c] : 0.0f;
      s += v[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / (float)D;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int c = lane + 64 * i;
      v[i] = c < D ? v[i] - mean : 0.0f;
      q += v[i] * v[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = rsqrtf(q / (float)D + a.eps);
    float sg = 0.0f, sgx = 0.0f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int c = lane + 64 * i;
      const float d = c < D ? dy[c] : 0.0f;
      v[i] *= rstd;   // xhat
      g[i] = d * gam[i];
      sg += g[i];
      sgx += g[i] * v[i];
      dg[i] += d * v[i];
      db[i] += d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sg += __shfl_xor(sg, o, 64);
      sgx += __shfl_xor(sgx, o, 64);
    }
    const float c1 = sg / (float)D, c2 = sgx / (float)D;
    float* dx = a.dx + m * a.lddx;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int c = lane + 64 * i;
      if (c < D) {
        const float r = rstd * (g[i] - c1 - v[i] * c2);
        dx[c] = a.accumulate ? dx[c] + r : r;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int c = lane + 64 * i;
    if (c < D) {
      a.part_g[w * D + c] = dg[i];
      a.part_b[w * D + c] = db[i];
    }
  }
}

void launch_layernorm_bwd(const LnBwdArgs& a, hipStream_t s) {
  if (a.M <= 0) return;
  const int64_t waves = (a.M + LN_RPW - 1) / LN_RPW;
  const unsigned grid = (unsigned)((waves + 3) / 4);
  const int per = (a.D + 63) / 64;
  if (per <= 2) hipLaunchKernelGGL(k_ln_bwd<2>, dim3(grid), dim3(256), 0, s, a);
  else if (per <= 4) hipLaunchKernelGGL(k_ln_bwd<4>, dim3(grid), dim3(256), 0, s, a);
  else if (per <= 8) hipLaunchKernelGGL(k_ln_bwd<8>, dim3(grid), dim3(256), 0, s, a);
  else if (per <= 16) hipLaunchKernelGGL(k_ln_bwd<16>, dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_ln_bwd<32>, dim3(grid), dim3(256), 0, s, a);   // D <= 2048
}

// ---------------------------------------------------------------------------
// quick_gelu on the kept bf16 pre-activation, and its derivative
//   y = x sig(1.702 x),  dy/dx = sig (1 + 1.702 x (1 - sig))
// ---------------------------------------------------------------------------
__global__ void k_qgelu(const uint16_t* pre, int64_t ldp, int64_t M, int N, uint16_t* out, int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * N) return;
  const int64_t m = i / N;
  const int n = (int)(i - m * N);
  const float x = bf2f(pre[m * ldp + n]);
  out[m * ldo + n] = f2bf(x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.45546696228f * x)));
}

__global__ void k_qgelu_bwd(const uint16_t* df, int64_t lddf, const uint16_t* pre, int64_t ldp, int64_t M, int N,
                            uint16_t* dpre, int64_t lddp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * N) return;
  const int64_t m = i / N;
  const int n = (int)(i - m * N);
  const float x = bf2f(pre[m * ldp + n]);
  const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.45546696228f * x));
  // beyond +-64 sg is exactly 1 or 0 and the derivative exactly 1 or 0; x itself would overflow 1.702 x
  // from 2e38 on (inf * 0): the clamp changes no finite result
  const float xc = fminf(fmaxf(x, -64.0f), 64.0f);
  dpre[m * lddp + n] = f2bf(bf2f(df[m * lddf + n]) * (sg * (1.0f + 1.702f * xc * (1.0f - sg))));
}

void launch_qgelu(const uint16_t* pre, int64_t ldp, int64_t M, int N, uint16_t* out, int64_t ldo, hipStream_t s) {
  const int64_t n = M * N;
  if (n > 0) hipLaunchKernelGGL(k_qgelu, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pre, ldp, M, N, out, ldo);
}

void launch_qgelu_bwd(const uint16_t* df, int64_t lddf, const uint16_t* pre, int64_t ldp, int64_t M, int N, uint16_t* dpre,
                      int64_t lddp, hipStream_t s) {
  const int64_t n = M * N;
  if (n > 0)
    hipLaunchKernelGGL(k_qgelu_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, df, lddf, pre, ldp, M, N, dpre, lddp);
}

// ---------------------------------------------------------------------------
// position-table gradient: out[row][c] = sum over tokens m with idx[m] == row
// of g[m][c], in token order.  One wave per (row, 64 columns): it reads 64
// indices at a time and walks the matching ones from the lowest token up.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pos_grad(const float* g, int64_t ldg, int64_t M, int D, const int64_t* idx,
                                                 int64_t istride, float* out) {
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int c = blockIdx.y * 64 + lane;
  float acc = 0.0f;
  for (int64_t m0 = 0; m0 < M; m0 += 64) {
    const int64_t m = m0 + lane;
    uint64_t hit = __ballot(m < M && idx[m * istride] == row);
    while (hit) {   // eight loads in flight, added in token order (an absent one adds 0)
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        v[u] = 0.0f;
        if (hit) {
          const int j = __builtin_ctzll(hit);
          hit &= hit - 1;
          if (c < D) v[u] = g[(m0 + j) * ldg + c];
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
  }
  if (c < D) out[row * D + c] = acc;
}

void launch_pos_grad(const float* g, int64_t ldg, int64_t M, int D, const int64_t* idx, int64_t istride, int rows,
                     float* out, hipStream_t s) {
  if (rows <= 0 || D <= 0) return;
  hipLaunchKernelGGL(k_pos_grad, dim3((unsigned)rows, (unsigned)((D + 63) / 64)), dim3(64), 0, s, g, ldg, M, D, idx, istride,
                     out);
}

}  // namespace dctae
