// The encode's sort / pack and pad-fill kernels, templates on the caller's code
// type.  Two units instantiate them, one code type each: dctae_kernels.hip the
// int64 kernels, dctae_codes16.hip the int16 ones (a second instantiation of
// the rocPRIM sort in one unit changes the inlining of the first, and with it
// the int64 kernels' instructions).
#pragma once
#include <rocprim/block/block_radix_sort.hpp>

#include "dctae_device.h"
#include "dctae_internal.h"

namespace dctae {

// ---------------------------------------------------------------------------
// per-image sort (score desc, flat index asc) + scatter into packed rows
// (FE:418-445 gather, FE:515-605 concatenation).  One block per image.
// ---------------------------------------------------------------------------


// Code: the caller's code type (int64_t or int16_t, CodeType), here and in
// k_sort_pack2 / k_pad_fill: the one store of each code sink
template <typename Code>
__global__ __launch_bounds__(1024) void k_sort_pack(const ImgDesc* __restrict__ imgs, int np2,
                                                    EncParams ep, TokenSinks st, PackSinks out) {
  extern __shared__ uint64_t keys[];
  const ImgDesc d = imgs[blockIdx.x];
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int i = tid; i < np2; i += nt) {
    uint64_t k = 0;
    if (i < d.T)
      k = ((uint64_t)float_key(st.scores[d.tok_off + stage_pos(d, i)]) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)i);
    keys[i] = k;
  }
  // bitonic sort, descending
  for (int size = 2; size <= np2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < (np2 >> 1); t += nt) {
        int i = 2 * t - (t & (stride - 1));
        int jx = i + stride;
        uint64_t a = keys[i], b = keys[jx];
        bool desc = (i & size) == 0;
        if (desc ? (a < b) : (a > b)) {
          keys[i] = b;
          keys[jx] = a;
        }
      }
    }
  }
  __syncthreads();
  const int S = ep.S, PP = ep.P * ep.P, C = ep.C;
  const int64_t base = (int64_t)d.row * S + d.col;
  for (int t = tid; t < d.k; t += nt) {
    const uint32_t f = 0xFFFFFFFFu - (uint32_t)(keys[t] & 0xFFFFFFFFu);
    const int c = f % C, s = f / C, h = s / d.qw, w = s % d.qw;
    const int64_t o = base + t;
    out.pos[2 * o] = h;
    out.pos[2 * o + 1] = w;
    out.ch[o] = c;
    out.ids[o] = d.local_id;
    if (out.key_pad) out.key_pad[o] = 0;
    if (out.scores) out.scores[o] = st.scores[d.tok_off + stage_pos(d, f)];
  }
  if (out.codes) {
    const int ncb = ep.ncb;
    for (int e = tid; e < d.k * ncb; e += nt) {
      const int t = e / ncb, q = e % ncb;
      const uint32_t f = stage_pos(d, 0xFFFFFFFFu - (uint32_t)(keys[t] & 0xFFFFFFFFu));
      static_cast<Code*>(out.codes)[(base + t) * ncb + q] =
          (Code)(int64_t)lfq_index_bits(st.codes[(d.tok_off + f) * ncb + q], ep.code_pos, ep.code_neg);
    }
  }
  if (out.patches || out.raw) {
    for (int64_t e = tid; e < (int64_t)d.k * PP; e += nt) {
      const int t = (int)(e / PP), q = (int)(e % PP);
      const uint32_t f = stage_pos(d, 0xFFFFFFFFu - (uint32_t)(keys[t] & 0xFFFFFFFFu));
      if (out.patches) out.patches[(base + t) * PP + q] = st.norm[(d.tok_off + f) * PP + q];
      if (out.raw) out.raw[(base + t) * PP + q] = st.raw[(d.tok_off + f) * PP + q];
    }
  }
}

// packed-order copy of the staged tokens (PP floats each) of one image:
// 16-byte pieces when PP % 4 == 0 and every base is 16-byte aligned (196 =
// 49 x 4 at P = 14), 32-bit index math (k * PP <= 3072 * 196)
__device__ __forceinline__ void gather_tokens(const ImgDesc& d, const uint16_t* order, int64_t base, int PP,
                                              const TokenSinks& st, const PackSinks& out, int tid, int nt) {
  const bool vec = (PP & 3) == 0 && ((reinterpret_cast<uintptr_t>(out.patches) | reinterpret_cast<uintptr_t>(out.raw) |
                                      reinterpret_cast<uintptr_t>(st.norm) | reinterpret_cast<uintptr_t>(st.raw)) & 15) == 0;
  if (vec) {
    const uint32_t P4 = (uint32_t)PP >> 2, n = (uint32_t)d.k * P4;
    for (uint32_t e = tid; e < n; e += nt) {
      const uint32_t t = e / P4, q = e - t * P4;
      const int64_t src = (d.tok_off + order[t]) * P4 + q, dst = (base + t) * P4 + q;
      if (out.patches) reinterpret_cast<float4*>(out.patches)[dst] = reinterpret_cast<const float4*>(st.norm)[src];
      if (out.raw) reinterpret_cast<float4*>(out.raw)[dst] = reinterpret_cast<const float4*>(st.raw)[src];
    }
    return;
  }
  const uint32_t n = (uint32_t)d.k * (uint32_t)PP;
  for (uint32_t e = tid; e < n; e += nt) {
    const uint32_t t = e / (uint32_t)PP, q = e - t * (uint32_t)PP;
    const int64_t src = (d.tok_off + order[t]) * PP + q, dst = (base + t) * PP + q;
    if (out.patches) out.patches[dst] = st.norm[src];
    if (out.raw) out.raw[dst] = st.raw[src];
  }
}

// Same contract with rocPRIM's block radix sort (LSD, stable): 32-bit score
// keys sorted descending, flat indices as values; stability keeps equal
// scores in ascending index order = the (score desc, index asc) order above.
// Tokens per image <= 512 x 6 = 3072 (max_patch 32 x 32, 3 channels); the
// 256 x 3 instance covers 224^2 images (768 tokens).
typedef unsigned v4u32 __attribute__((ext_vector_type(4)));
typedef unsigned v2u32s __attribute__((ext_vector_type(2)));

template <int kSortBS, int kSortIPT, typename Code>
__global__ __launch_bounds__(kSortBS) void k_sort_pack2(const ImgDesc* __restrict__ imgs, EncParams ep,
                                                        TokenSinks st, PackSinks out) {
  using Sort = rocprim::block_radix_sort<uint32_t, kSortBS, kSortIPT, uint32_t>;
  __shared__ typename Sort::storage_type tmp;
  __shared__ uint16_t order[kSortBS * kSortIPT];   // flat token index f of rank t
  __shared__ uint16_t spos[kSortBS * kSortIPT];    // its staging position (stage_pos)
  const int tid = threadIdx.x;
  const ImgDesc d = imgs[blockIdx.x];
  uint32_t keys[kSortIPT], vals[kSortIPT];
  {
    // all six score loads in flight at once (unconditional: past-the-end lanes
    // read 0 through the descriptor's num_records)
    const auto krs = __builtin_amdgcn_make_buffer_rsrc(st.scores + d.tok_off, 0, d.T * 4, 0x00020000);
#pragma unroll
    for (int i = 0; i < kSortIPT; ++i) {
      const int idx = tid * kSortIPT + i;   // blocked: input order = index order (stability -> index asc)
      keys[i] = __builtin_amdgcn_raw_buffer_load_b32(krs, idx < d.T ? stage_pos(d, idx) * 4 : 0x7ffffff0, 0, 0);
      vals[i] = (uint32_t)idx;
    }
#pragma unroll
    for (int i = 0; i < kSortIPT; ++i) keys[i] = (int)vals[i] < d.T ? float_key(__uint_as_float(keys[i])) : 0u;
  }
  Sort().sort_desc_to_striped(keys, vals, tmp);
#pragma unroll
  for (int i = 0; i < kSortIPT; ++i) {
    const int rank = tid + kSortBS * i;
    if (rank < d.k) {
      order[rank] = (uint16_t)vals[i];
      spos[rank] = (uint16_t)stage_pos(d, (int)vals[i]);
    }
  }
  __syncthreads();
  const int S = ep.S, PP = ep.P * ep.P, C = ep.C;
  const int64_t base = (int64_t)d.row * S + d.col;
  for (int t = tid; t < d.k; t += kSortBS) {
    const uint32_t f = order[t];
    const int c = f % C, s = f / C, h = s / d.qw, w = s % d.qw;
    const int64_t o = base + t;
    *reinterpret_cast<longlong2*>(out.pos + 2 * o) = make_longlong2(h, w);
    out.ch[o] = c;
    out.ids[o] = d.local_id;
    if (out.key_pad) out.key_pad[o] = 0;
    if (out.scores) out.scores[o] = st.scores[d.tok_off + spos[t]];
  }
  if (out.codes && ep.ncb == 14) {
    // two codes per lane: one u32 of the u16 staging -> one 16-byte int64 pair
    // (coalesced).  kCU gathers in flight per lane before any is used (one
    // gather + wait per iteration exposed the load latency 42 times per lane),
    // buffer descriptors on the image's staging / packed span (32-bit offsets;
    // past-the-end lanes clipped by num_records)
    constexpr int kCU = 14;
    const uint32_t pos2 = ep.code_pos | (ep.code_pos << 16), neg2 = ep.code_neg | (ep.code_neg << 16);
    const auto srs = __builtin_amdgcn_make_buffer_rsrc(st.codes + d.tok_off * 14, 0, d.T * 28, 0x00020000);
    const auto drs = __builtin_amdgcn_make_buffer_rsrc(static_cast<Code*>(out.codes) + base * 14, 0,
                                                       d.k * 14 * (int)sizeof(Code), 0x00020000);
    const int n = d.k * 7;
    for (int e0 = tid; e0 < n; e0 += kSortBS * kCU) {
      uint32_t v[kCU];
#pragma unroll
      for (int u = 0; u < kCU; ++u) {
        const int e = e0 + kSortBS * u;
        const int t = min(e / 7, d.k - 1), q = e - (e / 7) * 7;
        v[u] = __builtin_amdgcn_raw_buffer_load_b32(srs, (spos[t] * 7 + q) * 4, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < kCU; ++u) {
        const int e = e0 + kSortBS * u;
        const uint32_t c2 = (uint32_t)lfq_index_bits(v[u], pos2, neg2);
        // write-once outputs: nontemporal stores (their lines leave the L2 /
        // Infinity Cache early instead of being written back under the next
        // step's row kernel: sort 0.146 -> 0.143 ms, next rows 1.13 -> 1.11 ms)
        if constexpr (sizeof(Code) == 8)
          __builtin_amdgcn_raw_buffer_store_b128((v4u32){c2 & 0xFFFFu, 0u, c2 >> 16, 0u}, drs,
                                                 e < n ? e * 16 : 0x7ffffff0, 0, 2);
        else   // int16: the masked u32 is the two final codes (a 4-byte store: dctae_codes16.h's alignment rule)
          __builtin_amdgcn_raw_buffer_store_b32(c2, drs, e < n ? e * 4 : 0x7ffffff0, 0, 2);
      }
    }
  } else if (out.codes) {
    // any ncb: one u16 -> one int64 per lane, kCU gathers in flight (as above)
    constexpr int kCU = 16;
    const int ncb = ep.ncb, n = d.k * ncb;
    const auto srs = __builtin_amdgcn_make_buffer_rsrc(st.codes + d.tok_off * ncb, 0, d.T * ncb * 2, 0x00020000);
    const auto drs = __builtin_amdgcn_make_buffer_rsrc(static_cast<Code*>(out.codes) + base * ncb, 0,
                                                       n * (int)sizeof(Code), 0x00020000);
    for (int e0 = tid; e0 < n; e0 += kSortBS * kCU) {
      uint32_t v[kCU];
#pragma unroll
      for (int u = 0; u < kCU; ++u) {
        const int e = e0 + kSortBS * u;
        const int t = min(e / ncb, d.k - 1), q = e - (e / ncb) * ncb;
        v[u] = __builtin_amdgcn_raw_buffer_load_b16(srs, (spos[t] * ncb + q) * 2, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < kCU; ++u) {
        const int e = e0 + kSortBS * u;
        const uint32_t cv = (uint32_t)lfq_index_bits(v[u], ep.code_pos, ep.code_neg);
        if constexpr (sizeof(Code) == 8)
          __builtin_amdgcn_raw_buffer_store_b64((v2u32s){cv, 0u}, drs, e < n ? e * 8 : 0x7ffffff0, 0, 2);
        else   // int16: two bytes per code, rows at any 2-byte alignment (ncb odd)
          __builtin_amdgcn_raw_buffer_store_b16((uint16_t)cv, drs, e < n ? e * 2 : 0x7ffffff0, 0, 2);
      }
    }
  }
  if (out.patches || out.raw) gather_tokens(d, spos, base, PP, st, out, tid, kSortBS);
}

template <typename Code>
static void launch_sort_pack_t(const ImgDesc* imgs, int n_img, int np2, const EncParams& ep, const TokenSinks& st,
                               const PackSinks& out, hipStream_t s, int kernel, int max_T) {
  // 224^2 images (768 tokens): a quarter-size block (a full one sorted 3072
  // padded keys per image)
  if (kernel == 2 && max_T <= 256 * 3)
    hipLaunchKernelGGL((k_sort_pack2<256, 3, Code>), dim3(n_img), dim3(256), 0, s, imgs, ep, st, out);
  else if (kernel == 2 && max_T <= 512 * 6)
    hipLaunchKernelGGL((k_sort_pack2<512, 6, Code>), dim3(n_img), dim3(512), 0, s, imgs, ep, st, out);
  else
    hipLaunchKernelGGL(k_sort_pack<Code>, dim3(n_img), dim3(1024), (size_t)np2 * 8, s, imgs, np2, ep, st, out);
}

// pad positions j >= row_len[r] of each packed row: the reference pads
// patches with zeros (util.py:149-164), ids/pos/ch with 0 and then runs
// PatchNorm/LFQ on them like on any token (c = h = w = 0).
template <typename Code>
__global__ void k_pad_fill(const int32_t* __restrict__ row_len, int n_rows, EncParams ep, uint8_t* key_pad,
                           PackSinks out) {
  // the pad token (zeros at c = h = w = 0) normalises and quantises the same
  // at every pad position: its patch and codes once per block, in LDS
  __shared__ float pp[kMaxP * kMaxP];
  __shared__ int64_t pcode[kMaxCodebooks];
  const int r = blockIdx.y;
  const int S = ep.S, PP = ep.P * ep.P;
  const int len = row_len[r];
  if ((int)(blockIdx.x * blockDim.x) + (int)blockDim.x <= len) {   // no pads in this block's span
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < S; j += gridDim.x * blockDim.x)
      key_pad[(int64_t)r * S + j] = 0;
    if (gridDim.x * blockDim.x >= (unsigned)S) return;
  }
  if (out.patches || out.codes) {
    for (int e = threadIdx.x; e < PP; e += blockDim.x)
      pp[e] = pn_forward(0.0f, ep.median[e], ep.b[e], ep.eps, ep.min_val, ep.max_val);
    __syncthreads();
    if (out.codes)
      for (int q = threadIdx.x; q < ep.ncb; q += blockDim.x) {
        uint32_t code = 0;
        for (int dd = 0; dd < ep.cb_dim; ++dd) code |= (pp[q * ep.cb_dim + dd] > 0.0f ? 1u : 0u) << (ep.cb_dim - 1 - dd);
        pcode[q] = (int64_t)lfq_index_bits(code, ep.code_pos, ep.code_neg);
      }
    __syncthreads();
  }
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < S; j += gridDim.x * blockDim.x) {
    const int64_t o = (int64_t)r * S + j;
    key_pad[o] = (j >= len) ? 1 : 0;
    if (j < len) continue;
    out.pos[2 * o] = 0;
    out.pos[2 * o + 1] = 0;
    out.ch[o] = 0;
    out.ids[o] = 0;
    if (out.scores) out.scores[o] = 0.0f;
    if (out.raw)
      for (int e = 0; e < PP; ++e) out.raw[o * PP + e] = 0.0f;
    if (out.patches)
      for (int e = 0; e < PP; ++e) out.patches[o * PP + e] = pp[e];
    if (out.codes)
      for (int q = 0; q < ep.ncb; ++q) static_cast<Code*>(out.codes)[o * ep.ncb + q] = (Code)pcode[q];
  }
}

template <typename Code>
static void launch_pad_fill_t(const int32_t* row_len, int n_rows, const EncParams& ep, uint8_t* key_pad,
                              const PackSinks& out, hipStream_t s) {
  int gx = (ep.S + 255) / 256;
  hipLaunchKernelGGL(k_pad_fill<Code>, dim3(gx, n_rows), dim3(256), 0, s, row_len, n_rows, ep, key_pad, out);
}

// dctae_codes16.hip: the int16 instantiations
void launch_sort_pack_c16(const ImgDesc* imgs, int n_img, int np2, const EncParams& ep, const TokenSinks& st,
                          const PackSinks& out, hipStream_t s, int kernel, int max_T);
void launch_pad_fill_c16(const int32_t* row_len, int n_rows, const EncParams& ep, uint8_t* key_pad,
                         const PackSinks& out, hipStream_t s);

}  // namespace dctae
