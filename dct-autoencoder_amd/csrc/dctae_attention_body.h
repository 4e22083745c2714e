// The body of the attention kernels of dctae_model.hip, as text: included once
// into k_attention<LSE> and once into k_attention_varlen.  (A __device__
// function inlined into both compiles k_attention to other instructions than
// the kernel it was, in every form that was tried; the text included into the
// kernel itself does not: tools/isa_same.py)  The
// including kernel provides
//   AttnArgs a;  constexpr bool LSE, VARLEN;
//   const int64_t* seq_start;  const int32_t* seq_len;   (null unless VARLEN)
//
// The body reaches its row through two scalars only, the row's first token
// `rowbase` and its length `S`: k_attention takes them from the grid
// (rowbase = b S), k_attention_varlen from a table (sequence b is the token
// rows [seq_start[b], seq_start[b] + seq_len[b]) of a flat stream).  VARLEN has
// no bias term (a one-image unpadded row's mask adds 0) and no LSE, and never
// reads ids / key_pad; the arithmetic is the padded kernel's on a row without
// pad keys, so a sequence's rows equal that kernel's at R = 1, S = len bit for
// bit.  Loads are clamped to the sequence (min(k0 + key, S - 1)), so no row
// outside it is read, and only rows q < S are written.
  __shared__ __attribute__((aligned(16))) uint16_t Ks[AK * ASTR];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[AK * AVS];   // row-major; read transposed (ds_read_b64_tr_b16)
  __shared__ __attribute__((aligned(16))) int32_t kid[AK];   // key image id, or -1 for a non-pad key (no bias)
  __shared__ __attribute__((aligned(16))) uint16_t Os[AQ * ASTR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = VARLEN ? seq_len[blockIdx.z] : a.S, D = a.heads * AD;
  const int q0 = blockIdx.x * AQ, h = blockIdx.y, b = blockIdx.z;
  if (VARLEN && q0 >= S) return;   // before the first barrier: the whole block leaves
  const int64_t rowbase = VARLEN ? seq_start[b] : (int64_t)b * S;
  const int64_t ld = 3ll * D;
  const uint16_t* qkv = a.qkv;
  // this lane's query and its Q fragments (B operand: Q[q][d kk*16 + 8 (l/32) ..])
  const int ql = q0 + wave * 32 + (lane & 31);
  const int qc = min(ql, S - 1);
  bf16x8 qf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
    qf[kk] = *reinterpret_cast<const bf16x8*>(qkv + (rowbase + qc) * ld + h * AD + kk * 16 + (lane >> 5) * 8);
  const int32_t my_id = VARLEN ? 0 : (int32_t)a.ids[rowbase + qc];
  const float sc = a.scale * 1.4426950408889634f;   // logits in log2 units
  const float bias2 = 1.4426950408889634f;           // +1.0 bias in log2 units
  f32x16 o[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) o[t][v] = 0.0f;
  float mrun = -INFINITY, lsum = 0.0f;
  for (int k0 = 0; k0 < S; k0 += AK) {
    __syncthreads();   // previous block's K / V reads done
    // stage K and V rows: 64 keys x 64 d, 16 B per load (two per thread each)
#pragma unroll
    for (int j = 0; j < AK * 8 / ATH; ++j) {
      const int idx = tid + ATH * j, key = idx >> 3, seg = idx & 7;
      const int kg = min(k0 + key, S - 1);
      const uint16_t* src = qkv + (rowbase + kg) * ld + h * AD + seg * 8;
      const uint4 kv = *reinterpret_cast<const uint4*>(src + D);
      const uint4 vv = *reinterpret_cast<const uint4*>(src + 2 * D);
      *reinterpret_cast<uint4*>(Ks + key * ASTR + seg * 8) = kv;
      *reinterpret_cast<uint4*>(Vs + key * AVS + seg * 8) = vv;
    }
    bool pad = false;
    if (!VARLEN && tid < AK) {
      const int kg = k0 + tid;
      pad = kg < S && a.key_pad[rowbase + kg];
      kid[tid] = pad ? (int32_t)a.ids[rowbase + kg] : -1;
    }
    // block-uniform: the +1 bias only ever hits pad keys (VARLEN: the barrier alone)
    const bool any_pad = VARLEN ? (__syncthreads(), false) : (bool)__syncthreads_or(pad);
    // S^T tiles
    f32x16 st[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int v = 0; v < 16; ++v) st[t][v] = 0.0f;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + (t * 32 + (lane & 31)) * ASTR + kk * 16 + (lane >> 5) * 8);
        st[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], st[t], 0, 0, 0);
      }
    }
    // scale + bias, block max over the 64 keys of this query (lanes l and l ^ 32).
    // Without pad keys in the block the logits stay unscaled (sce = sc) and the
    // scale is applied inside the exponent's FMA; with pad keys they are scaled
    // and biased here (sce = 1).
    float bm = -INFINITY;
    float sce = sc;
    if (any_pad) {
      sce = 1.0f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const int4 ki = *reinterpret_cast<const int4*>(kid + t * 32 + 8 * q4 + 4 * (lane >> 5));
          st[t][4 * q4 + 0] = st[t][4 * q4 + 0] * sc + (ki.x == my_id ? bias2 : 0.0f);
          st[t][4 * q4 + 1] = st[t][4 * q4 + 1] * sc + (ki.y == my_id ? bias2 : 0.0f);
          st[t][4 * q4 + 2] = st[t][4 * q4 + 2] * sc + (ki.z == my_id ? bias2 : 0.0f);
          st[t][4 * q4 + 3] = st[t][4 * q4 + 3] * sc + (ki.w == my_id ? bias2 : 0.0f);
        }
    }
    if (k0 + AK > S) {   // last, partial key block
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v)
          if (k0 + t * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3) >= S) st[t][v] = -INFINITY;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) bm = fmaxf(bm, st[t][v]);
    {
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(bm), __float_as_uint(bm), false, false);
      bm = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1])) * sce;
    }
    // lazy rescale: the reference max moves only when the block max exceeds it
    // by more than 8 (log2 units), so p = 2^(s - m) <= 2^8 stays exact in fp32
    // and in range for bf16; O and the sum always share the same m, so the
    // normalised result is unchanged.  The O rescale (AGPR round trip) runs
    // only when some lane moved its max.
    if (bm > mrun + 8.0f) {
      const float alpha = __builtin_amdgcn_exp2f(mrun - bm);   // 0 on the first block (mrun = -inf)
      mrun = bm;
      lsum *= alpha;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) o[t][v] *= alpha;
    }
    const float nm = -mrun;
    // P (bf16) in B-operand order: key step kk = (tile kk / 2, quarters 2 (kk % 2), +1)
    bf16x8 pf[4];
    float ls2[2] = {0.0f, 0.0f};   // two partial sums (pairs for packed adds)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int t = kk >> 1, v0 = 8 * (kk & 1);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        // raw v_exp_f32: exp2f's denormal-range fix-up (5 VALU ops per call)
        // is not needed (results below 2^-126 are negligible probabilities)
        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[t][v0 + e], sce, nm));
        ls2[e & 1] += p;
        pf[kk][e] = (__bf16)p;
      }
    }
    lsum += ls2[0] + ls2[1];
    // O^T += V^T P^T; the A fragment V^T[d = 32 dt + lane % 32][keys kb + (0..3), kb + 8 + (0..3)] comes
    // from the row-major V tile by two transposed reads: lane 4q + p of each 16-lane group addresses key
    // row kb + q, columns 4p .. 4p + 3 of the group's 16 d columns, and receives its own column
    typedef short s4 __attribute__((ext_vector_type(4)));
    const int gq = (lane & 15) >> 2, gp = lane & 3, gx = (lane >> 4) & 1;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int kb = 32 * (kk >> 1) + 8 * (2 * (kk & 1)) + 4 * (lane >> 5);
        const uint16_t* vr = Vs + (kb + gq) * AVS + 32 * dt + 16 * gx + 4 * gp;
        const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)vr);
        const s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(vr + 8 * AVS));
        bf16x8 vf;
        short* vsh = reinterpret_cast<short*>(&vf);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          vsh[e] = lo[e];
          vsh[4 + e] = hi[e];
        }
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[kk], o[dt], 0, 0, 0);
      }
  }
  // normalise: the query's sum is split over lanes l and l ^ 32
  {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(lsum), __float_as_uint(lsum), false, false);
    lsum = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
  }
  const float inv = 1.0f / lsum;
  if (LSE && lane < 32 && ql < S) a.lse[((int64_t)b * a.heads + h) * S + ql] = mrun + __log2f(lsum);
  // O^T[d = 32 dt + 8 (v/4) + 4 (l/32) + v%4][query l%32] -> Os[query][d] -> coalesced rows
  const int qr = wave * 32 + (lane & 31);
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int d = 32 * dt + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
      Os[qr * ASTR + d] = f2bf(o[dt][v] * inv);
    }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < AQ * 8 / ATH; ++j) {
    const int idx = tid + ATH * j, r = idx >> 3, seg = idx & 7;
    if (q0 + r < S)
      *reinterpret_cast<uint4*>(a.out + (rowbase + q0 + r) * (int64_t)a.ldo + h * AD + seg * 8) =
          *reinterpret_cast<const uint4*>(Os + r * ASTR + seg * 8);
  }
