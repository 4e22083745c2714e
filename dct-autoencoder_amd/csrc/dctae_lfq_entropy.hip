// LFQ training losses (lfq.py:189-204 commit loss, util.py:355-387 entropy
// loss) and the entropy loss's gradient, without the dense distance tensor.
//
// The codebook is {-s, +s}^d, so the reference's softmax over the 2^d codes of
// one (token, codebook) row factorises over the d bits:
//   p_rj = prod_dd pi_r,dd(b_j,dd),  pi(+1) = sigmoid(u), pi(-1) = sigmoid(-u),
//   u = -4 s h / T
// (the reference's logit puts the mass on the FARTHEST code; kept).  With the
// bits split into a high group (hi = ceil(d / 2) bits, dimension 0 = MSB) and a
// low group (lo = d - hi), p_r = A_r (x) B_r, and
//   avg_probs = 1 / (M c) sum_r A_r (x) B_r
// is a (2^hi x rows) . (rows x 2^lo) GEMM on the exact-fp32 MFMA.  The
// backward is the two transposed products V_r = A_r^T G, U_r = G B_r against
// G = d avg_entropy / d avg_probs, and a per-row contraction that forms every
// product WITHOUT its own bit (never p / pi: pi is exactly 0 or 1 in fp32 for
// ordinary inputs at T = 0.01).
//
// Determinism: every block owns a fixed contiguous range of rows, partial
// histograms and sums go to the workspace and are reduced in a fixed order;
// no floating-point atomics.  Values of masked-out tokens are never read.
#include "dctae_launch.h"

namespace dctae {
namespace {

constexpr int kRows = 32;        // rows ((token, codebook) pairs) per chunk: the MFMA's k (forward) / m (backward)
constexpr int kThreads = 256;    // 4 waves
constexpr int kTile = 128;       // forward: histogram tile edge of one block (4 waves x 32 high codes, 4 x 32 low codes)
constexpr int kMinChunks = 4;    // a block takes at least this many chunks before the grid grows
constexpr int kMaxBlocks = 512;  // row blocks (partial histograms in the workspace)
constexpr int kMaxD = 16;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct RowPi {                  // odd row stride: lanes that differ in the row hit different banks
  float pp[kRows][kMaxD + 1];   // pi(+1) = sigmoid(u)
  float pm[kRows][kMaxD + 1];   // pi(-1) = sigmoid(-u)
  float u[kRows][kMaxD + 1];
  int valid[kRows];
};

struct Geo {
  int d, hi, lo, NH, NL, NHp, NLp;   // NHp / NLp: padded to the 32-wide MFMA tile
};

__host__ __device__ inline Geo geo(int d) {
  Geo g;
  g.d = d;
  g.hi = (d + 1) / 2;
  g.lo = d - g.hi;
  g.NH = 1 << g.hi;
  g.NL = 1 << g.lo;
  g.NHp = g.NH < 32 ? 32 : g.NH;
  g.NLp = g.NL < 32 ? 32 : g.NL;
  return g;
}

__device__ inline float softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }

// pi(+-1) of the chunk's rows into LDS; FWD: also this thread's share of the
// binary entropies, the commit loss's squared errors and the token count
template <bool FWD>
__device__ inline void chunk_pi(RowPi& sm, const float* __restrict__ h, const uint8_t* __restrict__ mask, int64_t row0,
                                int64_t n_rows, int c, int d, float s, float T, int tid, float& hb, float& cm,
                                int& cnt) {
  for (int e = tid; e < kRows * d; e += kThreads) {
    const int r = e / d, dd = e - r * d;
    const int64_t row = row0 + r;
    bool ok = row < n_rows;
    if (ok) ok = mask[row / c] != 0;
    float pp = 0.0f, pm = 0.0f, u = 0.0f;
    if (ok) {
      const float hv = h[row * d + dd];
      // the reference's fp32 ops: distance = -2 (h . (+-s)), logit = distance / T
      const float z = (2.0f * (hv * s)) / T;
      u = -2.0f * z;
      pp = 1.0f / (1.0f + expf(-u));
      pm = 1.0f / (1.0f + expf(u));
      if (FWD) {
        // Hb = -pi+ log pi+ - pi- log pi-, log pi(+-1) = -softplus(-+u)
        hb += pp * softplus(-u) + pm * softplus(u);
        const float q = hv > 0.0f ? s : -s;
        const float df = hv - q;
        cm += df * df;
      }
    }
    sm.pp[r][dd] = pp;
    sm.pm[r][dd] = pm;
    sm.u[r][dd] = u;
  }
  if (tid < kRows) {
    const int64_t row = row0 + tid;
    bool ok = row < n_rows;
    if (ok) ok = mask[row / c] != 0;
    sm.valid[tid] = ok ? 1 : 0;
    if (FWD && ok && row % c == 0) cnt += 1;
  }
}

// buf[r][jj] = prod_{dd < nb} pi_r,off+dd(bit nb-1-dd of j0 + jj), 0 for
// masked-out rows and for the padding codes j >= n.  One thread per (row, run
// of 16 codes): the product over the bits above the run, then the run's bits
// by doubling in registers (v[2 i + bit] = v[i] pi(bit), most significant bit
// first).  Adjacent threads take adjacent rows (odd LDS strides: conflict-free).
__device__ inline void build_group(float* buf, int ld, int width, int j0, int n, int nb, int off, const RowPi& sm,
                                   int tid) {
  const int lb = nb < 4 ? nb : 4;   // bits inside a run; nb < 4: the one run j = 0 holds all n = 2^nb codes
  for (int e = tid; e < kRows * (width >> 4); e += kThreads) {
    const int r = e % kRows, jj = (e / kRows) << 4;
    const int j = j0 + jj;
    const bool on = sm.valid[r] && j < n;
    float v[16];
    v[0] = 0.0f;
    if (on) {
      float base = 1.0f;
      for (int dd = 0; dd < nb - lb; ++dd) base *= ((j >> (nb - 1 - dd)) & 1) ? sm.pp[r][off + dd] : sm.pm[r][off + dd];
      v[0] = base;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      // the last lb levels double (dimension nb - 4 + t); the ones before them keep v[0] alone
      const bool lv = t >= 4 - lb;
      const int dd = off + (lv ? nb - 4 + t : 0);
      const float p1 = on ? sm.pp[r][dd] : 0.0f, p0 = on ? sm.pm[r][dd] : 0.0f;
#pragma unroll
      for (int i = (1 << t) - 1; i >= 0; --i) {
        const float x = v[i];
        v[2 * i + 1] = lv ? x * p1 : 0.0f;
        v[2 * i] = lv ? x * p0 : x;
      }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) buf[r * ld + jj + i] = v[i];
  }
}

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

// ---- forward ---------------------------------------------------------------
// grid (row blocks, histogram tiles): block (bx, by) accumulates the tile by
// of sum_r A_r (x) B_r over the chunks [bx cpb, (bx + 1) cpb) and writes it to
// part[bx]; the by = 0 blocks also write their entropy / commit / count sums.
// NT: 32-wide accumulators along the low codes of the block's tile (1, 2 or 4)
template <int NT>
__global__ __launch_bounds__(kThreads) void k_lfq_ent_fwd(const float* __restrict__ h,
                                                          const uint8_t* __restrict__ mask, int64_t n_rows,
                                                          int n_chunks, int cpb, int c, int d, float s, float T,
                                                          float* __restrict__ part, float* __restrict__ scf,
                                                          int* __restrict__ sci) {
  constexpr int LD = kTile + 1;
  __shared__ RowPi sm;
  __shared__ float A[kRows * LD];
  __shared__ float B[kRows * LD];
  __shared__ float redf[kThreads];
  __shared__ int redi[kThreads];
  const Geo g = geo(d);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, kh = lane >> 5;
  const int tilesL = (g.NLp + kTile - 1) / kTile;
  const int th0 = (blockIdx.y / tilesL) * kTile, tl0 = (blockIdx.y % tilesL) * kTile;
  const int THp = min(kTile, g.NHp - th0), TLp = 32 * NT;
  const bool sums = blockIdx.y == 0;
  f32x16 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = (f32x16)(0.0f);
  float hb = 0.0f, cm = 0.0f;
  int cnt = 0;
  const int ch0 = blockIdx.x * cpb, ch1 = min(n_chunks, ch0 + cpb);
  for (int ch = ch0; ch < ch1; ++ch) {
    const int64_t row0 = (int64_t)ch * kRows;
    if (sums)
      chunk_pi<true>(sm, h, mask, row0, n_rows, c, d, s, T, tid, hb, cm, cnt);
    else
      chunk_pi<false>(sm, h, mask, row0, n_rows, c, d, s, T, tid, hb, cm, cnt);
    __syncthreads();
    build_group(A, LD, THp, th0, g.NH, g.hi, 0, sm, tid);
    build_group(B, LD, TLp, tl0, g.NL, g.lo, g.hi, sm, tid);
    __syncthreads();
    if (32 * wave < THp) {
#pragma unroll
      for (int k0 = 0; k0 < kRows; k0 += 2) {
        // A operand: lane l holds [i = l & 31][k = l >> 5]; B operand: [k = l >> 5][j = l & 31]
        const float a = A[(k0 + kh) * LD + 32 * wave + l31];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          const float b = B[(k0 + kh) * LD + 32 * i + l31];
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  if (32 * wave < THp) {
    float* p = part + (size_t)blockIdx.x * g.NHp * g.NLp;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          // C/D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
          const int jh = th0 + 32 * wave + (q & 3) + 8 * (q >> 2) + 4 * kh;
          const int jl = tl0 + 32 * i + l31;
          p[(size_t)jh * g.NLp + jl] = acc[i][q];
        }
    }
  }
  if (sums) {
    const float hbs = block_sum(hb, redf, tid);
    const float cms = block_sum(cm, redf, tid);
    const int cs = block_sum(cnt, redi, tid);
    if (tid == 0) {
      scf[2 * blockIdx.x] = hbs;
      scf[2 * blockIdx.x + 1] = cms;
      sci[blockIdx.x] = cs;
    }
  }
}

// out[1] = sample_entropy, out[3] = commit_loss, out[4] = M (one block)
__global__ __launch_bounds__(kThreads) void k_lfq_ent_scalars(const float* __restrict__ scf,
                                                              const int* __restrict__ sci, int nbx, int c, int d,
                                                              float* __restrict__ out) {
  __shared__ float redf[kThreads];
  __shared__ int redi[kThreads];
  const int tid = threadIdx.x;
  float hb = 0.0f, cm = 0.0f;
  int cnt = 0;
  for (int b = tid; b < nbx; b += kThreads) {
    hb += scf[2 * b];
    cm += scf[2 * b + 1];
    cnt += sci[b];
  }
  const float hbs = block_sum(hb, redf, tid);
  const float cms = block_sum(cm, redf, tid);
  const int cs = block_sum(cnt, redi, tid);
  if (tid == 0) {
    const float M = (float)cs;   // M = 0: 0 / 0 = NaN, as the reference
    out[1] = hbs / M;
    out[3] = (cms / M) / (float)(c * d);
    out[4] = M;
  }
}

// avg_probs = sum of the partial histograms / M / c, in a fixed order: a block
// takes kHistJ codes; thread (q, jj) adds the partials b = q, q + kHistQ, ... of
// code jj, then the kHistQ sums are added in index order.  Each block writes
// its share of sum avg log(avg + eps).
constexpr int kHistJ = 32, kHistQ = kThreads / kHistJ;
__global__ __launch_bounds__(kThreads) void k_lfq_ent_hist(const float* __restrict__ part, int nbx, int c, int d,
                                                           float eps, const float* __restrict__ out,
                                                           float* __restrict__ avg, float* __restrict__ aep) {
  __shared__ float redf[kThreads];
  const Geo g = geo(d);
  const int tid = threadIdx.x, jj = tid % kHistJ, q = tid / kHistJ;
  const int j = blockIdx.x * kHistJ + jj;   // < NHp * NLp (a multiple of 32)
  const size_t stride = (size_t)g.NHp * g.NLp;
  float sum = 0.0f;
  for (int b = q; b < nbx; b += kHistQ) sum += part[b * stride + j];
  redf[tid] = sum;
  __syncthreads();
  float term = 0.0f;
  if (q == 0) {
    for (int i = 1; i < kHistQ; ++i) sum += redf[i * kHistJ + jj];
    const int jh = j / g.NLp, jl = j - jh * g.NLp;
    if (jh < g.NH && jl < g.NL) {
      const float a = (sum / out[4]) / (float)c;
      avg[jh * g.NL + jl] = a;
      term = a * logf(a + eps);
    }
  }
  const float t = block_sum(term, redf, tid);
  if (tid == 0) aep[blockIdx.x] = t;
}

// out[2] = avg_entropy, out[0] = sample_entropy - avg_entropy (one block)
__global__ __launch_bounds__(kThreads) void k_lfq_ent_finish(const float* __restrict__ aep, int n,
                                                             float* __restrict__ out) {
  __shared__ float redf[kThreads];
  const int tid = threadIdx.x;
  float v = 0.0f;
  for (int b = tid; b < n; b += kThreads) v += aep[b];
  const float t = block_sum(v, redf, tid);
  if (tid == 0) {
    const float ae = -t;
    out[2] = ae;
    out[0] = out[1] - ae;
  }
}

// ---- backward --------------------------------------------------------------
// G = d avg_entropy / d avg_probs as (NHp, NLp), zero in the padding, and its transpose
__global__ __launch_bounds__(kThreads) void k_lfq_ent_g(const float* __restrict__ avg, int d, float eps,
                                                        float* __restrict__ G, float* __restrict__ GT) {
  const Geo g = geo(d);
  const int j = blockIdx.x * kThreads + threadIdx.x;
  const int jh = j / g.NLp, jl = j - jh * g.NLp;
  float v = 0.0f;
  if (jh < g.NH && jl < g.NL) {
    const float a = avg[jh * g.NL + jl];
    v = -(logf(a + eps) + a / (a + eps));
  }
  G[(size_t)jh * g.NLp + jl] = v;
  GT[(size_t)jl * g.NHp + jh] = v;
}

// sum over the K bits of a group of v[bits] prod_L w(L, bit L): a binary tree
// over the code index, bit L of it weighted wp[L] (set) / wm[L] (clear)
template <int L, int K>
struct Node {
  static __device__ __forceinline__ float run(const float* v, int base, const float (&wp)[K], const float (&wm)[K]) {
    return fmaf(wp[L], Node<L - 1, K>::run(v, base | (1 << L), wp, wm), wm[L] * Node<L - 1, K>::run(v, base, wp, wm));
  }
};
template <int K>
struct Node<-1, K> {
  static __device__ __forceinline__ float run(const float* v, int base, const float (&)[K], const float (&)[K]) {
    return v[base];
  }
};

// D = sum_j v[j] b_j,pos prod_{L != pos} pi_L(bit L of j): the bit at `pos`
// (counted from the LSB) takes the weights +1 / -1 in place of its pi, so its
// own factor never enters the product.  pp / pm: the group's K dimensions,
// MSB first.
template <int K>
__device__ inline float contract(const float* v, const float* pp, const float* pm, int pos) {
  float wp[K], wm[K];
#pragma unroll
  for (int L = 0; L < K; ++L) {
    wp[L] = L == pos ? 1.0f : pp[K - 1 - L];
    wm[L] = L == pos ? -1.0f : pm[K - 1 - L];
  }
  return Node<K - 1, K>::run(v, 0, wp, wm);
}

__device__ inline float contract_k(int K, const float* v, const float* pp, const float* pm, int pos) {
  switch (K) {
    case 1: return contract<1>(v, pp, pm, pos);
    case 2: return contract<2>(v, pp, pm, pos);
    case 3: return contract<3>(v, pp, pm, pos);
    case 4: return contract<4>(v, pp, pm, pos);
    case 5: return contract<5>(v, pp, pm, pos);
    case 6: return contract<6>(v, pp, pm, pos);
    case 7: return contract<7>(v, pp, pm, pos);
    default: return contract<8>(v, pp, pm, pos);
  }
}

// dynamic LDS: bufA[kRows][NHp + 1] | bufB[kRows][NHp + 1] | RowPi | GL: G[NHp][NLp + 1]
// GL (d <= 14): the block keeps G in LDS for all its chunks, one copy with an
// odd stride serving both products; else G and G^T stream from L2
template <bool GL>
__global__ __launch_bounds__(kThreads, 2) void k_lfq_ent_bwd(const float* __restrict__ h,
                                                          const uint8_t* __restrict__ mask, int64_t n_rows,
                                                          int n_chunks, int cpb, int c, int d, float s, float T,
                                                          const float* __restrict__ G, const float* __restrict__ GT,
                                                          const float* __restrict__ out,
                                                          const float* __restrict__ gup, float* __restrict__ dh) {
  extern __shared__ float lds[];
  const Geo g = geo(d);
  const int LD = g.NHp + 1;
  float* bufA = lds;
  float* bufB = lds + kRows * LD;
  RowPi& sm = *reinterpret_cast<RowPi*>(lds + 2 * kRows * LD);
  float* gl = lds + 2 * kRows * LD + sizeof(RowPi) / sizeof(float);
  const int LDG = g.NLp + 1;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, kh = lane >> 5;
  const int nV = g.NLp / 32, nU = g.NHp / 32;   // 32 x 32 subtiles of V (rows x low codes) and U (rows x high codes)
  if (GL)   // visible after the chunk loop's first barrier
    for (int e = tid; e < g.NHp * g.NLp; e += kThreads) gl[(e / g.NLp) * LDG + e % g.NLp] = G[e];
  const float M = out[4];
  const float k4 = -(4.0f * s) / T;             // du / dh
  const float up = gup[0];
  float f0 = 0.0f, f1 = 0.0f;
  int i0 = 0;
  const int ch0 = blockIdx.x * cpb, ch1 = min(n_chunks, ch0 + cpb);
  for (int ch = ch0; ch < ch1; ++ch) {
    const int64_t row0 = (int64_t)ch * kRows;
    chunk_pi<false>(sm, h, mask, row0, n_rows, c, d, s, T, tid, f0, f1, i0);
    __syncthreads();
    build_group(bufA, LD, g.NHp, 0, g.NH, g.hi, 0, sm, tid);
    build_group(bufB, LD, g.NLp, 0, g.NL, g.lo, g.hi, sm, tid);
    __syncthreads();
    // V = A^T G (k = high codes), U = B G^T (k = low codes); wave w: subtiles w, w + 4, ...
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[i] = (f32x16)(0.0f);
      const int t = wave + 4 * i;
      if (t < nV + nU) {
        const bool isV = t < nV;
        const int n0 = 32 * (isV ? t : t - nV);
        const int K = isV ? g.NHp : g.NLp;
        const float* src = (isV ? bufA : bufB) + l31 * LD + kh;
        // B operand [k = l >> 5][j = l & 31]: V: G[k][n0 + j]; U: G[n0 + j][k]
        if (GL) {
          const float* gm = isV ? gl + kh * LDG + n0 + l31 : gl + (n0 + l31) * LDG + kh;
          const int gs = isV ? LDG : 1;
          for (int kb = 0; kb < K; kb += 16)   // K is a multiple of 32; 8 operand pairs in flight
#pragma unroll
            for (int k0 = kb; k0 < kb + 16; k0 += 2)
              acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(src[k0], gm[k0 * gs], acc[i], 0, 0, 0);
        } else {
          const int ldg = isV ? g.NLp : g.NHp;
          const float* gm = (isV ? G : GT) + (size_t)kh * ldg + n0 + l31;
          for (int kb = 0; kb < K; kb += 16)
#pragma unroll
            for (int k0 = kb; k0 < kb + 16; k0 += 2)
              acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(src[k0], gm[(size_t)k0 * ldg], acc[i], 0, 0, 0);
        }
      }
    }
    __syncthreads();
    // V over bufA, U over bufB (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), column = lane & 31)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = wave + 4 * i;
      if (t < nV + nU) {
        const bool isV = t < nV;
        float* dst = (isV ? bufA : bufB) + 32 * (isV ? t : t - nV) + l31;
#pragma unroll
        for (int q = 0; q < 16; ++q) dst[((q & 3) + 8 * (q >> 2) + 4 * kh) * LD] = acc[i][q];
      }
    }
    __syncthreads();
    for (int e = tid; e < kRows * d; e += kThreads) {
      const int dd = e / kRows, r = e - dd * kRows;   // a wave's lanes share the dimension (two per wave)
      const int64_t row = row0 + r;
      if (row >= n_rows) continue;
      float gr = 0.0f;   // masked-out tokens: exact zeros
      if (sm.valid[r]) {
        float D;
        if (dd < g.hi)
          D = contract_k(g.hi, bufB + r * LD, &sm.pp[r][0], &sm.pm[r][0], g.hi - 1 - dd);
        else
          D = contract_k(g.lo, bufA + r * LD, &sm.pp[r][g.hi], &sm.pm[r][g.hi], g.lo - 1 - (dd - g.hi));
        const float ppm = sm.pp[r][dd] * sm.pm[r][dd];
        // d sample_entropy / dh = (1 / M) (-u) pi+ pi- du/dh;  d avg_entropy / dh = (1 / (M c)) pi+ pi- D du/dh
        const float se = (-sm.u[r][dd]) / M;
        const float ae = (D / M) / (float)c;
        gr = up * (k4 * (ppm * (se - ae)));
      }
      dh[row * d + dd] = gr;
    }
    __syncthreads();
  }
}

// ---- project_out of the training forward, in a fixed summation order --------
// out[t][o] = (sum_k x[t][k] w[o][k], one fmaf per term, k ascending from 0) + b[o]:
// the order of a plain loop, so the result does not depend on a GEMM library's
// blocking and is the same on every device.  wt = w^T (K, D): lanes read
// consecutive outputs.  A block takes kLinTok tokens, their x rows in LDS.
constexpr int kLinTok = 16, kLinMaxK = 512;
__global__ __launch_bounds__(kThreads) void k_linear_ordered(const float* __restrict__ x, int64_t n, int K,
                                                             const float* __restrict__ wt,
                                                             const float* __restrict__ b, int D,
                                                             float* __restrict__ out) {
  __shared__ float xs[kLinTok * kLinMaxK];
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * kLinTok;
  for (int e = tid; e < kLinTok * K; e += kThreads) {
    const int t = e / K, k = e - t * K;
    xs[t * K + k] = t0 + t < n ? x[(t0 + t) * K + k] : 0.0f;
  }
  __syncthreads();
  for (int o = tid; o < D; o += kThreads) {
    float acc[kLinTok];
#pragma unroll
    for (int t = 0; t < kLinTok; ++t) acc[t] = 0.0f;
    for (int k = 0; k < K; ++k) {
      const float w = wt[(size_t)k * D + o];
#pragma unroll
      for (int t = 0; t < kLinTok; ++t) acc[t] = fmaf(xs[t * K + k], w, acc[t]);
    }
    const float bo = b ? b[o] : 0.0f;
#pragma unroll
    for (int t = 0; t < kLinTok; ++t)
      if (t0 + t < n) out[(t0 + t) * D + o] = acc[t] + bo;
  }
}

void chunking(int64_t n_rows, int* n_chunks, int* cpb, int* nbx) {
  const int64_t nc = std::max<int64_t>(1, (n_rows + kRows - 1) / kRows);
  int64_t per = std::max<int64_t>(kMinChunks, (nc + kMaxBlocks - 1) / kMaxBlocks);
  per = std::min(per, nc);
  *n_chunks = (int)nc;
  *cpb = (int)per;
  *nbx = (int)((nc + per - 1) / per);
}

}  // namespace

bool lfq_entropy_supported(int d, int c, int64_t n_tok) {
  return d >= 1 && d <= kMaxD && c >= 1 && c <= 32 && n_tok >= 0 && n_tok * c / kRows < (int64_t)INT32_MAX;
}

size_t lfq_entropy_fwd_ws_floats(int64_t n_tok, int c, int d) {
  const Geo g = geo(d);
  int nch, cpb, nbx;
  chunking(n_tok * c, &nch, &cpb, &nbx);
  const size_t hist = (size_t)g.NHp * g.NLp;
  return (size_t)nbx * hist + 3 * (size_t)nbx + hist / kHistJ;
}

void launch_lfq_entropy_fwd(const float* h, const uint8_t* mask, int64_t n_tok, int c, int d, float s, float T,
                            float eps, float* ws, float* avg, float* out, hipStream_t st) {
  const Geo g = geo(d);
  int nch, cpb, nbx;
  chunking(n_tok * c, &nch, &cpb, &nbx);
  const size_t hist = (size_t)g.NHp * g.NLp;
  float* part = ws;
  float* scf = part + (size_t)nbx * hist;
  int* sci = reinterpret_cast<int*>(scf + 2 * (size_t)nbx);
  float* aep = scf + 3 * (size_t)nbx;
  const int tiles = ((g.NHp + kTile - 1) / kTile) * ((g.NLp + kTile - 1) / kTile);
  const int nrb = (int)(hist / kHistJ);
  const dim3 grid(nbx, tiles);
  const int nt = std::min(kTile, g.NLp) / 32;   // every tile of a histogram has the same width
  if (nt == 1)
    k_lfq_ent_fwd<1><<<grid, kThreads, 0, st>>>(h, mask, n_tok * c, nch, cpb, c, d, s, T, part, scf, sci);
  else if (nt == 2)
    k_lfq_ent_fwd<2><<<grid, kThreads, 0, st>>>(h, mask, n_tok * c, nch, cpb, c, d, s, T, part, scf, sci);
  else
    k_lfq_ent_fwd<4><<<grid, kThreads, 0, st>>>(h, mask, n_tok * c, nch, cpb, c, d, s, T, part, scf, sci);
  k_lfq_ent_scalars<<<1, kThreads, 0, st>>>(scf, sci, nbx, c, d, out);
  k_lfq_ent_hist<<<nrb, kThreads, 0, st>>>(part, nbx, c, d, eps, out, avg, aep);
  k_lfq_ent_finish<<<1, kThreads, 0, st>>>(aep, nrb, out);
}

size_t lfq_entropy_bwd_ws_floats(int d) {
  const Geo g = geo(d);
  return 2 * (size_t)g.NHp * g.NLp;
}

int launch_lfq_entropy_bwd(const float* h, const uint8_t* mask, int64_t n_tok, int c, int d, float s, float T,
                           float eps, const float* avg, const float* out, const float* gup, float* ws, float* dh,
                           hipStream_t st) {
  const Geo g = geo(d);
  int nch, cpb, nbx;
  chunking(n_tok * c, &nch, &cpb, &nbx);
  const size_t hist = (size_t)g.NHp * g.NLp;
  float* G = ws;
  float* GT = ws + hist;
  const bool gl = d <= 14;   // G in LDS: up to 66 KB (d = 14) beside the 39 KB of buffers
  const size_t lds = (size_t)2 * kRows * (g.NHp + 1) * sizeof(float) + sizeof(RowPi) +
                     (gl ? (size_t)g.NHp * (g.NLp + 1) * sizeof(float) : 0);
  // above the 64 KB default (d = 13 ... 16), of the CU's 160 KB; per device, so set on every such call
  const void* fn = gl ? (const void*)k_lfq_ent_bwd<true> : (const void*)k_lfq_ent_bwd<false>;
  if (lds > 48 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return 1;
  }
  k_lfq_ent_g<<<(int)(hist / kThreads), kThreads, 0, st>>>(avg, d, eps, G, GT);
  if (gl)
    k_lfq_ent_bwd<true><<<nbx, kThreads, lds, st>>>(h, mask, n_tok * c, nch, cpb, c, d, s, T, G, GT, out, gup, dh);
  else
    k_lfq_ent_bwd<false><<<nbx, kThreads, lds, st>>>(h, mask, n_tok * c, nch, cpb, c, d, s, T, G, GT, out, gup, dh);
  return 0;
}

bool linear_ordered_supported(int K, int D) { return K >= 1 && K <= kLinMaxK && D >= 1; }

void launch_linear_ordered(const float* x, int64_t n, int K, const float* wt, const float* b, int D, float* out,
                           hipStream_t st) {
  const int64_t blocks = (n + kLinTok - 1) / kLinTok;
  k_linear_ordered<<<(unsigned)blocks, kThreads, 0, st>>>(x, n, K, wt, b, D, out);
}

}  // namespace dctae
