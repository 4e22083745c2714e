// Progressive decode through the transformer (include/dctae_model_prefix.h):
// the entry points of the variable-length attention (the kernel is
// k_attention_varlen of dctae_model.hip, the body of k_attention with its two
// row scalars read from a table) and the prefix token gather.
//
// A model prefix frame is (row, image id, m): the first m real tokens of one
// image of a packed batch, as a sequence of its own in a flat token stream.
// k_prefix_tokens copies them there: one block per frame scans the row's S
// slots for the predicate ids == id && !key_pad (ballot per wave, the wave
// totals through LDS) and the token of rank r < m goes to flat row start + r.
#include "dctae_ctx.h"
#include "dctae_model.h"
#include "../../include/dctae_model_prefix.h"

using namespace dctae;

namespace dctae {

constexpr int PGT = 256;   // threads of k_prefix_tokens: slots per scan step

__global__ __launch_bounds__(PGT) void k_prefix_tokens(PrefixGatherArgs a) {
  __shared__ int wtot[PGT / 64];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = a.frame_m[f];
  const int64_t id = a.frame_id[f], rowbase = (int64_t)a.frame_row[f] * a.S, dst0 = a.frame_start[f];
  int base = 0;   // real tokens of the image at slots below j0 (block-uniform)
  for (int j0 = 0; j0 < a.S && base < m; j0 += PGT) {
    const int j = j0 + tid;
    const bool mine = j < a.S && a.ids[rowbase + j] == id && !a.key_pad[rowbase + j];
    const unsigned long long bal = __ballot(mine);
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int rank = base + __popcll(bal & ((1ull << lane) - 1ull));
    int total = 0;
#pragma unroll
    for (int w = 0; w < PGT / 64; ++w) {
      if (w < wave) rank += wtot[w];
      total += wtot[w];
    }
    __syncthreads();   // wtot is rewritten by the next step
    if (mine && rank < m) {
      const int64_t src = rowbase + j, dst = dst0 + rank;
      a.out_ch[dst] = a.ch[src];
      a.out_pos[2 * dst] = a.pos[2 * src];
      a.out_pos[2 * dst + 1] = a.pos[2 * src + 1];
      for (int c = 0; c < a.ncb; ++c)
        a.out_codes[dst * a.ncb + c] = a.codes16 ? (int64_t) reinterpret_cast<const int16_t*>(a.codes)[src * a.ncb + c]
                                                 : reinterpret_cast<const int64_t*>(a.codes)[src * a.ncb + c];
    }
    base += total;
  }
}

void launch_prefix_tokens(const PrefixGatherArgs& a, int n_frames, hipStream_t s) {
  if (n_frames > 0) hipLaunchKernelGGL(k_prefix_tokens, dim3(n_frames), dim3(PGT), 0, s, a);
}

}  // namespace dctae

extern "C" {

int dctae_model_attention_varlen(dctae_ctx* ctx, int32_t n_seq, int32_t max_len, int32_t heads, int32_t head_dim,
                                 const uint16_t* qkv, const int64_t* seq_start, const int32_t* seq_len, uint16_t* out,
                                 int64_t ldo, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (head_dim != 64) return fail(ctx, DCTAE_EUNSUP, "model_attention_varlen: head_dim must be 64");
  if (n_seq < 0 || n_seq > 65535 || max_len < 0 || heads <= 0 || heads > 65535 || ldo < 64ll * heads || ldo % 8 ||
      ldo > INT32_MAX)
    return fail(ctx, DCTAE_EINVAL, "model_attention_varlen: bad shape (n_seq and heads in [0, 65535], max_len >= 0, "
                                   "ldo >= 64 heads, ldo % 8)");
  if (n_seq == 0 || max_len == 0) return 0;
  if (!qkv || !seq_start || !seq_len || !out || ((uintptr_t)qkv & 15) || ((uintptr_t)out & 15))
    return fail(ctx, DCTAE_EINVAL, "model_attention_varlen: null or unaligned tensor");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  AttnArgs a{qkv, nullptr, nullptr, out, 0, 0, heads, (int32_t)ldo, 0.125f, nullptr};
  Timer t(ctx, s, "model_attention_varlen");
  launch_attention_varlen(a, n_seq, max_len, seq_start, seq_len, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_prefix_tokens(dctae_ctx* ctx, int32_t R, int32_t S, const int64_t* ids, const uint8_t* key_pad,
                        const int64_t* positions, const int64_t* channels, const void* codes, int32_t codes_type,
                        int32_t ncb, int32_t n_frames, const int32_t* frame_row, const int64_t* frame_id,
                        const int32_t* frame_m, const int64_t* frame_start, int64_t* out_codes, int64_t* out_channels,
                        int64_t* out_positions, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (codes_type != DCTAE_CODES_I64 && codes_type != DCTAE_CODES_I16)
    return fail(ctx, DCTAE_EINVAL, "codes_type: DCTAE_CODES_I64 or DCTAE_CODES_I16, got " + std::to_string(codes_type));
  if (R < 0 || S < 1 || ncb < 1 || n_frames < 0)
    return fail(ctx, DCTAE_EINVAL, "prefix_tokens: bad shape (R >= 0, S >= 1, ncb >= 1, n_frames >= 0)");
  if (n_frames == 0) return 0;
  if (!frame_row || !frame_id || !frame_m || !frame_start) return fail(ctx, DCTAE_EINVAL, "prefix_tokens: NULL frame array");
  if (!ids || !key_pad || !positions || !channels || !codes || !out_codes || !out_channels || !out_positions)
    return fail(ctx, DCTAE_EINVAL, "prefix_tokens: NULL tensor");
  for (int f = 0; f < n_frames; ++f) {
    if (frame_row[f] < 0 || frame_row[f] >= R)
      return fail(ctx, DCTAE_EINVAL, "prefix_tokens: frame " + std::to_string(f) + ": row outside [0, R)");
    if (frame_m[f] < 0 || frame_m[f] > S || frame_start[f] < 0)
      return fail(ctx, DCTAE_EINVAL, "prefix_tokens: frame " + std::to_string(f) + ": m outside [0, S] or a negative start");
  }
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  OrderedCall oc(ctx, s);
  PlanBuf pb;
  const size_t r_off = pb.add(frame_row, (size_t)n_frames);
  const size_t i_off = pb.add(frame_id, (size_t)n_frames);
  const size_t m_off = pb.add(frame_m, (size_t)n_frames);
  const size_t s_off = pb.add(frame_start, (size_t)n_frames);
  uint8_t* pd;
  int rc;
  if ((rc = oc.upload(pb, &pd))) return rc;
  PrefixGatherArgs a{ids, key_pad, positions, channels, codes,
                     (const int32_t*)(pd + r_off), (const int64_t*)(pd + i_off), (const int32_t*)(pd + m_off),
                     (const int64_t*)(pd + s_off), out_codes, out_channels, out_positions,
                     S, ncb, codes_type == DCTAE_CODES_I16 ? 1 : 0};
  Timer t(ctx, s, "prefix_tokens");
  launch_prefix_tokens(a, n_frames, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

}  // extern "C"
