/* Progressive decode through the transformer: variable-length attention and
 * the prefix token gather.  An extension of dctae.h (same library, same
 * context, DCTAE_ABI_VERSION unchanged; nothing in dctae.h or the other
 * extension headers changes).
 *
 * The MODEL PREFIX FRAME (i, k) of a packed batch is what the trained decoder
 * rebuilds from the first m = min(k, n_i) real tokens of image i, placed as a
 * one-row batch of length m without padding (the reference's decode_gif.py:
 * decode_from_codes(codes[:, :i]) on its one-image row).  Truncation, not
 * masking: the reference ADDS its boolean mask to the logits, so a masked
 * token still acts as a key, and so do the row's other images and its
 * padding.  Every linear, LayerNorm and position kernel of the model is
 * token-wise, so N x P frames are one flat token stream; only attention knows
 * where a sequence begins and ends.
 *
 * Streams: both calls are stream-ordered and never wait on the host.
 * dctae_model_attention_varlen touches the caller's tensors only.
 * dctae_prefix_tokens uploads its frame tables through the context's plan
 * inside the context's ordered call scope like the entries of dctae.h, so it
 * is ordered after the context's previous call on another stream in the same
 * way. */
#ifndef DCTAE_MODEL_PREFIX_H
#define DCTAE_MODEL_PREFIX_H

#include "dctae.h"
#include "dctae_frames.h" /* DCTAE_CODES_I64 / DCTAE_CODES_I16 */

#ifdef __cplusplus
extern "C" {
#endif

/* Full softmax attention inside each of n_seq sequences of a flat token
 * stream.  qkv: (M, 3 * heads * 64) bf16, q | k | v, as dctae_model_attention
 * takes it; sequence j is the token rows [seq_start[j], seq_start[j] +
 * seq_len[j]) (device arrays: int64 starts, int32 lengths); out: (M, ldo) bf16,
 * head h at columns 64 h.  There is no bias term (a one-image unpadded row has
 * an all-False mask, which adds 0), and the rows of a sequence equal, bit for
 * bit, what dctae_model_attention writes for R = 1, S = seq_len[j] on that
 * slice with no pad key: the same kernel body with its row's first token and
 * length read from the table.  Loads are clamped to the sequence, so no row
 * outside it is read.  Rows of out outside every sequence, and the rows of a
 * sequence of length 0, are not touched.  Grid: (ceil(max_len / 256), heads,
 * n_seq); a query block at or beyond its sequence's length writes nothing.
 *
 * The caller guarantees (the call cannot read the device tables): sequences
 * lie inside the M rows and do not overlap, 0 <= seq_len[j] <= max_len (queries
 * at or beyond max_len rounded up to 256 would be left unwritten).
 * Refused with DCTAE_EINVAL: n_seq or heads outside [0, 65535] (heads = 0
 * too), max_len < 0, ldo < 64 heads or ldo % 8 != 0, a NULL or not 16-byte
 * aligned qkv / out, NULL tables; head_dim != 64 with DCTAE_EUNSUP.
 * n_seq = 0 or max_len = 0 returns 0 with nothing launched. */
int dctae_model_attention_varlen(dctae_ctx* ctx, int32_t n_seq, int32_t max_len, int32_t heads, int32_t head_dim,
                                 const uint16_t* qkv_dev, const int64_t* seq_start_dev, const int32_t* seq_len_dev,
                                 uint16_t* out_dev, int64_t ldo, void* stream);

/* The tokens of n_frames prefix frames, gathered from a packed batch
 * (ids, key_pad: (R, S); positions: (R, S, 2); channels: (R, S); codes:
 * (R, S, ncb) of codes_type) into a flat stream.  Frame f (host arrays of
 * n_frames entries) is the first frame_m[f] slots j of row frame_row[f], in
 * slot order, with ids[j] == frame_id[f] and key_pad[j] == 0; interior padded
 * slots are skipped.  The token of rank r < frame_m[f] goes to flat row
 * frame_start[f] + r of out_codes (M, ncb) int64, out_channels (M) and
 * out_positions (M, 2); int16 codes are widened, a code c meaning int64(c).
 * One block per frame; S is arbitrary.  Every output row of every frame is
 * written when frame_m[f] does not exceed the number of such slots (the
 * caller's plan is made from the same ids / key_pad): no memset, no
 * dependence on what the buffers held.  The frames' output ranges must not
 * overlap and must lie inside the output buffers.
 * Refused with DCTAE_EINVAL: R < 0, S < 1, ncb < 1, n_frames < 0, a codes_type
 * not listed in dctae_frames.h, NULL arrays or tensors with n_frames > 0, a
 * row outside [0, R), frame_m outside [0, S], a negative start.  n_frames = 0
 * returns 0 with nothing launched. */
int dctae_prefix_tokens(dctae_ctx* ctx, int32_t R, int32_t S, const int64_t* ids_dev, const uint8_t* key_pad_dev,
                        const int64_t* positions_dev, const int64_t* channels_dev, const void* codes_dev,
                        int32_t codes_type, int32_t ncb, int32_t n_frames, const int32_t* frame_row,
                        const int64_t* frame_id, const int32_t* frame_m, const int64_t* frame_start,
                        int64_t* out_codes_dev, int64_t* out_channels_dev, int64_t* out_positions_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DCTAE_MODEL_PREFIX_H */
