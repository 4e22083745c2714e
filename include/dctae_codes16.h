/* Compact LFQ codes: int16 out of the encode and into the decode.  An
 * extension of dctae.h (same library, same context, DCTAE_ABI_VERSION
 * unchanged; nothing in dctae.h, dctae_u8.h or dctae_u8_out.h changes).
 *
 * One rule: an int16 code c means the int64 code int64(c), the sign extension
 * that torch's `.long()` gives.  Every code an encode entry of this header
 * writes equals its dctae.h twin's code converted to int16, and every other
 * output is bit-identical to the twin's; every pixel a decode entry of this
 * header writes is bit-identical to its twin's on `codes.long()`, for any
 * int16 value (negative ones included), and every float a projection entry
 * writes is bit-identical in the same way.  The kernels that store or load
 * the caller's codes do so two bytes per code; nothing else of a call differs,
 * on every path and under every library option; no extra workspace.
 *
 * Limit: codes lie in [0, 2^codebook_dim), so the conversion is exact for
 * codebook_dim <= 15.  With codebook_dim >= 16 every entry of this header
 * fails with DCTAE_EINVAL before anything is launched, and dctae_last_error
 * names the limit.
 *
 * Alignment: an int16 code pointer must be 2-byte aligned.  The packed
 * encodes at num_codebooks = 14 store two codes per store, so there
 * out->codes_dev must be 4-byte aligned (every packed row of 14 codes then
 * is).  A pointer that misses its alignment fails with DCTAE_EINVAL before
 * anything is launched.  The decode and the projections load one code at a
 * time: 2-byte alignment is all they ask (where dctae_lfq_project_out asks
 * 16-byte alignment of its int64 indices).
 *
 * Streams: every entry runs inside the same ordered call scope as its dctae.h
 * / dctae_u8.h / dctae_u8_out.h counterpart (they are the same call: one
 * planner, the code type carried as a tag, the same workspace requests and
 * plan), so they are ordered after the context's previous call on another
 * stream in the same way.
 *
 * The packed metadata (positions, channels, image ids) stays int64. */
#ifndef DCTAE_CODES16_H
#define DCTAE_CODES16_H

#include "dctae.h"
#include "dctae_u8.h"
#include "dctae_u8_out.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dctae_packed_out with int16 codes; every other field as there. */
typedef struct {
  int16_t* codes_dev;        /* (R, S, num_codebooks) LFQ indices as int16 */
  int64_t* positions_dev;
  int64_t* channels_dev;
  int64_t* image_ids_dev;
  uint8_t* key_pad_dev;
  float* patches_dev;
  float* raw_patches_dev;
  float* scores_dev;
} dctae_packed_out16;

/* dctae_encode with int16 codes; everything else as there. */
int dctae_encode_c16(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images* imgs, const dctae_packing* pack,
                     const dctae_norm* norm, const dctae_lfq* lfq, const dctae_packed_out16* out, void* stream);

/* dctae_encode_u8 with int16 codes. */
int dctae_encode_u8_c16(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images_u8* imgs,
                        const dctae_packing* pack, const dctae_norm* norm, const dctae_lfq* lfq,
                        const dctae_packed_out16* out, void* stream);

/* dctae_encode_lfq_proj with int16 codes. */
int dctae_encode_lfq_proj_c16(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images* imgs,
                              const dctae_packing* pack, const dctae_norm* norm, const dctae_lfq* lfq,
                              const float* w_in_dev, const float* b_in_dev, const dctae_packed_out16* out,
                              void* stream);

/* dctae_encode_lfq_proj_u8 with int16 codes. */
int dctae_encode_lfq_proj_u8_c16(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images_u8* imgs,
                                 const dctae_packing* pack, const dctae_norm* norm, const dctae_lfq* lfq,
                                 const float* w_in_dev, const float* b_in_dev, const dctae_packed_out16* out,
                                 void* stream);

/* dctae_decode from int16 codes; everything else as there. */
int dctae_decode_c16(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut, int32_t lut_w,
                     int32_t n_img, const int32_t* out_hw, const int64_t* out_off, const int32_t* patch_hw,
                     const int64_t* ids_dev, const uint8_t* key_pad_dev, const int64_t* positions_dev,
                     const int64_t* channels_dev, const dctae_norm* norm, const dctae_lfq* lfq,
                     const int16_t* codes_dev, const float* patches_dev, float* rgb_dev, void* stream);

/* dctae_decode_u8 from int16 codes: two-byte codes in, byte pixels out. */
int dctae_decode_u8_c16(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut,
                        int32_t lut_w, int32_t n_img, const int32_t* out_hw, const int64_t* out_off,
                        const int32_t* patch_hw, const int64_t* ids_dev, const uint8_t* key_pad_dev,
                        const int64_t* positions_dev, const int64_t* channels_dev, const dctae_norm* norm,
                        const dctae_lfq* lfq, const int16_t* codes_dev, const float* patches_dev, uint8_t* rgb_dev,
                        void* stream);

/* dctae_lfq_project_in with int16 indices. */
int dctae_lfq_project_in_c16(dctae_ctx* ctx, const dctae_lfq* lfq, const float* x_dev, int64_t n, int32_t dim,
                             const float* w_in_dev, const float* b_in_dev, int16_t* indices_dev, void* stream);

/* dctae_lfq_project_in_bounded with int16 indices. */
int dctae_lfq_project_in_bounded_c16(dctae_ctx* ctx, const dctae_lfq* lfq, const float* x_dev, int64_t n, int32_t dim,
                                     const float* w_in_dev, const float* b_in_dev, float x_bound,
                                     int16_t* indices_dev, void* stream);

/* dctae_lfq_project_out from int16 indices. */
int dctae_lfq_project_out_c16(dctae_ctx* ctx, const dctae_lfq* lfq, const int16_t* indices_dev, int64_t n,
                              int32_t dim, const float* w_out_dev, const float* b_out_dev, float* out_dev,
                              void* stream);

/* dctae_lfq_project_out_inverse_norm from int16 indices. */
int dctae_lfq_project_out_inverse_norm_c16(dctae_ctx* ctx, const dctae_lfq* lfq, const int16_t* indices_dev, int64_t n,
                                           int32_t dim, const float* w_out_dev, const float* b_out_dev,
                                           const dctae_norm* norm, int32_t max_patch_h, int32_t max_patch_w,
                                           const int64_t* channels_dev, const int64_t* positions_dev, float* out_dev,
                                           void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DCTAE_CODES16_H */
