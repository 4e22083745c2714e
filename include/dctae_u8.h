/* Byte-pixel images for the encode: an extension of dctae.h (same library,
 * same context, DCTAE_ABI_VERSION unchanged; nothing in dctae.h changes).
 *
 * A byte image is a (3, H, W) uint8 RGB image and means exactly the fp32
 * image u / 255 (fp32 division, correctly rounded: what
 * `pil_to_tensor(img) / 255` or `u8.float() / 255` produce).  The row kernels
 * read the bytes themselves and convert in registers, so every output of a
 * byte call is bit-identical to the dctae.h call on that fp32 image, for
 * every kernel family and every library option; no extra workspace.
 *
 * Alignment: a 512-wide image whose row pass runs on the 512-wide row kernel
 * (the default for W = 512 at max_patch_w = 32, option rows_kernel = 4) is
 * read four pixels per load, so rgb_dev + img_off[i] must be 4-byte aligned
 * (every row and plane of it then is); otherwise the call fails with
 * DCTAE_EINVAL and dctae_last_error names the image.  Every other image may
 * start at any byte.
 *
 * Streams: the three encode entries run inside the same ordered call scope
 * as their dctae.h counterparts (they are the same call: one planner, the
 * pixel type carried as a tag), so they are ordered after the context's
 * previous call on another stream in the same way.  dctae_u8_to_f32 touches
 * no memory of the context. */
#ifndef DCTAE_U8_H
#define DCTAE_U8_H

#include "dctae.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Images: `n_img` uint8 RGB images of shape (3, H_i, W_i), contiguous, at
 * byte offsets img_off[i] of rgb_dev (host arrays). */
typedef struct {
  const uint8_t* rgb_dev;
  const int64_t* img_off;   /* host, n_img, bytes */
  const int32_t* hw;        /* host, 2*n_img: H0,W0,H1,W1,... */
  int32_t n_img;
} dctae_images_u8;

/* dctae_encode on byte images; everything else as there. */
int dctae_encode_u8(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images_u8* imgs,
                    const dctae_packing* pack, const dctae_norm* norm, const dctae_lfq* lfq,
                    const dctae_packed_out* out, void* stream);

/* dctae_encode_lfq_proj on byte images; everything else as there. */
int dctae_encode_lfq_proj_u8(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images_u8* imgs,
                             const dctae_packing* pack, const dctae_norm* norm, const dctae_lfq* lfq,
                             const float* w_in_dev, const float* b_in_dev, const dctae_packed_out* out,
                             void* stream);

/* dctae_spectrum_tokens on byte images; everything else as there. */
int dctae_spectrum_tokens_u8(dctae_ctx* ctx, const dctae_fe_cfg* cfg, const dctae_images_u8* imgs,
                             const int64_t* tok_off, float* tokens_dev, float* scores_dev, void* stream);

/* y[i] = x[i] / 255 in fp32 (the 256 values the byte entries mean), n
 * elements at any alignment: for callers that run the stages one by one on
 * byte images, and the direct probe of the conversion. */
int dctae_u8_to_f32(dctae_ctx* ctx, const uint8_t* x_dev, int64_t n, float* y_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DCTAE_U8_H */
