/* Byte-pixel images out of the decode: an extension of dctae.h (same library,
 * same context, DCTAE_ABI_VERSION unchanged; nothing in dctae.h or dctae_u8.h
 * changes).  The mirror of dctae_u8.h: bytes in, codes, bytes out, with no
 * fp32 image tensor outside the library.
 *
 * A byte of output is defined from the fp32 value x the dctae.h call writes
 * for the same inputs: t = x * 255 rounded to fp32, t = t + 0.5 rounded to
 * fp32, clamped to [0, 255], truncated -- torch's
 * `x.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)` on the CPU, the rounding
 * of torchvision's save_image.  NaN gives 0, +inf 255, -inf, -0 and negative
 * values 0.  The kernels that write the caller's images convert in registers
 * after the same arithmetic in the same order, so every byte a byte call
 * writes is bit-identical to that function of the fp32 call's value, on every
 * decode path and under every library option; no extra workspace.
 *
 * Alignment: 512 x 512 images decoded on the 512-wide row kernel (the default
 * at max_patch_w = 32, option dec_rows_kernel = 3) are written sixteen pixels
 * per store, so rgb_dev + out_off[i] must be 4-byte aligned (every row and
 * plane of the image then is); otherwise the call fails with DCTAE_EINVAL
 * before anything is launched and dctae_last_error names the image.  Every
 * other image may start at any byte.
 *
 * Streams: the two decode entries run inside the same ordered call scope as
 * their dctae.h counterparts (they are the same call: one planner, the pixel
 * type carried as a tag, the same workspace requests and plan), so they are
 * ordered after the context's previous call on another stream in the same
 * way.  dctae_f32_to_u8 touches no memory of the context.
 *
 * dctae_decode_backward and dctae_pixel_loss_forward stay fp32 only. */
#ifndef DCTAE_U8_OUT_H
#define DCTAE_U8_OUT_H

#include "dctae.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dctae_decode into uint8 images: image i is (3, H_i, W_i) bytes at byte
 * offset out_off[i] of rgb_dev; everything else as there. */
int dctae_decode_u8(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut, int32_t lut_w,
                    int32_t n_img, const int32_t* out_hw, const int64_t* out_off, const int32_t* patch_hw,
                    const int64_t* ids_dev, const uint8_t* key_pad_dev, const int64_t* positions_dev,
                    const int64_t* channels_dev, const dctae_norm* norm, const dctae_lfq* lfq,
                    const int64_t* codes_dev, const float* patches_dev, uint8_t* rgb_dev, void* stream);

/* dctae_decode_normed into uint8 images, out_off in bytes; everything else as there. */
int dctae_decode_normed_u8(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut,
                           int32_t lut_w, int32_t n_img, const int32_t* out_hw, const int64_t* out_off,
                           const int32_t* patch_hw, const int64_t* ids_dev, const uint8_t* key_pad_dev,
                           const int64_t* positions_dev, const int64_t* channels_dev, const dctae_norm* norm,
                           const float* normed_patches_dev, uint8_t* rgb_dev, void* stream);

/* y[i] = the byte of x[i] by the rule above, n elements, y at any alignment:
 * for callers that run the stages one by one, and the direct probe of the
 * conversion (the inverse twin of dctae_u8_to_f32). */
int dctae_f32_to_u8(dctae_ctx* ctx, const float* x_dev, int64_t n, uint8_t* y_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DCTAE_U8_OUT_H */
