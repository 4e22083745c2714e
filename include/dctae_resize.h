/* Antialiased bilinear resize of a ragged list of images in one launch: an
 * extension of dctae.h (same library, same context, DCTAE_ABI_VERSION
 * unchanged; nothing in dctae.h changes).  It is the resize of the
 * reference's dataset pipeline (dataset.py:59-73: torchvision's
 * Resize(antialias=True), i.e. torch's interpolate(mode="bilinear",
 * antialias=True, align_corners=False)), the one piece of arithmetic between
 * a decoded image and dctae_encode.
 *
 * Every image i of the input, (3, H_i, W_i) fp32 or bytes, is filtered to the
 * (3, OH_i, OW_i) fp32 image the output descriptor names; the sizes are the
 * caller's (any of them: down, up, or equal).  A byte pixel u means the fp32
 * value u / 255 (include/dctae_u8.h), converted before the filter, so a byte
 * call is bit-identical to the fp32 call on `u8.float() / 255`.  The
 * arithmetic is defined operation by operation in csrc/dctae_resize_math.h
 * (fp32, every operation rounded on its own, sums in ascending source index,
 * the horizontal pass first): a result does not depend on the other images of
 * the call or on how the kernel tiles it, and an axis whose size does not
 * change passes finite non-negative values through bit for bit.  Inputs must
 * be finite: a window's outermost tap can have weight zero, and zero times an
 * infinity is NaN, as in torch.
 *
 * Byte images may start at any byte address.  An output image must not share
 * a byte with any input image.  On n_img differing between the two
 * descriptors, a side <= 0 or such an overlap the call returns DCTAE_EINVAL
 * and dctae_last_error names the image.
 *
 * Streams: both entries run inside the context's ordered call scope like the
 * entries of dctae.h (the image table travels through the context's plan
 * buffer), so they are ordered after the context's previous call on another
 * stream in the same way. */
#ifndef DCTAE_RESIZE_H
#define DCTAE_RESIZE_H

#include "dctae.h"
#include "dctae_u8.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Output images: `n_img` fp32 RGB images of shape (3, OH_i, OW_i), contiguous,
 * at float offsets img_off[i] of rgb_dev (host arrays). */
typedef struct {
  float* rgb_dev;
  const int64_t* img_off;   /* host, n_img, floats */
  const int32_t* hw;        /* host, 2*n_img: OH0,OW0,OH1,OW1,... */
  int32_t n_img;
} dctae_images_out;

int dctae_resize_aa(dctae_ctx* ctx, const dctae_images* in, const dctae_images_out* out, void* stream);

/* dctae_resize_aa on byte images (img_off in bytes); everything else as there. */
int dctae_resize_aa_u8(dctae_ctx* ctx, const dctae_images_u8* in, const dctae_images_out* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DCTAE_RESIZE_H */
