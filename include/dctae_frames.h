/* Progressive decode: token-prefix frames of the images of a packed batch in
 * one launch sequence, and the reference's min-max image_clip.  An extension
 * of dctae.h (same library, same context, DCTAE_ABI_VERSION unchanged; nothing
 * in dctae.h or the other extension headers changes).
 *
 * The encode sorts every image's tokens by importance, so the first k tokens
 * of an image are already a usable picture (the reference's decode_gif.py
 * decodes codes[:, :i] for growing i).  A FRAME is one such picture: the
 * decode of image img[f] from the tokens of that image at row slots j < cut[f]
 * alone.  By definition frame f is, bit for bit, the image that dctae_decode
 * (or dctae_decode_normed) writes for image img[f] when key_pad is
 * additionally set on every token of that image at a slot j >= cut[f]: on
 * every decode path, for every token source and both output types.  So
 * cut = 0 is the decode of an empty spectrum, cut = max_seq_len the whole
 * image, and of two tokens at one place (c, h, w) below the cut the later slot
 * wins.  An image may have any number of frames, none included; the frames
 * may be listed in any order.
 *
 * One call builds the slot map of every frame (map[frame][c][w][h], one
 * atomicMax per token and frame that holds it), and from there on treats a
 * frame as an image: the decode's own column / row kernels, DCT GEMMs and
 * colour kernels run over one descriptor per frame.  The path is the one
 * dctae_decode takes for the same batch (the FFT path when every image of the
 * batch is 512 x 512 at patch size 14 and the tokens are patches or
 * recommended-LFQ codes; the GEMM path otherwise).
 *
 * clip = DCTAE_CLIP_MINMAX passes every frame through image_clip (util.py:143-147):
 *   y = (x - min) / (max - min),  min / max over the 3 H W values of the frame,
 * in fp32: min and max exact, one subtraction and one division per pixel, each
 * correctly rounded and never contracted.  A byte output is that fp32 value
 * through the quantiser of dctae_u8_out.h (NaN gives 0): the fp32 frames then
 * live in the context's scratch and only bytes reach `out`.  A constant image
 * gives NaN (fp32) / 0 (bytes).  Where min is a zero the sign of a zero result
 * is unspecified.  Inputs must be finite.  Min and max are integer atomics on
 * an order-preserving encoding of the fp32 bits: no floating-point atomics,
 * the same bits on every run.
 *
 * Refused with DCTAE_EINVAL before anything is launched (dctae_last_error says
 * which): everything dctae_decode refuses; a NULL frame table; n_frames < 0 or
 * above 65535; NULL frame arrays with n_frames > 0; img[f] outside
 * [0, n_img); cut[f] outside [0, max_seq_len]; a negative offset; a type tag
 * or clip value not listed below; a 512 x 512 byte frame written by the
 * 512-wide row kernel (dctae_u8_out.h; not with clip, whose bytes come from
 * the clip kernel) that does not start 4-byte aligned.  n_frames = 0 returns
 * 0 with nothing launched.
 *
 * Streams: both calls are stream-ordered, never wait on the host, and run
 * inside the context's ordered call scope like the entries of dctae.h (their
 * workspace and tables are the context's scratch and plan), so they are
 * ordered after the context's previous call on another stream in the same way. */
#ifndef DCTAE_FRAMES_H
#define DCTAE_FRAMES_H

#include "dctae.h"

#ifdef __cplusplus
extern "C" {
#endif

/* type tags */
#define DCTAE_PIXEL_F32 0   /* out: float, offsets in floats */
#define DCTAE_PIXEL_U8 1    /* out: uint8_t, offsets in bytes */
#define DCTAE_CODES_I64 0   /* codes: int64_t */
#define DCTAE_CODES_I16 1   /* codes: int16_t, a code c meaning int64(c) (dctae_codes16.h) */
#define DCTAE_CLIP_NONE 0
#define DCTAE_CLIP_MINMAX 1

/* the frames of one call (host arrays of n_frames entries) */
typedef struct {
  int32_t n_frames;
  const int32_t* img;      /* source image of frame f, 0 <= img[f] < n_img */
  const int32_t* cut;      /* frame f holds the tokens of that image at row slot j < cut[f], 0 <= cut[f] <= max_seq_len */
  const int64_t* out_off;  /* element offset of frame f's (3, H, W) image in `out` */
} dctae_frames;

/* The packed batch as dctae_decode takes it, without out_off (the frames carry
 * their own).  Token source, exactly one of:
 *   codes_dev (of codes_type), with norm and lfq   -- as dctae_decode / dctae_decode_c16
 *   patches_dev, normed = 0                         -- un-normalised patches, as dctae_decode
 *   patches_dev, normed = 1, with norm              -- PatchNorm-space patches, as dctae_decode_normed
 * out: the frames' images of out_type at frames->out_off. */
int dctae_decode_frames(dctae_ctx* ctx, const dctae_fe_cfg* cfg, int32_t n_rows, const int32_t* img_lut,
                        int32_t lut_w, int32_t n_img, const int32_t* out_hw, const int32_t* patch_hw,
                        const int64_t* ids_dev, const uint8_t* key_pad_dev, const int64_t* positions_dev,
                        const int64_t* channels_dev, const dctae_frames* frames, const dctae_norm* norm,
                        const dctae_lfq* lfq, const void* codes_dev, int32_t codes_type, const float* patches_dev,
                        int32_t normed, int32_t clip, void* out_dev, int32_t out_type, void* stream);

/* image_clip of n_img fp32 images: image i is the 3 hw[2 i] hw[2 i + 1] floats
 * at float offset in_off[i] of in_dev, its result the same number of elements
 * of out_type at element offset out_off[i] of out_dev (fp32 results may be
 * written over their inputs).  Refused: n_img < 0 or above 65535, NULL arrays
 * or buffers with n_img > 0, a side < 1, a negative offset, an unknown
 * out_type.  n_img = 0 returns 0 with nothing launched. */
int dctae_image_clip(dctae_ctx* ctx, int32_t n_img, const int32_t* hw, const int64_t* in_off, const float* in_dev,
                     const int64_t* out_off, void* out_dev, int32_t out_type, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DCTAE_FRAMES_H */
