"""ctypes binding of libdctae.so (the C ABI in include/dctae.h).

The product path has no fallback: if the library or a HIP device is missing,
every op raises ``DCTAEUnavailable``.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Dict, Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# DCTAE_LIBRARY: another build of the same ABI (e.g. a profiling variant)
LIB_PATH = os.environ.get("DCTAE_LIBRARY") or os.path.join(_HERE, "libdctae.so")
ABI_VERSION = 1


class DCTAEUnavailable(RuntimeError):
    pass


class DCTAEError(RuntimeError):
    pass


# ---- struct mirrors of include/dctae.h ------------------------------------


class FECfg(C.Structure):
    _fields_ = [("channels", C.c_int32), ("patch_size", C.c_int32), ("max_patch_h", C.c_int32),
                ("max_patch_w", C.c_int32), ("max_seq_len", C.c_int32),
                ("channel_importances", C.c_float * 3), ("magnitude_weight", C.c_float)]


class Norm(C.Structure):
    _fields_ = [("median_dev", C.c_void_p), ("b_dev", C.c_void_p), ("eps", C.c_float),
                ("min_val", C.c_float), ("max_val", C.c_float), ("thr_dev", C.c_void_p)]


class LFQCfg(C.Structure):
    _fields_ = [("codebook_dim", C.c_int32), ("num_codebooks", C.c_int32), ("codebook_scale", C.c_float)]


class Images(C.Structure):
    _fields_ = [("rgb_dev", C.c_void_p), ("img_off", C.POINTER(C.c_int64)), ("hw", C.POINTER(C.c_int32)),
                ("n_img", C.c_int32)]


class ImagesU8(C.Structure):
    """dctae_images_u8 (include/dctae_u8.h): uint8 pixels, img_off in bytes"""
    _fields_ = [("rgb_dev", C.c_void_p), ("img_off", C.POINTER(C.c_int64)), ("hw", C.POINTER(C.c_int32)),
                ("n_img", C.c_int32)]


class ImagesOut(C.Structure):
    """dctae_images_out (include/dctae_resize.h): fp32 output images, img_off in floats"""
    _fields_ = [("rgb_dev", C.c_void_p), ("img_off", C.POINTER(C.c_int64)), ("hw", C.POINTER(C.c_int32)),
                ("n_img", C.c_int32)]


class Frames(C.Structure):
    """dctae_frames (include/dctae_frames.h): the prefix frames of one call, host arrays"""
    _fields_ = [("n_frames", C.c_int32), ("img", C.POINTER(C.c_int32)), ("cut", C.POINTER(C.c_int32)),
                ("out_off", C.POINTER(C.c_int64))]


# the type tags of include/dctae_frames.h
PIXEL_F32, PIXEL_U8 = 0, 1
CODES_I64, CODES_I16 = 0, 1
CLIP_NONE, CLIP_MINMAX = 0, 1


class Packing(C.Structure):
    _fields_ = [("row", C.POINTER(C.c_int32)), ("col", C.POINTER(C.c_int32)), ("k", C.POINTER(C.c_int32)),
                ("local_id", C.POINTER(C.c_int32)), ("row_len", C.POINTER(C.c_int32)), ("n_rows", C.c_int32)]


class PackedOut(C.Structure):
    _fields_ = [("codes_dev", C.c_void_p), ("positions_dev", C.c_void_p), ("channels_dev", C.c_void_p),
                ("image_ids_dev", C.c_void_p), ("key_pad_dev", C.c_void_p), ("patches_dev", C.c_void_p),
                ("raw_patches_dev", C.c_void_p), ("scores_dev", C.c_void_p)]


class PackedOut16(C.Structure):
    """dctae_packed_out16 (include/dctae_codes16.h): codes_dev points at int16"""
    _fields_ = PackedOut._fields_


class VQCfg(C.Structure):
    _fields_ = [("dim", C.c_int32), ("heads", C.c_int32), ("codebook_dim", C.c_int32),
                ("codebook_size", C.c_int32), ("affine", C.c_int32), ("affine_decay", C.c_float),
                ("w_in_dev", C.c_void_p), ("b_in_dev", C.c_void_p), ("w_out_dev", C.c_void_p),
                ("b_out_dev", C.c_void_p), ("embed_dev", C.c_void_p), ("codebook_mean_dev", C.c_void_p),
                ("codebook_variance_dev", C.c_void_p), ("batch_mean_dev", C.c_void_p),
                ("batch_variance_dev", C.c_void_p), ("batch_initted_dev", C.c_void_p)]


class OptimSeg(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("w_dst", C.c_void_p), ("wt_dst", C.c_void_p), ("copy_dst", C.c_void_p),
                ("rows", C.c_int64), ("cols", C.c_int64), ("ldw", C.c_int64), ("ldwt", C.c_int64),
                ("w_row_off", C.c_int64), ("wt_col_off", C.c_int64), ("norm0", C.c_int64), ("work0", C.c_int64),
                ("group", C.c_int32), ("reserved", C.c_int32)]


class OptimGroup(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("decay", "w1", "beta2", "w2", "step_size", "bc2_sqrt", "eps", "reserved")]


OPTIM_MAX_GROUPS = 16

_P = C.c_void_p
_SIGS = {
    "dctae_abi_version": ([], C.c_int),
    "dctae_ctx_create": ([C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "dctae_ctx_destroy": ([_P], C.c_int),
    "dctae_last_error": ([_P], C.c_char_p),
    "dctae_set_color_matrices": ([_P, _P, _P, _P, _P], C.c_int),
    "dctae_encode": ([_P, C.POINTER(FECfg), C.POINTER(Images), C.POINTER(Packing), C.POINTER(Norm),
                      C.POINTER(LFQCfg), C.POINTER(PackedOut), _P], C.c_int),
    "dctae_encode_lfq_proj": ([_P, C.POINTER(FECfg), C.POINTER(Images), C.POINTER(Packing), C.POINTER(Norm),
                               C.POINTER(LFQCfg), _P, _P, C.POINTER(PackedOut), _P], C.c_int),
    "dctae_spectrum_tokens": ([_P, C.POINTER(FECfg), C.POINTER(Images), C.POINTER(C.c_int64), _P, _P, _P],
                              C.c_int),
    # include/dctae_u8.h: the byte-image entries
    "dctae_encode_u8": ([_P, C.POINTER(FECfg), C.POINTER(ImagesU8), C.POINTER(Packing), C.POINTER(Norm),
                         C.POINTER(LFQCfg), C.POINTER(PackedOut), _P], C.c_int),
    "dctae_encode_lfq_proj_u8": ([_P, C.POINTER(FECfg), C.POINTER(ImagesU8), C.POINTER(Packing), C.POINTER(Norm),
                                  C.POINTER(LFQCfg), _P, _P, C.POINTER(PackedOut), _P], C.c_int),
    "dctae_spectrum_tokens_u8": ([_P, C.POINTER(FECfg), C.POINTER(ImagesU8), C.POINTER(C.c_int64), _P, _P, _P],
                                 C.c_int),
    "dctae_u8_to_f32": ([_P, _P, C.c_int64, _P, _P], C.c_int),
    # include/dctae_resize.h: the antialiased resize of a ragged image list
    "dctae_resize_aa": ([_P, C.POINTER(Images), C.POINTER(ImagesOut), _P], C.c_int),
    "dctae_resize_aa_u8": ([_P, C.POINTER(ImagesU8), C.POINTER(ImagesOut), _P], C.c_int),
    # include/dctae_frames.h: the prefix frames of a packed batch, image_clip
    "dctae_decode_frames": ([_P, C.POINTER(FECfg), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                             C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _P, _P, _P, C.POINTER(Frames),
                             C.POINTER(Norm), C.POINTER(LFQCfg), _P, C.c_int32, _P, C.c_int32, C.c_int32, _P,
                             C.c_int32, _P], C.c_int),
    "dctae_image_clip": ([_P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), _P, C.POINTER(C.c_int64), _P,
                          C.c_int32, _P], C.c_int),
    # include/dctae_model_prefix.h: variable-length attention, the prefix token gather
    "dctae_model_attention_varlen": ([_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int64, _P],
                                     C.c_int),
    "dctae_prefix_tokens": ([_P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32,
                             C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                             _P, _P, _P, _P], C.c_int),
    "dctae_dct2": ([_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P], C.c_int),
    "dctae_patch_spectrum": ([_P, C.POINTER(FECfg), _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P],
                             C.c_int),
    "dctae_norm_forward": ([_P, C.POINTER(Norm), C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_int64, _P, _P],
                           C.c_int),
    "dctae_norm_inverse": ([_P, C.POINTER(Norm), C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_int64, _P, _P],
                           C.c_int),
    "dctae_norm_inverse_backward": ([_P, C.POINTER(Norm), C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_int64, _P,
                                     _P], C.c_int),
    "dctae_rec_loss_forward": ([_P, C.POINTER(Norm), C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P,
                                C.c_int64, _P, _P, _P], C.c_int),
    "dctae_rec_loss_backward": ([_P, C.POINTER(Norm), C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P,
                                 C.c_int64, _P, _P, _P, _P, _P], C.c_int),
    "dctae_lfq_forward": ([_P, C.POINTER(LFQCfg), _P, C.c_int64, _P, _P, _P], C.c_int),
    "dctae_lfq_indices_to_codes": ([_P, C.POINTER(LFQCfg), _P, C.c_int64, _P, _P], C.c_int),
    "dctae_lfq_entropy_forward": ([_P, C.POINTER(LFQCfg), _P, _P, C.c_int64, C.c_float, C.c_float, _P, _P, _P],
                                  C.c_int),
    "dctae_lfq_entropy_backward": ([_P, C.POINTER(LFQCfg), _P, _P, C.c_int64, C.c_float, C.c_float, _P, _P, _P, _P,
                                    _P], C.c_int),
    "dctae_linear_ordered": ([_P, _P, C.c_int64, C.c_int32, _P, _P, C.c_int32, _P, _P], C.c_int),
    "dctae_lfq_project_in": ([_P, C.POINTER(LFQCfg), _P, C.c_int64, C.c_int32, _P, _P, _P, _P], C.c_int),
    "dctae_lfq_project_in_bounded": ([_P, C.POINTER(LFQCfg), _P, C.c_int64, C.c_int32, _P, _P, C.c_float, _P, _P],
                                     C.c_int),
    "dctae_lfq_project_out": ([_P, C.POINTER(LFQCfg), _P, C.c_int64, C.c_int32, _P, _P, _P, _P], C.c_int),
    "dctae_lfq_project_out_inverse_norm": ([_P, C.POINTER(LFQCfg), _P, C.c_int64, C.c_int32, _P, _P, C.POINTER(Norm),
                                            C.c_int32, C.c_int32, _P, _P, _P, _P], C.c_int),
    "dctae_decode": ([_P, C.POINTER(FECfg), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                      C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), _P, _P, _P, _P,
                      C.POINTER(Norm), C.POINTER(LFQCfg), _P, _P, _P, _P], C.c_int),
    "dctae_decode_normed": ([_P, C.POINTER(FECfg), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                             C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), _P, _P, _P, _P,
                             C.POINTER(Norm), _P, _P, _P], C.c_int),
    # include/dctae_u8_out.h: the byte-output entries
    "dctae_decode_u8": ([_P, C.POINTER(FECfg), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                         C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), _P, _P, _P, _P,
                         C.POINTER(Norm), C.POINTER(LFQCfg), _P, _P, _P, _P], C.c_int),
    "dctae_decode_normed_u8": ([_P, C.POINTER(FECfg), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                                C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), _P, _P, _P, _P,
                                C.POINTER(Norm), _P, _P, _P], C.c_int),
    "dctae_f32_to_u8": ([_P, _P, C.c_int64, _P, _P], C.c_int),
    # include/dctae_codes16.h: the int16-code entries (their twins' arguments, the code pointer's type apart)
    "dctae_encode_c16": ([_P, C.POINTER(FECfg), C.POINTER(Images), C.POINTER(Packing), C.POINTER(Norm),
                          C.POINTER(LFQCfg), C.POINTER(PackedOut16), _P], C.c_int),
    "dctae_encode_u8_c16": ([_P, C.POINTER(FECfg), C.POINTER(ImagesU8), C.POINTER(Packing), C.POINTER(Norm),
                             C.POINTER(LFQCfg), C.POINTER(PackedOut16), _P], C.c_int),
    "dctae_encode_lfq_proj_c16": ([_P, C.POINTER(FECfg), C.POINTER(Images), C.POINTER(Packing), C.POINTER(Norm),
                                   C.POINTER(LFQCfg), _P, _P, C.POINTER(PackedOut16), _P], C.c_int),
    "dctae_encode_lfq_proj_u8_c16": ([_P, C.POINTER(FECfg), C.POINTER(ImagesU8), C.POINTER(Packing), C.POINTER(Norm),
                                      C.POINTER(LFQCfg), _P, _P, C.POINTER(PackedOut16), _P], C.c_int),
    "dctae_decode_c16": ([_P, C.POINTER(FECfg), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                          C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), _P, _P, _P, _P,
                          C.POINTER(Norm), C.POINTER(LFQCfg), _P, _P, _P, _P], C.c_int),
    "dctae_decode_u8_c16": ([_P, C.POINTER(FECfg), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                             C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), _P, _P, _P, _P,
                             C.POINTER(Norm), C.POINTER(LFQCfg), _P, _P, _P, _P], C.c_int),
    "dctae_lfq_project_in_c16": ([_P, C.POINTER(LFQCfg), _P, C.c_int64, C.c_int32, _P, _P, _P, _P], C.c_int),
    "dctae_lfq_project_in_bounded_c16": ([_P, C.POINTER(LFQCfg), _P, C.c_int64, C.c_int32, _P, _P, C.c_float, _P, _P],
                                         C.c_int),
    "dctae_lfq_project_out_c16": ([_P, C.POINTER(LFQCfg), _P, C.c_int64, C.c_int32, _P, _P, _P, _P], C.c_int),
    "dctae_lfq_project_out_inverse_norm_c16": ([_P, C.POINTER(LFQCfg), _P, C.c_int64, C.c_int32, _P, _P,
                                                C.POINTER(Norm), C.c_int32, C.c_int32, _P, _P, _P, _P], C.c_int),
    "dctae_decode_backward": ([_P, C.POINTER(FECfg), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                               C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), _P, _P, _P, _P,
                               _P, _P, _P, _P, _P, _P, _P], C.c_int),
    "dctae_pixel_loss_forward": ([_P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), _P, _P, _P, _P],
                                 C.c_int),
    "dctae_vq_forward": ([_P, C.POINTER(VQCfg), _P, _P, C.c_int64, _P, _P, _P], C.c_int),
    "dctae_vq_codes_from_indices": ([_P, C.POINTER(VQCfg), _P, C.c_int64, _P, _P], C.c_int),
    "dctae_vq_output_from_indices": ([_P, C.POINTER(VQCfg), _P, C.c_int64, _P, _P], C.c_int),
    "dctae_check_device_errors": ([_P, _P], C.c_int),
    "dctae_synth_images": ([_P, C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P], C.c_int),
    "dctae_set_timing": ([_P, C.c_int], C.c_int),
    "dctae_timing_collect": ([_P], C.c_int),
    "dctae_timing_get": ([_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_int64)],
                         C.c_int),
    "dctae_timing_reset": ([_P], C.c_int),
    "dctae_set_workspace_limit": ([_P, C.c_int64], C.c_int),
    "dctae_norm_thresholds": ([_P, C.POINTER(Norm), C.c_int64, _P, _P], C.c_int),
    "dctae_set_fft": ([_P, C.c_int], C.c_int),
    "dctae_set_chunk_bytes": ([_P, C.c_int64], C.c_int),
    "dctae_set_option": ([_P, C.c_char_p, C.c_int64], C.c_int),
    "dctae_norm_batch_stats": ([_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int64, _P, _P,
                                _P], C.c_int),
    "dctae_norm_batch_mad": ([_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int64, _P, _P,
                              _P], C.c_int),
    "dctae_norm_merge": ([_P, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, _P], C.c_int),
    "dctae_norm_train_step": ([_P, C.POINTER(Norm), _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P,
                               C.c_int64, _P, _P], C.c_int),
    # DCTAutoencoder transformer operators
    "dctae_model_linear": ([_P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64, _P, C.c_int32, C.c_int64, _P,
                            C.c_int32, _P, C.c_int64, _P], C.c_int),
    "dctae_model_attention": ([_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int64, _P],
                              C.c_int),
    "dctae_model_layernorm": ([_P, C.c_int64, C.c_int32, _P, C.c_int64, _P, _P, C.c_float, _P, C.c_int64, _P],
                              C.c_int),
    "dctae_model_embed_norm": ([_P, C.c_int64, C.c_int32, _P, C.c_int64, _P, _P, C.c_float, _P, _P, _P, _P, _P, _P,
                                C.c_int64, _P], C.c_int),
    "dctae_model_pos_add": ([_P, C.c_int64, C.c_int32, _P, C.c_int64, _P, _P, _P, _P, _P, _P], C.c_int),
    "dctae_model_to_bf16": ([_P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int32, _P, _P], C.c_int),
    "dctae_model_lfq": ([_P, C.c_int64, C.c_int32, C.c_int32, C.c_float, _P, C.c_int64, _P, _P, _P, C.c_int64, _P],
                        C.c_int),
    "dctae_model_attention_lse": ([_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int64, _P, _P],
                                  C.c_int),
    "dctae_model_attention_bwd": ([_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int64, _P,
                                   C.c_int64, _P, _P, _P, _P], C.c_int),
    "dctae_model_transpose_pack": ([_P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int64, _P, _P], C.c_int),
    "dctae_model_colsum": ([_P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int32, _P, _P, _P], C.c_int),
    "dctae_model_layernorm_bwd": ([_P, C.c_int64, C.c_int32, _P, C.c_int64, _P, C.c_float, _P, C.c_int64, _P,
                                   C.c_int64, C.c_int32, _P, _P, _P], C.c_int),
    "dctae_model_qgelu": ([_P, C.c_int64, C.c_int32, _P, C.c_int64, _P, C.c_int64, _P], C.c_int),
    "dctae_model_qgelu_bwd": ([_P, C.c_int64, C.c_int32, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, _P], C.c_int),
    "dctae_model_pos_grad": ([_P, C.c_int64, C.c_int32, _P, C.c_int64, _P, C.c_int64, C.c_int32, _P, _P], C.c_int),
    # fused optimizer step; the table is an OptimSeg array
    "dctae_optim_plan": ([_P, _P, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)], C.c_int),
    "dctae_optim_gradnorm": ([_P, _P, C.c_int32, C.c_int64, C.c_float, _P, _P, _P], C.c_int),
    "dctae_optim_adamw_pack": ([_P, _P, C.c_int32, C.c_int64, C.POINTER(OptimGroup), C.c_int32, _P, _P], C.c_int),
}

_lib = None
_lib_lock = threading.Lock()


def load_library():
    """dlopen libdctae.so and bind every symbol of include/dctae.h (no GPU needed)."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise DCTAEUnavailable(f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C csrc)")
        lib = C.CDLL(LIB_PATH)
        for name, (args, res) in _SIGS.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = res
        v = lib.dctae_abi_version()
        if v != ABI_VERSION:
            raise DCTAEUnavailable(f"libdctae ABI {v} != {ABI_VERSION}")
        _lib = lib
        return lib


class Context:
    """One dctae_ctx per (device, thread)."""

    def __init__(self, device: int):
        lib = load_library()
        h = C.c_void_p()
        rc = lib.dctae_ctx_create(int(device), C.byref(h))
        if rc != 0:
            raise DCTAEUnavailable(f"dctae_ctx_create(device={device}) failed ({rc}): "
                                   f"{lib.dctae_last_error(None).decode()}")
        self.lib = lib
        self.h = h
        self.device = device
        from . import color
        m = color.matrices()
        keep = [m[k].contiguous().float().cpu() for k in ("rgb2lms", "lms2ipt", "ipt2lms", "lms2rgb")]
        self.check(lib.dctae_set_color_matrices(h, *[C.c_void_p(t.data_ptr()) for t in keep]))

    def check(self, rc: int, what: str = ""):
        if rc != 0:
            msg = self.lib.dctae_last_error(self.h).decode()
            if rc == -1:
                raise AssertionError(f"{what}: {msg}")
            raise DCTAEError(f"{what} failed ({rc}): {msg}")

    def __del__(self):
        try:
            if getattr(self, "h", None) is not None and self.h.value:
                self.lib.dctae_ctx_destroy(self.h)
        except Exception:
            pass


_ctx_by_key: Dict = {}


def context(device: Optional[torch.device] = None) -> Context:
    if not torch.cuda.is_available():
        raise DCTAEUnavailable("no HIP device visible (torch.cuda.is_available() is False)")
    if device is None:
        idx = torch.cuda.current_device()
    else:
        device = torch.device(device)
        if device.type != "cuda":
            raise DCTAEUnavailable(f"tensor on {device}: the MI355X path needs HIP device tensors")
        idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, threading.get_ident())
    ctx = _ctx_by_key.get(key)
    if ctx is None:
        ctx = Context(idx)
        _ctx_by_key[key] = ctx
    return ctx


def stream_ptr(device=None) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def i32(vals):
    arr = (C.c_int32 * max(1, len(vals)))(*[int(v) for v in vals])
    return arr


def i64(vals):
    arr = (C.c_int64 * max(1, len(vals)))(*[int(v) for v in vals])
    return arr
