"""The dataset's crop in front of the encode (the reference's dataset.py:53-73):
every image whose longer side exceeds ``max_size`` is shrunk by an
antialiased bilinear resize before ``preprocess`` sees it.  The resize runs on
the GPU, one launch for a ragged list of fp32 or uint8 images
(dctae_resize_aa, include/dctae_resize.h); its arithmetic is defined in
csrc/dctae_resize_math.h and mirrored in numpy by tests/resize_mirror.py.

  dataset_max_size(patch_size, max_patch_h, max_patch_w)   dataset.py:53-57
  dataset_crop_size(h, w, max_size)                        dataset.py:59-71 + torchvision 0.16.1's Resize(int)
  resize_antialias(images, sizes)                          interpolate(mode="bilinear", antialias=True)
  dataset_crop(images, max_size)                           dataset.py:59-73 for a list of images

Inputs must be finite: the outermost tap of a window can have weight zero,
and zero times an infinity is NaN (as in torch).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib, _ops
from ._lib import i32, i64, ptr


def dataset_max_size(patch_size: int, max_patch_h: int, max_patch_w: int) -> int:
    """dataset.py:53-57: "some buffer room, gives you better dct features to use bigger images" """
    return max(int(patch_size) * max(int(max_patch_w), int(max_patch_h)), 768)


def dataset_crop_size(h: int, w: int, max_size: int) -> Optional[Tuple[int, int]]:
    """The (height, width) the reference's crop gives an (h, w) image, or None
    where it leaves the image alone.  dataset.py:59-71 picks the target of the
    shorter side, and torchvision 0.16.1's Resize(int) derives the longer one
    from the original aspect ratio with a truncation of its own, so the longer
    side often ends below max_size: part of the contract."""
    h, w, max_size = int(h), int(w), int(max_size)
    if h <= 0 or w <= 0 or max_size <= 0:
        raise ValueError(f"dataset_crop_size: sizes must be positive, got h={h}, w={w}, max_size={max_size}")
    if max(h, w) <= max_size:
        return None
    ar = h / w
    if h > w:
        th = max_size
        tw = int(th / ar)
    else:
        tw = max_size
        th = int(ar * tw)
    s = min(th, tw)
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = s, int(s * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def _check_images(images, what: str) -> List[torch.Tensor]:
    images = list(images)
    for im in images:
        if not isinstance(im, torch.Tensor) or im.dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"{what}: float32 or uint8 tensors expected, got {getattr(im, 'dtype', type(im))}")
    if len({im.dtype for im in images}) > 1:
        raise TypeError(f"{what}: all images must have one dtype, got float32 and uint8")
    for im in images:
        if im.dim() != 3 or im.shape[0] != 3 or im.shape[1] < 1 or im.shape[2] < 1:
            raise ValueError(f"{what}: expected (3, h, w) images, got {tuple(im.shape)}")
    return images


@torch.no_grad()
def resize_antialias(images: Sequence[torch.Tensor], sizes: Sequence[Tuple[int, int]]) -> List[torch.Tensor]:
    """``interpolate(im[None], size, mode="bilinear", antialias=True)[0]`` for
    every (3, H, W) image of a list on the GPU, fp32 or uint8 (all of one
    dtype; a byte means ``u8.float() / 255``), in one library call with one
    output allocation: the results are fp32 views of it.  An fp32 image whose
    size already matches is returned as it is, as torchvision's Resize does; a
    byte image of matching size comes back as exactly ``u8 / 255``."""
    images = _check_images(images, "resize_antialias")
    sizes = [tuple(int(v) for v in s) for s in sizes]
    if len(sizes) != len(images):
        raise ValueError(f"resize_antialias: {len(images)} images, {len(sizes)} sizes")
    for s in sizes:
        if len(s) != 2 or s[0] < 1 or s[1] < 1:
            raise ValueError(f"resize_antialias: a size is (height, width), both positive, got {s}")
    if not images:
        return []
    u8 = images[0].dtype == torch.uint8
    todo = [i for i, (im, s) in enumerate(zip(images, sizes)) if u8 or tuple(im.shape[1:]) != s]
    outs = list(images)
    if not todo:
        _ops._check_dev(*images)
        return outs
    src = [images[i] if images[i].is_contiguous() else images[i].contiguous() for i in todo]
    dev = _ops._check_dev(*src)
    ctx = _lib.context(dev)
    ptrs = [im.data_ptr() for im in src]
    base = min(ptrs)
    in_off = i64([(p - base) // (1 if u8 else 4) for p in ptrs])
    in_hw = i32([v for im in src for v in im.shape[1:]])
    desc = (_lib.ImagesU8 if u8 else _lib.Images)(C.c_void_p(base), C.cast(in_off, C.POINTER(C.c_int64)),
                                                  C.cast(in_hw, C.POINTER(C.c_int32)), len(src))
    offs, total = [], 0
    for i in todo:
        offs.append(total)
        total += 3 * sizes[i][0] * sizes[i][1]
    buf = torch.empty(total, dtype=torch.float32, device=dev)
    out_off = i64(offs)
    out_hw = i32([v for i in todo for v in sizes[i]])
    odesc = _lib.ImagesOut(ptr(buf), C.cast(out_off, C.POINTER(C.c_int64)), C.cast(out_hw, C.POINTER(C.c_int32)),
                           len(src))
    name = "dctae_resize_aa_u8" if u8 else "dctae_resize_aa"
    ctx.check(getattr(ctx.lib, name)(ctx.h, C.byref(desc), C.byref(odesc), _lib.stream_ptr(dev)), name)
    for i, o in zip(todo, offs):
        oh, ow = sizes[i]
        outs[i] = buf[o:o + 3 * oh * ow].view(3, oh, ow)
    return outs


@torch.no_grad()
def dataset_crop(images: Sequence[torch.Tensor], max_size: int) -> List[torch.Tensor]:
    """dataset.py:59-73 for a list of (3, H, W) images on the GPU: those with a
    side above max_size are resized to dataset_crop_size, in one launch.  If
    none is, the list comes back untouched (bytes stay bytes).  If any is and
    the images are bytes, all of them go through the one call (those that keep
    their size become exactly ``u8 / 255``), so the result is fp32 throughout."""
    images = _check_images(images, "dataset_crop")
    new = [dataset_crop_size(im.shape[1], im.shape[2], max_size) for im in images]
    if all(s is None for s in new):
        return images
    return resize_antialias(images, [s if s is not None else tuple(im.shape[1:]) for im, s in zip(images, new)])
