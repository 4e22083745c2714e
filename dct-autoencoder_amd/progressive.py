"""Progressive decode (include/dctae_frames.h): the token-prefix frames of the
images of a packed batch in one launch sequence, and the reference's min-max
``image_clip`` (util.py:143-147).

The encode sorts every image's tokens by importance, so a prefix of the stream
is already a usable image; the reference's decode_gif.py decodes
``codes[:, :i]`` for growing ``i`` and passes each frame through ``image_clip``.

The contract.  A packed batch enumerates its images as everywhere else in the
package: rows in order, ids ascending within a row (the order of
``patch_sizes`` / ``original_sizes``).  Image ``i`` has ``n_i`` real tokens:
the slots of its row with its id and ``key_pad_mask == False``, in slot order.
The PREFIX FRAME ``(i, k)``, ``k >= 0``, is what ``postprocess`` (or
``decode_batch``) returns for image ``i`` when ``key_pad_mask`` is additionally
set on every token of image ``i`` except its first ``min(k, n_i)`` real
tokens -- bit for bit, on every decode path, for every token source and both
output types.  So ``k = 0`` is the decode of an empty spectrum, ``k >= n_i``
the full image, interior padded slots do not count towards ``k``, and of two
tokens at one place inside the prefix the later slot wins.

``prefixes`` is one sequence of ints applied to every image, or one sequence
per image; the result is a list per image of that image's frames, in the order
of its prefixes.

Through the transformer (include/dctae_model_prefix.h).  The frames
above cut the token stream in front of the feature extractor's decode; the
reference's decode_gif.py cuts it in front of the trained decoder:
``autoenc.decode_from_codes(codes[:, :i], ...)`` on a one-image row, then
``proc.postprocess``.  The MODEL PREFIX FRAME ``(i, k)``, ``k >= 0``, with
``m = min(k, n_i)``:

  * ``m >= 1``: take the first ``m`` real tokens of image ``i`` (interior padded
    slots skipped), place them as a one-row batch of length ``m`` with
    ``key_pad_mask`` all False and ``batched_image_ids`` all 0, run
    ``model.decode_from_codes(codes_row, do_inv_norm=True, **that_row)`` in
    ``.eval()``, then ``fe.postprocess``.  The frame equals that result bit for
    bit (decode_gif.py:60-77 on its one-image row).
  * ``m == 0``: the decode of an empty spectrum, bit for bit what
    ``fe.postprocess_prefixes(dp, [0])`` returns for image ``i``.

So a frame does not depend on which other images or how much padding share the
row, and the ``k >= n_i`` frame is the image decoded alone in an unpadded row.
That is in general NOT image ``i`` of ``model.decode_from_codes`` on the packed
batch: there the row's other images and its pad keys take part in every
softmax, because the reference's boolean ``attn_mask`` is added to the logits
and masks nothing.  For the same reason a frame is a truncated row, not a
masked one.  ``model_decode_prefixes`` batches the frames without padding: every
linear, LayerNorm and position kernel is token-wise, and the attention kernel
reads its row's first token and length from a table.
"""
from __future__ import annotations

import ctypes as C
import numbers
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib, _ops
from ._lib import Frames, i32, i64, ptr

# One library call's scratch (per frame the spectrum corner, the column pass's
# output and the IPT image of the GEMM path, the frame's slot map and, for
# clipped bytes, its fp32 pixels) stays under this many bytes: the frame list is
# cut into chunks of consecutive frames, at least one frame each.  A frame's
# pixels do not depend on the other frames of its call, so the result does not
# depend on the cut.
FRAME_SCRATCH_BYTES = 1 << 30
MAX_FRAMES_PER_CALL = 65535   # the library's bound on n_frames
# The model prefix frames of one pass through the decoder hold at most this many
# tokens together (one frame at least): the frame list is cut into chunks of
# consecutive frames.  Every kernel but attention is token-wise and attention
# stays inside a frame, so a frame's values do not depend on the cut.
PREFIX_TOKENS_PER_CALL = 32768


def _check_clip(clip) -> int:
    if clip is None:
        return _lib.CLIP_NONE
    if clip == "minmax":
        return _lib.CLIP_MINMAX
    raise ValueError(f'clip: None or "minmax", got {clip!r}')


def _pixel_tag(dtype: torch.dtype, what: str) -> int:
    return _lib.PIXEL_U8 if _ops.out_dtype_suffix(dtype, what) else _lib.PIXEL_F32


def _split_prefixes(prefixes):
    """(shared, lists): ``prefixes`` as one list of ints for every image (shared) or as one list per image;
    a negative prefix or a mix of ints and sequences is a ValueError"""
    prefixes = list(prefixes)
    shared = all(isinstance(k, numbers.Integral) for k in prefixes)
    if not shared and any(isinstance(k, numbers.Integral) for k in prefixes):
        raise ValueError("prefixes: either ints, or one sequence of ints per image")
    lists = [[int(k) for k in prefixes]] if shared else [[int(k) for k in ks] for ks in prefixes]
    for ks in lists:
        for k in ks:
            if k < 0:
                raise ValueError(f"prefixes: a prefix length must be >= 0, got {k}")
    return shared, lists


def per_image_prefixes(prefixes, n_img: int) -> List[List[int]]:
    """``prefixes`` as one list of ints per image: a sequence of ints is every
    image's; a sequence of sequences must have one per image (ValueError).  A
    negative prefix is a ValueError."""
    shared, lists = _split_prefixes(prefixes)
    if shared:
        return [list(lists[0]) for _ in range(n_img)]
    if len(lists) != n_img:
        raise ValueError(f"prefixes: {len(lists)} per-image sequences for {n_img} images")
    return lists


def _places(ids: torch.Tensor) -> List[Tuple[int, int]]:
    """(row, id) of image 0, 1, ...: rows in order, ids ascending (FE:619-633)"""
    return [(r, int(i)) for r in range(ids.shape[0]) for i in torch.unique(ids[r]).tolist()]


def frame_cuts(ids: torch.Tensor, key_pad: torch.Tensor, prefixes) -> Tuple[List[int], List[int]]:
    """The frames of ``prefixes`` on the batch (``ids`` (R, S) integer,
    ``key_pad`` (R, S) bool, CPU tensors), image by image and within an image in
    the order of its prefixes: ``(img, cut)``, frame ``f`` holding the tokens of
    image ``img[f]`` at row slots ``j < cut[f]``.  The cut of prefix ``k`` is 0
    for ``min(k, n_i) = 0``, else one past the slot of the image's
    ``min(k, n_i)``-th real token.  A pure host function."""
    ids = torch.as_tensor(ids).long()
    key_pad = torch.as_tensor(key_pad).to(torch.bool)
    if ids.is_cuda or key_pad.is_cuda:
        raise TypeError("frame_cuts works on CPU tensors: pass ids.cpu() / key_pad.cpu()")
    if ids.dim() != 2 or ids.shape != key_pad.shape:
        raise ValueError(f"ids {tuple(ids.shape)} and key_pad {tuple(key_pad.shape)} must be (R, S) both")
    places = _places(ids)
    per = per_image_prefixes(prefixes, len(places))
    img, cut = [], []
    for i, (r, lid) in enumerate(places):
        if not per[i]:
            continue
        slots = torch.nonzero((ids[r] == lid) & ~key_pad[r]).flatten().tolist()   # ascending
        for k in per[i]:
            kk = min(k, len(slots))
            img.append(i)
            cut.append(slots[kk - 1] + 1 if kk else 0)
    return img, cut


def prefix_key_pad(ids: torch.Tensor, key_pad: torch.Tensor, cut_of_image: Sequence[Optional[int]]) -> torch.Tensor:
    """``key_pad`` (CPU) with every slot ``j >= cut_of_image[i]`` of image ``i``'s
    row slots set as well (None: the image as it is): the batch whose decode
    is, by definition, the frame of every image at that cut."""
    ids = torch.as_tensor(ids).long()
    out = torch.as_tensor(key_pad).to(torch.bool).clone()
    slot = torch.arange(ids.shape[1])
    for i, (r, lid) in enumerate(_places(ids)):
        if cut_of_image[i] is not None:
            out[r] |= (ids[r] == lid) & (slot >= int(cut_of_image[i]))
    return out


def _frame_scratch_bytes(p, hw, phw, staged: bool) -> int:
    """an upper bound of one frame's share of a call's scratch (the GEMM path's; the FFT path needs less)"""
    (h, w), (ph, pw) = hw, phw
    kh, kw = p.patch_size * min(ph, p.max_patch_h), p.patch_size * min(pw, p.max_patch_w)
    n = 3 * (kh * kw + h * kw + h * w) + 3 * p.max_patch_h * p.max_patch_w + 64 * 4
    if staged:
        n += 3 * h * w + 64
    return 4 * n


def _chunks(costs: Sequence[int], budget: int) -> List[Tuple[int, int]]:
    """[begin, end) runs of consecutive frames whose costs stay within the budget (one frame at least)"""
    out, b, acc = [], 0, 0
    for f, c in enumerate(costs):
        if f > b and (acc + c > budget or f - b >= MAX_FRAMES_PER_CALL):
            out.append((b, f))
            b, acc = f, 0
        acc += c
    if len(costs) > b:
        out.append((b, len(costs)))
    return out


@torch.no_grad()
def decode_frames(p, ids, key_pad, positions, channels, patch_sizes, original_sizes, prefixes,
                  output_dtype: torch.dtype = torch.float32, clip=None, codes: Optional[torch.Tensor] = None,
                  patches: Optional[torch.Tensor] = None, norm=None, lfq=None, normed: bool = False
                  ) -> List[List[torch.Tensor]]:
    """dctae_decode_frames on a packed batch (the arguments of ``_ops.decode``):
    per image the list of its prefix frames, (3, H, W) tensors of
    ``output_dtype``.  Reading ``ids`` and ``key_pad`` on the host is the call's
    one host synchronisation."""
    px = _pixel_tag(output_dtype, "prefix frames output_dtype")
    cl = _check_clip(clip)
    if codes is not None:
        _ops.codes_dtype_suffix(codes.dtype, "prefix frames codes")
        if codes.dtype == torch.int16 and lfq is not None:
            _ops.check_codes16(lfq, "prefix frames")
    _split_prefixes(prefixes)   # a negative prefix is refused before anything is read
    ids_h, kp_h = ids.cpu(), key_pad.cpu()
    img, cut = frame_cuts(ids_h, kp_h, prefixes)
    dev = _ops._check_dev(ids, key_pad, positions, channels, codes, patches)
    if normed and (norm is None or codes is not None):
        raise AssertionError("normed decode needs the PatchNorm state and patches (no codes)")
    table = _ops.DecodeTable(p, ids, key_pad, positions, channels, patch_sizes, original_sizes, ids_host=ids_h.long())
    cc = _ops.codes_in(codes, lfq, "prefix frames")[0] if codes is not None else None
    pp = patches.detach().float().contiguous() if patches is not None else None
    ctype = _lib.CODES_I16 if cc is not None and cc.dtype == torch.int16 else _lib.CODES_I64
    ncfg = norm.c() if norm is not None else None
    hw = [(table.hw[2 * i], table.hw[2 * i + 1]) for i in range(table.n_img)]
    phw = [(table.phw[2 * i], table.phw[2 * i + 1]) for i in range(table.n_img)]
    staged = cl == _lib.CLIP_MINMAX and px == _lib.PIXEL_U8
    numel = [3 * hw[i][0] * hw[i][1] for i in img]
    costs = [_frame_scratch_bytes(p, hw[i], phw[i], staged) for i in img]
    ctx = _lib.context(dev)
    cfg = p.c(table.S)
    lut, lut_w, n_img, out_hw, _, patch_hw = table.c_args()
    frames: List[torch.Tensor] = []
    for b, e in _chunks(costs, FRAME_SCRATCH_BYTES):
        offs, total = [], 0
        for f in range(b, e):
            offs.append(total)
            total += (numel[f] + 3) & ~3   # every frame starts 4-byte aligned in a byte buffer
        out = torch.empty(total, dtype=output_dtype, device=dev)
        keep = (i32(img[b:e]), i32(cut[b:e]), i64(offs))
        fr = Frames(e - b, C.cast(keep[0], C.POINTER(C.c_int32)), C.cast(keep[1], C.POINTER(C.c_int32)),
                    C.cast(keep[2], C.POINTER(C.c_int64)))
        rc = ctx.lib.dctae_decode_frames(ctx.h, C.byref(cfg), table.R, lut, lut_w, n_img, out_hw, patch_hw,
                                         ptr(table.ids), ptr(table.key_pad), ptr(table.pos), ptr(table.ch),
                                         C.byref(fr), C.byref(ncfg) if ncfg is not None else None,
                                         C.byref(lfq) if lfq is not None else None, ptr(cc), ctype, ptr(pp),
                                         1 if normed else 0, cl, ptr(out), px, _lib.stream_ptr(dev))
        ctx.check(rc, "dctae_decode_frames")
        for f, o in zip(range(b, e), offs):
            h, w = hw[img[f]]
            frames.append(out[o: o + numel[f]].view(3, h, w))
    if normed:
        _ops.check_device_errors(dev)
    res: List[List[torch.Tensor]] = [[] for _ in range(table.n_img)]
    for i, t in zip(img, frames):
        res[i].append(t)
    return res


def _clip_images(images: Sequence[torch.Tensor], output_dtype: torch.dtype) -> List[torch.Tensor]:
    px = _pixel_tag(output_dtype, "image_clip output_dtype")
    ims = []
    for im in images:
        if not isinstance(im, torch.Tensor) or im.dtype != torch.float32:
            raise TypeError(f"image_clip: fp32 tensors expected, got {getattr(im, 'dtype', type(im))}")
        if im.dim() != 3 or im.shape[0] != 3 or im.numel() == 0:
            raise ValueError(f"image_clip: (3, H, W) images expected, got {tuple(im.shape)}")
        ims.append(im.detach() if im.is_contiguous() else im.detach().contiguous())
    if not ims:
        return []
    dev = _ops._check_dev(*ims)
    base = min(im.data_ptr() for im in ims)
    if any((im.data_ptr() - base) % 4 for im in ims):
        ims = [im.clone() if (im.data_ptr() - base) % 4 else im for im in ims]   # never for torch's own allocations
        base = min(im.data_ptr() for im in ims)
    hw, in_off, out_off, total = [], [], [], 0
    for im in ims:
        hw += [im.shape[1], im.shape[2]]
        in_off.append((im.data_ptr() - base) // 4)
        out_off.append(total)
        total += (im.numel() + 3) & ~3
    out = torch.empty(total, dtype=output_dtype, device=dev)
    ctx = _lib.context(dev)
    keep = (i32(hw), i64(in_off), i64(out_off))
    rc = ctx.lib.dctae_image_clip(ctx.h, len(ims), C.cast(keep[0], C.POINTER(C.c_int32)),
                                  C.cast(keep[1], C.POINTER(C.c_int64)), C.c_void_p(base),
                                  C.cast(keep[2], C.POINTER(C.c_int64)), ptr(out), px, _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_image_clip")
    return [out[o: o + im.numel()].view(im.shape) for o, im in zip(out_off, ims)]


@torch.no_grad()
def image_clip_many(images: Sequence[torch.Tensor], output_dtype: torch.dtype = torch.float32) -> List[torch.Tensor]:
    """``image_clip`` of a list of (3, H, W) fp32 device images of any sizes in
    one launch sequence (dctae_image_clip): per image
    ``(x - x.min()) / (x.max() - x.min())`` over its 3 H W values, in fp32 (min
    and max exact, one subtraction and one division per pixel, each correctly
    rounded).  ``output_dtype=torch.uint8``: that value through the byte
    decode's quantiser (NaN gives 0).  A constant image gives NaN / 0.  Inputs
    must be finite."""
    return _clip_images(list(images), output_dtype)


def image_clip(x: torch.Tensor, output_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """util.py:143-147 on one fp32 device tensor: ``(x - x.min()) / (x.max() - x.min())``
    over all its values (a (3, H, W) image; any shape whose element count is a multiple of 3)."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise TypeError(f"image_clip: an fp32 tensor expected, got {getattr(x, 'dtype', type(x))}")
    if x.numel() == 0 or x.numel() % 3:
        raise ValueError(f"image_clip: the element count must be a positive multiple of 3, got shape {tuple(x.shape)}")
    (y,) = image_clip_many([x.detach().contiguous().view(3, -1, 1)], output_dtype)
    return y.view(x.shape)


def _staged_frames(fe, x, prefixes, output_dtype, clip) -> List[List[torch.Tensor]]:
    """the frames through an overridden revert_patching / _transform_image_out: the reference's stage sequence
    on one masked batch per prefix position (correct, not fast)"""
    ids_h, kp_h = x.batched_image_ids.cpu(), x.key_pad_mask.cpu()
    img, cut = frame_cuts(ids_h, kp_h, prefixes)
    n_img = len(_places(ids_h.long()))
    per: List[List[int]] = [[] for _ in range(n_img)]
    for i, c in zip(img, cut):
        per[i].append(c)
    res: List[List[torch.Tensor]] = [[] for _ in range(n_img)]
    for j in range(max((len(c) for c in per), default=0)):
        cuts = [c[j] if j < len(c) else None for c in per]
        dp = x.shallow_copy()
        dp.key_pad_mask = prefix_key_pad(ids_h, kp_h, cuts).to(x.key_pad_mask.device)
        images = fe._postprocess_no_grad(dp, torch.float32)
        for i in range(n_img):
            if cuts[i] is not None:
                res[i].append(images[i])
    if clip is not None or output_dtype == torch.uint8:
        flat = [im.float() for ims in res for im in ims]
        flat = (_clip_images(flat, output_dtype) if clip is not None else [_ops.f32_to_u8(im) for im in flat])
        it = iter(flat)
        res = [[next(it) for _ in ims] for ims in res]
    return res


@torch.no_grad()
def postprocess_prefixes(fe, x, prefixes, output_dtype: torch.dtype = torch.float32, clip=None
                         ) -> List[List[torch.Tensor]]:
    """The prefix frames of un-normalised DCTPatches (``fe.postprocess`` of every
    image at every prefix): see the module docstring.  ``clip="minmax"``: every
    frame through ``image_clip``.  Frames carry no grad_fn.  With an overridden
    revert_patching / _transform_image_out the frames come from the
    reference's stage sequence, frame by frame."""
    _pixel_tag(output_dtype, "postprocess_prefixes output_dtype")
    _check_clip(clip)
    if fe._staged_out():
        return _staged_frames(fe, x, prefixes, output_dtype, clip)
    return decode_frames(fe.params(x.patches.shape[1]), x.batched_image_ids, x.key_pad_mask, x.patch_positions,
                         x.patch_channels, x.patch_sizes, x.original_sizes, prefixes, output_dtype, clip,
                         patches=x.patches)


@torch.no_grad()
def decode_prefixes(fe, dct_patches, codes: torch.Tensor, patchnorm, lfq, prefixes,
                    output_dtype: torch.dtype = torch.float32, clip=None) -> List[List[torch.Tensor]]:
    """The prefix frames from LFQ codes (``fe.decode_batch`` of every image at
    every prefix), on decode_batch's branches: fused from the codes; with LFQ
    projections through project_out and a PatchNorm-space decode; with
    overridden hooks through the stages.  codes: int64, or int16 read as they are."""
    _pixel_tag(output_dtype, "decode_prefixes output_dtype")
    _check_clip(clip)
    _ops.codes_dtype_suffix(codes.dtype, "decode_prefixes codes")
    if codes.dtype == torch.int16:
        _ops.check_codes16(lfq.cfg(), "decode_prefixes")
    dp = dct_patches
    args = lambda: (fe.params(dp.key_pad_mask.shape[1]), dp.batched_image_ids, dp.key_pad_mask,   # noqa: E731
                    dp.patch_positions, dp.patch_channels, dp.patch_sizes, dp.original_sizes, prefixes,
                    output_dtype, clip)
    staged = fe._staged_out()
    if lfq.has_projections or staged:
        if lfq.has_projections and lfq._fused_proj() and lfq.dim == fe.patch_size ** 2 and not staged:
            w, b = lfq._proj_w(lfq.project_out, codes.device)
            x = _ops.lfq_project_out(codes, w, b, lfq.cfg())
            return decode_frames(*args(), patches=x, norm=patchnorm.state(thresholds=False), normed=True)
        dp = dct_patches.shallow_copy()
        dp.patches = lfq.indices_to_codes(codes)
        dp.patches = patchnorm.inverse_norm(dp)
        return postprocess_prefixes(fe, dp, prefixes, output_dtype, clip)
    return decode_frames(*args(), codes=codes, norm=patchnorm.state(), lfq=lfq.cfg())


# ---- model prefix frames (through the transformer decoder) -----------------------------------
class ModelFrames(NamedTuple):
    """the frames of ``prefixes``, image by image and within an image in prefix
    order: frame ``f`` is image ``img[f]`` at prefix ``k[f]``, the first ``m[f]``
    real tokens of id ``lid[f]`` in row ``row[f]``; ``n_img`` images in the batch"""
    img: List[int]
    k: List[int]
    row: List[int]
    lid: List[int]
    m: List[int]
    n_img: int


def model_frames(ids: torch.Tensor, key_pad: torch.Tensor, prefixes) -> ModelFrames:
    """The model prefix frames of ``prefixes`` on the batch (``ids`` (R, S)
    integer, ``key_pad`` (R, S) bool, CPU tensors), ``m = min(k, n_i)`` each
    (0: the frame goes round the model).  A pure host function."""
    ids = torch.as_tensor(ids).long()
    key_pad = torch.as_tensor(key_pad).to(torch.bool)
    if ids.is_cuda or key_pad.is_cuda:
        raise TypeError("model_frames works on CPU tensors: pass ids.cpu() / key_pad.cpu()")
    if ids.dim() != 2 or ids.shape != key_pad.shape:
        raise ValueError(f"ids {tuple(ids.shape)} and key_pad {tuple(key_pad.shape)} must be (R, S) both")
    places = _places(ids)
    per = per_image_prefixes(prefixes, len(places))
    out = ModelFrames([], [], [], [], [], len(places))
    for i, (r, lid) in enumerate(places):
        if not per[i]:
            continue
        n = int(((ids[r] == lid) & ~key_pad[r]).sum())
        for k in per[i]:
            out.img.append(i)
            out.k.append(k)
            out.row.append(r)
            out.lid.append(lid)
            out.m.append(min(k, n))
    return out


def model_frame_chunks(ms: Sequence[int], budget: Optional[int] = None) -> List[Tuple[int, int]]:
    """[begin, end) runs of consecutive frames of ``ms`` tokens each whose token
    total stays within ``budget`` (default PREFIX_TOKENS_PER_CALL), one frame at
    least per run (a frame longer than the budget is a run of its own)"""
    return _chunks(list(ms), PREFIX_TOKENS_PER_CALL if budget is None else budget)


def _fft_sized(fe, size) -> bool:
    """the images whose one-image batch the decode sends down its 512 x 512 path (dctae_frames.h)"""
    return tuple(int(v) for v in size) == (512, 512) and fe.patch_size == 14


@torch.no_grad()
def model_decode_prefixes(fe, model, dct_patches, codes: torch.Tensor, prefixes,
                          output_dtype: torch.dtype = torch.float32, clip=None) -> List[List[torch.Tensor]]:
    """The model prefix frames of a packed batch (module docstring): per image
    the list of its (3, H, W) frames of ``output_dtype`` in prefix order, the
    decoder run once per chunk of frames (``model.decode_prefixes``) and the
    frames batch passed through ``fe.postprocess`` (overridden stage hooks
    included); ``clip="minmax"``: every frame through ``image_clip``, bytes
    from the clipped fp32 value.  Frames with ``min(k, n_i) == 0`` come from
    ``postprocess_prefixes`` at prefix 0."""
    _pixel_tag(output_dtype, "model_decode_prefixes output_dtype")
    _check_clip(clip)
    dp, which, plan, layout = model._decode_prefixes(dct_patches, codes, prefixes, do_inv_norm=True)
    post_dtype = torch.float32 if clip is not None else output_dtype
    live: List[torch.Tensor] = []
    if dp is not None:
        # the decode picks its path from the whole batch it is given: the frames of images that a one-image
        # batch sends down the 512 x 512 path are kept apart from the others, run by run within a row
        kind = [(row, _fft_sized(fe, dp.original_sizes[f])) for f, (row, _, _) in enumerate(layout)]
        b = 0
        while b < len(layout):
            e = b + 1
            while e < len(layout) and kind[e] == kind[b]:
                e += 1
            row, lo, hi = layout[b][0], layout[b][1], layout[e - 1][1] + layout[e - 1][2]
            sub = dp.shallow_copy()
            sub.attn_mask = None
            sub.patches = dp.patches[row:row + 1, lo:hi].contiguous()
            sub.key_pad_mask = dp.key_pad_mask[row:row + 1, lo:hi].contiguous()
            sub.batched_image_ids = (dp.batched_image_ids[row:row + 1, lo:hi] - dp.batched_image_ids[row, lo]).contiguous()
            sub.patch_channels = dp.patch_channels[row:row + 1, lo:hi].contiguous()
            sub.patch_positions = dp.patch_positions[row:row + 1, lo:hi].contiguous()
            sub.patch_sizes, sub.original_sizes = dp.patch_sizes[b:e], dp.original_sizes[b:e]
            live += fe._postprocess_no_grad(sub, post_dtype)
            b = e
        if clip is not None:
            live = _clip_images([im.float() for im in live], output_dtype)
    # the frames that hold no token: the k = 0 frames of the batch as it is (no patch value is read)
    zero_of = {}
    need = sorted({i for i, m in zip(plan.img, plan.m) if m == 0})
    if need:
        dp0 = dct_patches.shallow_copy()
        r, s = dct_patches.key_pad_mask.shape
        dp0.patches = torch.zeros(r, s, fe.patch_size ** 2, device=dct_patches.key_pad_mask.device)
        z = postprocess_prefixes(fe, dp0, [[0] if i in need else [] for i in range(plan.n_img)], output_dtype, clip)
        zero_of = {i: z[i][0] for i in need}
    res: List[List[torch.Tensor]] = [[] for _ in range(plan.n_img)]
    it = iter(live)
    used = set()
    for i, m in zip(plan.img, plan.m):
        if m > 0:
            res[i].append(next(it))
        else:
            res[i].append(zero_of[i].clone() if i in used else zero_of[i])
            used.add(i)
    return res
