"""Thin torch-tensor wrappers around the C ABI (include/dctae.h).

Every function enqueues work on torch's current stream of the tensors'
device and returns device tensors; nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import FECfg, Images, ImagesU8, LFQCfg, Norm, PackedOut, PackedOut16, Packing, VQCfg, i32, i64, ptr


@dataclass(frozen=True)
class FEParams:
    channels: int = 3
    patch_size: int = 14
    max_patch_h: int = 32
    max_patch_w: int = 32
    max_seq_len: int = 3072
    channel_importances: Tuple[float, float, float] = (8.0, 1.0, 1.0)
    magnitude_weight: float = 0.1

    def c(self, max_seq_len: Optional[int] = None) -> FECfg:
        ci = tuple(float(x) for x in self.channel_importances)
        if len(ci) != 3:
            raise AssertionError("channel_importances must have 3 entries")
        return FECfg(self.channels, self.patch_size, self.max_patch_h, self.max_patch_w,
                     int(max_seq_len if max_seq_len is not None else self.max_seq_len),
                     (C.c_float * 3)(*ci), float(self.magnitude_weight))


@dataclass
class NormState:
    median: torch.Tensor   # (C, mh, mw, P*P) fp32 on device, contiguous
    b: torch.Tensor
    eps: float = 1e-6
    min_val: float = -6.0
    max_val: float = 6.0
    thr: Optional[torch.Tensor] = None   # LFQ-bit thresholds (norm_thresholds), optional

    def c(self) -> Norm:
        return Norm(C.c_void_p(self.median.data_ptr()), C.c_void_p(self.b.data_ptr()), float(self.eps),
                    float(self.min_val), float(self.max_val), ptr(self.thr))


def norm_thresholds(norm: NormState) -> torch.Tensor:
    """thr = smallest fp32 x with PatchNorm(x) > 0 per table element (exact;
    see dctae_norm_thresholds)."""
    dev = _check_dev(norm.median, norm.b)
    ctx = _lib.context(dev)
    thr = torch.empty_like(norm.median)
    n0 = NormState(norm.median, norm.b, norm.eps, norm.min_val, norm.max_val, None)
    rc = ctx.lib.dctae_norm_thresholds(ctx.h, C.byref(n0.c()), thr.numel(), ptr(thr), _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_norm_thresholds")
    return thr


def set_fft(enable: bool, device=None):
    ctx = _lib.context(device)
    ctx.check(ctx.lib.dctae_set_fft(ctx.h, int(bool(enable))), "dctae_set_fft")


def set_option(key: str, value: int, device=None):
    ctx = _lib.context(device)
    ctx.check(ctx.lib.dctae_set_option(ctx.h, key.encode(), int(value)), f"dctae_set_option({key})")


def set_chunk_bytes(nbytes: int, device=None):
    ctx = _lib.context(device)
    ctx.check(ctx.lib.dctae_set_chunk_bytes(ctx.h, int(nbytes)), "dctae_set_chunk_bytes")


def _check_dev(*ts):
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.DCTAEUnavailable("the MI355X path needs HIP device tensors (got a CPU tensor)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise AssertionError("tensors on different devices")
    return dev


def image_set(images: Sequence[torch.Tensor]) -> Tuple[Images, torch.device, list]:
    """Describe a list of (3,H,W) fp32 contiguous device images by a base
    pointer and element offsets (no copies)."""
    imgs = [im if (im.dtype == torch.float32 and im.is_contiguous()) else im.float().contiguous()
            for im in images]
    dev = _check_dev(*imgs)
    for im in imgs:
        if im.dim() != 3:
            raise AssertionError(f"expected a (c, h, w) image, got {tuple(im.shape)}")
    ptrs = [im.data_ptr() for im in imgs]
    base = min(ptrs) if ptrs else 0
    offs = [(p - base) // 4 for p in ptrs]
    hw = []
    for im in imgs:
        hw += [im.shape[1], im.shape[2]]
    offs, hw = i64(offs), i32(hw)
    desc = Images(C.c_void_p(base), C.cast(offs, C.POINTER(C.c_int64)), C.cast(hw, C.POINTER(C.c_int32)), len(imgs))
    return desc, dev, [imgs, offs, hw]


def batch_image_set(x: torch.Tensor) -> Tuple[Images, torch.device, list]:
    """(B,3,H,W) fp32 contiguous device tensor."""
    if x.dim() != 4:
        raise AssertionError("expected (B, c, h, w)")
    x = x if (x.dtype == torch.float32 and x.is_contiguous()) else x.float().contiguous()
    dev = _check_dev(x)
    B, c, H, W = x.shape
    per = c * H * W
    offs, hw = i64([i * per for i in range(B)]), i32([H, W] * B)
    desc = Images(C.c_void_p(x.data_ptr()), C.cast(offs, C.POINTER(C.c_int64)), C.cast(hw, C.POINTER(C.c_int32)), B)
    return desc, dev, [x, offs, hw]


def _u8_image(im: torch.Tensor) -> torch.Tensor:
    """a uint8 tensor as the kernels read it: itself when contiguous, else a contiguous copy (as
    image_set does for fp32 images: the kernels take dense (3, H, W) planes only)"""
    if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8:
        raise TypeError(f"uint8 images expected, got {getattr(im, 'dtype', type(im))}")
    return im if im.is_contiguous() else im.contiguous()


def image_set_u8(images: Sequence[torch.Tensor]) -> Tuple[ImagesU8, torch.device, list]:
    """image_set for (3,H,W) uint8 device images: byte offsets and no copies
    of contiguous images, with one exception: a 512-wide image at a base not
    4-byte aligned is cloned (the 512-wide row kernel loads four pixels at
    once: include/dctae_u8.h).  A non-contiguous image is copied dense."""
    imgs = [_u8_image(im) for im in images]
    dev = _check_dev(*imgs)
    for im in imgs:
        if im.dim() != 3:
            raise AssertionError(f"expected a (c, h, w) image, got {tuple(im.shape)}")
    imgs = [im.clone() if (im.shape[2] == 512 and im.data_ptr() % 4) else im for im in imgs]
    ptrs = [im.data_ptr() for im in imgs]
    base = min(ptrs) if ptrs else 0
    offs = [p - base for p in ptrs]
    hw = []
    for im in imgs:
        hw += [im.shape[1], im.shape[2]]
    offs, hw = i64(offs), i32(hw)
    desc = ImagesU8(C.c_void_p(base), C.cast(offs, C.POINTER(C.c_int64)), C.cast(hw, C.POINTER(C.c_int32)), len(imgs))
    return desc, dev, [imgs, offs, hw]


def batch_image_set_u8(x: torch.Tensor) -> Tuple[ImagesU8, torch.device, list]:
    """(B,3,H,W) uint8 contiguous device tensor (a 512-wide batch at a base not
    4-byte aligned is cloned: 3 * H * 512 keeps every image of it aligned)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise AssertionError("expected (B, c, h, w)")
    x = _u8_image(x)
    dev = _check_dev(x)
    B, c, H, W = x.shape
    if W == 512 and x.data_ptr() % 4:
        x = x.clone()
    per = c * H * W
    offs, hw = i64([i * per for i in range(B)]), i32([H, W] * B)
    desc = ImagesU8(C.c_void_p(x.data_ptr()), C.cast(offs, C.POINTER(C.c_int64)), C.cast(hw, C.POINTER(C.c_int32)), B)
    return desc, dev, [x, offs, hw]


def u8_to_f32(x: torch.Tensor) -> torch.Tensor:
    """dctae_u8_to_f32: the fp32 tensor x / 255 of a uint8 device tensor (the
    values the byte-image encode means)."""
    x = _u8_image(x)
    dev = _check_dev(x)
    ctx = _lib.context(dev)
    y = torch.empty(x.shape, dtype=torch.float32, device=dev)
    ctx.check(ctx.lib.dctae_u8_to_f32(ctx.h, ptr(x), x.numel(), ptr(y), _lib.stream_ptr(dev)), "dctae_u8_to_f32")
    return y


def out_dtype_suffix(dtype: torch.dtype, what: str) -> str:
    """the entry-point suffix of a decode output dtype: "" (fp32) or "_u8";
    anything else is a TypeError naming ``what``"""
    if dtype == torch.float32:
        return ""
    if dtype == torch.uint8:
        return "_u8"
    raise TypeError(f"{what}: torch.float32 or torch.uint8, got {dtype}")


def codes_dtype_suffix(dtype: torch.dtype, what: str) -> str:
    """the entry-point suffix of a code dtype: "" (int64) or "_c16" (int16,
    include/dctae_codes16.h: an int16 code c means the int64 code int64(c));
    anything else is a TypeError naming ``what``"""
    if dtype == torch.int64:
        return ""
    if dtype == torch.int16:
        return "_c16"
    raise TypeError(f"{what}: torch.int64 or torch.int16, got {dtype}")


def check_codes16(cfg: LFQCfg, what: str):
    """int16 codes hold codebook_dim <= 15 bits (include/dctae_codes16.h)"""
    if cfg.codebook_dim > 15:
        raise ValueError(f"{what}: int16 codes hold codebook_dim <= 15 bits, got codebook_dim = {cfg.codebook_dim}")


def codes_in(codes: torch.Tensor, cfg: Optional[LFQCfg], what: str):
    """codes as a kernel reads them, and their entry-point suffix: int16 as it
    is (the ``_c16`` entries, no widened copy), anything else as int64"""
    if codes.dtype == torch.int16:
        if cfg is not None:
            check_codes16(cfg, what)
        return codes.contiguous(), "_c16"
    return codes.long().contiguous(), ""


def f32_to_u8(x: torch.Tensor) -> torch.Tensor:
    """dctae_f32_to_u8: the uint8 tensor of an fp32 device tensor by the byte
    decode's rule, ``x.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)`` as
    torch computes it on the CPU (NaN gives 0): include/dctae_u8_out.h."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise TypeError(f"fp32 tensor expected, got {getattr(x, 'dtype', type(x))}")
    x = x if x.is_contiguous() else x.contiguous()
    dev = _check_dev(x)
    ctx = _lib.context(dev)
    y = torch.empty(x.shape, dtype=torch.uint8, device=dev)
    ctx.check(ctx.lib.dctae_f32_to_u8(ctx.h, ptr(x), x.numel(), ptr(y), _lib.stream_ptr(dev)), "dctae_f32_to_u8")
    return y


def encode(imgs_desc: Images, dev: torch.device, p: FEParams, plan, n_rows: int, seq_len: int,
           norm: Optional[NormState], lfq: Optional[LFQCfg], want_codes=True, want_patches=False,
           want_raw=False, want_scores=False, out=None, codes_dtype: torch.dtype = torch.int64):
    """dctae_encode (dctae_encode_u8 for an ImagesU8 descriptor): returns dict of packed device tensors.
    codes_dtype=torch.int16: the codes as int16 (dctae_encode_c16 / dctae_encode_u8_c16), each the int64
    call's code converted; every other output the same."""
    c16 = codes_dtype_suffix(codes_dtype, "encode codes_dtype") if want_codes else ""
    if c16:
        check_codes16(lfq, "encode")
    ctx = _lib.context(dev)
    S = seq_len
    PP = p.patch_size ** 2
    o = out or {}
    def alloc(name, shape, dtype):
        t = o.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev:
            t = torch.empty(shape, dtype=dtype, device=dev)
            o[name] = t
        return t
    res = {
        "positions": alloc("positions", (n_rows, S, 2), torch.long),
        "channels": alloc("channels", (n_rows, S), torch.long),
        "image_ids": alloc("image_ids", (n_rows, S), torch.long),
        "key_pad_mask": alloc("key_pad_mask", (n_rows, S), torch.bool),
    }
    if want_codes:
        res["codes"] = alloc("codes", (n_rows, S, lfq.num_codebooks), codes_dtype)
    if want_patches:
        res["patches"] = alloc("patches", (n_rows, S, PP), torch.float32)
    if want_raw:
        res["raw"] = alloc("raw", (n_rows, S, PP), torch.float32)
    if want_scores:
        res["scores"] = alloc("scores", (n_rows, S), torch.float32)
    pk_keep = [i32(plan.row), i32(plan.col), i32(plan.k), i32(plan.local_id), i32(plan.row_len)]
    pk = Packing(*[C.cast(a, C.POINTER(C.c_int32)) for a in pk_keep], n_rows)
    po = (PackedOut16 if c16 else PackedOut)(ptr(res.get("codes")), ptr(res["positions"]), ptr(res["channels"]), ptr(res["image_ids"]),
                   ptr(res["key_pad_mask"]), ptr(res.get("patches")), ptr(res.get("raw")), ptr(res.get("scores")))
    nc = norm.c() if norm is not None else None
    name = ("dctae_encode_u8" if isinstance(imgs_desc, ImagesU8) else "dctae_encode") + c16
    rc = getattr(ctx.lib, name)(ctx.h, C.byref(p.c(S)), C.byref(imgs_desc), C.byref(pk),
                                C.byref(nc) if nc is not None else None,
                                C.byref(lfq) if lfq is not None else None, C.byref(po), _lib.stream_ptr(dev))
    ctx.check(rc, name)
    return res


def norm_apply(x: torch.Tensor, channels: torch.Tensor, positions: torch.Tensor, norm: NormState, p: FEParams,
               inverse: bool) -> torch.Tensor:
    dev = _check_dev(x, channels, positions, norm.median, norm.b)
    ctx = _lib.context(dev)
    PP = p.patch_size ** 2
    if x.shape[-1] != PP:
        raise AssertionError(f"token dim {x.shape[-1]} != patch_size**2")
    xs = x.float().contiguous()
    ch = channels.long().contiguous()
    pos = positions.long().contiguous()
    n = xs.numel() // PP
    if ch.numel() != n or pos.numel() != 2 * n:
        raise AssertionError("channels/positions do not match patches")
    y = torch.empty_like(xs)
    fn = ctx.lib.dctae_norm_inverse if inverse else ctx.lib.dctae_norm_forward
    rc = fn(ctx.h, C.byref(norm.c()), p.patch_size, p.max_patch_h, p.max_patch_w, ptr(xs), ptr(ch), ptr(pos), n,
            ptr(y), _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_norm")
    return y


def _stats_inputs(x, channels, positions, key_pad, p: FEParams):
    dev = _check_dev(x, channels, positions)
    PP = p.patch_size ** 2
    if x.shape[-1] != PP:
        raise AssertionError(f"token dim {x.shape[-1]} != patch_size**2")
    xs = x.float().contiguous()
    n = xs.numel() // PP
    ch = channels.long().contiguous()
    pos = positions.long().contiguous()
    if ch.numel() != n or pos.numel() != 2 * n:
        raise AssertionError("channels/positions do not match patches")
    kp = None
    if key_pad is not None:
        kp = key_pad.to(device=dev, dtype=torch.bool).contiguous()
        if kp.numel() != n:
            raise AssertionError("key_pad_mask does not match patches")
    return dev, xs, ch, pos, kp, n


def norm_batch_stats(x, channels, positions, key_pad, p: FEParams):
    """patchnorm.py:104-130 on the GPU: (batch_n (C,mh,mw), batch_median (C,mh,mw,P*P))."""
    dev, xs, ch, pos, kp, n = _stats_inputs(x, channels, positions, key_pad, p)
    ctx = _lib.context(dev)
    PP = p.patch_size ** 2
    bn = torch.empty(p.channels, p.max_patch_h, p.max_patch_w, device=dev)
    bm = torch.empty(p.channels, p.max_patch_h, p.max_patch_w, PP, device=dev)
    rc = ctx.lib.dctae_norm_batch_stats(ctx.h, p.patch_size, p.channels, p.max_patch_h, p.max_patch_w, ptr(xs),
                                        ptr(ch), ptr(pos), ptr(kp), n, ptr(bn), ptr(bm), _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_norm_batch_stats")
    return bn, bm


def norm_batch_mad(x, channels, positions, key_pad, median, p: FEParams):
    """patchnorm.py:140-144 on the GPU: batch_b around `median` (C,mh,mw,P*P)."""
    dev, xs, ch, pos, kp, n = _stats_inputs(x, channels, positions, key_pad, p)
    ctx = _lib.context(dev)
    med = median.float().contiguous()
    bb = torch.empty_like(med)
    rc = ctx.lib.dctae_norm_batch_mad(ctx.h, p.patch_size, p.channels, p.max_patch_h, p.max_patch_w, ptr(xs),
                                      ptr(ch), ptr(pos), ptr(kp), n, ptr(med), ptr(bb), _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_norm_batch_mad")
    return bb


def norm_merge_(table, batch, n, batch_n, n_update: bool):
    """patchnorm.py:135-138 / 146-150 in place: table <- (table*n + batch*bn)/clamp(n+bn,1); n += bn."""
    dev = _check_dev(table, batch, n, batch_n)
    for t in (table, batch, n, batch_n):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise AssertionError("PatchNorm tables must be contiguous float32")
    cells = n.numel()
    PP = table.numel() // max(1, cells)
    ctx = _lib.context(dev)
    rc = ctx.lib.dctae_norm_merge(ctx.h, cells, PP, ptr(table), ptr(batch), ptr(n), ptr(batch_n), int(n_update),
                                  _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_norm_merge")


def norm_train_step(x, channels, positions, key_pad, n, median, b, p: FEParams, want_output=True):
    """patchnorm.py:101-155 in one call: updates n / median / b in place,
    returns x with the pad rows zeroed (or None)."""
    dev, xs, ch, pos, kp, ntok = _stats_inputs(x, channels, positions, key_pad, p)
    _check_dev(n, median, b)
    ctx = _lib.context(dev)
    y = torch.empty_like(xs) if want_output else None
    st = NormState(median, b)
    rc = ctx.lib.dctae_norm_train_step(ctx.h, C.byref(st.c()), ptr(n), p.patch_size, p.channels, p.max_patch_h,
                                       p.max_patch_w, ptr(xs), ptr(ch), ptr(pos), ptr(kp), ntok, ptr(y),
                                       _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_norm_train_step")
    return y


def _norm_tables(norm: NormState, p: FEParams, dev):
    _check_dev(norm.median, norm.b)
    tshape = (3, p.max_patch_h, p.max_patch_w, p.patch_size ** 2)
    for t in (norm.median, norm.b):
        if tuple(t.shape) != tshape or not t.is_contiguous() or t.dtype != torch.float32 or t.device != dev:
            raise AssertionError(f"PatchNorm tables must be contiguous fp32 {tshape} on {dev}, got {tuple(t.shape)}")


def norm_inverse_backward(grad: torch.Tensor, channels: torch.Tensor, positions: torch.Tensor, norm: NormState,
                          p: FEParams) -> torch.Tensor:
    """grad * (b*sqrt(2) + eps) gathered per token (dctae_norm_inverse_backward):
    the gradient of PatchNorm.inverse_norm with respect to its input, fp32."""
    dev, gs, ch, pos, _, n = _stats_inputs(grad, channels, positions, None, p)
    _norm_tables(norm, p, dev)
    ctx = _lib.context(dev)
    dy = torch.empty_like(gs)
    rc = ctx.lib.dctae_norm_inverse_backward(ctx.h, C.byref(norm.c()), p.patch_size, p.max_patch_h, p.max_patch_w,
                                             ptr(gs), ptr(ch), ptr(pos), n, ptr(dy), _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_norm_inverse_backward")
    return dy


def _rec_loss_inputs(out, tn, raw, channels, positions, key_pad, norm: NormState, p: FEParams):
    if key_pad is None:
        raise AssertionError("the reconstruction losses need the key_pad_mask")
    dev, os_, ch, pos, kp, n = _stats_inputs(out.detach(), channels, positions, key_pad, p)
    _check_dev(tn, raw)
    _norm_tables(norm, p, dev)
    ts, rs = tn.detach().float().contiguous(), raw.detach().float().contiguous()
    if ts.shape != os_.shape or rs.shape != os_.shape:
        raise AssertionError(f"targets {tuple(ts.shape)} / {tuple(rs.shape)} do not match the output {tuple(os_.shape)}")
    return dev, os_, ts, rs, ch, pos, kp.view(torch.uint8), n


def rec_loss_forward(out, tn, raw, channels, positions, key_pad, norm: NormState, p: FEParams, want_unnorm=True):
    """The masked L1 pair of a training step (dctae_rec_loss_forward): scalars
    (3) = [rec_loss, rec_loss_unnormalized, M] fp32 on the device, and
    inverse_norm(out) at every token (None unless wanted).  key_pad: True at
    padding."""
    dev, os_, ts, rs, ch, pos, kp, n = _rec_loss_inputs(out, tn, raw, channels, positions, key_pad, norm, p)
    ctx = _lib.context(dev)
    sc = torch.empty(3, dtype=torch.float32, device=dev)
    un = torch.empty_like(os_) if want_unnorm else None
    rc = ctx.lib.dctae_rec_loss_forward(ctx.h, C.byref(norm.c()), p.patch_size, p.max_patch_h, p.max_patch_w, ptr(os_),
                                        ptr(ts), ptr(rs), ptr(ch), ptr(pos), ptr(kp), n, ptr(un), ptr(sc),
                                        _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_rec_loss_forward")
    return sc, un


def rec_loss_backward(out, tn, raw, channels, positions, key_pad, norm: NormState, p: FEParams, sc: torch.Tensor,
                      grad: torch.Tensor, grad_unnorm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d(g0 rec_loss + g1 rec_loss_unnormalized + <grad_unnorm, unnorm>) / d out,
    fp32, out's shape (dctae_rec_loss_backward).  sc: rec_loss_forward's
    scalars for the same tensors; grad: the two upstream gradients, (2) on the
    device."""
    dev, os_, ts, rs, ch, pos, kp, n = _rec_loss_inputs(out, tn, raw, channels, positions, key_pad, norm, p)
    _check_dev(sc, grad, grad_unnorm)
    ctx = _lib.context(dev)
    g = grad.detach().to(device=dev, dtype=torch.float32).reshape(2).contiguous()
    gu = None
    if grad_unnorm is not None:
        gu = grad_unnorm.detach().float().contiguous()
        if gu.shape != os_.shape:
            raise AssertionError("the gradient of the unnormalized patches does not match the output")
    dout = torch.empty_like(os_)
    rc = ctx.lib.dctae_rec_loss_backward(ctx.h, C.byref(norm.c()), p.patch_size, p.max_patch_h, p.max_patch_w,
                                         ptr(os_), ptr(ts), ptr(rs), ptr(ch), ptr(pos), ptr(kp), n, ptr(sc), ptr(g),
                                         ptr(gu), ptr(dout), _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_rec_loss_backward")
    return dout


def check_device_errors(dev):
    ctx = _lib.context(dev)
    ctx.check(ctx.lib.dctae_check_device_errors(ctx.h, _lib.stream_ptr(dev)), "device index check")


def lfq_forward(x: torch.Tensor, cfg: LFQCfg, want_quantized=True):
    dev = _check_dev(x)
    ctx = _lib.context(dev)
    xs = x.float().contiguous()
    d = cfg.codebook_dim * cfg.num_codebooks
    if xs.shape[-1] != d:
        raise AssertionError(f"expected dimension of {d} but received {xs.shape[-1]}")
    n = xs.numel() // d
    q = torch.empty_like(xs) if want_quantized else None
    idx = torch.empty((*xs.shape[:-1], cfg.num_codebooks), dtype=torch.long, device=dev)
    rc = ctx.lib.dctae_lfq_forward(ctx.h, C.byref(cfg), ptr(xs), n, ptr(q), ptr(idx), _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_lfq_forward")
    return q, idx


def _lfq_entropy_args(h: torch.Tensor, mask: torch.Tensor, cfg: LFQCfg):
    dev = _check_dev(h, mask)
    if cfg.codebook_dim > 16 or cfg.num_codebooks > 32:
        raise NotImplementedError("the fused LFQ entropy loss serves codebook_dim <= 16 and num_codebooks <= 32 "
                                  f"(got {cfg.codebook_dim}, {cfg.num_codebooks})")
    d = cfg.codebook_dim * cfg.num_codebooks
    hs = h.detach().float().contiguous()
    if hs.numel() % d:
        raise AssertionError(f"{hs.numel()} features are no whole number of tokens of dimension {d}")
    n = hs.numel() // d
    if mask.numel() != n:
        raise AssertionError(f"mask of {mask.numel()} entries for {n} tokens")
    ms = mask.to(torch.bool).contiguous().view(torch.uint8)
    return dev, hs, ms, n


def lfq_entropy_forward(h: torch.Tensor, mask: torch.Tensor, cfg: LFQCfg, temperature=0.01, eps=1e-9):
    """The LFQ training losses of projected features h (..., num_codebooks *
    codebook_dim) without the dense distance tensor (dctae_lfq_entropy_forward).
    mask (...): True at real tokens.  Returns avg_probs (2**codebook_dim) and
    scalars (5) = [entropy loss, sample_entropy, avg_entropy, commit_loss, M],
    fp32 on h's device."""
    dev, hs, ms, n = _lfq_entropy_args(h, mask, cfg)
    ctx = _lib.context(dev)
    avg = torch.empty(2 ** cfg.codebook_dim, dtype=torch.float32, device=dev)
    sc = torch.empty(5, dtype=torch.float32, device=dev)
    rc = ctx.lib.dctae_lfq_entropy_forward(ctx.h, C.byref(cfg), ptr(hs), ptr(ms), n, float(temperature), float(eps),
                                           ptr(avg), ptr(sc), _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_lfq_entropy_forward")
    return avg, sc


def lfq_entropy_backward(h: torch.Tensor, mask: torch.Tensor, cfg: LFQCfg, avg: torch.Tensor, sc: torch.Tensor,
                         grad: torch.Tensor, temperature=0.01, eps=1e-9) -> torch.Tensor:
    """grad * d(entropy loss) / dh, fp32, h's shape; exact zeros at masked-out
    tokens.  avg / sc: lfq_entropy_forward's outputs for the same arguments;
    grad: the upstream gradient, a scalar tensor on the device."""
    dev, hs, ms, n = _lfq_entropy_args(h, mask, cfg)
    _check_dev(avg, sc, grad)
    ctx = _lib.context(dev)
    g = grad.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
    dh = torch.empty_like(hs)
    rc = ctx.lib.dctae_lfq_entropy_backward(ctx.h, C.byref(cfg), ptr(hs), ptr(ms), n, float(temperature), float(eps),
                                            ptr(avg), ptr(sc), ptr(g), ptr(dh), _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_lfq_entropy_backward")
    return dh


def linear_ordered(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor]) -> torch.Tensor:
    """x (..., K) w (D, K)^T + b with every output summed over k in index
    order, bias last (dctae_linear_ordered); fp32, no autograd."""
    dev = _check_dev(x, w, b)
    ctx = _lib.context(dev)
    xs = x.detach().float().contiguous()
    K = xs.shape[-1]
    if w.shape[1] != K:
        raise AssertionError(f"expected dimension of {w.shape[1]} but received {K}")
    if K > 512:
        raise NotImplementedError("ordered linear: at most 512 input features")
    wt = w.detach().float().t().contiguous()
    bs = None if b is None else b.detach().float().contiguous()
    out = torch.empty((*xs.shape[:-1], w.shape[0]), dtype=torch.float32, device=dev)
    rc = ctx.lib.dctae_linear_ordered(ctx.h, ptr(xs), xs.numel() // K, K, ptr(wt), ptr(bs), w.shape[0], ptr(out),
                                      _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_linear_ordered")
    return out


def lfq_codes(idx: torch.Tensor, cfg: LFQCfg) -> torch.Tensor:
    dev = _check_dev(idx)
    ctx = _lib.context(dev)
    ii = idx.long().contiguous()
    if ii.shape[-1] != cfg.num_codebooks:
        raise AssertionError("last dim of indices must be num_codebooks")
    n = ii.numel() // cfg.num_codebooks
    out = torch.empty((*ii.shape[:-1], cfg.num_codebooks * cfg.codebook_dim), dtype=torch.float32, device=dev)
    rc = ctx.lib.dctae_lfq_indices_to_codes(ctx.h, C.byref(cfg), ptr(ii), n, ptr(out), _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_lfq_indices_to_codes")
    return out


def lfq_project_in(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], cfg: LFQCfg,
                   x_bound: Optional[float] = None, codes_dtype: torch.dtype = torch.int64) -> torch.Tensor:
    """LFQ.forward's indices with project_in fused (dctae_lfq_project_in):
    x (..., dim) -> (..., num_codebooks) int64.  w / b: project_in's fp32
    weight (ncb*cd, dim) and bias on x's device.  x_bound: the caller's bound
    |x| <= x_bound (dctae_lfq_project_in_bounded: the fp16 kernels).
    codes_dtype=torch.int16: int16 indices (dctae_lfq_project_in_c16 /
    dctae_lfq_project_in_bounded_c16), each the int64 call's index converted."""
    return lfq_project_in_into(x, w, b, cfg, None, x_bound, codes_dtype)


def lfq_project_in_into(x, w, b, cfg: LFQCfg, idx: Optional[torch.Tensor],
                        x_bound: Optional[float] = None, codes_dtype: torch.dtype = torch.int64) -> torch.Tensor:
    c16 = codes_dtype_suffix(codes_dtype, "project_in codes_dtype")
    if c16:
        check_codes16(cfg, "project_in")
    dev = _check_dev(x, w, b)
    ctx = _lib.context(dev)
    xs = x.float().contiguous()
    dim = xs.shape[-1]
    n = xs.numel() // dim
    shape = (*xs.shape[:-1], cfg.num_codebooks)
    if idx is None or idx.shape != shape or idx.dtype != codes_dtype or not idx.is_contiguous() or idx.device != dev:
        idx = torch.empty(shape, dtype=codes_dtype, device=dev)
    if x_bound is not None:
        name = "dctae_lfq_project_in_bounded" + c16
        rc = getattr(ctx.lib, name)(ctx.h, C.byref(cfg), ptr(xs), n, dim, ptr(w), ptr(b), float(x_bound), ptr(idx),
                                    _lib.stream_ptr(dev))
        ctx.check(rc, name)
        return idx
    name = "dctae_lfq_project_in" + c16
    rc = getattr(ctx.lib, name)(ctx.h, C.byref(cfg), ptr(xs), n, dim, ptr(w), ptr(b), ptr(idx), _lib.stream_ptr(dev))
    ctx.check(rc, name)
    return idx


def lfq_project_out(idx: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], cfg: LFQCfg) -> torch.Tensor:
    """LFQ.indices_to_codes with project_out fused (dctae_lfq_project_out):
    idx (..., num_codebooks) -> (..., dim) fp32; w (dim, ncb*cd), b (dim).
    int16 indices are read as they are (dctae_lfq_project_out_c16)."""
    dev = _check_dev(idx, w, b)
    ctx = _lib.context(dev)
    ii, c16 = codes_in(idx, cfg, "project_out")
    if ii.shape[-1] != cfg.num_codebooks:
        raise AssertionError("last dim of indices must be num_codebooks")
    dim = w.shape[0]
    n = ii.numel() // cfg.num_codebooks
    out = torch.empty((*ii.shape[:-1], dim), dtype=torch.float32, device=dev)
    name = "dctae_lfq_project_out" + c16
    rc = getattr(ctx.lib, name)(ctx.h, C.byref(cfg), ptr(ii), n, dim, ptr(w), ptr(b), ptr(out), _lib.stream_ptr(dev))
    ctx.check(rc, name)
    return out


def lfq_project_out_inverse_norm(idx: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], cfg: LFQCfg,
                                 norm: NormState, p: FEParams, channels: torch.Tensor,
                                 positions: torch.Tensor) -> torch.Tensor:
    """LFQ.indices_to_codes (project_out) + PatchNorm.inverse_norm in one kernel
    (dctae_lfq_project_out_inverse_norm): idx (..., ncb) -> (..., P*P) fp32.
    int16 indices are read as they are (dctae_lfq_project_out_inverse_norm_c16)."""
    dev = _check_dev(idx, w, b, channels, positions, norm.median, norm.b)
    ctx = _lib.context(dev)
    ii, c16 = codes_in(idx, cfg, "project_out")
    if ii.shape[-1] != cfg.num_codebooks:
        raise AssertionError("last dim of indices must be num_codebooks")
    dim = w.shape[0]
    if dim != p.patch_size ** 2:
        raise AssertionError(f"project_out dim {dim} != patch_size**2")
    n = ii.numel() // cfg.num_codebooks
    ch = channels.long().contiguous()
    pos = positions.long().contiguous()
    if ch.numel() != n or pos.numel() != 2 * n:
        raise AssertionError("channels/positions do not match the indices")
    tshape = (3, p.max_patch_h, p.max_patch_w, dim)
    for t in (norm.median, norm.b):
        if tuple(t.shape) != tshape or not t.is_contiguous() or t.dtype != torch.float32:
            raise AssertionError(f"PatchNorm tables must be contiguous fp32 {tshape}, got {tuple(t.shape)}")
    out = torch.empty((*ii.shape[:-1], dim), dtype=torch.float32, device=dev)
    name = "dctae_lfq_project_out_inverse_norm" + c16
    rc = getattr(ctx.lib, name)(ctx.h, C.byref(cfg), ptr(ii), n, dim, ptr(w), ptr(b), C.byref(norm.c()),
                                p.max_patch_h, p.max_patch_w, ptr(ch), ptr(pos), ptr(out), _lib.stream_ptr(dev))
    ctx.check(rc, name)
    return out


def vq_forward(cfg: VQCfg, x: torch.Tensor, mask: Optional[torch.Tensor], want_quantized=True):
    """x (n, dim) fp32 contiguous on the device; mask (n) bool or None.
    Returns quantize (n, dim) (None unless wanted) and indices (n, heads)."""
    dev = _check_dev(x)
    ctx = _lib.context(dev)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.ndim != 2 or x.shape[1] != cfg.dim:
        raise AssertionError(f"VectorQuantize input must be contiguous fp32 (n, {cfg.dim})")
    n = x.shape[0]
    m = None
    if mask is not None:
        if mask.shape != (n,):
            raise AssertionError("mask must be (n,)")
        m = mask.to(device=dev, dtype=torch.uint8).contiguous()
    q = torch.empty_like(x) if want_quantized else None
    idx = torch.empty((n, cfg.heads), dtype=torch.long, device=dev)
    rc = ctx.lib.dctae_vq_forward(ctx.h, C.byref(cfg), ptr(x), ptr(m), n, ptr(q), ptr(idx), _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_vq_forward")
    return q, idx


def vq_from_indices(cfg: VQCfg, idx: torch.Tensor, project_out: bool) -> torch.Tensor:
    """idx (n, heads) -> codes (n, heads*codebook_dim) or project_out(codes) (n, dim)."""
    dev = _check_dev(idx)
    ctx = _lib.context(dev)
    ii = idx.long().contiguous()
    if ii.ndim != 2 or ii.shape[1] != cfg.heads:
        raise AssertionError("indices must be (n, heads)")
    n = ii.shape[0]
    width = cfg.dim if project_out else cfg.heads * cfg.codebook_dim
    out = torch.empty((n, width), dtype=torch.float32, device=dev)
    fn = ctx.lib.dctae_vq_output_from_indices if project_out else ctx.lib.dctae_vq_codes_from_indices
    rc = fn(ctx.h, C.byref(cfg), ptr(ii), n, ptr(out), _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_vq_from_indices")
    check_device_errors(dev)
    return out


class DecodeTable:
    """The host-side image table of one packed batch (the descriptor arguments
    of dctae_decode / dctae_decode_backward / dctae_pixel_loss_forward) and
    the batch tensors in the layout the library reads.  Building it from the
    batch walks ``ids.cpu()``: the one host synchronisation of a decode."""

    def __init__(self, p: FEParams, ids, key_pad, positions, channels, patch_sizes, original_sizes, ids_host=None):
        """ids_host: ``ids`` on the host when the caller has read them already (no second read)"""
        self.dev = _check_dev(ids, key_pad, positions, channels)
        self.R, self.S = ids.shape
        self.ids = ids.long().contiguous()
        self.key_pad = key_pad.to(torch.bool).contiguous()
        self.pos = positions.long().contiguous()
        self.ch = channels.long().contiguous()
        # image enumeration: rows in order, ids ascending (FE:619-633); host view
        ids_h = self.ids.cpu() if ids_host is None else ids_host
        places = [(r, im) for r in range(self.R) for im in torch.unique(ids_h[r]).tolist()]
        if len(places) > len(patch_sizes) or len(places) > len(original_sizes):
            raise IndexError("more images in the batch than patch_sizes / original_sizes entries")
        self._lay_out(p.channels, places, int(ids_h.max().item()) + 1 if ids_h.numel() else 1,
                      original_sizes, patch_sizes)

    @classmethod
    def from_layout(cls, p: FEParams, dev, n_rows, seq_len, rows, local_ids, hw, patch_hw) -> "DecodeTable":
        """the table of a packing layout (image i in row rows[i] under the id
        local_ids[i], every image hw = (H, W) with the patch grid patch_hw):
        no device tensor is read, and the batch tensors come with each call"""
        t = cls.__new__(cls)
        t.dev, t.R, t.S = dev, n_rows, seq_len
        places = sorted(zip(rows, local_ids))
        t._lay_out(p.channels, places, max(local_ids) + 1, [hw] * len(places), [patch_hw] * len(places))
        return t

    def _lay_out(self, channels, places, lut_w, original_sizes, patch_sizes):
        """places: (row, id in the row) of image 0, 1, ... in the enumeration order"""
        self.channels, self.lut_w, self.n_img = channels, lut_w, len(places)
        lut = [-1] * (self.R * lut_w)
        self.hw, self.phw, self.offs = [], [], []
        total = 0
        for i, (r, im) in enumerate(places):
            lut[r * lut_w + im] = i
            h, w = (int(v) for v in original_sizes[i])
            ph, pw = (int(v) for v in patch_sizes[i])
            self.hw += [h, w]
            self.phw += [ph, pw]
            self.offs.append(total)
            total += channels * h * w
        self.total = total
        self.keep = k = [i32(lut), i32(self.hw), i64(self.offs), i32(self.phw)]
        self._c = (C.cast(k[0], C.POINTER(C.c_int32)), lut_w, self.n_img, C.cast(k[1], C.POINTER(C.c_int32)),
                   C.cast(k[2], C.POINTER(C.c_int64)), C.cast(k[3], C.POINTER(C.c_int32)))

    def c_args(self):
        """img_lut, lut_w, n_img, out_hw, out_off, patch_hw as the C ABI takes them"""
        return self._c

    def images(self, flat: torch.Tensor) -> List[torch.Tensor]:
        """the (3, H, W) views of a flat buffer in the decode's output layout
        (fp32 or uint8: the offsets count elements of either)"""
        return [flat[o: o + self.channels * self.hw[2 * i] * self.hw[2 * i + 1]].view(
            self.channels, self.hw[2 * i], self.hw[2 * i + 1]) for i, o in enumerate(self.offs)]


def decode_table(p: FEParams, ids, key_pad, positions, channels, patch_sizes, original_sizes) -> DecodeTable:
    return DecodeTable(p, ids, key_pad, positions, channels, patch_sizes, original_sizes)


def _decode_call(ctx, cfg: FECfg, table: DecodeTable, ids, key_pad, pos, ch, norm: Optional[Norm],
                 lfq: Optional[LFQCfg], codes, patches, out, normed: bool, out_dtype: torch.dtype = torch.float32):
    """dctae_decode (from codes, or from patches when codes is None) or, normed,
    dctae_decode_normed of the packed batch into the flat buffer ``out``; the
    tensors as the library reads them (int64 / bool / fp32, contiguous).
    out_dtype=torch.uint8: the byte-output twin of either (dctae_decode_u8 /
    dctae_decode_normed_u8), ``out`` a uint8 buffer in the same layout.
    codes: int64, or int16 read as they are (dctae_decode_c16 / dctae_decode_u8_c16);
    any other dtype is a TypeError."""
    name = ("dctae_decode_normed" if normed else "dctae_decode") + out_dtype_suffix(out_dtype, "decode out_dtype")
    if codes is not None and not normed:
        name += codes_dtype_suffix(codes.dtype, "decode codes")
        if codes.dtype == torch.int16 and lfq is not None:
            check_codes16(lfq, "decode")
    if out.dtype != out_dtype:
        raise TypeError(f"{name}: the output buffer is {out.dtype}")
    batch = (ctx.h, C.byref(cfg), table.R, *table.c_args(), ptr(ids), ptr(key_pad), ptr(pos), ptr(ch))
    if normed:
        rc = getattr(ctx.lib, name)(*batch, C.byref(norm), ptr(patches), ptr(out), _lib.stream_ptr(table.dev))
    else:
        rc = getattr(ctx.lib, name)(*batch, C.byref(norm) if norm is not None else None,
                                    C.byref(lfq) if lfq is not None else None, ptr(codes), ptr(patches), ptr(out),
                                    _lib.stream_ptr(table.dev))
    ctx.check(rc, name)


def pixel_loss_forward(table: DecodeTable, rgb_hat: torch.Tensor, rgb: torch.Tensor) -> torch.Tensor:
    """dctae_pixel_loss_forward on two flat image buffers in the decode's output
    layout: (1 + n_img) fp32 on the device = [pixel_loss, mse_0 ...]."""
    dev = _check_dev(rgb_hat, rgb)
    for t in (rgb_hat, rgb):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != table.total:
            raise AssertionError("pixel loss: the image buffers must be contiguous fp32 in the decode's layout")
    ctx = _lib.context(dev)
    sc = torch.empty(1 + table.n_img, dtype=torch.float32, device=dev)
    _, _, n_img, hw, off, _ = table.c_args()
    rc = ctx.lib.dctae_pixel_loss_forward(ctx.h, n_img, hw, off, ptr(rgb_hat), ptr(rgb), ptr(sc), _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_pixel_loss_forward")
    return sc


def decode_backward(p: FEParams, table: DecodeTable, patches: torch.Tensor, grad_rgb: Optional[torch.Tensor] = None,
                    rgb_hat: Optional[torch.Tensor] = None, rgb: Optional[torch.Tensor] = None,
                    g: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dctae_decode_backward: the gradient of the decode's images with respect
    to ``patches`` (R, S, PP), fp32.  Upstream either ``grad_rgb`` (flat, the
    decode's output layout) or the pixel loss's (``rgb_hat``, ``rgb``, the
    flat buffers of pixel_loss_forward, and ``g``, the loss's upstream
    gradient, one fp32 on the device)."""
    dev = _check_dev(patches, grad_rgb, rgb_hat, rgb, g)
    pp = patches.detach().float().contiguous()
    if tuple(pp.shape) != (table.R, table.S, p.patch_size ** 2):
        raise AssertionError(f"patches {tuple(pp.shape)} do not match the batch ({table.R}, {table.S}, "
                             f"{p.patch_size ** 2})")
    flats = [grad_rgb] if grad_rgb is not None else [rgb_hat, rgb]
    if any(t is None or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != table.total for t in flats):
        raise AssertionError("decode backward: the image buffers must be contiguous fp32 in the decode's layout")
    if grad_rgb is None:
        g = g.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
    ctx = _lib.context(dev)
    dp = torch.empty_like(pp)
    rc = ctx.lib.dctae_decode_backward(ctx.h, C.byref(p.c(table.S)), table.R, *table.c_args(), ptr(table.ids),
                                       ptr(table.key_pad), ptr(table.pos), ptr(table.ch), ptr(pp), ptr(grad_rgb),
                                       ptr(rgb_hat), ptr(rgb), ptr(g if grad_rgb is None else None), ptr(dp),
                                       _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_decode_backward")
    return dp


def decode(p: FEParams, ids: torch.Tensor, key_pad: torch.Tensor, positions: torch.Tensor, channels: torch.Tensor,
           patch_sizes: Sequence, original_sizes: Sequence, codes: Optional[torch.Tensor] = None,
           patches: Optional[torch.Tensor] = None, norm: Optional[NormState] = None,
           lfq: Optional[LFQCfg] = None, normed: bool = False, table: Optional[DecodeTable] = None,
           return_flat: bool = False, out_dtype: torch.dtype = torch.float32) -> List[torch.Tensor]:
    """dctae_decode; returns a list of (3, H, W) fp32 device images, or with
    out_dtype=torch.uint8 uint8 images whose every byte is the fp32 call's value
    through ``x.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)`` (dctae_decode_u8,
    include/dctae_u8_out.h; torch's allocations keep the flat buffer and so
    every 512 x 512 image of it 4-byte aligned).  normed:
    patches are PatchNorm outputs and the inverse_norm runs inside the decode
    (dctae_decode_normed; norm required, no codes).  table: the batch's
    DecodeTable when the caller already built it; return_flat: also the flat
    buffer the images are views of, as (images, flat)."""
    dev = _check_dev(ids, key_pad, positions, channels, codes, patches)
    if table is None:
        table = decode_table(p, ids, key_pad, positions, channels, patch_sizes, original_sizes)
    out_dtype_suffix(out_dtype, "decode out_dtype")
    out = torch.empty(table.total, dtype=out_dtype, device=dev)
    cc = codes_in(codes, lfq, "decode")[0] if codes is not None else None   # int16 codes: no widened copy
    pp = patches.float().contiguous() if patches is not None else None
    if normed and (norm is None or codes is not None):
        raise AssertionError("normed decode needs the PatchNorm state and patches (no codes)")
    _decode_call(_lib.context(dev), p.c(table.S), table, table.ids, table.key_pad, table.pos, table.ch,
                 norm.c() if norm is not None else None, lfq, cc, pp, out, normed, out_dtype)
    if normed:
        check_device_errors(dev)
    imgs = table.images(out)
    return (imgs, out) if return_flat else imgs


def dct2(x: torch.Tensor, inverse: bool, color: bool) -> torch.Tensor:
    """dctae_dct2 on a (3, H, W) or (B, 3, H, W) fp32 device tensor: full-image
    orthonormal DCT-II of rgb_to_ipt(x) (FE._transform_image_in, FE:129-142) or
    ipt_to_rgb of the DCT-III (FE._transform_image_out, FE:144-152); color=False
    is util.dct2 / util.idct2 alone (util.py:333-338)."""
    one = x.dim() == 3
    xb = x[None] if one else x
    if xb.dim() != 4 or xb.shape[1] != 3:
        raise AssertionError(f"expected (3, h, w) or (b, 3, h, w), got {tuple(x.shape)}")
    xb = xb if (xb.dtype == torch.float32 and xb.is_contiguous()) else xb.float().contiguous()
    dev = _check_dev(xb)
    ctx = _lib.context(dev)
    y = torch.empty_like(xb)
    B, _, H, W = xb.shape
    color = int(color) if not isinstance(color, bool) else int(color)   # 0 / 1, or 2 / 3: fp16 / bf16 colour
    rc = ctx.lib.dctae_dct2(ctx.h, ptr(xb), B, H, W, int(bool(inverse)), color, ptr(y),
                            _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_dct2")
    return y[0] if one else y


def patch_spectrum(x: torch.Tensor, p: FEParams, k: int):
    """dctae_patch_spectrum: FE._patch_image (FE:364-452) of a cropped (3, h, w)
    spectrum on the device -> (patches (k, P*P), positions (k, 2), channels (k))."""
    x = x if (x.dtype == torch.float32 and x.is_contiguous()) else x.float().contiguous()
    dev = _check_dev(x)
    if x.dim() != 3:
        raise AssertionError(f"expected a (c, h, w) spectrum, got {tuple(x.shape)}")
    ctx = _lib.context(dev)
    P = p.patch_size
    patches = torch.empty((k, P * P), dtype=torch.float32, device=dev)
    pos = torch.empty((k, 2), dtype=torch.long, device=dev)
    ch = torch.empty((k,), dtype=torch.long, device=dev)
    cfg = p.c(p.max_seq_len)
    rc = ctx.lib.dctae_patch_spectrum(ctx.h, C.byref(cfg), ptr(x), x.shape[1], x.shape[2], int(k), ptr(patches),
                                      ptr(pos), ptr(ch), None, _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_patch_spectrum")
    return patches, pos, ch


def synth_images(n: int, h: int, w: int, seed: int, first_index: int = 0, device=None) -> torch.Tensor:
    """(n, 3, h, w) counter-RNG images generated on the device (oracle/rng.py hash)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    ctx = _lib.context(dev)
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
    rc = ctx.lib.dctae_synth_images(ctx.h, C.c_uint64(seed), first_index, n, h, w, ptr(out), _lib.stream_ptr(dev))
    ctx.check(rc, "dctae_synth_images")
    return out
