"""DCTAutoencoderFeatureExtractor — drop-in for the reference's
dct_autoencoder/feature_extraction_dct_autoencoder.py:107-656 (FE below),
running on MI355X through libdctae.

Reference methods keep their names, arguments and results:
  preprocess(im)                 FE:154-177   -> dict(patches, positions, channels, original_sizes, patch_sizes)
  iter_batches(loader, bs)       FE:179-287   -> DCTPatches generator (same emission quirks)
  postprocess(dct_patches)       FE:289-310   -> list of (3, H, W) RGB images
  revert_patching(dct_patches)   FE:607-656   -> list of (3, 14ph, 14pw) spectra
  _transform_image_in / _transform_image_out   FE:129-152 (dctae_dct2)
  _get_crop_dims / _crop_image / _patch_image (dctae_patch_spectrum) / _group_patches_by_max_seq_len / _batch_groups
Stage hooks: callers replace these per instance or in a subclass (the
reference's decode_gif.py:86-91 sets ``_transform_image_out = lambda x: x`` to
render the spectrum; its tests/testpatching.py:42-43 makes both transforms the
identity).  preprocess / postprocess / iter_batches / encode_batch then run the
reference's stage sequence (FE:154-177, 179-287, 289-310) through the hooks,
each default stage still a HIP kernel; with no override they run the fused
launch sequence.
Additive fused entry points (the MI355X hot path):
  encode_batch(images, patchnorm, lfq, batch_size)  preprocess + pack + PatchNorm + LFQ in one launch sequence
  decode_batch(dct_patches, codes, patchnorm, lfq)  indices_to_codes + inverse_norm + postprocess

Deviations (documented in DESIGN.md):
  * tokens of equal importance score are ordered by flat index (the
    reference's CPU sort is unstable at ties, FE:418);
  * everything stays on the input's HIP device (the reference round-trips
    through the CPU for the FFT, FE:138-141, and keeps batches on the CPU,
    FE:204-207);
  * ``DCTPatches.attn_mask`` is computed lazily.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass
from typing import Any, Dict, Iterator, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _ops, packing
from . import resize as _resize
from ._ops import FEParams
from .dct_patches import DCTPatches


@dataclass
class GroupPatchesState:
    """FE:96-104"""
    groups: List[List[torch.Tensor]]
    groups_pos: List[List[torch.Tensor]]
    group: List[torch.Tensor]
    group_pos: List[torch.Tensor]
    groups_channels: List[List[torch.Tensor]]
    group_channels: List[torch.Tensor]
    seq_len: int


class DCTAutoencoderFeatureExtractor:
    def __init__(self, channels: int, patch_size: int, sample_patches_beta: float, max_patch_h: int,
                 max_patch_w: int, max_seq_len: int, channel_importances: Tuple[float, float, float] = (8.0, 1.0, 1.0),
                 patch_sample_magnitude_weight: float = 0.1, device=None):
        self.channels = channels
        self.patch_size = patch_size
        self.sample_patches_beta = sample_patches_beta
        self.max_patch_h = max_patch_h
        self.max_patch_w = max_patch_w
        self.max_seq_len = max_seq_len
        self.channel_importances = torch.Tensor(channel_importances)
        self.patch_sample_magnitude_weight = patch_sample_magnitude_weight
        self.device = device
        self.rng = random  # python ``random`` stream used for k ~ Exp(beta) (util.py:171)

    # ------------------------------------------------------------------ helpers
    def params(self, max_seq_len: Optional[int] = None) -> FEParams:
        return FEParams(channels=self.channels, patch_size=self.patch_size, max_patch_h=self.max_patch_h,
                        max_patch_w=self.max_patch_w,
                        max_seq_len=self.max_seq_len if max_seq_len is None else max_seq_len,
                        channel_importances=tuple(float(v) for v in self.channel_importances.tolist()),
                        magnitude_weight=float(self.patch_sample_magnitude_weight))

    def _dev(self, t: torch.Tensor) -> torch.Tensor:
        if t.is_cuda:
            return t
        if not torch.cuda.is_available():
            from ._lib import DCTAEUnavailable
            raise DCTAEUnavailable("no HIP device: the MI355X path has no CPU fallback")
        dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        return t.to(dev)

    def _tokens(self, h: int, w: int) -> int:
        return packing.tokens_per_image(h, w, self.channels, self.patch_size, self.max_patch_h, self.max_patch_w)

    def _k(self, h: int, w: int) -> int:
        return packing.choose_k(self._tokens(h, w), self.sample_patches_beta, self.max_seq_len, self.rng)

    # ------------------------------------------------------------- stage hooks
    def _overridden(self, name: str) -> bool:
        """True when a caller replaced the stage `name` on this instance or in a subclass."""
        return name in self.__dict__ or getattr(type(self), name) is not getattr(DCTAutoencoderFeatureExtractor, name)

    def _staged_in(self) -> bool:
        return any(self._overridden(n) for n in ("_transform_image_in", "_crop_image", "_patch_image"))

    def _staged_out(self) -> bool:
        return any(self._overridden(n) for n in ("_transform_image_out", "revert_patching"))

    @torch.no_grad()
    def _transform_image_in(self, x: torch.Tensor) -> torch.Tensor:
        """FE:129-142: rgb_to_ipt, then the orthonormal dct2 of the whole
        (c, h, w) image (dctae_dct2); result in x's dtype and on x's device.
        The reference runs rgb_to_ipt in the input's dtype before ``.float()``:
        fp16 / bf16 inputs get that arithmetic (dctae_dct2 color 2 / 3)."""
        color = {torch.float16: 2, torch.bfloat16: 3}.get(x.dtype, 1)
        y = _ops.dct2(self._dev(x).float(), inverse=False, color=color)
        return y.to(x.dtype).to(x.device)

    def _transform_image_out(self, x: torch.Tensor) -> torch.Tensor:
        """FE:144-152: idct2 of the whole (c, h, w) spectrum, then ipt_to_rgb (dctae_dct2)."""
        y = _ops.dct2(self._dev(x).float(), inverse=True, color=True)
        return y.to(x.dtype).to(x.device)

    # ------------------------------------------------------------- reference API
    def _get_crop_dims(self, h: int, w: int):
        """FE:312-345"""
        return packing.crop_dims(h, w, self.patch_size)

    @torch.no_grad()
    def _crop_image(self, x: torch.Tensor) -> torch.Tensor:
        """FE:347-362"""
        c, h, w = x.shape
        assert c == self.channels
        ch, cw = self._get_crop_dims(h, w)
        return x[:, :ch, :cw]

    @torch.no_grad()
    def _patch_image(self, x: torch.Tensor):
        """FE:364-452 on a cropped (c, h, w) spectrum (dctae_patch_spectrum):
        tiles of the kept corner, importance order (score desc, flat index asc),
        top k (k drawn like the reference, FE:429-435)."""
        c, h, w = x.shape
        P = self.patch_size
        assert h % P == 0
        assert w % P == 0
        assert c == self.channels
        k = self._k(h, w)
        patches, pos, channels = _ops.patch_spectrum(self._dev(x), self.params(), k)
        patches = patches.to(x.dtype)   # the reference's patches keep the spectrum's dtype
        s, z = patches.shape
        assert z == P ** 2, f"{z} != {P ** 2}"
        assert s <= self.max_seq_len
        return patches, pos, channels

    @torch.no_grad()
    def preprocess(self, im: torch.Tensor) -> Dict[str, Any]:
        """FE:154-177 for one (c, h, w) RGB image in [0, 1]: IPT + DCT +
        spectral patching + importance order + top-k, all on the GPU.  With
        an overridden stage hook the reference's stage sequence runs instead."""
        if self._staged_in():
            return self._preprocess_staged(im)
        return self.preprocess_many([im])[0]

    @torch.no_grad()
    def _preprocess_staged(self, im: torch.Tensor) -> Dict[str, Any]:
        """FE:154-177 stage by stage, every stage through its (possibly replaced) hook."""
        im = self._transform_image_in(im)
        _, h, w = im.shape
        original_size = (h, w)
        im = self._crop_image(im)
        _, ch, cw = im.shape
        patch_size = (ch // self.patch_size, cw // self.patch_size)
        patches, pos, channels = self._patch_image(im)
        return dict(patches=patches, positions=pos, channels=channels, original_sizes=original_size,
                    patch_sizes=patch_size)

    @torch.no_grad()
    def preprocess_many(self, images: Sequence[torch.Tensor], dataset_crop: bool = False) -> List[Dict[str, Any]]:
        """``preprocess`` for several images in one launch sequence.
        dataset_crop=True: the images go through ``self.dataset_crop`` first
        (fp32 or uint8 images; the stages see the resized fp32 images)."""
        if dataset_crop:
            images = self.dataset_crop(images)
            if images and images[0].dtype == torch.uint8:   # none needed the resize: the fp32 images the bytes mean
                images = [_ops.u8_to_f32(im) for im in images]
        if self._staged_in() or any(im.dtype != torch.float32 for im in images):
            # fp16 / bf16 images: the reference's stage sequence, whose colour
            # transform runs in the input dtype (FE:135-141)
            return [self._preprocess_staged(im) for im in images]
        images = [self._dev(im) for im in images]
        for im in images:
            assert im.shape[0] == self.channels
        ks = [self._k(im.shape[1], im.shape[2]) for im in images]
        S = max(ks)
        rows = [[i] for i in range(len(images))]
        plan = packing.layout(rows, dict(enumerate(ks)))
        desc, dev, keep = _ops.image_set(images)
        res = _ops.encode(desc, dev, self.params(S), plan, len(images), S, None, None, want_codes=False,
                          want_raw=True)
        out = []
        for i, im in enumerate(images):
            k = ks[i]
            h, w = im.shape[1], im.shape[2]
            out.append(dict(patches=res["raw"][i, :k], positions=res["positions"][i, :k],
                            channels=res["channels"][i, :k], original_sizes=(h, w),
                            patch_sizes=packing.patch_grid(h, w, self.patch_size)))
        return out

    @torch.no_grad()
    def iter_batches(self, dataloader, batch_size: Optional[int] = None) -> Iterator[DCTPatches]:
        """FE:179-287: greedy packing of preprocessed items into rows of
        max_seq_len; same emission rules (see packing.iter_batch_plans)."""
        if self._overridden("_group_patches_by_max_seq_len"):
            yield from self._iter_batches_staged(dataloader, batch_size)
            return
        fixed = {"patches", "positions", "channels", "original_sizes", "patch_sizes"}
        items: Dict[int, Tuple] = {}
        cum_o: List = []
        cum_p: List = []
        cum_x: Dict[str, List] = {}
        st = None
        nxt = 0
        max_tok = self.max_patch_h * self.max_patch_w * self.channels
        while True:
            try:
                d = next(dataloader)
            except StopIteration:
                return
            ids = list(range(nxt, nxt + len(d["patches"])))
            nxt += len(ids)
            for i, pt, ps, ch in zip(ids, d["patches"], d["positions"], d["channels"]):
                items[i] = (pt, ps, ch)
            cum_o = cum_o + list(d["original_sizes"])
            cum_p = cum_p + list(d["patch_sizes"])
            for k, v in d.items():
                if k not in fixed:
                    cum_x.setdefault(k, []).extend(v)
            st = packing.group([items[i][0].shape[0] for i in ids], ids, self.max_seq_len, max_tok, st)
            if batch_size is None and st.cur:
                st.rows.append(st.cur)
                st.cur, st.seq_len = [], 0
            if batch_size is None or len(st.rows) > batch_size:
                emit = st.rows[:batch_size]
                st = packing.GroupState(rows=st.rows[batch_size:], cur=st.cur, seq_len=st.seq_len)
                n = sum(len(r) for r in emit)
                o_now, cum_o = cum_o[:n], cum_o[n:]
                p_now, cum_p = cum_p[:n], cum_p[n:]
                x_now = {k: v[:n] for k, v in cum_x.items()}
                cum_x = {k: v[n:] for k, v in cum_x.items()}
                batch = self._batch_groups([[items[i][0] for i in r] for r in emit],
                                           [[items[i][1] for i in r] for r in emit],
                                           [[items[i][2] for i in r] for r in emit],
                                           original_sizes=o_now, patch_sizes=p_now, _data=x_now)
                if batch_size is not None:
                    assert batch.patches.shape[0] == batch_size
                    # emitted groups leave the state for good (FE:235-243): drop their items
                    for r in emit:
                        for i in r:
                            items.pop(i, None)
                yield batch

    @torch.no_grad()
    def _iter_batches_staged(self, dataloader, batch_size: Optional[int]) -> Iterator[DCTPatches]:
        """FE:179-287 step by step through the (replaced) _group_patches_by_max_seq_len
        and _batch_groups hooks."""
        fixed = {"patches", "positions", "channels", "original_sizes", "patch_sizes"}
        state = None
        cum_o, cum_p, cum_x = [], [], {}
        while True:
            try:
                d = next(dataloader)
            except StopIteration:
                return
            cum_o = cum_o + list(d["original_sizes"])
            cum_p = cum_p + list(d["patch_sizes"])
            for k, v in d.items():
                if k not in fixed:
                    cum_x.setdefault(k, []).extend(v)
            state = self._group_patches_by_max_seq_len(d["patches"], d["positions"], d["channels"], state)
            if batch_size is None and len(state.group) > 0:
                state.groups.append(state.group)
                state.groups_pos.append(state.group_pos)
                state.groups_channels.append(state.group_channels)
                state.seq_len, state.group, state.group_pos, state.group_channels = 0, [], [], []
            if batch_size is None or len(state.groups) > batch_size:
                keep = GroupPatchesState(state.groups[batch_size:], state.groups_pos[batch_size:], state.group,
                                         state.group_pos, state.groups_channels[batch_size:], state.group_channels,
                                         state.seq_len)
                emit = (state.groups[:batch_size], state.groups_pos[:batch_size], state.groups_channels[:batch_size])
                n = sum(len(g) for g in emit[0])
                batch = self._batch_groups(*emit, original_sizes=cum_o[:n], patch_sizes=cum_p[:n],
                                           _data={k: v[:n] for k, v in cum_x.items()})
                if batch_size is not None:
                    assert batch.patches.shape[0] == batch_size
                cum_o, cum_p = cum_o[n:], cum_p[n:]
                cum_x = {k: v[n:] for k, v in cum_x.items()}
                state = keep
                yield batch

    @torch.no_grad()
    def _group_patches_by_max_seq_len(self, batched_patches, batched_positions, batched_channels, state=None):
        """FE:454-513 (kept for callers that drive the grouping themselves)."""
        if state is None:
            state = GroupPatchesState([], [], [], [], [], [], 0)
        for patches, pos, channels in zip(batched_patches, batched_positions, batched_channels):
            k = patches.shape[0]
            assert k <= self.max_patch_h * self.max_patch_w * self.channels and k <= self.max_seq_len, \
                f"patch with len {k} exceeds maximum sequence length"
            assert k == channels.shape[0]
            if state.seq_len + k > self.max_seq_len:
                state.groups.append(state.group)
                state.groups_pos.append(state.group_pos)
                state.groups_channels.append(state.group_channels)
                state.group, state.group_pos, state.group_channels, state.seq_len = [], [], [], 0
            state.group.append(patches)
            state.group_pos.append(pos)
            state.group_channels.append(channels)
            state.seq_len += k
        return state

    @torch.no_grad()
    def _batch_groups(self, grouped_batched_patches, grouped_batched_positions, grouped_batched_channels,
                      device=None, **dct_patch_kwargs) -> DCTPatches:
        """FE:515-605: concatenate rows, zero-pad to max_seq_len, image ids,
        key_pad_mask (True at padding).  attn_mask is lazy."""
        S = self.max_seq_len
        first = grouped_batched_patches[0][0]
        dev = device if device is not None else first.device
        R = len(grouped_batched_patches)
        z = first.shape[-1]
        patches = torch.zeros((R, S, z), dtype=first.dtype, device=dev)
        positions = torch.zeros((R, S, 2), dtype=torch.long, device=dev)
        channels = torch.zeros((R, S), dtype=torch.long, device=dev)
        ids = torch.zeros((R, S), dtype=torch.long, device=dev)
        lengths = []
        for r, (gp, gpos, gch) in enumerate(zip(grouped_batched_patches, grouped_batched_positions,
                                                grouped_batched_channels)):
            assert len(gp) == len(gpos) == len(gch)
            col = 0
            for j, (pt, ps, ch) in enumerate(zip(gp, gpos, gch)):
                k = pt.shape[0]
                assert pt.shape[1] == self.patch_size ** 2
                assert ps.shape[0] == k and ch.shape[0] == k
                patches[r, col:col + k] = pt
                positions[r, col:col + k] = ps
                channels[r, col:col + k] = ch
                ids[r, col:col + k] = j
                col += k
            assert col <= S
            lengths.append(col)
        lengths = torch.tensor(lengths, dtype=torch.long, device=dev)
        key_pad_mask = lengths[:, None] <= torch.arange(S, device=dev)[None, :]
        return DCTPatches(patches=patches, key_pad_mask=key_pad_mask, attn_mask=None, batched_image_ids=ids,
                          patch_positions=positions, patch_channels=channels, **dct_patch_kwargs)

    @torch.no_grad()
    def revert_patching(self, output: DCTPatches) -> List[torch.Tensor]:
        """FE:607-656: per image a zero (c, 14ph, 14pw) spectrum holding its tokens."""
        x = output.patches
        p = self.patch_size
        ids = output.batched_image_ids
        pad = output.key_pad_mask
        images = []
        for bi in range(x.shape[0]):
            for image_id in torch.unique(ids[bi]).tolist():
                sel = (ids[bi] == image_id) & ~pad[bi]
                ph, pw = output.patch_sizes[len(images)]
                img = torch.zeros(self.channels, ph, pw, x.shape[-1], dtype=x.dtype, device=x.device)
                pos = output.patch_positions[bi, sel]
                img[output.patch_channels[bi, sel], pos[:, 0], pos[:, 1]] = x[bi, sel]
                img = img.view(self.channels, ph, pw, p, p).permute(0, 1, 3, 2, 4).reshape(self.channels, ph * p, pw * p)
                images.append(img)
        return images

    def postprocess(self, x: DCTPatches, output_dtype: torch.dtype = torch.float32) -> List[torch.Tensor]:
        """FE:289-310: un-normalised DCTPatches -> RGB images (revert_patching,
        zero pad, DCT-III, IPT -> RGB fused on the GPU).  With an overridden
        _transform_image_out / revert_patching the reference's stage sequence
        runs through the hooks (e.g. the spectrum itself for decode_gif.py:86-91).

        Differentiable in the patches: patches that require grad (with grad
        enabled) give the same images, bit for bit, with a grad_fn whose
        backward is dctae_decode_backward; fp16 / bf16 patches are upcast to
        fp32 and the gradient is cast back.  The staged-hook path stays
        without a grad_fn.

        output_dtype=torch.uint8: uint8 images written by the decode itself
        (dctae_decode_u8), every byte the fp32 image's value through
        ``x.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)`` (save_image's
        rounding).  Bytes carry no grad_fn: patches that require grad take the
        no-grad path.  With overridden hooks the stages run in fp32 and each
        hook result is converted by dctae_f32_to_u8."""
        _ops.out_dtype_suffix(output_dtype, "postprocess output_dtype")
        if (output_dtype == torch.float32 and x.patches.requires_grad and torch.is_grad_enabled()
                and x.patches.is_cuda and not self._staged_out()):
            from . import losses
            return losses.differentiable_postprocess(self, x)
        return self._postprocess_no_grad(x, output_dtype)

    @torch.no_grad()
    def _postprocess_no_grad(self, x: DCTPatches, output_dtype: torch.dtype = torch.float32) -> List[torch.Tensor]:
        if self._staged_out():
            images = []
            for image, (h, w) in zip(self.revert_patching(x), x.original_sizes):
                ch, cw = image.shape[-2:]
                im_pad = torch.zeros(self.channels, h, w, device=image.device, dtype=image.dtype)
                im_pad[:, :ch, :cw] = image
                im = self._transform_image_out(im_pad)
                images.append(_ops.f32_to_u8(im.float()) if output_dtype == torch.uint8 else im)
            return images
        return _ops.decode(self.params(x.patches.shape[1]), x.batched_image_ids, x.key_pad_mask,
                           x.patch_positions, x.patch_channels, x.patch_sizes, x.original_sizes,
                           patches=x.patches, out_dtype=output_dtype)

    # ------------------------------------------------------------ dataset crop
    @property
    def dataset_max_size(self) -> int:
        """the reference's dataset.py:53-57 for this extractor: max(patch_size * max(max_patch_w, max_patch_h), 768)"""
        return _resize.dataset_max_size(self.patch_size, self.max_patch_h, self.max_patch_w)

    @torch.no_grad()
    def dataset_crop(self, images: Sequence[torch.Tensor], max_size: Optional[int] = None) -> List[torch.Tensor]:
        """The reference's dataset crop (dataset.py:59-73) for a list of
        (3, H, W) fp32 or uint8 images: every image with a side above max_size
        (default ``self.dataset_max_size``) is shrunk by the antialiased
        bilinear resize, all in one launch (resize.dataset_crop)."""
        images = [self._dev(im) if isinstance(im, torch.Tensor) else im for im in images]
        return _resize.dataset_crop(images, self.dataset_max_size if max_size is None else max_size)

    # ------------------------------------------------------- fused MI355X path
    @torch.no_grad()
    def encode_batch(self, images, patchnorm=None, lfq=None, batch_size: Optional[int] = None,
                     return_patches: bool = False, return_raw: bool = False, return_scores: bool = False,
                     ks: Optional[Sequence[int]] = None, uint8_images: bool = False,
                     codes_dtype: torch.dtype = torch.int64,
                     dataset_crop: bool = False) -> List[Tuple[DCTPatches, Optional[torch.Tensor]]]:
        """preprocess every image, pack (iter_batches over ONE dataloader item
        holding all images, FE:179-287), PatchNorm (eval) and LFQ — the
        encode half of SURVEY §3.1-3.3 — in one launch sequence per batch.

        images: (B, 3, H, W) tensor or a list of (3, H, W) tensors on the GPU.
        Returns [(DCTPatches, codes)] per emitted batch; DCTPatches.patches
        holds the PatchNorm output if return_patches, the raw DCT tokens if
        return_raw, else an empty (R, S, 0) tensor.  codes is None without lfq.
        With an overridden stage hook the reference's stages run one by one.

        uint8_images=True: `images` holds uint8 RGB bytes (any other dtype
        raises TypeError), each meaning the fp32 image ``u8.float() / 255``;
        the row kernels read the bytes themselves and every output is
        bit-identical to the call on that fp32 image (dctae_encode_u8).  The
        stage hooks, where overridden, are handed those fp32 images.  The
        bytes are read in place; only a non-contiguous image, or a 512-wide
        one at an address that is not 4-byte aligned, is copied first.

        codes_dtype=torch.int16: the codes as int16 (any dtype but int64 and
        int16 raises TypeError), each the int64 call's code converted with
        ``.to(torch.int16)`` and so ``codes.long()`` the int64 call's codes;
        every other output is bit-identical.  The sort / pack kernels store
        two bytes per code (dctae_encode_c16, include/dctae_codes16.h).  Codes
        lie in [0, 2^codebook_dim): codebook_dim >= 16 raises ValueError.  On
        the staged path (an overridden hook) and with projections that are not
        the fused ones the int16 codes come from a torch conversion: correct,
        not fast.  The DCTPatches metadata stays int64.

        dataset_crop=True: the images go through ``self.dataset_crop`` first
        (the reference's dataset.py:59-73, one resize launch for all of them),
        and every output is bit-identical to the call on
        ``self.dataset_crop(images)``.  Byte images that needed a resize
        continue as the fp32 images it wrote; where none did, the bytes are
        encoded in place as without the option.  The stage hooks, where
        overridden, are handed the resized fp32 images.
        """
        _ops.codes_dtype_suffix(codes_dtype, "encode_batch codes_dtype")
        if codes_dtype == torch.int16 and lfq is not None:
            _ops.check_codes16(lfq.cfg(), "encode_batch")
        if uint8_images:
            batched = isinstance(images, torch.Tensor) and images.dim() == 4
            if not batched:
                images = list(images)   # once: the check below must not use up an iterator
            for im in ([images] if batched else images):
                if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8:
                    raise TypeError(f"uint8_images=True needs uint8 tensors, got {getattr(im, 'dtype', type(im))}")
        if dataset_crop:
            if isinstance(images, torch.Tensor) and images.dim() == 4:
                if _resize.dataset_crop_size(images.shape[2], images.shape[3], self.dataset_max_size) is not None:
                    images = list(images.unbind(0))
            if not isinstance(images, torch.Tensor):
                images = self.dataset_crop(images)
                uint8_images = uint8_images and bool(images) and images[0].dtype == torch.uint8
        if self._staged_in() or self._overridden("_group_patches_by_max_seq_len") or \
                self._overridden("_batch_groups"):
            if uint8_images:   # the hooks see the fp32 images the bytes mean (dctae_u8_to_f32)
                images = [_ops.u8_to_f32(self._dev(im)) for im in images]
            outs = self._encode_staged(images, patchnorm, lfq, batch_size, return_patches, return_raw)
            return [(dp, c if c is None else c.to(codes_dtype)) for dp, c in outs]
        if isinstance(images, torch.Tensor) and images.dim() == 4:
            x = self._dev(images)
            B, _, H, W = x.shape
            sizes = [(H, W)] * B
            desc, dev, keep = (_ops.batch_image_set_u8 if uint8_images else _ops.batch_image_set)(x)
            img_list = None
        else:
            img_list = [self._dev(im) for im in images]
            sizes = [(im.shape[1], im.shape[2]) for im in img_list]
            desc, dev, keep = (_ops.image_set_u8 if uint8_images else _ops.image_set)(img_list)
        if ks is None:
            ks = [self._k(h, w) for h, w in sizes]
        max_tok = self.max_patch_h * self.max_patch_w * self.channels
        plans = list(packing.iter_batch_plans([(ks, list(range(len(ks))))], self.max_seq_len, max_tok, batch_size))
        if lfq is not None and patchnorm is None:
            raise AssertionError("LFQ codes need a PatchNorm")
        # LFQ with projections (dim != codebook_dim * num_codebooks, lfq.py:54-62,
        # e.g. conf/patch14-l.json's 196 -> 16 x 13): the fused launch stops at the
        # PatchNorm output and the fused project_in + sign + pack kernel
        # (dctae_lfq_project_in) follows on the same stream
        proj = lfq is not None and lfq.has_projections
        want_norm = return_patches or proj
        norm = patchnorm.state(thresholds=not want_norm) if patchnorm is not None else None
        lcfg = lfq.cfg() if lfq is not None and not proj else None
        outs = []
        for rows in plans:
            plan = packing.layout(rows, dict(enumerate(ks)))
            sub = self._subset(desc, keep, plan.images) if len(plan.images) != len(ks) else desc
            plan_local = packing.layout([[plan.images.index(i) for i in r] for r in rows],
                                        {j: ks[i] for j, i in enumerate(plan.images)}) \
                if len(plan.images) != len(ks) else plan
            res = _ops.encode(sub, dev, self.params(), plan_local, plan.n_rows, self.max_seq_len, norm, lcfg,
                              want_codes=lcfg is not None, want_patches=want_norm, want_raw=return_raw,
                              want_scores=return_scores, codes_dtype=codes_dtype)
            if proj:   # codes only: lfq.py:136-187 without the quantized output's project_out
                # fused project_in + sign + pack on the PatchNorm output, whose clamp
                # (patchnorm.py:163) bounds it: the kernels of BatchEncoder's staged path
                xb = max(abs(norm.min_val), abs(norm.max_val))
                res["codes"] = lfq.project_codes(res["patches"], x_bound=xb if 0.0 < xb < math.inf else None,
                                                 codes_dtype=codes_dtype)
            pt = res["patches"] if return_patches else res.get("raw")
            if pt is None:
                pt = torch.empty((plan.n_rows, self.max_seq_len, 0), device=dev)
            dp = DCTPatches(patches=pt, key_pad_mask=res["key_pad_mask"], attn_mask=None,
                            batched_image_ids=res["image_ids"], patch_channels=res["channels"],
                            patch_positions=res["positions"],
                            patch_sizes=[packing.patch_grid(*sizes[i], self.patch_size) for i in plan.images],
                            original_sizes=[tuple(sizes[i]) for i in plan.images])
            if return_patches and return_raw:
                dp._data = {"raw_patches": res["raw"]}
            if return_scores:
                dp._data = (dp._data or {}) | {"scores": res["scores"]}
            outs.append((dp, res.get("codes")))
        return outs

    @torch.no_grad()
    def _encode_staged(self, images, patchnorm, lfq, batch_size, return_patches, return_raw):
        """encode_batch through the stage hooks: preprocess -> iter_batches ->
        PatchNorm (eval) -> LFQ (eval), each stage on its own launch."""
        items = [self.preprocess(im) for im in images]
        loader = iter([{k: [it[k] for it in items] for k in items[0]}])
        outs = []
        for batch in self.iter_batches(loader, batch_size):
            codes, normed = None, None
            if patchnorm is not None:
                normed = patchnorm(batch.shallow_copy())
                if lfq is not None:
                    _, codes, _, _ = lfq(normed, mask=~batch.key_pad_mask)
            if not return_raw:
                batch.patches = normed if (return_patches and normed is not None) else \
                    torch.empty((*batch.patches.shape[:2], 0), device=batch.patches.device)
            elif return_patches and normed is not None:
                batch._data = (batch._data or {}) | {"normalised_patches": normed}
            outs.append((batch, codes))
        return outs

    @staticmethod
    def _subset(desc, keep, idx):
        import ctypes as C
        from ._lib import i32, i64
        offs = [keep[1][i] for i in idx]
        hw = []
        for i in idx:
            hw += [keep[2][2 * i], keep[2][2 * i + 1]]
        k2 = [i64(offs), i32(hw)]
        keep.append(k2)
        return type(desc)(desc.rgb_dev, C.cast(k2[0], C.POINTER(C.c_int64)), C.cast(k2[1], C.POINTER(C.c_int32)),
                          len(idx))   # Images or ImagesU8, as the call's descriptor

    @torch.no_grad()
    def decode_batch(self, dct_patches: DCTPatches, codes: torch.Tensor, patchnorm, lfq,
                     output_dtype: torch.dtype = torch.float32) -> List[torch.Tensor]:
        """LFQ.indices_to_codes -> PatchNorm.inverse_norm -> postprocess, fused
        (the decode half of SURVEY §3.4 without the transformer).  With LFQ
        projections the codes go through the fused codes -> project_out kernel and the HIP
        inverse PatchNorm first, and the fused decode starts from the tokens.
        output_dtype=torch.uint8: uint8 images, as postprocess gives them.
        codes: int64, or int16 (an int16 code c means int64(c); read two bytes
        per code by the kernels, no widened copy; every pixel is bit-identical
        to the decode of ``codes.long()``).  Any other dtype raises TypeError;
        int16 codes with codebook_dim >= 16 raise ValueError."""
        _ops.out_dtype_suffix(output_dtype, "decode_batch output_dtype")
        _ops.codes_dtype_suffix(codes.dtype, "decode_batch codes")
        if codes.dtype == torch.int16:
            _ops.check_codes16(lfq.cfg(), "decode_batch")
        staged = self._staged_out()   # an overridden revert_patching / _transform_image_out (FE:289-310)
        if lfq.has_projections or staged:
            dp = dct_patches.shallow_copy()
            if lfq.has_projections and lfq._fused_proj() and lfq.dim == self.patch_size ** 2 and not staged:
                # project_out alone, the inverse PatchNorm inside the decode
                # (dctae_decode_normed)
                w, b = lfq._proj_w(lfq.project_out, codes.device)
                x = _ops.lfq_project_out(codes, w, b, lfq.cfg())
                return _ops.decode(self.params(dp.key_pad_mask.shape[1]), dp.batched_image_ids, dp.key_pad_mask,
                                   dp.patch_positions, dp.patch_channels, dp.patch_sizes, dp.original_sizes,
                                   patches=x, norm=patchnorm.state(thresholds=False), normed=True,
                                   out_dtype=output_dtype)
            else:
                dp.patches = lfq.indices_to_codes(codes)
                dp.patches = patchnorm.inverse_norm(dp)
            return self.postprocess(dp, output_dtype)
        return _ops.decode(self.params(dct_patches.key_pad_mask.shape[1]), dct_patches.batched_image_ids,
                           dct_patches.key_pad_mask, dct_patches.patch_positions, dct_patches.patch_channels,
                           dct_patches.patch_sizes, dct_patches.original_sizes, codes=codes,
                           norm=patchnorm.state(), lfq=lfq.cfg(), out_dtype=output_dtype)

    # ------------------------------------------------------------ progressive decode
    def postprocess_prefixes(self, x: DCTPatches, prefixes, output_dtype: torch.dtype = torch.float32,
                             clip=None) -> List[List[torch.Tensor]]:
        """The token-prefix frames of every image of un-normalised DCTPatches in
        one launch sequence (progressive.postprocess_prefixes): frame (i, k) is,
        bit for bit, image i of ``postprocess`` with all but the image's first
        min(k, n_i) real tokens padded.  prefixes: ints for every image, or one
        sequence per image; clip: None or "minmax" (``image_clip`` of every frame)."""
        from . import progressive
        return progressive.postprocess_prefixes(self, x, prefixes, output_dtype, clip)

    def decode_prefixes(self, dct_patches: DCTPatches, codes: torch.Tensor, patchnorm, lfq, prefixes,
                        output_dtype: torch.dtype = torch.float32, clip=None) -> List[List[torch.Tensor]]:
        """postprocess_prefixes from LFQ codes, on ``decode_batch``'s branches (progressive.decode_prefixes)."""
        from . import progressive
        return progressive.decode_prefixes(self, dct_patches, codes, patchnorm, lfq, prefixes, output_dtype, clip)

    def model_decode_prefixes(self, model, dct_patches: DCTPatches, codes: torch.Tensor, prefixes,
                              output_dtype: torch.dtype = torch.float32, clip=None) -> List[List[torch.Tensor]]:
        """The prefix frames through the transformer decoder (progressive.model_decode_prefixes): frame (i, k)
        is, bit for bit, ``postprocess`` of ``model.decode_from_codes`` on the first min(k, n_i) real tokens of
        image i as a one-row batch without padding (decode_gif.py), all frames in one pass per chunk."""
        from . import progressive
        return progressive.model_decode_prefixes(self, model, dct_patches, codes, prefixes, output_dtype, clip)

    def image_clip(self, images: Sequence[torch.Tensor], output_dtype: torch.dtype = torch.float32
                   ) -> List[torch.Tensor]:
        """util.py:143-147 on a list of (3, H, W) fp32 device images of any sizes, in one launch sequence
        (progressive.image_clip_many)."""
        from . import progressive
        return progressive.image_clip_many(images, output_dtype)


class BatchEncoder:
    """Pre-planned fused encode for a fixed batch geometry (the bench and
    serving path): packing plan, ctypes descriptors and output buffers are
    built once; each call only enqueues the kernels (dctae_encode).
    input_dtype=torch.uint8: the calls take (B, 3, H, W) uint8 bytes meaning
    ``u8.float() / 255`` (dctae_encode_u8 / dctae_encode_lfq_proj_u8), outputs
    bit-identical to the fp32 encoder's on that tensor.
    codes_dtype=torch.int16: ``out["codes"]`` is int16, each code the int64
    encoder's converted (the ``_c16`` entries of include/dctae_codes16.h; any
    other dtype raises TypeError, codebook_dim >= 16 ValueError); every other
    output the same."""

    def __init__(self, fe: DCTAutoencoderFeatureExtractor, batch: int, height: int, width: int, patchnorm, lfq,
                 device=None, want_patches: bool = False, input_dtype: torch.dtype = torch.float32,
                 codes_dtype: torch.dtype = torch.int64):
        import ctypes as C
        from ._lib import Images, LFQCfg, Packing, PackedOut, PackedOut16, i32, i64, ptr
        self.fe = fe
        self.dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.dev.index is None:   # "cuda" -> the current device, as tensors report it
            self.dev = torch.device(self.dev.type, torch.cuda.current_device())
        self.B, self.H, self.W = batch, height, width
        if input_dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"BatchEncoder input_dtype: torch.float32 or torch.uint8, got {input_dtype}")
        self.input_dtype = input_dtype
        self.codes_dtype = codes_dtype
        self._sfx = ("_u8" if input_dtype == torch.uint8 else "") + \
            _ops.codes_dtype_suffix(codes_dtype, "BatchEncoder codes_dtype")
        if codes_dtype == torch.int16:
            _ops.check_codes16(lfq.cfg(), "BatchEncoder")
        if fe.sample_patches_beta > 0:
            raise AssertionError("BatchEncoder needs sample_patches_beta == 0 (fixed k)")
        k = fe._tokens(height, width)
        k = min(k, fe.max_seq_len)
        max_tok = fe.max_patch_h * fe.max_patch_w * fe.channels
        (rows,) = list(packing.iter_batch_plans([([k] * batch, list(range(batch)))], fe.max_seq_len, max_tok, None))
        self.plan = packing.layout(rows, {i: k for i in range(batch)})
        self.k = k
        self.n_rows = self.plan.n_rows
        self.S = fe.max_seq_len
        # LFQ with projections (lfq.py:54-62): with every packed row full,
        # dctae_encode_lfq_proj runs project_in + sign + pack on the staged
        # PatchNorm output before the sort / pack; otherwise the fused launch
        # stops at the packed PatchNorm output and dctae_lfq_project_in follows
        self.lfq = lfq
        self.proj = lfq.has_projections
        if self.proj and not lfq._fused_proj():
            raise NotImplementedError("BatchEncoder: LFQ projections of this shape run through encode_batch")
        self.proj_staged = (self.proj and all(n == fe.max_seq_len for n in self.plan.row_len)
                            and lfq.codebook_dim <= 16 and (fe.patch_size ** 2) % 4 == 0)
        want_norm = want_patches or (self.proj and not self.proj_staged)
        self.patchnorm, self._thr = patchnorm, not want_norm
        self._take_norm()
        self.lcfg = lfq.cfg()
        self.p = fe.params()
        per = 3 * height * width
        self._keep = [i64([i * per for i in range(batch)]), i32([height, width] * batch)]
        pl = self.plan
        self._pk_keep = [i32(pl.row), i32(pl.col), i32(pl.k), i32(pl.local_id), i32(pl.row_len)]
        self.packing = Packing(*[C.cast(a, C.POINTER(C.c_int32)) for a in self._pk_keep], self.n_rows)
        R, S = self.n_rows, self.S
        self.out = {
            "codes": torch.empty((R, S, self.lcfg.num_codebooks), dtype=codes_dtype, device=self.dev),
            "positions": torch.empty((R, S, 2), dtype=torch.long, device=self.dev),
            "channels": torch.empty((R, S), dtype=torch.long, device=self.dev),
            "image_ids": torch.empty((R, S), dtype=torch.long, device=self.dev),
            "key_pad_mask": torch.empty((R, S), dtype=torch.bool, device=self.dev),
        }
        if want_norm:
            self.out["patches"] = torch.empty((R, S, fe.patch_size ** 2), dtype=torch.float32, device=self.dev)
        o = self.out
        self.po = (PackedOut16 if codes_dtype == torch.int16 else PackedOut)(ptr(None if self.proj and not self.proj_staged else o["codes"]), ptr(o["positions"]), ptr(o["channels"]), ptr(o["image_ids"]),
                            ptr(o["key_pad_mask"]), ptr(o.get("patches")), None, None)
        self._cfg = self.p.c(S)
        from . import _lib
        self.ctx = _lib.context(self.dev)

    def _take_norm(self):
        """The PatchNorm tables (and thresholds) as they are now; taken again
        only when the module's stamp has moved (an in-place update, a
        load_state_dict, a training step, another eps or clamp)."""
        self._norm_stamp = self.patchnorm._stamp()
        self.norm = self.patchnorm.state(thresholds=self._thr)
        self._ncfg = self.norm.c()

    def __call__(self, x: torch.Tensor):
        import ctypes as C
        from ._lib import Images, ImagesU8, ptr, stream_ptr
        assert x.shape == (self.B, 3, self.H, self.W) and x.dtype == self.input_dtype and x.is_contiguous()
        assert x.device == self.dev
        if self.patchnorm._stamp() != self._norm_stamp:   # host compare; unchanged tables add no device work
            self._take_norm()
        u8 = self.input_dtype == torch.uint8
        if u8 and self.W == 512 and x.data_ptr() % 4:   # the 512-wide row kernel's dword loads (include/dctae_u8.h)
            x = x.clone()
        imgs = (ImagesU8 if u8 else Images)(C.c_void_p(x.data_ptr()), C.cast(self._keep[0], C.POINTER(C.c_int64)),
                      C.cast(self._keep[1], C.POINTER(C.c_int32)), self.B)
        if self.proj_staged:
            w, b = self.lfq._proj_w(self.lfq.project_in, self.dev)
            name = "dctae_encode_lfq_proj" + self._sfx
            rc = getattr(self.ctx.lib, name)(self.ctx.h, C.byref(self._cfg), C.byref(imgs), C.byref(self.packing),
                                             C.byref(self._ncfg), C.byref(self.lcfg), ptr(w), ptr(b),
                                             C.byref(self.po), stream_ptr(self.dev))
            self.ctx.check(rc, name)
            return self.out
        name = "dctae_encode" + self._sfx
        rc = getattr(self.ctx.lib, name)(self.ctx.h, C.byref(self._cfg), C.byref(imgs), C.byref(self.packing),
                                         C.byref(self._ncfg), None if self.proj else C.byref(self.lcfg),
                                         C.byref(self.po), stream_ptr(self.dev))
        self.ctx.check(rc, name)
        if self.proj:
            w, b = self.lfq._proj_w(self.lfq.project_in, self.dev)
            from . import _ops
            self.out["codes"] = _ops.lfq_project_in_into(self.out["patches"], w, b, self.lcfg, self.out["codes"],
                                                         codes_dtype=self.codes_dtype)
        return self.out


class BatchDecoder:
    """Pre-planned fused decode for a BatchEncoder's fixed geometry (config 3
    round trip): LFQ.indices_to_codes -> PatchNorm.inverse_norm ->
    revert_patching -> IDCT -> IPT -> RGB of the encoder's packed outputs
    (dctae_decode), images in the reference's enumeration order (rows in
    order, image ids ascending, FE:619-633) into one (B, 3, H, W) tensor.
    output_dtype=torch.uint8: ``out`` is a (B, 3, H, W) uint8 tensor written by
    the decode itself (dctae_decode_u8 / dctae_decode_normed_u8), every byte the
    fp32 decoder's value through ``mul(255).add(0.5).clamp(0, 255)`` truncated.
    ``packed["codes"]``: int64, or int16 read as it is (the ``_c16`` entries of
    include/dctae_codes16.h; pixels bit-identical to those from
    ``codes.long()``); any other dtype raises TypeError."""

    def __init__(self, enc: "BatchEncoder", patchnorm, lfq, output_dtype: torch.dtype = torch.float32):
        _ops.out_dtype_suffix(output_dtype, "BatchDecoder output_dtype")
        self.output_dtype = output_dtype
        self.enc = enc
        pl, p = enc.plan, enc.fe.patch_size
        self.table = _ops.DecodeTable.from_layout(enc.p, enc.dev, enc.n_rows, enc.S, pl.row, pl.local_id,
                                                  (enc.H, enc.W), (enc.H // p, enc.W // p))
        self.lfq, self.patchnorm = lfq, patchnorm
        self._take_norm()
        self.lcfg = lfq.cfg()
        self.proj = lfq.has_projections
        # LFQ with projections (lfq.py:54-62).  True: project_out alone (dctae_lfq_project_out) and the inverse
        # PatchNorm inside the decode's column kernel (dctae_decode_normed: per-block (c, strip) tables instead
        # of a per-token table gather); False: project_out with the inverse fused
        # (dctae_lfq_project_out_inverse_norm), then dctae_decode
        self.normed_decode = True
        self.out = torch.empty((enc.B, 3, enc.H, enc.W), dtype=output_dtype, device=enc.dev)

    def _decode(self, packed, norm, lcfg, codes, patches, normed=False) -> torch.Tensor:
        e = self.enc
        _ops._decode_call(e.ctx, e._cfg, self.table, packed["image_ids"], packed["key_pad_mask"],
                          packed["positions"], packed["channels"], norm, lcfg, codes, patches, self.out, normed,
                          self.output_dtype)
        return self.out

    def _take_norm(self):
        """As BatchEncoder._take_norm: the tables now, retaken when the stamp moves."""
        self._norm_stamp = self.patchnorm._stamp()
        self.norm = self.patchnorm.state(thresholds=False)
        self._ncfg = self.norm.c()

    def __call__(self, packed) -> torch.Tensor:
        e = self.enc
        if self.patchnorm._stamp() != self._norm_stamp:
            self._take_norm()
        _ops.codes_dtype_suffix(packed["codes"].dtype, "BatchDecoder codes")
        if packed["codes"].dtype == torch.int16:
            _ops.check_codes16(self.lcfg, "BatchDecoder")
        if not self.proj:
            return self._decode(packed, self._ncfg, self.lcfg, packed["codes"], None)
        if not self.lfq._fused_proj():
            x = self.lfq.indices_to_codes(packed["codes"]).float()
            x = _ops.norm_apply(x, packed["channels"], packed["positions"], self.norm, e.fe.params(), inverse=True)
            return self._decode(packed, None, None, None, x)
        w, b = self.lfq._proj_w(self.lfq.project_out, e.dev)
        if self.normed_decode:
            x = _ops.lfq_project_out(packed["codes"], w, b, self.lcfg)
            return self._decode(packed, self._ncfg, None, None, x, normed=True)
        x = _ops.lfq_project_out_inverse_norm(packed["codes"], w, b, self.lcfg, self.norm, e.fe.params(),
                                              packed["channels"], packed["positions"])
        return self._decode(packed, None, None, None, x)
