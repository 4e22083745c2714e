"""DCTAutoencoder — drop-in for the reference's transformer autoencoder around
the LFQ bottleneck (dct_autoencoder/modeling_dct_autoencoder.py, with the
CLIPEncoder of transformers==4.35.2), inference and training on MI355X
(DESIGN.md §4b / §4e).

Same constructor (a ``DCTAutoencoderConfig``), parameter names / state-dict
keys (a reference checkpoint loads with ``load_state_dict``), and methods
``normalize_`` / ``inv_normalize_`` / ``encode`` / ``decode`` /
``decode_from_codes`` / ``forward`` / ``get_pos_embedding_decoder`` /
``add_pos_embedding_{en,de}coder_`` (modeling:86-200).  Every op of the
forward runs on libdctae's HIP kernels (dctae_model_*: bf16 MFMA linear
layers with fused bias / quick_gelu / residual epilogues, flash attention,
LayerNorm, LFQ codes); weights are kept as fp32 parameters and packed once
into bf16 device copies (K zero-padded to 64).  The residual stream and every
accumulation are fp32; the reference runs this model in fp16 / bf16 autocast
(main.py:331-347, prepare_autoregressive_dataset.py:21).

Attention reproduces the reference exactly as 4.35.2 executes it: the bool
``DCTPatches.attn_mask`` is ADDED to the logits (+1.0 where the query's image
id equals the key's and the key is padding, FE:580-584) and nothing is masked
(modeling:131-133 passes it as ``attention_mask``).  A caller-assigned
``attn_mask`` tensor is not consulted: the kernel derives the mask from
``batched_image_ids`` / ``key_pad_mask``, which is how the feature extractor
defines it.

``.eval()``: ``encode`` / ``decode`` / ``decode_from_codes`` / ``forward`` run
under ``no_grad``.  ``.train()``: the same methods run under autograd
(model_train.py: one ``torch.autograd.Function`` per CLIP layer, one each for
the patch embedding, the decoder position add and ``proj_out``), forward and
backward on HIP kernels with bf16 operands, fp32 master weights, fp32 residual
and gradient streams and no floating-point atomics, so a step repeats bit for
bit.  ``encode`` then goes through the quantizer's training forward
(``self.vq_model(h, mask=~key_pad_mask)``: straight-through output, codes,
commit loss, ``LFQDistance``, as modeling:153), and ``forward``'s dict feeds
``losses.step_losses`` unchanged.  Training refuses, with NotImplementedError
and before the input is looked at, a model whose parameters are not on a HIP
device or not fp32, and ``dropout`` / ``attention_dropout`` != 0.  The
``vq_type='vq'`` variant (VectorQuantize and its codebook updates) is not here.
"""
from __future__ import annotations

import ctypes as C
import itertools
from dataclasses import dataclass
from typing import Dict, Optional

import torch
from torch import nn

from . import _lib
from . import model_train as _train
from ._tracked import _TrackedParameter, _param_stamp   # noqa: F401  (optim imports the stamp from here)
from .dct_patches import DCTPatches
from .lfq import LFQ
from .losses import compute_entropy_loss
from .patchnorm import PatchNorm


def _f32(t: torch.Tensor) -> torch.Tensor:
    """fp32 contiguous view / copy of a parameter for a kernel's float* operand."""
    return t.detach().float().contiguous()

LIN_F32, LIN_BF16, LIN_BF16_QGELU, LIN_F32_RESIDUAL = 0, 1, 2, 3
LN_BWD_MAX_D = 2048   # dctae_model_layernorm_bwd's widest row (the forward LayerNorm takes 4096)


@dataclass
class CLIPEncoderConfig:
    """The CLIPVisionConfig fields the encoder reads (transformers 4.35.2 defaults)."""
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_attention_heads: int = 12
    num_hidden_layers: int = 12
    layer_norm_eps: float = 1e-5
    hidden_act: str = "quick_gelu"
    attention_dropout: float = 0.0
    dropout: float = 0.0

    @classmethod
    def from_any(cls, c):
        if isinstance(c, cls):
            return c
        if c is None:
            return cls()
        if not isinstance(c, dict):
            c = {k: getattr(c, k) for k in cls.__dataclass_fields__ if hasattr(c, k)}
        return cls(**{k: v for k, v in c.items() if k in cls.__dataclass_fields__})


class DCTAutoencoderConfig:
    """configuration_dct_autoencoder.py:5-41: same argument names and defaults;
    sub-configs may be dicts or CLIPVisionConfig-like objects, extra keys
    (e.g. ``transformers_version`` of a saved config.json) are kept as attributes."""

    def __init__(self, image_channels: int = 3, patch_size: int = 16, max_patch_h: int = 32, max_patch_w: int = 32,
                 vq_codebook_size: int = 4096, vq_num_codebooks: int = 8, vq_type: str = "lfq",
                 encoder_config=None, decoder_config=None, **kwargs):
        self.image_channels = image_channels
        self.patch_size = patch_size
        self.max_patch_h = max_patch_h
        self.max_patch_w = max_patch_w
        self.vq_codebook_size = vq_codebook_size
        self.vq_num_codebooks = vq_num_codebooks
        self.vq_type = vq_type
        self.encoder_config = CLIPEncoderConfig.from_any(encoder_config)
        self.decoder_config = CLIPEncoderConfig.from_any(decoder_config)
        for k, v in kwargs.items():
            setattr(self, k, v)


class _Attention(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (nn.Linear(d, d) for _ in range(4))


class _MLP(nn.Module):
    def __init__(self, d, i):
        super().__init__()
        self.fc1 = nn.Linear(d, i)
        self.fc2 = nn.Linear(i, d)


class _Layer(nn.Module):
    def __init__(self, c: CLIPEncoderConfig):
        super().__init__()
        self.self_attn = _Attention(c.hidden_size)
        self.layer_norm1 = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.mlp = _MLP(c.hidden_size, c.intermediate_size)
        self.layer_norm2 = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)


class CLIPEncoder(nn.Module):
    """Parameter container with transformers' CLIPEncoder names (layers.N.*)."""

    def __init__(self, c: CLIPEncoderConfig):
        super().__init__()
        if c.hidden_act != "quick_gelu":
            raise NotImplementedError(f"hidden_act={c.hidden_act!r}: the fused MLP epilogue is quick_gelu")
        if c.hidden_size % c.num_attention_heads or c.hidden_size // c.num_attention_heads != 64:
            raise NotImplementedError("head_dim must be 64 (the attention kernel's tile)")
        self.config = c
        self.layers = nn.ModuleList([_Layer(c) for _ in range(c.num_hidden_layers)])


def _pad64(k: int) -> int:
    return (k + 63) // 64 * 64


def _bf16_padded(w: torch.Tensor, kp: int) -> torch.Tensor:
    """(N, K) fp32 weight -> (N, kp) bf16 bit patterns, zero columns K .. kp."""
    out = torch.zeros(w.shape[0], kp, dtype=torch.bfloat16, device=w.device)
    out[:, :w.shape[1]] = w.detach().to(torch.bfloat16)
    return out.view(torch.int16)


_pack_generation = itertools.count(1)


def _packed_linears(model: "DCTAutoencoder"):
    """(name in _Packed, the nn.Linear modules stacked in that pack), as _Packed lays them out."""
    for side in ("encoder", "decoder"):
        for i, L in enumerate(getattr(model, side).layers):
            a = L.self_attn
            yield f"{side}.{i}.qkv", [a.q_proj, a.k_proj, a.v_proj]
            yield f"{side}.{i}.out", [a.out_proj]
            yield f"{side}.{i}.fc1", [L.mlp.fc1]
            yield f"{side}.{i}.fc2", [L.mlp.fc2]
    yield "embed", [model.to_patch_embedding[0]]
    if model.vq_model.has_projections:
        yield "proj_in", [model.vq_model.project_in]
        yield "proj_out_vq", [model.vq_model.project_out]
    yield "proj_out", [model.proj_out[1]]


class _Packed:
    """bf16 device copies of the linear weights, built once per parameter version."""

    def __init__(self, model: "DCTAutoencoder", training: Optional[bool] = None):
        self.w: Dict[str, torch.Tensor] = {}
        self.b: Dict[str, Optional[torch.Tensor]] = {}
        # training: (K, pad64(N)) transposed packs, the "weight" of dX = dY W on the same GEMM
        self.wt: Dict[str, torch.Tensor] = {}
        self.training = model.training if training is None else training
        # what a forward's Meta records and its backward checks: optim.FusedAdamW rewrites its
        # pack in place and moves it to a new generation (model_train.Meta.check)
        self.gen = next(_pack_generation)
        for side in ("encoder", "decoder"):
            for i, L in enumerate(getattr(model, side).layers):
                a = L.self_attn
                self._put(f"{side}.{i}.qkv", torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0),
                          torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], 0))
                self._put(f"{side}.{i}.out", a.out_proj.weight, a.out_proj.bias)
                self._put(f"{side}.{i}.fc1", L.mlp.fc1.weight, L.mlp.fc1.bias)
                self._put(f"{side}.{i}.fc2", L.mlp.fc2.weight, L.mlp.fc2.bias)
        self._put("embed", model.to_patch_embedding[0].weight, None)
        vq = model.vq_model
        if vq.has_projections:
            self._put("proj_in", vq.project_in.weight, vq.project_in.bias)
            self._put("proj_out_vq", vq.project_out.weight, vq.project_out.bias)
        self._put("proj_out", model.proj_out[1].weight, None)

    def _put(self, name, w, b):
        self.w[name] = _bf16_padded(w, _pad64(w.shape[1]))
        if self.training:
            self.wt[name] = _bf16_padded(w.t(), _pad64(w.shape[0]))
        self.b[name] = b.detach().float().contiguous() if b is not None else None


class SeqTable:
    """The sequences of a flat token stream of ``n_rows`` rows for the
    variable-length attention (include/dctae_model_prefix.h): sequence ``j`` is
    the rows ``[starts[j], starts[j] + lens[j])``.  Built from host lists and
    checked there, since the library call cannot read the device tables: a
    negative start or length, a sequence beyond ``n_rows``, two sequences that
    overlap, or ``max_len`` (default: the longest) below some length is a
    ValueError."""

    def __init__(self, starts, lens, n_rows: int, device, max_len: Optional[int] = None):
        starts, lens = [int(v) for v in starts], [int(v) for v in lens]
        if len(starts) != len(lens):
            raise ValueError(f"SeqTable: {len(starts)} starts for {len(lens)} lengths")
        if len(starts) > 65535:
            raise ValueError(f"SeqTable: at most 65535 sequences per call, got {len(starts)}")
        longest = max(lens, default=0)
        self.max_len = longest if max_len is None else int(max_len)
        if self.max_len < longest:
            raise ValueError(f"SeqTable: max_len = {self.max_len} is below the longest sequence ({longest})")
        end = 0
        for s, n in sorted(zip(starts, lens)):
            if s < 0 or n < 0 or s + n > n_rows:
                raise ValueError(f"SeqTable: sequence [{s}, {s + n}) outside the {n_rows} rows of the stream")
            if n and s < end:
                raise ValueError(f"SeqTable: the sequence at row {s} overlaps the one before it")
            end = max(end, s + n)
        self.n_seq, self.n_rows = len(starts), int(n_rows)
        self.start = torch.tensor(starts, dtype=torch.int64, device=device)
        self.len = torch.tensor(lens, dtype=torch.int32, device=device)


def attention_varlen(qkv: torch.Tensor, seqs: SeqTable, heads: int, out: torch.Tensor) -> torch.Tensor:
    """dctae_model_attention_varlen: full softmax attention inside each sequence
    of ``seqs`` on ``qkv`` (M, 3 * 64 * heads) bf16 bits (int16), into the rows
    of ``out`` (M, >= 64 * heads) bf16 bits that belong to a sequence; every
    other row of ``out`` is left as it is."""
    if qkv.dim() != 2 or qkv.shape[0] != seqs.n_rows or out.shape[0] != seqs.n_rows or qkv.shape[1] != 192 * heads:
        raise ValueError(f"attention_varlen: qkv {tuple(qkv.shape)} / out {tuple(out.shape)} for {seqs.n_rows} rows, "
                         f"{heads} heads")
    if qkv.device != seqs.start.device or out.device != qkv.device:
        raise RuntimeError("attention_varlen: qkv, out and the sequence table must be on one device")
    ctx = _lib.context(qkv.device)
    ctx.check(ctx.lib.dctae_model_attention_varlen(ctx.h, seqs.n_seq, seqs.max_len, heads, 64, _lib.ptr(qkv),
                                                   _lib.ptr(seqs.start), _lib.ptr(seqs.len), _lib.ptr(out),
                                                   out.stride(0), _lib.stream_ptr(qkv.device)), "self_attn_varlen")
    return out


class DCTAutoencoder(nn.Module):
    def __init__(self, config: DCTAutoencoderConfig):
        super().__init__()
        if not isinstance(config, DCTAutoencoderConfig):
            keys = ("image_channels", "patch_size", "max_patch_h", "max_patch_w", "vq_codebook_size",
                    "vq_num_codebooks", "vq_type", "encoder_config", "decoder_config")
            config = DCTAutoencoderConfig(**{k: getattr(config, k) for k in keys if hasattr(config, k)})
        self.config = config
        d = config.encoder_config.hidden_size
        if config.decoder_config.hidden_size != d:
            raise ValueError("encoder and decoder hidden_size differ")
        self.patchnorm = PatchNorm(max_patch_h=config.max_patch_h, max_patch_w=config.max_patch_w,
                                   patch_size=config.patch_size, channels=config.image_channels)
        pd = config.patch_size ** 2
        c_, h_, w_ = config.image_channels, config.max_patch_h, config.max_patch_w
        self.encoder_pos_embed_channel = nn.Parameter(torch.randn(c_, d))
        self.encoder_pos_embed_height = nn.Parameter(torch.randn(h_, d))
        self.encoder_pos_embed_width = nn.Parameter(torch.randn(w_, d))
        self.decoder_pos_embed_channel = nn.Parameter(torch.randn(c_, d))
        self.decoder_pos_embed_height = nn.Parameter(torch.randn(h_, d))
        self.decoder_pos_embed_width = nn.Parameter(torch.randn(w_, d))
        self.to_patch_embedding = nn.Sequential(nn.Linear(pd, d, bias=False), nn.LayerNorm(d, eps=1e-4))
        self.encoder = CLIPEncoder(config.encoder_config)
        if config.vq_type == "lfq":
            self.vq_model = LFQ(dim=d, num_codebooks=config.vq_num_codebooks, codebook_size=config.vq_codebook_size)
        elif config.vq_type == "vq":
            raise NotImplementedError("vq_type='vq' autoencoder: use the VectorQuantize module directly")
        else:
            raise ValueError(config.vq_type)
        self.decoder = CLIPEncoder(config.decoder_config)
        self.proj_out = nn.Sequential(nn.LayerNorm(d, eps=1e-4), nn.Linear(d, pd, bias=False))
        self._packed: Optional[_Packed] = None
        self._packed_key = None
        for _, linears in _packed_linears(self):
            for lin in linears:
                for q in lin.parameters(recurse=False):
                    q.__class__ = _TrackedParameter

    # ---- reference helpers (modeling:86-117) ----
    def get_pos_embedding_decoder(self, dct_patches: DCTPatches):
        return (self.decoder_pos_embed_height[dct_patches.h_indices]
                + self.decoder_pos_embed_width[dct_patches.w_indices]
                + self.decoder_pos_embed_channel[dct_patches.patch_channels])

    def add_pos_embedding_decoder_(self, dct_patches: DCTPatches):
        x = dct_patches.patches.float().contiguous().clone()
        self._pos_add(x, "decoder", dct_patches)
        dct_patches.patches = x
        return dct_patches

    def add_pos_embedding_encoder_(self, dct_patches: DCTPatches):
        x = dct_patches.patches.float().contiguous().clone()
        self._pos_add(x, "encoder", dct_patches)
        dct_patches.patches = x
        return dct_patches

    @torch.no_grad()
    def normalize_(self, x: DCTPatches):
        x.patches = self.patchnorm(x)
        return x

    def inv_normalize_(self, x: DCTPatches):
        x.patches = self.patchnorm.inverse_norm(x)
        return x

    def entropy_loss(self, distances, mask):
        """modeling:196-200.  distances: the fourth return value of the
        quantizer's training forward (an ``LFQDistance``: the fused HIP loss
        and gradient) or a dense tensor (evaluated in fp32 with torch ops)."""
        if torch.is_tensor(distances):
            og_dtype = distances.dtype
            return compute_entropy_loss(distances.float(), mask).to(og_dtype)
        return compute_entropy_loss(distances, mask)

    # ---- plumbing ----
    @staticmethod
    def _ctx(t):
        return _lib.context(t.device)

    def _param_key(self):
        return tuple(_param_stamp(p) for p in self.parameters())

    def _install_packed(self, pk: _Packed):
        """optim.FusedAdamW(model=self): the pack its kernel has just written is the current
        one for the parameters as they are now; any later change of a parameter
        (load_state_dict, an in-place op, a write through .data, another optimizer) rebuilds
        it with torch ops."""
        pk.gen = next(_pack_generation)
        self._packed = pk
        self._packed_key = self._param_key()

    def _weights(self) -> _Packed:
        key = self._param_key()
        if self._packed is None or self._packed_key != key or (self.training and not self._packed.training):
            self._packed = _Packed(self)
            self._packed_key = key
        return self._packed

    def _check_train(self):
        """Training-mode refusals, before the input is looked at."""
        for n, p in self.named_parameters():
            if p.device.type != "cuda":
                raise NotImplementedError(f"DCTAutoencoder training runs on HIP kernels: parameter {n} is on "
                                          f"{p.device} (move the model to the GPU, or call .eval())")
            if p.dtype != torch.float32:
                raise NotImplementedError(f"DCTAutoencoder training keeps fp32 master weights (bf16 operands are "
                                          f"packed from them): parameter {n} is {p.dtype}")
        for side in ("encoder_config", "decoder_config"):
            c = getattr(self.config, side)
            if c.dropout != 0 or c.attention_dropout != 0:
                raise NotImplementedError(f"{side}: dropout / attention_dropout != 0 has no kernel in training")
        d = self.config.encoder_config.hidden_size
        if d > LN_BWD_MAX_D:
            raise NotImplementedError(f"hidden_size={d}: the LayerNorm backward kernel takes rows of at most "
                                      f"{LN_BWD_MAX_D} (the forward, and so .eval(), takes 4096)")

    def _check_mode(self, dp: Optional[DCTPatches] = None):
        if self.training:
            self._check_train()
        if dp is not None:
            dev = dp.patches.device
            # kernels take raw device pointers: a parameter left on another device (or the
            # CPU) would be read as garbage, so refuse it like torch's device mismatch error
            for n, p in self.named_parameters():
                if p.device != dev:
                    raise RuntimeError(f"parameter {n} is on {p.device}, the input on {dev}: move the model with .to()")

    @staticmethod
    def _linear(ctx, x, w, bias, n, epi, out):
        m, kx = x.shape
        rows, kw = w.shape
        ctx.check(ctx.lib.dctae_model_linear(ctx.h, m, n, kw, _lib.ptr(x), kx, _lib.ptr(w), rows, kw, _lib.ptr(bias),
                                             epi, _lib.ptr(out), out.shape[1], _lib.stream_ptr(x.device)),
                  "model_linear")
        return out

    def _pos_tables(self, side):
        return [getattr(self, f"{side}_pos_embed_{k}").detach().float().contiguous()
                for k in ("height", "width", "channel")]

    @staticmethod
    def _ch_pos(dp: DCTPatches):
        return (dp.patch_channels.reshape(-1).long().contiguous(),
                dp.patch_positions.reshape(-1, 2).long().contiguous())

    def _pos_add(self, x, side, dp):
        ctx = self._ctx(x)
        d = x.shape[-1]
        ch, pos = self._ch_pos(dp)
        tabs = self._pos_tables(side)
        ctx.check(ctx.lib.dctae_model_pos_add(ctx.h, x.numel() // d, d, _lib.ptr(x), d, *[_lib.ptr(t) for t in tabs],
                                              _lib.ptr(ch), _lib.ptr(pos), _lib.stream_ptr(x.device)), "model_pos_add")

    @staticmethod
    def _layernorm(ctx, h, ln, out):
        m, d = h.shape
        g, b = _f32(ln.weight), _f32(ln.bias)   # fp32 copies when the model was cast (e.g. .half())
        ctx.check(ctx.lib.dctae_model_layernorm(ctx.h, m, d, _lib.ptr(h), d, _lib.ptr(g), _lib.ptr(b),
                                                C.c_float(ln.eps), _lib.ptr(out), out.shape[1],
                                                _lib.stream_ptr(h.device)), "layer_norm")
        return out

    def _clip(self, side: str, h: torch.Tensor, dp: DCTPatches, seqs: Optional[SeqTable] = None):
        """CLIPEncoder.forward (transformers 4.35.2 CLIPEncoderLayer) on the f32
        residual stream h (M, D), in place.  ``seqs``: attention inside the
        sequences of that table instead of the padded rows of ``dp``."""
        ctx = self._ctx(h)
        pk = self._weights()
        enc = getattr(self, side)
        c = enc.config
        r, s = dp.key_pad_mask.shape
        m, d = h.shape
        dev = h.device
        st = _lib.stream_ptr(dev)
        ids = dp.batched_image_ids.long().contiguous()
        kp = dp.key_pad_mask.to(torch.uint8).contiguous()
        a = torch.empty(m, d, dtype=torch.int16, device=dev)
        qkv = torch.empty(m, 3 * d, dtype=torch.int16, device=dev)
        o = torch.empty(m, d, dtype=torch.int16, device=dev)
        f = torch.zeros(m, _pad64(c.intermediate_size), dtype=torch.int16, device=dev)
        for i, L in enumerate(enc.layers):
            self._layernorm(ctx, h, L.layer_norm1, a)
            self._linear(ctx, a, pk.w[f"{side}.{i}.qkv"], pk.b[f"{side}.{i}.qkv"], 3 * d, LIN_BF16, qkv)
            if seqs is not None:
                attention_varlen(qkv, seqs, c.num_attention_heads, o)
            else:
                ctx.check(ctx.lib.dctae_model_attention(ctx.h, r, s, c.num_attention_heads, 64, _lib.ptr(qkv),
                                                        _lib.ptr(ids), _lib.ptr(kp), _lib.ptr(o), d, st), "self_attn")
            self._linear(ctx, o, pk.w[f"{side}.{i}.out"], pk.b[f"{side}.{i}.out"], d, LIN_F32_RESIDUAL, h)
            self._layernorm(ctx, h, L.layer_norm2, a)
            self._linear(ctx, a, pk.w[f"{side}.{i}.fc1"], pk.b[f"{side}.{i}.fc1"], c.intermediate_size,
                         LIN_BF16_QGELU, f)
            self._linear(ctx, f, pk.w[f"{side}.{i}.fc2"], pk.b[f"{side}.{i}.fc2"], d, LIN_F32_RESIDUAL, h)
        return h

    def _bf16(self, x: torch.Tensor, kp: int) -> torch.Tensor:
        ctx = self._ctx(x)
        m, k = x.shape
        out = torch.empty(m, kp, dtype=torch.int16, device=x.device)
        ctx.check(ctx.lib.dctae_model_to_bf16(ctx.h, m, k, _lib.ptr(x), x.stride(0), kp, _lib.ptr(out),
                                              _lib.stream_ptr(x.device)), "to_bf16")
        return out

    # ---- modeling:119-200 ----
    def encode(self, dct_patches: DCTPatches, do_normalize: bool = False):
        """modeling:119-147.  ``.eval()``: no_grad, LFQ codes only.  ``.train()``:
        under autograd, through the quantizer's training forward (straight-through
        output, codes, commit loss, ``LFQDistance``), as modeling:153."""
        if self.training:
            self._check_mode()
            return self._encode_train(dct_patches, do_normalize)
        return self._encode_eval(dct_patches, do_normalize)

    def _meta(self, dp: DCTPatches, side: str):
        tabs = [getattr(self, f"{side}_pos_embed_{k}") for k in ("height", "width", "channel")]
        return _train.Meta(self._weights(), dp, getattr(self.config, f"{side}_config").num_attention_heads, tabs), tabs

    def _encode_train(self, dct_patches: DCTPatches, do_normalize: bool):
        if do_normalize:
            dct_patches = self.normalize_(dct_patches)
        r, s, d = *dct_patches.key_pad_mask.shape, self.config.encoder_config.hidden_size
        h = self._encode_hidden(dct_patches)
        xq, codes, commit_loss, distances = self.vq_model(h.view(r, s, d), mask=~dct_patches.key_pad_mask)
        dct_patches.patches = xq
        return dct_patches, codes, commit_loss, distances

    def _encode_hidden(self, dct_patches: DCTPatches) -> torch.Tensor:
        """The encoder's hidden state (R * S, D) before the quantizer, under autograd."""
        self._check_mode(dct_patches)
        meta, tabs = self._meta(dct_patches, "encoder")
        x = dct_patches.patches
        r, s, pd = x.shape
        ln = self.to_patch_embedding[1]
        h = _train.EmbedFn.apply(x.reshape(r * s, pd).float().contiguous(), meta, ln.eps,
                                 self.to_patch_embedding[0].weight, ln.weight, ln.bias, *tabs)
        return _train.clip_stack(self.encoder, "encoder", h, meta)

    @torch.no_grad()
    def _encode_eval(self, dct_patches: DCTPatches, do_normalize: bool = False):
        self._check_mode(dct_patches)
        if do_normalize:
            dct_patches = self.normalize_(dct_patches)
        pk = self._weights()
        x = dct_patches.patches
        r, s, pd = x.shape
        d = self.config.encoder_config.hidden_size
        dev = x.device
        ctx = self._ctx(x)
        xb = self._bf16(x.reshape(r * s, pd).float().contiguous(), pk.w["embed"].shape[1])
        e = self._linear(ctx, xb, pk.w["embed"], None, d, LIN_F32, torch.empty(r * s, d, device=dev))
        h = torch.empty(r * s, d, device=dev)
        ln = self.to_patch_embedding[1]
        ch, pos = self._ch_pos(dct_patches)
        tabs = self._pos_tables("encoder")
        g, b = _f32(ln.weight), _f32(ln.bias)
        ctx.check(ctx.lib.dctae_model_embed_norm(ctx.h, r * s, d, _lib.ptr(e), d, _lib.ptr(g),
                                                 _lib.ptr(b), C.c_float(ln.eps), *[_lib.ptr(t) for t in tabs],
                                                 _lib.ptr(ch), _lib.ptr(pos), _lib.ptr(h), d, _lib.stream_ptr(dev)),
                  "to_patch_embedding")
        self._clip("encoder", h, dct_patches)
        xq, codes = self._lfq(h)
        dct_patches.patches = xq.view(r, s, d)
        zero = torch.zeros((), device=dev)
        return dct_patches, codes.view(r, s, -1), zero, zero

    def _lfq(self, h: torch.Tensor):
        """LFQ.forward eval (lfq.py:136-227) on (M, D) f32 features."""
        vq = self.vq_model
        pk = self._weights()
        ctx = self._ctx(h)
        m, d = h.shape
        dev = h.device
        st = _lib.stream_ptr(dev)
        ncb, cbd = vq.num_codebooks, vq.codebook_dim
        codes = torch.empty(m, ncb, dtype=torch.long, device=dev)
        if vq.has_projections:
            hb = self._bf16(h, pk.w["proj_in"].shape[1])
            p = self._linear(ctx, hb, pk.w["proj_in"], pk.b["proj_in"], ncb * cbd, LIN_F32,
                             torch.empty(m, ncb * cbd, device=dev))
            kq = pk.w["proj_out_vq"].shape[1]
            q = torch.empty(m, kq, dtype=torch.int16, device=dev)
            ctx.check(ctx.lib.dctae_model_lfq(ctx.h, m, ncb, cbd, C.c_float(vq.codebook_scale), _lib.ptr(p),
                                              ncb * cbd, _lib.ptr(codes), _lib.ptr(q), None, kq, st), "lfq")
            xq = self._linear(ctx, q, pk.w["proj_out_vq"], pk.b["proj_out_vq"], d, LIN_F32,
                              torch.empty(m, d, device=dev))
        else:
            xq = torch.empty(m, d, device=dev)
            ctx.check(ctx.lib.dctae_model_lfq(ctx.h, m, ncb, cbd, C.c_float(vq.codebook_scale), _lib.ptr(h), d,
                                              _lib.ptr(codes), None, _lib.ptr(xq), d, st), "lfq")
        return xq, codes

    def decode_from_codes(self, codes: torch.LongTensor, do_inv_norm: bool = False, **dct_patches_kwargs) -> DCTPatches:
        """modeling:149-158: LFQ.indices_to_codes (HIP kernel) + project_out (bf16
        MFMA linear; in ``.train()`` the quantizer's differentiable project_out)."""
        if self.training:
            self._check_mode()
            vq = self.vq_model
            q = vq._project_out_train(vq.indices_to_codes(codes, project_out=False).float())
            return self.decode(DCTPatches(patches=q, **dct_patches_kwargs), do_inv_norm=do_inv_norm)
        return self._decode_from_codes_eval(codes, do_inv_norm, **dct_patches_kwargs)

    @torch.no_grad()
    def _decode_from_codes_eval(self, codes, do_inv_norm=False, _seqs=None, **dct_patches_kwargs) -> DCTPatches:
        vq = self.vq_model
        q = vq.indices_to_codes(codes, project_out=False)
        if vq.has_projections:
            pk = self._weights()
            lead = q.shape[:-1]
            qm = q.reshape(-1, q.shape[-1]).float().contiguous()
            ctx = self._ctx(qm)
            qb = self._bf16(qm, pk.w["proj_out_vq"].shape[1])
            q = self._linear(ctx, qb, pk.w["proj_out_vq"], pk.b["proj_out_vq"], vq.dim, LIN_F32,
                             torch.empty(qm.shape[0], vq.dim, device=qm.device)).view(*lead, vq.dim)
        x = DCTPatches(patches=q, **dct_patches_kwargs)
        if _seqs is not None:
            return self._decode_eval(x, do_inv_norm, _seqs)
        return self.decode(x, do_inv_norm=do_inv_norm)

    def decode_prefixes(self, dct_patches: DCTPatches, codes: torch.Tensor, prefixes, do_inv_norm: bool = True):
        """The model prefix frames of a packed batch (progressive.py's module
        docstring) through the decoder in one pass per chunk: frame
        ``(i, k)`` is ``decode_from_codes`` of the first ``min(k, n_i)`` real
        tokens of image ``i`` as a one-row batch without padding, bit for bit.
        ``.eval()`` only, under ``no_grad``.  ``prefixes``: ints for every image,
        or one sequence per image.  ``codes``: int64 or int16.

        Returns ``(frames, which)``: ``frames`` a DCTPatches in the ordinary
        packed format whose images are, in order, the frames with
        ``min(k, n_i) >= 1`` (one row per chunk of at most
        ``progressive.PREFIX_TOKENS_PER_CALL`` tokens, a frame's id its number
        in the row, rows padded at the end to the longest; None without such a
        frame), ``which`` their ``(image, k)``.  Frames with
        ``min(k, n_i) == 0`` decode nothing through the model and are left out
        (``progressive.model_decode_prefixes`` builds them).  Reading
        ``batched_image_ids`` / ``key_pad_mask`` on the host is the call's one
        host synchronisation."""
        dp, which, _, _ = self._decode_prefixes(dct_patches, codes, prefixes, do_inv_norm)
        return dp, which

    @torch.no_grad()
    def _decode_prefixes(self, dct_patches: DCTPatches, codes: torch.Tensor, prefixes, do_inv_norm: bool = True):
        from . import _ops, progressive
        if self.training:
            raise NotImplementedError("decode_prefixes runs in .eval() only (no gradients through frames)")
        vq = self.vq_model
        if not isinstance(codes, torch.Tensor):
            raise TypeError(f"decode_prefixes codes: a tensor expected, got {type(codes)}")
        _ops.codes_dtype_suffix(codes.dtype, "decode_prefixes codes")
        if codes.dtype == torch.int16:
            _ops.check_codes16(vq.cfg(), "decode_prefixes")
        progressive._split_prefixes(prefixes)   # a negative prefix is refused before anything is read
        ids, kp = dct_patches.batched_image_ids, dct_patches.key_pad_mask
        dev = codes.device
        for n, p in self.named_parameters():
            if p.device != dev:
                raise RuntimeError(f"parameter {n} is on {p.device}, the codes on {dev}: move the model with .to()")
        for name, v in (("batched_image_ids", ids), ("key_pad_mask", kp), ("patch_channels", dct_patches.patch_channels),
                        ("patch_positions", dct_patches.patch_positions)):
            if v.device != dev:
                raise RuntimeError(f"{name} is on {v.device}, the codes on {dev}")
        r, s = kp.shape
        if codes.dim() != 3 or tuple(codes.shape[:2]) != (r, s) or codes.shape[2] != vq.num_codebooks:
            raise ValueError(f"decode_prefixes codes: ({r}, {s}, {vq.num_codebooks}) expected, got {tuple(codes.shape)}")
        plan = progressive.model_frames(ids.cpu(), kp.cpu(), prefixes)   # the one host read
        live = [f for f in range(len(plan.m)) if plan.m[f] > 0]
        which = [(plan.img[f], plan.k[f]) for f in live]
        if not live:
            return None, which, plan, []
        ctx = self._ctx(codes)
        st = _lib.stream_ptr(dev)
        ncb = vq.num_codebooks
        ids_d, kp_d = ids.long().contiguous(), kp.to(torch.uint8).contiguous()
        ch_d, pos_d = self._ch_pos(dct_patches)
        cc = codes.contiguous()
        ctype = _lib.CODES_I16 if cc.dtype == torch.int16 else _lib.CODES_I64
        ms = [plan.m[f] for f in live]
        chunks = progressive.model_frame_chunks(ms, progressive.PREFIX_TOKENS_PER_CALL)
        width = max(sum(ms[b:e]) for b, e in chunks)
        pd = self.proj_out[1].weight.shape[0]
        out = DCTPatches(patches=torch.zeros(len(chunks), width, pd, device=dev),
                         key_pad_mask=torch.ones(len(chunks), width, dtype=torch.bool, device=dev),
                         batched_image_ids=torch.zeros(len(chunks), width, dtype=torch.long, device=dev),
                         patch_channels=torch.zeros(len(chunks), width, dtype=torch.long, device=dev),
                         patch_positions=torch.zeros(len(chunks), width, 2, dtype=torch.long, device=dev),
                         patch_sizes=[dct_patches.patch_sizes[plan.img[f]] for f in live],
                         original_sizes=[dct_patches.original_sizes[plan.img[f]] for f in live])
        layout = []   # (row, first slot, tokens) of every frame in the frames batch
        for c, (b, e) in enumerate(chunks):
            lens = ms[b:e]
            starts = [sum(lens[:j]) for j in range(len(lens))]
            layout += [(c, s0, n) for s0, n in zip(starts, lens)]
            m = sum(lens)
            fr = [live[j] for j in range(b, e)]
            g_codes = torch.empty(m, ncb, dtype=torch.long, device=dev)
            g_ch = torch.empty(m, dtype=torch.long, device=dev)
            g_pos = torch.empty(m, 2, dtype=torch.long, device=dev)
            keep = (_lib.i32([plan.row[f] for f in fr]), _lib.i64([plan.lid[f] for f in fr]), _lib.i32(lens),
                    _lib.i64(starts))
            ctx.check(ctx.lib.dctae_prefix_tokens(
                ctx.h, r, s, _lib.ptr(ids_d), _lib.ptr(kp_d), _lib.ptr(pos_d), _lib.ptr(ch_d), _lib.ptr(cc), ctype, ncb,
                len(fr), C.cast(keep[0], C.POINTER(C.c_int32)), C.cast(keep[1], C.POINTER(C.c_int64)),
                C.cast(keep[2], C.POINTER(C.c_int32)), C.cast(keep[3], C.POINTER(C.c_int64)), _lib.ptr(g_codes),
                _lib.ptr(g_ch), _lib.ptr(g_pos), st), "dctae_prefix_tokens")
            seqs = SeqTable(starts, lens, m, dev)
            fid = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens)).to(dev).view(1, m)
            x = self._decode_from_codes_eval(
                g_codes.view(1, m, ncb), do_inv_norm, _seqs=seqs, key_pad_mask=torch.zeros(1, m, dtype=torch.bool, device=dev),
                batched_image_ids=fid, patch_channels=g_ch.view(1, m), patch_positions=g_pos.view(1, m, 2),
                patch_sizes=out.patch_sizes[b:e], original_sizes=out.original_sizes[b:e])
            out.patches[c, :m] = x.patches[0]
            out.key_pad_mask[c, :m] = False
            out.batched_image_ids[c, :m] = fid[0]
            out.patch_channels[c, :m] = g_ch
            out.patch_positions[c, :m] = g_pos
        return out, which, plan, layout

    def decode(self, x: DCTPatches, do_inv_norm: bool = False) -> DCTPatches:
        if self.training:
            self._check_mode()
            return self._decode_train(x, do_inv_norm)
        return self._decode_eval(x, do_inv_norm)

    def _decode_train(self, x: DCTPatches, do_inv_norm: bool) -> DCTPatches:
        self._check_mode(x)
        meta, tabs = self._meta(x, "decoder")
        r, s, d = x.patches.shape
        h = _train.PosAddFn.apply(x.patches.reshape(r * s, d).float().contiguous(), meta, *tabs)
        h = _train.clip_stack(self.decoder, "decoder", h, meta)
        ln, lin = self.proj_out
        y = _train.ProjOutFn.apply(h, meta, ln.eps, ln.weight, ln.bias, lin.weight)
        x.patches = y.view(r, s, -1)
        if do_inv_norm:
            x = self.inv_normalize_(x)
        return x

    @torch.no_grad()
    def _decode_eval(self, x: DCTPatches, do_inv_norm: bool = False, seqs: Optional[SeqTable] = None) -> DCTPatches:
        self._check_mode(x)
        pk = self._weights()
        r, s, d = x.patches.shape
        dev = x.patches.device
        ctx = self._ctx(x.patches)
        x = self.add_pos_embedding_decoder_(x)
        h = x.patches.view(r * s, d)
        self._clip("decoder", h, x, seqs)
        a = self._layernorm(ctx, h, self.proj_out[0], torch.empty(r * s, d, dtype=torch.int16, device=dev))
        pd = self.proj_out[1].weight.shape[0]
        y = self._linear(ctx, a, pk.w["proj_out"], None, pd, LIN_F32, torch.empty(r * s, pd, device=dev))
        x.patches = y.view(r, s, pd)
        if do_inv_norm:
            x = self.inv_normalize_(x)
        return x

    def forward(self, dct_patches: DCTPatches, do_normalize: bool = False):
        """modeling:160-194; the dict feeds ``losses.step_losses`` unchanged."""
        dct_patches, codes, commit_loss, distances = self.encode(dct_patches, do_normalize=do_normalize)
        dct_patches = self.decode(dct_patches)
        return dict(dct_patches=dct_patches, commit_loss=commit_loss, codes=codes, distances=distances)
