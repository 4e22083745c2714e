"""DCTAutoencoder training step on libdctae's HIP kernels: the
operator wrappers of the backward (dctae_model_*: attention with its
log-sum-exp, attention backward, the dX / dW / db of a linear layer on the
forward's bf16 MFMA GEMM, LayerNorm / quick_gelu backward, position-table
gradients) and the ``torch.autograd.Function``s ``model.DCTAutoencoder`` runs
in ``.train()``: one per CLIP layer, one each for the patch embedding, the
decoder position add and ``proj_out``.

Master weights and the residual stream (forward and gradient) are fp32; GEMM
and attention operands are bf16; ``dW`` / ``db`` / LayerNorm and position-table
gradients are fp32.  No kernel uses floating-point atomics, so a step repeats
bit for bit.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

LIN_F32, LIN_BF16, LIN_BF16_QGELU, LIN_F32_RESIDUAL = 0, 1, 2, 3
LN_RPW = 8   # rows per wave of the LayerNorm backward (dctae_model.h)


def pad64(k: int) -> int:
    return (k + 63) // 64 * 64


def _c(t):
    return _lib.context(t.device)


def _st(t):
    return _lib.stream_ptr(t.device)


def _i16(*shape, dev, zero=False):
    return (torch.zeros if zero else torch.empty)(*shape, dtype=torch.int16, device=dev)


# ---- operators (2-D tensors; bf16 tensors are int16 bit patterns) ----
def linear(x, w, bias, n, epi, out):
    """out (M, >= n) = x (M, K) w (rows >= n, K)^T (+ bias), K % 64 == 0."""
    ctx = _c(x)
    ctx.check(ctx.lib.dctae_model_linear(ctx.h, x.shape[0], n, w.shape[1], _lib.ptr(x), x.stride(0), _lib.ptr(w),
                                         w.shape[0], w.stride(0), _lib.ptr(bias), epi, _lib.ptr(out), out.stride(0),
                                         _st(x)), "model_linear")
    return out


def to_bf16(x, kp):
    ctx = _c(x)
    m, k = x.shape
    out = _i16(m, kp, dev=x.device)
    ctx.check(ctx.lib.dctae_model_to_bf16(ctx.h, m, k, _lib.ptr(x), x.stride(0), kp, _lib.ptr(out), _st(x)), "to_bf16")
    return out


def transpose_pack(x, c):
    """bf16 (M, >= c) -> (c, pad64(M)), zero tail."""
    ctx = _c(x)
    m = x.shape[0]
    mp = pad64(m)
    out = _i16(c, mp, dev=x.device)
    ctx.check(ctx.lib.dctae_model_transpose_pack(ctx.h, m, c, _lib.ptr(x), x.stride(0), mp, _lib.ptr(out), _st(x)),
              "transpose_pack")
    return out


def colsum(x, n):
    """fp32 (n,) column sums of x (M, >= n), fp32 or bf16 bits, in a fixed order."""
    ctx = _c(x)
    m = x.shape[0]
    ws = torch.empty((m + 63) // 64, n, device=x.device) if m > 256 else None
    out = torch.empty(n, device=x.device)
    ctx.check(ctx.lib.dctae_model_colsum(ctx.h, m, n, _lib.ptr(x), x.stride(0), int(x.dtype == torch.int16),
                                         _lib.ptr(ws), _lib.ptr(out), _st(x)), "colsum")
    return out


def linear_dx(dy_b, wt, k, epi, out, bias=None):
    """dX (M, k) = dY W on the forward's GEMM: dy_b (M, pad64(N)) bf16 with zero
    padding, wt (k, pad64(N)) the transposed pack of W."""
    return linear(dy_b, wt, bias, k, epi, out)


def linear_dw(dy_b, n, x_b, k):
    """dW (n, k) fp32 = dY^T X: both operands transposed into (rows, pad64(M))
    packs, so the sum over the M tokens is the GEMM's K dimension (zero tail)."""
    dyt = transpose_pack(dy_b, n)
    xt = transpose_pack(x_b, k)
    return linear(dyt, xt, None, k, LIN_F32, torch.empty(n, k, device=dy_b.device))


def layernorm(h, g, b, eps, out):
    ctx = _c(h)
    m, d = h.shape
    ctx.check(ctx.lib.dctae_model_layernorm(ctx.h, m, d, _lib.ptr(h), h.stride(0), _lib.ptr(g), _lib.ptr(b),
                                            C.c_float(eps), _lib.ptr(out), out.stride(0), _st(h)), "layer_norm")
    return out


def layernorm_bwd(x, g, eps, dy, dx, accumulate):
    """dx (+)= LayerNorm backward of (x, gamma, dy); returns (dgamma, dbeta)."""
    ctx = _c(x)
    m, d = x.shape
    parts = torch.empty(2, (m + LN_RPW - 1) // LN_RPW, d, device=x.device)
    ctx.check(ctx.lib.dctae_model_layernorm_bwd(ctx.h, m, d, _lib.ptr(x), x.stride(0), _lib.ptr(g), C.c_float(eps),
                                                _lib.ptr(dy), dy.stride(0), _lib.ptr(dx), dx.stride(0),
                                                int(bool(accumulate)), _lib.ptr(parts[0]), _lib.ptr(parts[1]),
                                                _st(x)), "layer_norm_bwd")
    return colsum(parts[0], d), colsum(parts[1], d)


def qgelu(pre, n, out):
    ctx = _c(pre)
    ctx.check(ctx.lib.dctae_model_qgelu(ctx.h, pre.shape[0], n, _lib.ptr(pre), pre.stride(0), _lib.ptr(out),
                                        out.stride(0), _st(pre)), "qgelu")
    return out


def qgelu_bwd(df, pre, n, out):
    ctx = _c(pre)
    ctx.check(ctx.lib.dctae_model_qgelu_bwd(ctx.h, pre.shape[0], n, _lib.ptr(df), df.stride(0), _lib.ptr(pre),
                                            pre.stride(0), _lib.ptr(out), out.stride(0), _st(pre)), "qgelu_bwd")
    return out


def attention_lse(qkv, ids, kp, r, s, heads):
    """(out (R*S, D) bf16, lse (R, heads, S) fp32 in log2 units)."""
    ctx = _c(qkv)
    d = 64 * heads
    out = _i16(r * s, d, dev=qkv.device)
    lse = torch.empty(r, heads, s, device=qkv.device)
    ctx.check(ctx.lib.dctae_model_attention_lse(ctx.h, r, s, heads, 64, _lib.ptr(qkv), _lib.ptr(ids), _lib.ptr(kp),
                                                _lib.ptr(out), d, _lib.ptr(lse), _st(qkv)), "self_attn")
    return out, lse


def attention_bwd(qkv, ids, kp, out, d_out, lse, r, s, heads):
    """dqkv (R*S, 3 D) bf16 laid out like qkv."""
    ctx = _c(qkv)
    dqkv = _i16(r * s, 3 * 64 * heads, dev=qkv.device)
    delta = torch.empty(r, heads, s, device=qkv.device)
    ctx.check(ctx.lib.dctae_model_attention_bwd(ctx.h, r, s, heads, 64, _lib.ptr(qkv), _lib.ptr(ids), _lib.ptr(kp),
                                                _lib.ptr(out), out.stride(0), _lib.ptr(d_out), d_out.stride(0),
                                                _lib.ptr(lse), _lib.ptr(delta), _lib.ptr(dqkv), _st(qkv)),
              "self_attn_bwd")
    return dqkv


def pos_grad(g, idx, rows):
    """(rows, D) fp32: row r = sum of g[m] over tokens with idx[m] == r, in token
    order.  idx: int64 (M,), possibly a strided view."""
    ctx = _c(g)
    m, d = g.shape
    out = torch.empty(rows, d, device=g.device)
    ctx.check(ctx.lib.dctae_model_pos_grad(ctx.h, m, d, _lib.ptr(g), g.stride(0), _lib.ptr(idx), idx.stride(0), rows,
                                           _lib.ptr(out), _st(g)), "pos_grad")
    return out


def _pos_grads(dh, meta):
    ch, pos = meta.ch, meta.pos
    return (pos_grad(dh, pos[:, 0], meta.rows_h), pos_grad(dh, pos[:, 1], meta.rows_w),
            pos_grad(dh, ch, meta.rows_c))


class Meta:
    """What the Functions of one encode / decode call share: the packed weights
    of this parameter version and the batch's index tensors."""

    def __init__(self, pk, dp, heads, tabs):
        self.pk = pk
        self.gen = pk.gen
        self.r, self.s = dp.key_pad_mask.shape
        self.heads = heads
        self.ids = dp.batched_image_ids.long().contiguous()
        self.kp = dp.key_pad_mask.to(torch.uint8).contiguous()
        self.ch = dp.patch_channels.reshape(-1).long().contiguous()
        self.pos = dp.patch_positions.reshape(-1, 2).long().contiguous()
        self.rows_h, self.rows_w, self.rows_c = (t.shape[0] for t in tabs)

    def check(self):
        """Every backward reads pk.wt: refuse a pack that an optimizer step has rewritten in
        place since the forward (for torch-op packs autograd's version check does the same)."""
        if self.pk.gen != self.gen:
            raise RuntimeError("backward through a stale graph: the optimizer step rewrote the packed bf16 weights "
                               "this forward used (run the forward again after optimizer.step())")


# ---- autograd ----
class LayerFn(torch.autograd.Function):
    """One CLIPEncoderLayer (transformers 4.35.2) on the fp32 residual stream."""

    @staticmethod
    def forward(ctx, h, meta, name, eps, ln1w, ln1b, qw, qb, kw, kb, vw, vb, ow, ob, ln2w, ln2b, f1w, f1b, f2w, f2b):
        pk = meta.pk
        m, d = h.shape
        dev = h.device
        inter = f1w.shape[0]
        a1 = layernorm(h, ln1w, ln1b, eps, _i16(m, d, dev=dev))
        qkv = linear(a1, pk.w[name + ".qkv"], pk.b[name + ".qkv"], 3 * d, LIN_BF16, _i16(m, 3 * d, dev=dev))
        o, lse = attention_lse(qkv, meta.ids, meta.kp, meta.r, meta.s, meta.heads)
        hm = linear(o, pk.w[name + ".out"], pk.b[name + ".out"], d, LIN_F32_RESIDUAL, h.clone())
        a2 = layernorm(hm, ln2w, ln2b, eps, _i16(m, d, dev=dev))
        # fc1 keeps its bf16 pre-activation for quick_gelu's derivative
        pre = linear(a2, pk.w[name + ".fc1"], pk.b[name + ".fc1"], inter, LIN_BF16, _i16(m, pad64(inter), dev=dev, zero=True))
        f = qgelu(pre, inter, _i16(m, pad64(inter), dev=dev, zero=True))
        out = linear(f, pk.w[name + ".fc2"], pk.b[name + ".fc2"], d, LIN_F32_RESIDUAL, hm.clone())
        ctx.save_for_backward(h, a1, qkv, o, lse, hm, a2, pre, f, ln1w, ln2w)
        ctx.meta, ctx.name, ctx.eps, ctx.inter = meta, name, eps, inter
        return out

    @staticmethod
    def backward(ctx, dout):
        ctx.meta.check()
        h, a1, qkv, o, lse, hm, a2, pre, f, ln1w, ln2w = ctx.saved_tensors
        meta, name, eps, inter = ctx.meta, ctx.name, ctx.eps, ctx.inter
        pk = meta.pk
        m, d = h.shape
        dev = h.device
        dh = dout.float().contiguous().clone()   # the fp32 gradient stream, updated in place below
        # mlp
        dhb = to_bf16(dh, d)
        df2w = linear_dw(dhb, d, f, inter)
        df2b = colsum(dh, d)
        df = linear_dx(dhb, pk.wt[name + ".fc2"], inter, LIN_BF16, _i16(m, pad64(inter), dev=dev, zero=True))
        dpre = qgelu_bwd(df, pre, inter, df)
        df1w = linear_dw(dpre, inter, a2, d)
        df1b = colsum(dpre, inter)
        da = linear_dx(dpre, pk.wt[name + ".fc1"], d, LIN_F32, torch.empty(m, d, device=dev))
        dln2w, dln2b = layernorm_bwd(hm, ln2w, eps, da, dh, True)
        # attention
        dhb = to_bf16(dh, d)
        dow = linear_dw(dhb, d, o, d)
        dob = colsum(dh, d)
        do = linear_dx(dhb, pk.wt[name + ".out"], d, LIN_BF16, _i16(m, d, dev=dev))
        dqkv = attention_bwd(qkv, meta.ids, meta.kp, o, do, lse, meta.r, meta.s, meta.heads)
        dqkvw = linear_dw(dqkv, 3 * d, a1, d)
        dqkvb = colsum(dqkv, 3 * d)
        da = linear_dx(dqkv, pk.wt[name + ".qkv"], d, LIN_F32, da)
        dln1w, dln1b = layernorm_bwd(h, ln1w, eps, da, dh, True)
        dqw, dkw, dvw = dqkvw[:d], dqkvw[d:2 * d], dqkvw[2 * d:]
        dqb, dkb, dvb = dqkvb[:d], dqkvb[d:2 * d], dqkvb[2 * d:]
        return (dh, None, None, None, dln1w, dln1b, dqw, dqb, dkw, dkb, dvw, dvb, dow, dob, dln2w, dln2b,
                df1w, df1b, df2w, df2b)


class EmbedFn(torch.autograd.Function):
    """to_patch_embedding (Linear without bias, LayerNorm) + encoder position terms."""

    @staticmethod
    def forward(ctx, x, meta, eps, w, lnw, lnb, ph, pw, pc):
        pk = meta.pk
        m = x.shape[0]
        d = w.shape[0]
        c = _c(x)
        xb = to_bf16(x, pk.w["embed"].shape[1])
        e = linear(xb, pk.w["embed"], None, d, LIN_F32, torch.empty(m, d, device=x.device))
        h = torch.empty(m, d, device=x.device)
        c.check(c.lib.dctae_model_embed_norm(c.h, m, d, _lib.ptr(e), d, _lib.ptr(lnw), _lib.ptr(lnb), C.c_float(eps),
                                             _lib.ptr(ph), _lib.ptr(pw), _lib.ptr(pc), _lib.ptr(meta.ch),
                                             _lib.ptr(meta.pos), _lib.ptr(h), d, _st(x)), "to_patch_embedding")
        ctx.save_for_backward(xb, e, lnw)
        ctx.meta, ctx.eps, ctx.pd = meta, eps, x.shape[1]
        return h

    @staticmethod
    def backward(ctx, dh):
        ctx.meta.check()
        xb, e, lnw = ctx.saved_tensors
        meta, pd = ctx.meta, ctx.pd
        m, d = e.shape
        dh = dh.float().contiguous()
        dph, dpw, dpc = _pos_grads(dh, meta)
        de = torch.empty_like(e)
        dlnw, dlnb = layernorm_bwd(e, lnw, ctx.eps, dh, de, False)
        deb = to_bf16(de, d)
        dw = linear_dw(deb, d, xb, pd)
        dx = linear_dx(deb, meta.pk.wt["embed"], pd, LIN_F32, torch.empty(m, pd, device=e.device))
        return dx, None, None, dw, dlnw, dlnb, dph, dpw, dpc


class PosAddFn(torch.autograd.Function):
    """x + decoder position terms (modeling:88-93)."""

    @staticmethod
    def forward(ctx, x, meta, ph, pw, pc):
        c = _c(x)
        m, d = x.shape
        y = x.clone()
        c.check(c.lib.dctae_model_pos_add(c.h, m, d, _lib.ptr(y), d, _lib.ptr(ph), _lib.ptr(pw), _lib.ptr(pc),
                                          _lib.ptr(meta.ch), _lib.ptr(meta.pos), _st(x)), "model_pos_add")
        ctx.meta = meta
        return y

    @staticmethod
    def backward(ctx, dy):
        ctx.meta.check()
        dy = dy.float().contiguous()
        return (dy, None) + _pos_grads(dy, ctx.meta)


class ProjOutFn(torch.autograd.Function):
    """proj_out: LayerNorm, Linear without bias (modeling:76)."""

    @staticmethod
    def forward(ctx, h, meta, eps, lnw, lnb, w):
        m, d = h.shape
        pd = w.shape[0]
        a = layernorm(h, lnw, lnb, eps, _i16(m, d, dev=h.device))
        y = linear(a, meta.pk.w["proj_out"], None, pd, LIN_F32, torch.empty(m, pd, device=h.device))
        ctx.save_for_backward(h, a, lnw)
        ctx.meta, ctx.eps, ctx.pd = meta, eps, pd
        return y

    @staticmethod
    def backward(ctx, dy):
        ctx.meta.check()
        h, a, lnw = ctx.saved_tensors
        meta, pd = ctx.meta, ctx.pd
        m, d = h.shape
        dyb = to_bf16(dy.float().contiguous(), pad64(pd))
        dw = linear_dw(dyb, pd, a, d)
        da = linear_dx(dyb, meta.pk.wt["proj_out"], d, LIN_F32, torch.empty(m, d, device=h.device))
        dh = torch.empty_like(h)
        dlnw, dlnb = layernorm_bwd(h, lnw, ctx.eps, da, dh, False)
        return dh, None, None, dlnw, dlnb, dw


def clip_stack(enc, side, h, meta):
    """CLIPEncoder.forward under autograd: one LayerFn per layer."""
    for i, L in enumerate(enc.layers):
        a, p = L.self_attn, L.mlp
        h = LayerFn.apply(h, meta, f"{side}.{i}", L.layer_norm1.eps, L.layer_norm1.weight, L.layer_norm1.bias,
                          a.q_proj.weight, a.q_proj.bias, a.k_proj.weight, a.k_proj.bias, a.v_proj.weight,
                          a.v_proj.bias, a.out_proj.weight, a.out_proj.bias, L.layer_norm2.weight,
                          L.layer_norm2.bias, p.fc1.weight, p.fc1.bias, p.fc2.weight, p.fc2.bias)
    return h
