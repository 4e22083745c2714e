"""TEST INFRASTRUCTURE ONLY — the attention edge cases of
tests/test_gpu_model_edges.py and tests/test_model_edges_host.py: their input
builders, the float64 reference with the bf16-autocast yardstick, and a torch
emulation of the arithmetic the HIP kernels are meant to perform
(dctae_model.hip k_attention, dctae_model_bwd.hip k_attn_bwd_*).

Inputs: q, k, v and d_out are randn rounded to bf16; then, per head,
coordinate 0 of every query is 8 and coordinate 0 of key j (its position in
the row) is a ramp r(j) rounded to bf16, which adds r(j) to the logit
(8 r(j) / sqrt(64)).  One 64-key block of the forward spans 64 positions:

  plain  no ramp
  fast   j / 8     11.5 log2 units per block: the running maximum moves at every block
  slow   j / 32    2.9 per block: it moves about every third block, p reaches 2^8 in between
  down   -j / 8    the maximum is in block 0, later p underflow
  saw    2 ((j // 64) % 2) + j / 64

Masks (the +1 bias of the reference hits a pad key of the query's image):
  nopad    three images per row, no pad
  allpad   row 0 entirely pad, the other rows pad from S / 2
  scatter  ids uniform in 0..3, every key pad with probability 0.3, anywhere
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import torch

from oracle import ref_model as R

KINDS = ("plain", "fast", "slow", "down", "saw")
MASKS = ("nopad", "allpad", "scatter")
SHAPES = ((2, 1, 1), (2, 31, 1), (2, 65, 2), (2, 129, 1), (2, 200, 3), (2, 257, 2), (2, 321, 2))
LOG2E = 1.4426950408889634
BLOCK = 64        # keys per block of the forward
LAZY = 8.0        # the running maximum moves when a block's maximum exceeds it by more than this (log2 units)


def bf(x):
    return x.to(torch.bfloat16).float()


def ramp(kind, s):
    j = torch.arange(s, dtype=torch.float32)
    if kind == "fast":
        return j / 8
    if kind == "slow":
        return j / 32
    if kind == "down":
        return -j / 8
    if kind == "saw":
        return 2.0 * ((j // 64) % 2) + j / 64
    assert kind == "plain"
    return None


def mask(name, r, s, g):
    """(ids int64 (r, s), key_pad bool (r, s))."""
    thirds = (torch.arange(s) * 3) // s
    if name == "nopad":
        return thirds.repeat(r, 1), torch.zeros(r, s, dtype=torch.bool)
    if name == "allpad":
        kp = torch.zeros(r, s, dtype=torch.bool)
        kp[0] = True
        kp[1:, s // 2:] = True
        return thirds.repeat(r, 1), kp
    assert name == "scatter"
    return torch.randint(0, 4, (r, s), generator=g), torch.rand(r, s, generator=g) < 0.3


def inputs(kind, mask_name, r, s, heads):
    """qkv (r s, 3 d) and d_out (r s, d), fp32 holding bf16 values; ids, key_pad."""
    d = 64 * heads
    seed = 1000 * KINDS.index(kind) + 100 * MASKS.index(mask_name) + 7 * s + heads
    g = torch.Generator().manual_seed(seed)
    qkv = bf(torch.randn(r * s, 3 * d, generator=g))
    d_out = bf(torch.randn(r * s, d, generator=g))
    ids, kp = mask(mask_name, r, s, g)
    rj = ramp(kind, s)
    if rj is not None:
        for h in range(heads):
            qkv[:, 64 * h] = 8.0
            qkv[:, d + 64 * h] = bf(rj).repeat(r)
    return qkv, d_out, ids, kp


def _heads(x, r, s, heads):
    return x.view(r, s, heads, 64).transpose(1, 2)


def reference(qkv, d_out, ids, kp, r, s, heads):
    """float64: out, the elementwise forward bound, lse (natural log), dqkv; and the same gradient
    under torch bf16 autocast (the yardstick)."""
    d = 64 * heads
    bias = R.attn_bias(ids, kp)

    def run(dtype, autocast):
        x = qkv.to(dtype).requires_grad_(True)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            q, k, v = (_heads(x[:, i * d:(i + 1) * d], r, s, heads) for i in range(3))
            logits = q @ k.transpose(-1, -2) * 0.125 + bias.to(dtype)
            p = torch.softmax(logits, -1)
            o = (p @ v).transpose(1, 2).reshape(r * s, d)
        gr, = torch.autograd.grad(o, x, d_out.to(o.dtype))
        return o.detach(), logits.detach(), p.detach(), v.detach(), gr.double()

    o64, logits, p64, v64, g64 = run(torch.float64, False)
    gac = run(torch.float32, True)[4]
    # P is rounded to bf16 (2^-9 relative) before P V and the output once more (2^-9): 2^-8 sum p |v|; doubled
    bound = 2.0 ** -7 * (p64 @ v64.abs()).transpose(1, 2).reshape(r * s, d) + 1e-6
    lse = torch.logsumexp(logits, -1)
    return SimpleNamespace(out=o64, bound=bound, lse=lse, g=g64, g_autocast=gac,
                           g_floor=_fp32_floor(qkv.double(), d_out.double(), p64, lse, r, s, heads))


def _fp32_floor(qkv, d_out, p, lse, r, s, heads):
    """What an fp32 log-sum-exp costs the gradients, (r s, 3 d): the backward takes p = 2^(s - lse) from
    fp32 logits and an fp32 lse in log2 units, each off by up to half an ulp, so every p carries a
    relative error of up to eta = 2^-22 max(1, max |lse| log2 e) (two half-ulps of the larger of the two,
    times ln 2, rounded up to a power of two).  dS = p (dP - delta) / 8 with delta = sum p dP then moves
    by up to eta p (|dP| + sum p |dP|) / 8 =: eta A, and dq, dk, dv by eta (A |K|, A^T |Q|, P^T |dO|).
    This is the allowance where the gradient itself is zero (one key: dq = dk = 0 exactly, and so is
    the yardstick's deviation), which max(4 x yardstick, 2^-8 ||g||) alone would set to 0."""
    d = 64 * heads
    q, k, v = (_heads(qkv[:, i * d:(i + 1) * d], r, s, heads) for i in range(3))
    do = _heads(d_out, r, s, heads)
    dp = (do @ v.transpose(-1, -2)).abs()
    a = p * (dp + (p * dp).sum(-1, keepdim=True)) * 0.125
    eta = 2.0 ** -22 * max(1.0, lse.abs().max().item() * LOG2E)
    parts = (a @ k.abs(), a.transpose(-1, -2) @ q.abs(), p.transpose(-1, -2) @ do.abs())
    return eta * torch.cat([t.transpose(1, 2).reshape(r * s, d) for t in parts], 1)


def emulate(qkv, d_out, ids, kp, r, s, heads):
    """The kernels' arithmetic in torch: fp32 logits in log2 units, 64-key blocks with the lazy (+8)
    rescale, P rounded to bf16, fp32 accumulation, bf16 output, lse = m + log2(sum); backward: P from
    the lse, fp32 delta = sum P dP, dS and P rounded to bf16, bf16 gradients.  Returns out (r s, d),
    lse (r, heads, s) in log2 units, dqkv (r s, 3 d), the number of (row, head, query) rescales after
    block 0 and the largest p.  Both passes use one rounded logit here; the kernels' forward takes the
    exponent with one fma and their backward from the rounded product, an ulp apart (_fp32_floor)."""
    d = 64 * heads
    sc = torch.tensor(0.125 * LOG2E, dtype=torch.float32)
    q, k, v = (_heads(qkv[:, i * d:(i + 1) * d], r, s, heads) for i in range(3))
    do = _heads(d_out, r, s, heads)
    s2 = (q @ k.transpose(-1, -2)) * sc + R.attn_bias(ids, kp) * torch.tensor(LOG2E, dtype=torch.float32)
    mrun = torch.full((r, heads, s), -math.inf)
    lsum = torch.zeros(r, heads, s)
    o = torch.zeros(r, heads, s, 64)
    rescales, pmax = 0, 0.0
    for k0 in range(0, s, BLOCK):
        blk = s2[..., k0:k0 + BLOCK]
        bm = blk.max(-1).values
        move = bm > mrun + LAZY
        alpha = torch.where(move, torch.exp2(mrun - bm), torch.ones_like(bm))
        mrun = torch.where(move, bm, mrun)
        lsum, o = lsum * alpha, o * alpha[..., None]
        if k0:
            rescales += int(move.sum())
        p = torch.exp2(blk - mrun[..., None])
        pmax = max(pmax, p.max().item())
        lsum = lsum + p.sum(-1)
        o = o + bf(p) @ v[:, :, k0:k0 + BLOCK]
    out = bf(o / lsum[..., None]).transpose(1, 2).reshape(r * s, d)
    lse = mrun + torch.log2(lsum)
    p = torch.exp2(s2 - lse[..., None])
    dp = do @ v.transpose(-1, -2)
    delta = (p * dp).sum(-1, keepdim=True)
    ds = bf(p * (dp - delta) * 0.125)
    parts = (ds @ k, ds.transpose(-1, -2) @ q, bf(p).transpose(-1, -2) @ do)
    dqkv = torch.cat([bf(t).transpose(1, 2).reshape(r * s, d) for t in parts], 1)
    return SimpleNamespace(out=out, lse=lse, dqkv=dqkv, rescales=rescales, pmax=pmax)


@functools.lru_cache(maxsize=None)
def case(kind, mask_name, r, s, heads):
    """Inputs and references of one case, computed once and shared (treat as read-only)."""
    qkv, d_out, ids, kp = inputs(kind, mask_name, r, s, heads)
    return SimpleNamespace(qkv=qkv, d_out=d_out, ids=ids, kp=kp, ref=reference(qkv, d_out, ids, kp, r, s, heads))


# ---- the checks, shared by the emulation's test and the kernels' ----
def forward_ratio(out, ref):
    """max |out - o64| / bound over the elements (<= 1 passes)."""
    return ((out.double() - ref.out).abs() / ref.bound).max().item()


def lse_error(lse_log2, ref):
    return (lse_log2.double() * math.log(2.0) - ref.lse).abs().max().item()


def grad_ratios(dqkv, ref, d, dq_row_widen=1.0):
    """The project's rule per dq, dk, dv: ||ours - float64||_2 / max(4 x the autocast yardstick's
    deviation, 2^-8 ||g||_2, the fp32 floor of _fp32_floor), and the same rule for every query's row
    of dq (its own yardstick deviation, its own norm), the allowance times dq_row_widen.  The floor is
    2^-19 or less of a gradient-sized tensor, so it decides only where the gradient vanishes.
    Returns {name: ratio} (<= 1 passes)."""
    got, out = dqkv.double(), {}
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * d, (i + 1) * d)
        ours, yard, gn = (got[:, sl] - ref.g[:, sl]).norm(), (ref.g_autocast[:, sl] - ref.g[:, sl]).norm(), ref.g[:, sl].norm()
        allow = torch.maximum(torch.maximum(4 * yard, 2.0 ** -8 * gn), ref.g_floor[:, sl].norm())
        out[name] = (ours / allow.clamp_min(1e-300)).item()
    ours = (got[:, :d] - ref.g[:, :d]).norm(dim=1)
    yard = (ref.g_autocast[:, :d] - ref.g[:, :d]).norm(dim=1)
    allow = torch.maximum(4 * yard, 2.0 ** -8 * ref.g[:, :d].norm(dim=1))
    allow = dq_row_widen * torch.maximum(allow, ref.g_floor[:, :d].norm(dim=1))
    out["dq rows"] = (ours / allow.clamp_min(1e-300)).max().item()
    return out
