#!/usr/bin/env python3
"""Time of one DCTAutoencoder training step on MI355X: forward +
backward of the whole step (model, quantizer, step_losses, the weighted sum of
main.py:311-314) at patch14-l (hidden 1024, 16 heads, MLP 4096, 8 + 8 layers,
LFQ 16 x 2^13), R rows of S = 3072 tokens, random init.

Two legs on the same GPU in the same call, alternating, device events after
warm-up:
  hip    the package in ``.train()``: HIP kernels forward and backward
  torch  the same formula with torch ops: the package's parameters through
         torch.nn.functional under bf16 autocast with autograd (attention =
         scaled_dot_product_attention with the additive +1.0 bias); quantizer
         and losses are the package's in both legs
Reports ms per step and peak memory of each leg, per-kernel time of the hip
leg, and TFLOP/s of the backward linear and attention kernels from
shape-derived FLOPs (attention backward is two-pass with a delta sweep, nine
products: 18 R heads S^2 64).

    python tools/model_train_time.py [--rows R] [--steps K] [--warmup W]
"""
import argparse
import ctypes as C
import json
import os
import sys
from importlib import import_module

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF16_PEAK_TF = 2500.0
WEIGHTS = dict(rec_loss=0.1, rec_loss_unnormalized=1.0, commit_loss=0.1, entropy_loss=0.1)


def torch_forward(m, dp):
    """modeling:119-194 with torch ops on the package's parameters (call under autocast)."""
    r, s = dp.key_pad_mask.shape
    ids, kp = dp.batched_image_ids, dp.key_pad_mask
    bias = ((ids[:, None, :, None] == ids[:, None, None, :]) & kp[:, None, None, :]).to(torch.bfloat16)
    pos, ch = dp.patch_positions, dp.patch_channels

    def stack(enc, h):
        c = enc.config
        for L in enc.layers:
            a = L.self_attn
            x = L.layer_norm1(h)
            q, k, v = (p(x).view(r, s, c.num_attention_heads, 64).transpose(1, 2) for p in (a.q_proj, a.k_proj, a.v_proj))
            o = F.scaled_dot_product_attention(q, k, v, attn_mask=bias).transpose(1, 2).reshape(r, s, -1)
            h = h + a.out_proj(o)
            x = L.mlp.fc1(L.layer_norm2(h))
            h = h + L.mlp.fc2(x * torch.sigmoid(1.702 * x))
        return h

    def pos_embed(side):
        return (getattr(m, f"{side}_pos_embed_height")[pos[..., 0]] + getattr(m, f"{side}_pos_embed_width")[pos[..., 1]]
                + getattr(m, f"{side}_pos_embed_channel")[ch])

    h = stack(m.encoder, m.to_patch_embedding(dp.patches) + pos_embed("encoder"))
    xq, codes, commit, dist = m.vq_model(h.float(), mask=~kp)
    out = dp.shallow_copy()
    out.patches = m.proj_out(stack(m.decoder, xq + pos_embed("decoder"))).float()
    return dict(dct_patches=out, commit_loss=commit, codes=codes, distances=dist)


def run(rows=4, steps=3, warmup=1, dev=None):
    import _pkgload
    pkg = _pkgload.load()
    losses = import_module("dct_autoencoder_amd.losses")
    L = import_module("dct_autoencoder_amd._lib")
    dev = dev or torch.device("cuda", 0)
    torch.manual_seed(0)
    d, heads, inter, layers, s = 1024, 16, 4096, 8, 3072
    enc = dict(hidden_size=d, intermediate_size=inter, num_attention_heads=heads, num_hidden_layers=layers)
    cfg = pkg.DCTAutoencoderConfig(image_channels=3, patch_size=14, max_patch_h=32, max_patch_w=32,
                                   vq_codebook_size=8192, vq_num_codebooks=16, vq_type="lfq",
                                   encoder_config=enc, decoder_config=enc)
    m = pkg.DCTAutoencoder(cfg).to(dev).train()
    m.patchnorm.frozen = True
    g = torch.Generator(device="cpu").manual_seed(1)
    patches = torch.randn(rows, s, 196, generator=g).clamp(-6, 6).to(dev)
    pos = torch.stack(torch.meshgrid(torch.arange(32), torch.arange(32), indexing="ij"), -1).reshape(-1, 2)
    pos = pos.repeat_interleave(3, 0)[None].expand(rows, s, 2).contiguous().to(dev)
    ch = torch.arange(3).repeat(1024)[None].expand(rows, s).contiguous().to(dev)

    def batch(x):
        return pkg.DCTPatches(patches=x, key_pad_mask=torch.zeros(rows, s, dtype=torch.bool, device=dev),
                              batched_image_ids=torch.zeros(rows, s, dtype=torch.long, device=dev),
                              patch_channels=ch, patch_positions=pos, patch_sizes=[(36, 36)] * rows,
                              original_sizes=[(512, 512)] * rows)

    with torch.no_grad():
        raw = batch(m.patchnorm.inverse_norm(batch(patches.clone())))

    def step(leg, backward=True):
        m.zero_grad(set_to_none=True)
        normalized = batch(patches)
        if leg == "hip":
            res = m(normalized.shallow_copy())
        else:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                res = torch_forward(m, normalized.shallow_copy())
        out = losses.step_losses(res, raw, normalized, m.patchnorm, cfg.vq_codebook_size)
        total = sum(w * out[k] for k, w in WEIGHTS.items())
        if backward:
            total.backward()
        return total

    main_ctx = L.context(dev)

    def contexts():
        """The library keeps one context per host thread: the calling thread's runs the forward,
        autograd's device thread has its own for the backward (it exists after the warm-up)."""
        return [("forward" if c is main_ctx else "backward", c) for (idx, _), c in L._ctx_by_key.items()
                if idx == dev.index]

    def kernels(n):
        kern = {}
        for side, ctx in contexts():
            ctx.lib.dctae_set_timing(ctx.h, 0)
            ctx.lib.dctae_timing_collect(ctx.h)
            i = 0
            while True:
                name, ms, cnt = C.c_char_p(), C.c_double(), C.c_int64()
                if ctx.lib.dctae_timing_get(ctx.h, i, C.byref(name), C.byref(ms), C.byref(cnt)) != 0:
                    break
                kern[f"{side}.{name.value.decode()}"] = {"ms_per_step": round(ms.value / n, 4),
                                                         "launches_per_step": int(cnt.value) // n}
                i += 1
        return kern

    out = {"workload": f"DCTAutoencoder training step (forward + backward, losses included), patch14-l, {rows} rows x "
                       f"{s} tokens"}
    times, peak = {"hip": [], "torch": []}, {}
    for leg in ("hip", "torch"):
        for _ in range(warmup):
            step(leg)
        torch.cuda.synchronize(dev)
    for _ in range(steps):
        for leg in ("hip", "torch"):   # alternating
            torch.cuda.reset_peak_memory_stats(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss = step(leg)
            e1.record()
            torch.cuda.synchronize(dev)
            times[leg].append(e0.elapsed_time(e1))
            peak[leg] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
            out[f"{leg}_loss"] = round(loss.item(), 5)
    for leg in times:
        t = sorted(times[leg])
        out[f"{leg}_ms_per_step"] = {"median": round(t[len(t) // 2], 2), "min": round(t[0], 2), "max": round(t[-1], 2)}
        out[f"{leg}_peak_GiB"] = peak[leg]
    out["hip_over_torch"] = round(out["hip_ms_per_step"]["median"] / out["torch_ms_per_step"]["median"], 3)
    # per-kernel time of the hip leg (event pairs around every library call; adds host time between launches)
    for _, ctx in contexts():
        ctx.lib.dctae_timing_reset(ctx.h)
        ctx.lib.dctae_set_timing(ctx.h, 1)
    for _ in range(steps):
        step("hip")
    torch.cuda.synchronize(dev)
    per = kernels(steps)
    out["kernels"] = per
    mt = rows * s
    lin_fwd = 2 * layers * 2 * mt * d * (3 * d + d + 2 * inter) + 2 * 2 * mt * 196 * d   # CLIP stacks, embed, proj_out
    lin_bwd_ms = per["backward.model_linear"]["ms_per_step"]   # the dX and dW GEMMs: twice the forward's FLOPs
    out["linear_backward"] = {"ms_per_step": round(lin_bwd_ms, 3), "flops": 2 * lin_fwd,
                              "achieved_tflops": round(2 * lin_fwd / (lin_bwd_ms / 1e3) / 1e12, 1), "peak": BF16_PEAK_TF}
    ab = per.get("backward.model_attention_bwd")
    if ab:
        fl = 2 * layers * 18 * rows * heads * s * s * 64
        out["attention_backward"] = {"ms_per_step": ab["ms_per_step"], "flops": fl,
                                     "achieved_tflops": round(fl / (ab["ms_per_step"] / 1e3) / 1e12, 1),
                                     "peak": BF16_PEAK_TF}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    print(json.dumps(run(a.rows, a.steps, a.warmup)))
