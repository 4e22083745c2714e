#!/usr/bin/env python3
"""Time of the parameter update of a DCTAutoencoder training iteration
 on MI355X, at patch14-l's parameter shapes (hidden 1024,
16 heads, MLP 4096, 8 + 8 layers, LFQ 16 x 2^13) with random gradients; no
forward is run.  Every leg ends with ``model._weights()``, the bf16 operand
packs the next training forward needs.

Three legs on the same GPU in the same call, alternating, device events after
warm-up, each on its own copy of the model:
  foreach  clip_grad_norm_(5.0) + torch.optim.AdamW (default foreach) + repack by torch ops
  fused    the same with torch.optim.AdamW(fused=True)
  hip      FusedAdamW(max_grad_norm=5.0, model=model): norm, clip, AdamW and packs on HIP kernels
Reports ms per leg, the hip leg's kernels, and its GB/s on the count of 36 B per
parameter (g read twice, p / exp_avg / exp_avg_sq read and written, two bf16
packs) against the 6.3 TB/s achievable on this part.

    python tools/optim_time.py [--steps K] [--warmup W]
"""
import argparse
import copy
import ctypes as C
import json
import os
import sys
from importlib import import_module

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE_GBS = 6300.0
HYPER = dict(lr=1e-4, betas=(0.9, 0.99), weight_decay=0.1)   # main.py:420-425


def run(steps=10, warmup=3, dev=None):
    import _pkgload
    pkg = _pkgload.load()
    L = import_module("dct_autoencoder_amd._lib")
    dev = dev or torch.device("cuda", 0)
    torch.manual_seed(0)
    enc = dict(hidden_size=1024, intermediate_size=4096, num_attention_heads=16, num_hidden_layers=8)
    cfg = pkg.DCTAutoencoderConfig(image_channels=3, patch_size=14, max_patch_h=32, max_patch_w=32,
                                   vq_codebook_size=8192, vq_num_codebooks=16, vq_type="lfq",
                                   encoder_config=enc, decoder_config=enc)
    base = pkg.DCTAutoencoder(cfg).to(dev).train()
    models = {leg: copy.deepcopy(base) for leg in ("foreach", "fused", "hip")}
    del base
    g = torch.Generator(device=dev).manual_seed(1)
    for m in models.values():
        g.manual_seed(1)
        for p in m.parameters():
            if p.requires_grad:
                p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
    opts = {"foreach": torch.optim.AdamW(models["foreach"].parameters(), **HYPER),
            "fused": torch.optim.AdamW(models["fused"].parameters(), fused=True, **HYPER),
            "hip": pkg.FusedAdamW(models["hip"].parameters(), max_grad_norm=5.0, model=models["hip"], **HYPER)}

    def step(leg):
        m, opt = models[leg], opts[leg]
        if leg != "hip":
            torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
        opt.step()
        return m._weights()

    n_param = sum(p.numel() for p in models["hip"].parameters() if p.requires_grad)
    n_packed = sum(e["rows"] * e["cols"] for e in import_module("dct_autoencoder_amd.optim").segment_plan(models["hip"])
                   if "pack" in e)
    out = {"workload": f"clip_grad_norm_(5.0) + AdamW + bf16 repack, patch14-l, {n_param} trainable parameters "
                       f"({n_packed} in packed linear weights), random gradients"}
    times = {leg: [] for leg in models}
    for leg in models:
        for _ in range(warmup):
            step(leg)
        torch.cuda.synchronize(dev)
    for _ in range(steps):
        for leg in models:   # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(leg)
            e1.record()
            torch.cuda.synchronize(dev)
            times[leg].append(e0.elapsed_time(e1))
    for leg, t in times.items():
        t = sorted(t)
        out[f"{leg}_ms_per_step"] = {"median": round(t[len(t) // 2], 3), "min": round(t[0], 3), "max": round(t[-1], 3)}
    med = {leg: out[f"{leg}_ms_per_step"]["median"] for leg in times}
    out["hip_over_fused"] = round(med["hip"] / med["fused"], 3)
    out["hip_over_foreach"] = round(med["hip"] / med["foreach"], 3)
    out["hip_not_slower_than_fused"] = bool(med["hip"] <= med["fused"])
    nbytes = 36 * n_param
    out["hip_bytes_at_36B_per_parameter"] = nbytes
    out["hip_GBps_whole_leg"] = round(nbytes / (med["hip"] / 1e3) / 1e9, 1)
    out["hbm_achievable_GBps"] = HBM_ACHIEVABLE_GBS
    # the hip leg's kernels (event pairs around every library call; adds host time between launches)
    ctx = L.context(dev)
    ctx.lib.dctae_timing_reset(ctx.h)
    ctx.lib.dctae_set_timing(ctx.h, 1)
    for _ in range(steps):
        step("hip")
    torch.cuda.synchronize(dev)
    ctx.lib.dctae_set_timing(ctx.h, 0)
    ctx.lib.dctae_timing_collect(ctx.h)
    kern, i = {}, 0
    while True:
        name, ms, cnt = C.c_char_p(), C.c_double(), C.c_int64()
        if ctx.lib.dctae_timing_get(ctx.h, i, C.byref(name), C.byref(ms), C.byref(cnt)) != 0:
            break
        kern[name.value.decode()] = {"ms_per_step": round(ms.value / steps, 4), "launches_per_step": int(cnt.value) // steps}
        i += 1
    out["hip_kernels"] = kern
    k_ms = sum(v["ms_per_step"] for k, v in kern.items() if k.startswith("optim_"))
    if k_ms > 0:
        out["hip_GBps_kernels_only"] = round(nbytes / (k_ms / 1e3) / 1e9, 1)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    print(json.dumps(run(a.steps, a.warmup)))
