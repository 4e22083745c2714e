"""Time forward + backward of the pixel loss (main.py:95-110: two decodes, the
mean per-image MSE, the gradient with respect to the output patches) on
  sq512   32 rows x 3072 tokens, one 512 x 512 image per row (the FFT decode), and
  ragged  a packed batch of mixed sizes up to 448 x 768 (the GEMM decode):
the fused HIP path (pixel_loss on device tensors, autograd.grad) against the
same formula written with torch ops on the same device in the same process --
index assignment with pre-built index tensors, torch.matmul with the truncated
DCT matrices, the colour ops -- with events, after warm-up.  Also times the
library calls alone, reads the backward's stages from the library's timing
table and states the three new kernels against their byte models at the
6.29 TB/s achievable:
  pixel_loss_forward (d)  2 passes over the images              (x_hat, x read)
  color_bwd (a)           4 passes over the images, fused form  (ipt, x_hat, x read; g_ipt written)
  gather_tokens (c)       2 passes over the tokens              (dY tiles read, dpatches written)
Prints one JSON line.

    python tools/pixel_loss_time.py
"""
import ctypes as C
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload  # noqa: E402

pkg = _pkgload.load()
from dct_autoencoder_amd import _lib, _ops, color  # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
P, PP, S = 14, 196, 3072
PEAK = 6.29e12
RAGGED = [(448, 768), (224, 224), (300, 500), (150, 420), (512, 140), (100, 300), (384, 384), (64, 64)]


def problem(kind):
    fe = pkg.DCTAutoencoderFeatureExtractor(3, P, 0.0, 32, 32, S)
    if kind == "sq512":
        images = [im for im in _ops.synth_images(32, 512, 512, 7, device=dev)]
    else:
        images = [_ops.synth_images(1, h, w, 100 + i, device=dev)[0] for i, (h, w) in enumerate(RAGGED * 10)]
    ((dp, _),) = fe.encode_batch(images, return_raw=True)
    g = torch.Generator().manual_seed(3)
    out = (dp.patches + 0.05 * torch.randn(dp.patches.shape, generator=g).to(dev)).requires_grad_(True)
    return fe, dp, out


def with_patches(dp, x):
    d = dp.shallow_copy()
    d.patches = x
    return d


def dct_matrix(n, rows):
    k = torch.arange(rows, dtype=torch.float64)[:, None]
    x = torch.arange(n, dtype=torch.float64)[None, :]
    m = torch.cos(math.pi * (2 * x + 1) * k / (2 * n)) * math.sqrt(2.0 / n)
    m[0] *= math.sqrt(0.5)
    return m.float().to(dev)


class TorchOps:
    """FE:289-310 with torch ops; the per-image index tensors are built once, outside the timing"""

    def __init__(self, fe, dp):
        m = color.matrices()
        self.ipt2lms, self.lms2rgb = m["ipt2lms"].to(dev), m["lms2rgb"].to(dev)
        self.items = []
        ids, kp = dp.batched_image_ids.cpu(), dp.key_pad_mask.cpu()
        n = 0
        for r in range(ids.shape[0]):
            for i in torch.unique(ids[r]).tolist():
                idx = torch.nonzero((ids[r] == i) & ~kp[r])[:, 0].to(dev)
                (ph, pw), (h, w) = dp.patch_sizes[n], dp.original_sizes[n]
                qh, qw = min(ph, fe.max_patch_h), min(pw, fe.max_patch_w)
                self.items.append((r, idx, dp.patch_channels[r, idx], dp.patch_positions[r, idx, 0],
                                   dp.patch_positions[r, idx, 1], qh, qw, dct_matrix(h, P * qh), dct_matrix(w, P * qw)))
                n += 1

    def images(self, patches):
        out = []
        for r, idx, c, h, w, qh, qw, ch_m, cw_m in self.items:
            y = torch.zeros(3, qh, qw, PP, device=dev)
            y[c, h, w] = patches[r, idx]
            y = y.view(3, qh, qw, P, P).permute(0, 1, 3, 2, 4).reshape(3, qh * P, qw * P)
            ipt = ch_m.t() @ y @ cw_m
            l = torch.einsum("ij,jhw->ihw", self.ipt2lms, ipt)
            l = torch.sign(l) * l.abs() ** (1 / 0.43)
            out.append(torch.einsum("ij,jhw->ihw", self.lms2rgb, l))
        return out

    def step(self, out, target):
        with torch.no_grad():
            x = self.images(target)
        x_hat = self.images(out)
        loss = sum(F.mse_loss(a, b) for a, b in zip(x, x_hat)) / len(x_hat)
        g, = torch.autograd.grad(loss, out)
        return loss, g


def t(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def stages(fn, reps):
    """mean ms per stage of the library's timing table over reps calls of fn on this thread"""
    ctx = _lib.context(dev)
    ctx.lib.dctae_timing_reset(ctx.h)
    ctx.lib.dctae_set_timing(ctx.h, 1)
    try:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    finally:
        ctx.lib.dctae_set_timing(ctx.h, 0)
    ctx.lib.dctae_timing_collect(ctx.h)
    res = {}
    for i in range(256):
        name, ms, n = C.c_char_p(), C.c_double(), C.c_int64()
        if ctx.lib.dctae_timing_get(ctx.h, i, C.byref(name), C.byref(ms), C.byref(n)) != 0:
            break
        res[name.value.decode()] = ms.value / reps
    ctx.lib.dctae_timing_reset(ctx.h)
    return res


def fused_step(fe, dp, out):
    loss, _, _ = pkg.pixel_loss(with_patches(dp, out), dp, fe)
    g, = torch.autograd.grad(loss, out)
    return loss, g


res = {}
for kind in ("sq512", "ragged"):
    fe, dp, out = problem(kind)
    tops = TorchOps(fe, dp)
    target, o = dp.patches, out.detach()
    r = {"rows": int(out.shape[0]), "images": len(dp.original_sizes),
         "image_floats": int(sum(3 * h * w for h, w in dp.original_sizes)), "token_floats": int(out.numel())}
    r["fused_ms"] = t(lambda: fused_step(fe, dp, out), 3, 10)
    r["torch_ms"] = t(lambda: tops.step(out, target), 2, 5)
    prm = fe.params(S)
    tab = _ops.decode_table(prm, dp.batched_image_ids, dp.key_pad_mask, dp.patch_positions, dp.patch_channels,
                            dp.patch_sizes, dp.original_sizes)

    def dec(x):
        return _ops.decode(prm, tab.ids, tab.key_pad, tab.pos, tab.ch, None, None, patches=x, table=tab,
                           return_flat=True)[1]
    fh, fx = dec(o), dec(target)
    one = torch.ones((), device=dev)
    r["decode_ms"] = t(lambda: dec(o), 3, 10)
    r["pixel_loss_forward_ms"] = t(lambda: _ops.pixel_loss_forward(tab, fh, fx), 3, 20)
    r["decode_backward_fused_ms"] = t(lambda: _ops.decode_backward(prm, tab, o, rgb_hat=fh, rgb=fx, g=one), 3, 10)
    r["decode_backward_vjp_ms"] = t(lambda: _ops.decode_backward(prm, tab, o, grad_rgb=fh), 3, 10)
    r["backward_stages_ms"] = {k: round(v, 4) for k, v in
                               stages(lambda: _ops.decode_backward(prm, tab, o, rgb_hat=fh, rgb=fx, g=one), 5).items()}
    img_b, tok_b = 4 * r["image_floats"], 4 * r["token_floats"]
    model = {"pixel_loss_forward": 2 * img_b / PEAK * 1e3, "color_bwd": 4 * img_b / PEAK * 1e3,
             "gather_tokens": 2 * tok_b / PEAK * 1e3}
    r["byte_model_ms"] = {k: round(v, 4) for k, v in model.items()}
    r["fraction_of_achievable"] = {
        "pixel_loss_forward": round(model["pixel_loss_forward"] / r["pixel_loss_forward_ms"], 3),
        "color_bwd": round(model["color_bwd"] / r["backward_stages_ms"]["color_bwd"], 3),
        "gather_tokens": round(model["gather_tokens"] / r["backward_stages_ms"]["gather_tokens"], 3)}
    a, b = fused_step(fe, dp, out), tops.step(out, target)
    r["loss_fused"], r["loss_torch"] = a[0].item(), b[0].item()
    r["grad_max_diff_over_max"] = ((a[1] - b[1]).abs().max() / b[1].abs().max()).item()
    res[kind] = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in r.items()}
    del fe, dp, out, tops, target, o, fh, fx, tab
    torch.cuda.empty_cache()
print(json.dumps(res))
