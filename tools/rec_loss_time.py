"""Time forward + backward of the reconstruction losses (rec_loss,
rec_loss_unnormalized and the unnormalized patches, the gradient of
0.1 rec + 1.0 unn + <w, unnorm> with respect to the output) at 4 x 3072 and
32 x 3072 tokens of 196 floats with about 10 % padding: the fused HIP path
(reconstruction_losses on device tensors) against the package's own torch-op
formulation of main.py:71, 79-83 on the same device, in one process, with
events, after warm-up.  Also times the fused forward and backward alone and
states them against the byte model (four passes over n * 196 * 4 bytes each,
6.29 TB/s achievable).  Prints one JSON line.

    python tools/rec_loss_time.py
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload  # noqa: E402

pkg = _pkgload.load()
from dct_autoencoder_amd import _ops  # noqa: E402

dev = torch.device("cuda", 0)
P, PP, S = 14, 196, 3072
PEAK = 6.29e12
W0, W1 = 0.1, 1.0


def problem(rows):
    g = torch.Generator().manual_seed(rows)
    tabs = np.load(os.path.join(ROOT, "tests", "golden", "patchnorm_ref.npz"))
    pn = pkg.PatchNorm(32, 32, P, 3)
    pn.median.data.copy_(torch.from_numpy(tabs["median"]))
    pn.b.data.copy_(torch.from_numpy(tabs["b"]))
    pn.frozen = True
    pn = pn.eval().to(dev)
    ch = torch.randint(0, 3, (rows, S), generator=g).to(dev)
    pos = torch.randint(0, 32, (rows, S, 2), generator=g).to(dev)
    key_pad = (torch.rand(rows, S, generator=g) < 0.1).to(dev)
    tn = torch.randn(rows, S, PP, generator=g).to(dev)
    out = (tn + 0.3 * torch.randn(rows, S, PP, generator=g).to(dev)).requires_grad_(True)
    raw = pn.inverse_norm(pkg.DCTPatches(tn, key_pad, None, torch.zeros_like(ch), ch, pos, [], [])) * 1.01
    w = torch.randn(rows, S, PP, generator=g).to(dev)

    def dp(x):
        return pkg.DCTPatches(x, key_pad, None, torch.zeros_like(ch), ch, pos, [], [])
    return pn, dp, out, tn, raw, w, key_pad


def fused_step(pn, dp, out, tn, raw, w, key_pad):
    rec, unn, un = pkg.reconstruction_losses(dp(out), dp(tn), dp(raw), pn)
    g, = torch.autograd.grad(W0 * rec + W1 * unn + (un * w).sum(), out)
    return rec, unn, g


def torch_step(pn, dp, out, tn, raw, w, key_pad):
    mask = ~key_pad
    d = dp(out)
    c, h, ww = d.patch_channels, d.h_indices, d.w_indices
    rec = F.l1_loss(out[mask], tn[mask])
    un = out * (pn.b[c, h, ww] * 2 ** 0.5 + pn.eps) + pn.median[c, h, ww]
    unn = F.l1_loss(un[mask], raw[mask])
    g, = torch.autograd.grad(W0 * rec + W1 * unn + (un * w).sum(), out)
    return rec, unn, g


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


res = {}
for rows in (4, 32):
    args = problem(rows)
    pn, dp, out, tn, raw, w, key_pad = args
    n = rows * S
    r = {"tokens": n}
    r["fused_ms"] = t(lambda: fused_step(*args), 5, 30)
    r["torch_ms"] = t(lambda: torch_step(*args), 3, 10)
    st, prm = pn.state(), pn._params()
    d = dp(out)
    o = out.detach()
    sc, _ = _ops.rec_loss_forward(o, tn, raw, d.patch_channels, d.patch_positions, key_pad, st, prm, True)
    gg = torch.tensor([W0, W1], device=dev)
    r["forward_kernels_ms"] = t(lambda: _ops.rec_loss_forward(o, tn, raw, d.patch_channels, d.patch_positions, key_pad,
                                                               st, prm, True), 5, 30)
    r["backward_kernel_ms"] = t(lambda: _ops.rec_loss_backward(o, tn, raw, d.patch_channels, d.patch_positions,
                                                                key_pad, st, prm, sc, gg, w), 5, 30)
    model_s = 4 * n * PP * 4 / PEAK          # four tensor passes, forward and backward alike
    r["byte_model_ms_each"] = model_s * 1e3
    r["forward_fraction_of_achievable"] = model_s * 1e3 / r["forward_kernels_ms"]
    r["backward_fraction_of_achievable"] = model_s * 1e3 / r["backward_kernel_ms"]
    a, b = fused_step(*args), torch_step(*args)
    r["rec_fused"], r["rec_torch"], r["unn_fused"], r["unn_torch"] = (x.item() for x in (a[0], b[0], a[1], b[1]))
    r["grad_max_diff"] = (a[2] - b[2]).abs().max().item()
    res[f"{rows}x{S}"] = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in r.items()}
    del args, pn, dp, out, tn, raw, w, key_pad, d, o
    torch.cuda.empty_cache()
print(json.dumps(res))
