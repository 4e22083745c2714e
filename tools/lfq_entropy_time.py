"""Time forward + backward of the LFQ entropy loss on conf/patch14-l.json's
quantizer (codebook_dim 13, 16 codebooks): the fused HIP path
(compute_entropy_loss on an LFQDistance) against the package's own dense
branch (compute_entropy_loss on dist.materialize(), about 2 GB per copy of the
dense tensor at 4,096 tokens), in one process, with events, after warm-up.
The fused path is also timed at 16 x the tokens, where the dense form is not
attempted.  Prints one JSON line.

    python tools/lfq_entropy_time.py [tokens]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload  # noqa: E402

pkg = _pkgload.load()

dev = torch.device("cuda", 0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
CD, NCB = 13, 16


def problem(tokens):
    g = torch.Generator().manual_seed(0)
    h = (torch.randn(1, tokens, NCB, CD, generator=g) * 0.01).to(dev).requires_grad_(True)
    mask = (torch.rand(1, tokens, generator=g) < 0.9).to(dev)
    return h, mask


def step(h, mask, dense):
    dist = pkg.LFQDistance(h, 1.0, CD, NCB)
    loss = pkg.compute_entropy_loss(dist.materialize() if dense else dist, mask)
    g, = torch.autograd.grad(loss, h)
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


h, mask = problem(n)
torch.cuda.synchronize()
free0, res0 = torch.cuda.mem_get_info(dev)[0], torch.cuda.memory_reserved(dev)
lf, gf = step(h, mask, False)
torch.cuda.synchronize()
# device memory the library took outside torch's allocator (contexts + workspace)
lib_bytes = (free0 - torch.cuda.mem_get_info(dev)[0]) - (torch.cuda.memory_reserved(dev) - res0)
torch.cuda.reset_peak_memory_stats(dev)
base = torch.cuda.memory_allocated(dev)
res = {"tokens": n, "codebook_dim": CD, "num_codebooks": NCB}
res["fused_ms"] = t(lambda: step(h, mask, False), 3, 20)
res["fused_torch_peak_bytes"] = torch.cuda.max_memory_allocated(dev) - base
res["fused_library_bytes"] = lib_bytes
torch.cuda.reset_peak_memory_stats(dev)
ld, gd = step(h, mask, True)
res["dense_ms"] = t(lambda: step(h, mask, True), 1, 3)
res["dense_torch_peak_bytes"] = torch.cuda.max_memory_allocated(dev) - base
res["loss_fused"], res["loss_dense"] = lf.item(), ld.item()
res["grad_max_diff_over_max"] = ((gf - gd).abs().max() / gd.abs().max()).item()
del ld, gd
torch.cuda.empty_cache()
h16, mask16 = problem(16 * n)
res["fused_16x_tokens"] = 16 * n
res["fused_16x_ms"] = t(lambda: step(h16, mask16, False), 2, 10)
print(json.dumps({k: (round(v, 6) if isinstance(v, float) else v) for k, v in res.items()}))
