"""Time the antialiased resize of the dataset crop (resize.resize_antialias: one
launch for the whole list) against torch's `interpolate(antialias=True)` called
image by image, in one process on one GPU, every input resident:
  set1    64 x 1536 x 1024 -> 768 x 512 (scale 2 on both axes)
  ragged  a fixed list of 64 sizes, long side in (768, 3072], aspect ratio in
          [0.4, 1], either orientation (seed 7), each to dataset_crop_size(h, w, 768)
for fp32 images and for the uint8 images they come from (the torch baseline of
the byte input is `interpolate(u8.float().div(255))`, the chain the byte call
replaces).  Per set and input: the call time by events after warm-up, the
library and the torch timings interleaved (one timed group of each per repeat),
median / min / max over the repeats; the kernel's own time from the library's
timing table; the bytes the resize has to move (every input byte read once, every
output byte written once) over the kernel time as a fraction of the 6.29 TB/s
achievable on this GPU; the largest difference from torch's result; and every
size torch refuses (its kernel needs shared memory in proportion to the scale),
which the baseline then leaves out.  Prints one JSON line.

    python tools/resize_time.py [--repeats 7] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload  # noqa: E402

pkg = _pkgload.load()
from dct_autoencoder_amd import _lib, _ops, resize  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--quick", action="store_true", help="an eighth of every list (a functional check of the tool)")
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
ACHIEVABLE_TBS = 6.29
MAX_SIZE = 768


def ragged_sizes(n):
    g = np.random.default_rng(7)
    out = []
    for _ in range(n):
        long = int(g.integers(MAX_SIZE + 1, 3073))
        short = max(1, int(long * g.uniform(0.4, 1.0)))
        out.append((long, short) if g.integers(0, 2) else (short, long))
    return out


def group_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def interleaved(fns, calls, warm=3):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, fn in fns.items():
            out[k].append(group_ms(fn, calls))
    return out


def summary(ms):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / med, 4)}


def kernel_ms(fn, reps):
    """mean ms per call of the resize kernel, from the library's timing table"""
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
    got = None
    for i in range(256):
        name, ms, n = C.c_char_p(), C.c_double(), C.c_int64()
        if ctx.lib.dctae_timing_get(ctx.h, i, C.byref(name), C.byref(ms), C.byref(n)) != 0:
            break
        if name.value.decode() == "resize_aa" and n.value:
            got = ms.value / reps
    ctx.lib.dctae_timing_reset(ctx.h)
    return got


def torch_one(x, size):
    x = x if x.dtype == torch.float32 else x.float().div(255)
    return F.interpolate(x[None], size=size, mode="bilinear", antialias=True, align_corners=False)[0]


def report(images, sizes, calls):
    """one input type of one set"""
    refused, ok = [], []
    for i, (x, s) in enumerate(zip(images, sizes)):
        try:
            torch_one(x, s)
            torch.cuda.synchronize()
            ok.append(i)
        except RuntimeError as e:
            refused.append({"input": list(x.shape[1:]), "output": list(s), "error": str(e).splitlines()[0][:160]})
    ours = resize.resize_antialias(images, sizes)
    diff = max((float((ours[i] - torch_one(images[i], sizes[i])).abs().max()) for i in ok), default=None)

    def lib_call():
        return resize.resize_antialias(images, sizes)

    def torch_loop():
        return [torch_one(images[i], sizes[i]) for i in ok]
    ms = interleaved({"library": lib_call, "torch_loop": torch_loop}, calls)
    in_bytes = sum(x.numel() * x.element_size() for x in images)
    out_bytes = sum(12 * h * w for h, w in sizes)
    k_ms = kernel_ms(lib_call, 5)
    r = {"images": len(images), "calls_per_group": calls, "repeats": args.repeats,
         "library": summary(ms["library"]), "torch_loop": summary(ms["torch_loop"]),
         "torch_loop_images": len(ok), "torch_refused": refused,
         "torch_over_library": round(statistics.median(ms["torch_loop"]) / statistics.median(ms["library"]), 3),
         "kernel_ms": round(k_ms, 4), "input_MB": round(in_bytes / 1e6, 2), "output_MB": round(out_bytes / 1e6, 2),
         "kernel_TB_per_s": round((in_bytes + out_bytes) / (k_ms * 1e-3) / 1e12, 3),
         "fraction_of_achievable": round((in_bytes + out_bytes) / (k_ms * 1e-3) / 1e12 / ACHIEVABLE_TBS, 3),
         "max_abs_diff_from_torch": diff}
    return r


def main():
    n = 8 if args.quick else 64
    res = {"device": torch.cuda.get_device_name(dev), "quick": args.quick, "achievable_TB_per_s": ACHIEVABLE_TBS}
    gen = torch.Generator(device=dev).manual_seed(7)
    sets = {"set1": [(1536, 1024)] * n, "ragged": ragged_sizes(64)[:n]}
    for name, hw in sets.items():
        sizes = [resize.dataset_crop_size(h, w, MAX_SIZE) for h, w in hw]
        u8 = [torch.randint(0, 256, (3, h, w), dtype=torch.uint8, device=dev, generator=gen) for h, w in hw]
        f32 = [_ops.u8_to_f32(u) for u in u8]
        a, b = resize.resize_antialias(u8, sizes), resize.resize_antialias(f32, sizes)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "byte and fp32 results differ"
        del a, b
        res[name] = {"sizes": [list(s) for s in hw[:4]] + ["..."], "f32": report(f32, sizes, 5),
                     "u8": report(u8, sizes, 5)}
        del u8, f32
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
