"""Time the progressive decode (fe.decode_prefixes: every prefix frame in one
launch sequence) against the way the same frames were obtained before it: a
loop of fe.decode_batch over masked copies of the batch, one call per prefix
position.  One process on one GPU, inputs resident, the loop's masked batches
built beforehand (they are not timed):
  one512   one 512 x 512 image from int16 codes, prefixes 64, 128, ..., 3072
           (48 frames), to fp32 and to uint8
  ragged16 16 ragged images with the long side at most 448, 8 prefixes each
           (n_i j / 8), from int16 codes, to fp32
Per workload: the wall time of a call that ends in a device synchronise (both
ways read the batch on the host, so the host is part of either), the two ways
interleaved (one timed group of each per repeat, so clock and thermal drift
hit both alike), median / min / max over the repeats; the per-stage split of
the new call from the library's timing table (dec_map, scatter_tokens,
idct_cols, idct_rows, ipt_to_rgb, clip_minmax, clip_store) with
clip="minmax"; and the achieved rate of the two clip kernels on the bytes
they have to move (clip_minmax reads 4 bytes per value, clip_store reads 4 and
writes 4 or 1) against the 6.29 TB/s achievable.  The new call's frames are
checked equal, bit for bit, to the loop's before anything is timed.  Exit
status 1, with a line on stderr, if on any workload the new call's median
exceeds the loop's.  Prints one JSON line.

    python tools/progressive_time.py [--repeats 7] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload  # noqa: E402

pkg = _pkgload.load()
from dct_autoencoder_amd import _lib, _ops, progressive  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--quick", action="store_true", help="a sixth of the prefixes (a functional check of the tool)")
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
U8, F32 = torch.uint8, torch.float32
HBM_TBPS = 6.29
STAGES = ("dec_map", "scatter_tokens", "idct_cols", "idct_rows", "ipt_to_rgb", "clip_minmax", "clip_store")


def models():
    tabs = np.load(os.path.join(ROOT, "tests", "golden", "patchnorm_ref.npz"))
    pn = pkg.PatchNorm(32, 32, 14, 3).to(dev)
    pn.median.data.copy_(torch.from_numpy(tabs["median"]))
    pn.b.data.copy_(torch.from_numpy(tabs["b"]))
    pn.frozen = True
    lfq = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).to(dev).eval()
    return pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072), pn.eval(), lfq


def group_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def interleaved(fns, calls, warm=3):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, fn in fns.items():
            out[k].append(group_ms(fn, calls))
    return out


def summary(ms):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / med, 4)}


def stages(fn, reps):
    """mean ms per call of every stage of the library's timing table over reps calls"""
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
        if n.value and name.value.decode() in STAGES:
            res[name.value.decode()] = round(ms.value / reps, 4)
    ctx.lib.dctae_timing_reset(ctx.h)
    return res


def workload(fe, pn, lfq, imgs, per_of_n, dtypes):
    ((dp, codes),) = fe.encode_batch(imgs, pn, lfq, codes_dtype=torch.int16)
    ids_h, kp_h = dp.batched_image_ids.cpu(), dp.key_pad_mask.cpu()
    n_img = len(dp.original_sizes)
    counts = [int(((ids_h[r] == lid) & ~kp_h[r]).sum()) for r, lid in progressive._places(ids_h.long())]   # n_i
    per = [per_of_n(n) for n in counts]
    L = len(per[0])
    assert all(len(p) == L for p in per) and len(counts) == n_img
    # the loop's masked batches: position j cuts every image at its j-th prefix
    _, cuts = progressive.frame_cuts(ids_h, kp_h, per)
    masked = []
    for j in range(L):
        m = dp.shallow_copy()
        m.key_pad_mask = progressive.prefix_key_pad(ids_h, kp_h, [cuts[i * L + j] for i in range(n_img)]).to(dev)
        masked.append(m)
    res = {"images": n_img, "frames": n_img * L, "repeats": args.repeats}
    frame_values = sum(3 * h * w for h, w in dp.original_sizes) * L
    for dtype in dtypes:
        tag = "u8" if dtype == U8 else "f32"
        new = lambda: fe.decode_prefixes(dp, codes, pn, lfq, per, output_dtype=dtype)              # noqa: E731
        loop = lambda: [fe.decode_batch(m, codes, pn, lfq, output_dtype=dtype) for m in masked]  # noqa: E731
        got, want = new(), loop()
        torch.cuda.synchronize()
        for i in range(n_img):
            for j in range(L):
                assert torch.equal(got[i][j], want[j][i]), "a frame differs from the masked decode"
        ms = interleaved({"new": new, "loop": loop}, 3)
        r = {"new": summary(ms["new"]), "loop": summary(ms["loop"]),
             "new_over_loop": round(statistics.median(ms["new"]) / statistics.median(ms["loop"]), 4)}
        clipped = lambda: fe.decode_prefixes(dp, codes, pn, lfq, per, output_dtype=dtype, clip="minmax")  # noqa: E731
        clipped()
        r["stages_ms"] = st = stages(clipped, 5)
        px = 1 if dtype == U8 else 4
        for k, nbytes in (("clip_minmax", 4 * frame_values), ("clip_store", (4 + px) * frame_values)):
            r[f"{k}_MB"] = round(nbytes / 1e6, 2)
            r[f"{k}_TBps"] = round(nbytes / (st[k] * 1e-3) / 1e12, 3)
            r[f"{k}_of_achievable"] = round(r[f"{k}_TBps"] / HBM_TBPS, 3)
        r["new_not_slower"] = bool(r["new"]["median_ms"] <= r["loop"]["median_ms"])
        res[tag] = r
    return res


def main():
    fe, pn, lfq = models()
    res = {"device": torch.cuda.get_device_name(dev), "quick": args.quick}
    step = 6 if args.quick else 1
    x = _ops.synth_images(1, 512, 512, seed=7, device=dev)
    res["one512"] = workload(fe, pn, lfq, [x[0]], lambda n: list(range(64, n + 1, 64))[step - 1::step], (F32, U8))
    hw = np.random.default_rng(11).integers(100, 449, size=(16, 2))
    imgs = [_ops.synth_images(1, int(h), int(w), seed=11, first_index=i, device=dev)[0] for i, (h, w) in enumerate(hw)]
    eighths = range(8, 0, -6) if args.quick else range(1, 9)
    res["ragged16"] = workload(fe, pn, lfq, imgs, lambda n: [max(1, n * j // 8) for j in sorted(eighths)], (F32,))
    print(json.dumps(res))
    slower = [f"{k}/{t}" for k in ("one512", "ragged16") for t in ("f32", "u8")
              if t in res[k] and not res[k][t]["new_not_slower"]]
    if slower:
        print(f"decode_prefixes slower than the loop of masked decodes on: {', '.join(slower)}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
