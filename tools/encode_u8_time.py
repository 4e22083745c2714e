"""Time the encode from uint8 images against the encode from the fp32 images
they mean (u8.float() / 255), in one process on one GPU, both inputs resident:
  sq512    BatchEncoder, 1024 x 512 x 512
  sq224    BatchEncoder, 256 x 224 x 224
  config4  encode_batch on bench.py's config-4 set (1024 ragged images,
           (H, W) ~ U{14..1024}^2, seed 7; the bytes drawn with the same seed),
           host planning and packing included
Per workload: the call time by events after warm-up, the fp32 and the byte
timings interleaved (one timed group of each per repeat, so clock and thermal
drift hit both alike), median / min / max over the repeats; the row-pass
stages (fft_rows, rows_fused, rgb_to_ipt, ...) from the library's timing table
for either input; and the torch `x.float().div(255)` that the byte path makes
unnecessary.  Exit status 1, with a line on stderr, if the byte call is slower
than the fp32 call on any workload by more than the spread over the repeats.  The resident fp32 images are the exact ones (dctae_u8_to_f32:
fp32 division; torch's GPU division by a scalar multiplies by the reciprocal
and is an ulp off for about half of the byte values), so the two calls'
outputs are checked equal before they are timed.  Also the pixel bytes read
per image.  Prints one JSON line.

    python tools/encode_u8_time.py [--repeats 7] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload  # noqa: E402

pkg = _pkgload.load()
from dct_autoencoder_amd import _lib, _ops, feature_extraction as fe_mod  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--quick", action="store_true", help="an eighth of every batch (a functional check of the tool)")
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
ROW_STAGES = ("fft_rows", "rows_fused", "rows_fixup", "rgb_to_ipt", "gemm_rows", "bs_rows")


def models():
    tabs = np.load(os.path.join(ROOT, "tests", "golden", "patchnorm_ref.npz"))
    pn = pkg.PatchNorm(32, 32, 14, 3).to(dev)
    pn.median.data.copy_(torch.from_numpy(tabs["median"]))
    pn.b.data.copy_(torch.from_numpy(tabs["b"]))
    pn.frozen = True
    lfq = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).to(dev).eval()
    return pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072), pn.eval(), lfq


def group_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def interleaved(fns, calls, warm=3):
    """{name: [ms per call, one per repeat]}: per repeat one timed group of every fn, in turn"""
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


def stages(fn, reps):
    """mean ms per call of the row-pass stages (and the whole table's sum) over reps calls"""
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
    res, total = {}, 0.0
    for i in range(256):
        name, ms, n = C.c_char_p(), C.c_double(), C.c_int64()
        if ctx.lib.dctae_timing_get(ctx.h, i, C.byref(name), C.byref(ms), C.byref(n)) != 0:
            break
        total += ms.value / reps
        if name.value.decode() in ROW_STAGES and n.value:
            res[name.value.decode()] = round(ms.value / reps, 4)
    ctx.lib.dctae_timing_reset(ctx.h)
    res["all_stages"] = round(total, 4)
    return res


def report(name, f32_call, u8_call, convert, calls, n_img, pixels):
    ms = interleaved({"f32": f32_call, "u8": u8_call, "torch_div255": convert}, calls)
    r = {"images": n_img, "calls_per_group": calls, "repeats": args.repeats,
         "f32": summary(ms["f32"]), "u8": summary(ms["u8"]), "torch_div255": summary(ms["torch_div255"]),
         "u8_over_f32": round(statistics.median(ms["u8"]) / statistics.median(ms["f32"]), 4),
         "stages_f32_ms": stages(f32_call, 3), "stages_u8_ms": stages(u8_call, 3),
         "rgb_MB_per_image_f32": round(12 * pixels / n_img / 1e6, 3),
         "rgb_MB_per_image_u8": round(3 * pixels / n_img / 1e6, 3)}
    # what has to hold: the byte call is not slower than the fp32 call beyond the run-to-run spread seen here
    slack = max(r["f32"]["spread"], r["u8"]["spread"])
    r["u8_not_slower"] = bool(r["u8"]["median_ms"] <= r["f32"]["median_ms"] * (1 + slack))
    return name, r


def main():
    fe, pn, lfq = models()
    div = 8 if args.quick else 1
    res = {"device": torch.cuda.get_device_name(dev), "quick": args.quick}
    gen = torch.Generator(device=dev).manual_seed(7)
    for name, B, H, calls in (("sq512", 1024 // div, 512, 10), ("sq224", 256 // div, 224, 50)):
        u8 = torch.randint(0, 256, (B, 3, H, H), dtype=torch.uint8, device=dev, generator=gen)
        f32 = _ops.u8_to_f32(u8)
        ef = fe_mod.BatchEncoder(fe, B, H, H, pn, lfq, device=dev)
        e8 = fe_mod.BatchEncoder(fe, B, H, H, pn, lfq, device=dev, input_dtype=torch.uint8)
        a = {k: v.clone() for k, v in e8(u8).items()}
        b = ef(f32)
        assert all(torch.equal(a[k], b[k]) for k in a), "byte and fp32 outputs differ"
        k, r = report(name, lambda: ef(f32), lambda: e8(u8), lambda: u8.float().div(255), calls, B, B * H * H)
        res[k] = r
        del u8, f32, ef, e8, a, b
        torch.cuda.empty_cache()
    hw = np.random.default_rng(7).integers(14, 1025, size=(1024, 2))[:1024 // div]
    imgs8 = [torch.randint(0, 256, (3, int(h), int(w)), dtype=torch.uint8, device=dev, generator=gen) for h, w in hw]
    imgsf = [_ops.u8_to_f32(u) for u in imgs8]
    oa, ob = fe.encode_batch(imgs8, pn, lfq, uint8_images=True), fe.encode_batch(imgsf, pn, lfq)
    assert len(oa) == len(ob) and all(torch.equal(ca, cb) and torch.equal(da.patch_positions, db.patch_positions)
                                      for (da, ca), (db, cb) in zip(oa, ob)), "byte and fp32 outputs differ"
    del oa, ob
    k, r = report("config4", lambda: fe.encode_batch(imgsf, pn, lfq),
                  lambda: fe.encode_batch(imgs8, pn, lfq, uint8_images=True),
                  lambda: [u.float().div(255) for u in imgs8], 3, len(imgs8), int((hw[:, 0] * hw[:, 1]).sum()))
    res[k] = r
    print(json.dumps(res))
    # what has to hold: the byte call not slower than the fp32 call, beyond the spread seen in this process
    slower = [k for k in ("sq512", "sq224", "config4") if not res[k]["u8_not_slower"]]
    if slower:
        print(f"byte call slower than the fp32 call on: {', '.join(slower)}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
