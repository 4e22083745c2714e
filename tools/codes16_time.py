"""Time the encode and the decode with int16 codes against int64 codes
(include/dctae_codes16.h), in one process on one GPU, both code types resident:
  enc512_f32 / enc512_u8   BatchEncoder, 1024 x 512 x 512, from fp32 / uint8 images
  enc224                   BatchEncoder, 256 x 224 x 224
  enc512_proj              BatchEncoder, 1024 x 512 x 512, LFQ 196 -> 16 x 13 projections
  dec512_f32 / dec512_u8   BatchDecoder, 1024 x 512 x 512 from codes, to fp32 / uint8 images
  dec512_proj_f32 / _u8    the same with the 16 x 13 projections
  config4                  encode_batch on bench.py's config-4 set (1024 ragged images,
                           (H, W) ~ U{14..1024}^2, seed 7), host planning and packing included
  d2h512                   the codes tensor of 1024 x 512^2 copied into pinned host memory
Per workload: the call time by events after warm-up, the int64 and the int16
timings interleaved (one timed group of each per repeat, so clock and thermal
drift hit both alike), median / min / max over the repeats; for every
BatchEncoder the `sort_pack` stage from the library's timing table and for every
BatchDecoder `idct_cols`; the bytes of the codes tensor.  The two calls' outputs
are checked equal (the int16 codes after .long()) before they are timed.
Exit status 1, with a line on stderr, if an int16 call is slower than its
int64 call by more than the spread over the repeats.  Prints one JSON line.

    python tools/codes16_time.py [--repeats 7] [--quick]
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
from dct_autoencoder_amd import _lib, feature_extraction as fe_mod  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--quick", action="store_true", help="an eighth of every batch (a functional check of the tool)")
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
I16, I64, U8 = torch.int16, torch.int64, torch.uint8


def models():
    tabs = np.load(os.path.join(ROOT, "tests", "golden", "patchnorm_ref.npz"))
    pn = pkg.PatchNorm(32, 32, 14, 3).to(dev)
    pn.median.data.copy_(torch.from_numpy(tabs["median"]))
    pn.b.data.copy_(torch.from_numpy(tabs["b"]))
    pn.frozen = True
    lfq = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).to(dev).eval()
    torch.manual_seed(5)
    lfq_p = pkg.LFQ(dim=196, codebook_size=2 ** 13, num_codebooks=16).to(dev).eval()
    return pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072), pn.eval(), lfq, lfq_p


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


def stage_ms(fn, stage, reps=3):
    """mean ms per call of one stage of the library's timing table over reps calls"""
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
        if name.value.decode() == stage and n.value:
            got = round(ms.value / reps, 4)
    ctx.lib.dctae_timing_reset(ctx.h)
    return got


def report(call64, call16, calls, stage=None, code_elems=0):
    ms = interleaved({"int64": call64, "int16": call16}, calls)
    r = {"calls_per_group": calls, "repeats": args.repeats, "int64": summary(ms["int64"]),
         "int16": summary(ms["int16"]),
         "int16_over_int64": round(statistics.median(ms["int16"]) / statistics.median(ms["int64"]), 4)}
    if stage:
        r[stage + "_ms"] = {"int64": stage_ms(call64, stage), "int16": stage_ms(call16, stage)}
    if code_elems:
        r["codes_MB"] = {"int64": round(8 * code_elems / 1e6, 2), "int16": round(2 * code_elems / 1e6, 2)}
    # what has to hold: the int16 call is not slower than the int64 call beyond the run-to-run spread seen here
    slack = max(r["int64"]["spread"], r["int16"]["spread"])
    r["int16_not_slower"] = bool(r["int16"]["median_ms"] <= r["int64"]["median_ms"] * (1 + slack))
    return r


def encoders(fe, pn, lfq, x, **kw):
    """the int64 and the int16 BatchEncoder on x, outputs checked equal"""
    B, _, H, W = x.shape
    e64 = fe_mod.BatchEncoder(fe, B, H, W, pn, lfq, device=dev, **kw)
    e16 = fe_mod.BatchEncoder(fe, B, H, W, pn, lfq, device=dev, codes_dtype=I16, **kw)
    a, b = e64(x), e16(x)
    torch.cuda.synchronize()
    assert b["codes"].dtype == I16 and torch.equal(b["codes"].long(), a["codes"]), "int16 and int64 codes differ"
    assert all(torch.equal(a[k], b[k]) for k in a if k != "codes"), "int16 and int64 outputs differ"
    return e64, e16


def decoders(enc, pn, lfq, packed64, packed16, out_dtype):
    d64 = fe_mod.BatchDecoder(enc, pn, lfq, output_dtype=out_dtype)
    d16 = fe_mod.BatchDecoder(enc, pn, lfq, output_dtype=out_dtype)
    a, b = d64(packed64), d16(packed16)
    torch.cuda.synchronize()
    assert torch.equal(a, b), "images from int16 and from int64 codes differ"
    return d64, d16


def main():
    fe, pn, lfq, lfq_p = models()
    div = 8 if args.quick else 1
    res = {"device": torch.cuda.get_device_name(dev), "quick": args.quick}
    gen = torch.Generator(device=dev).manual_seed(7)
    B = 1024 // div
    u8 = torch.randint(0, 256, (B, 3, 512, 512), dtype=U8, device=dev, generator=gen)
    f32 = u8.float().div(255)
    n_codes = B * 3072 * 14

    # ---- encode 512^2
    e64, e16 = encoders(fe, pn, lfq, f32)
    res["enc512_f32"] = report(lambda: e64(f32), lambda: e16(f32), 10, "sort_pack", n_codes)
    packed64 = {k: v.clone() for k, v in e64(f32).items()}
    packed16 = dict(packed64, codes=e16(f32)["codes"].clone())
    b64, b16 = encoders(fe, pn, lfq, u8, input_dtype=U8)
    res["enc512_u8"] = report(lambda: b64(u8), lambda: b16(u8), 10, "sort_pack", n_codes)
    del b64, b16

    # ---- device-to-host copy of the codes into pinned memory
    h64 = torch.empty(packed64["codes"].shape, dtype=I64, pin_memory=True)
    h16 = torch.empty(packed16["codes"].shape, dtype=I16, pin_memory=True)
    res["d2h512"] = report(lambda: h64.copy_(packed64["codes"], non_blocking=True),
                           lambda: h16.copy_(packed16["codes"], non_blocking=True), 5, None, n_codes)
    del h64, h16

    # ---- decode 512^2 from codes
    for name, dt in (("dec512_f32", torch.float32), ("dec512_u8", U8)):
        d64, d16 = decoders(e64, pn, lfq, packed64, packed16, dt)
        res[name] = report(lambda: d64(packed64), lambda: d16(packed16), 10, "idct_cols", n_codes)
        del d64, d16
    del e64, e16, packed64, packed16
    torch.cuda.empty_cache()

    # ---- 512^2 with the 16 x 13 projections
    p64, p16 = encoders(fe, pn, lfq_p, f32)
    assert p16.proj_staged
    res["enc512_proj"] = report(lambda: p64(f32), lambda: p16(f32), 10, "sort_pack", B * 3072 * 16)
    packed64 = {k: v.clone() for k, v in p64(f32).items()}
    packed16 = dict(packed64, codes=p16(f32)["codes"].clone())
    for name, dt in (("dec512_proj_f32", torch.float32), ("dec512_proj_u8", U8)):
        d64, d16 = decoders(p64, pn, lfq_p, packed64, packed16, dt)
        res[name] = report(lambda: d64(packed64), lambda: d16(packed16), 10, "lfq_project_out", B * 3072 * 16)
        del d64, d16
    del p64, p16, packed64, packed16, u8, f32
    torch.cuda.empty_cache()

    # ---- encode 224^2
    B2 = 256 // div
    x = torch.rand((B2, 3, 224, 224), device=dev, generator=gen)
    s64, s16 = encoders(fe, pn, lfq, x)
    res["enc224"] = report(lambda: s64(x), lambda: s16(x), 50, "sort_pack", s64.n_rows * 3072 * 14)
    del s64, s16, x

    # ---- encode_batch on the config-4 set
    hw = np.random.default_rng(7).integers(14, 1025, size=(1024, 2))[:1024 // div]
    imgs = [torch.rand((3, int(h), int(w)), device=dev, generator=gen) for h, w in hw]
    oa, ob = fe.encode_batch(imgs, pn, lfq), fe.encode_batch(imgs, pn, lfq, codes_dtype=I16)
    assert len(oa) == len(ob) and all(torch.equal(ca, cb.long()) and torch.equal(da.patch_positions, db.patch_positions)
                                      for (da, ca), (db, cb) in zip(oa, ob)), "int16 and int64 outputs differ"
    n4 = sum(c.numel() for _, c in oa)
    del oa, ob
    res["config4"] = report(lambda: fe.encode_batch(imgs, pn, lfq),
                            lambda: fe.encode_batch(imgs, pn, lfq, codes_dtype=I16), 3, None, n4)
    print(json.dumps(res))
    slower = [k for k, v in res.items() if isinstance(v, dict) and not v["int16_not_slower"]]
    if slower:
        print(f"int16 call slower than the int64 call on: {', '.join(slower)}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
