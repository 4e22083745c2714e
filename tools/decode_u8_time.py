"""Time the decode to uint8 images against the decode to fp32 images, in one
process on one GPU, inputs resident:
  sq512_codes  BatchDecoder, 1024 x 512 x 512, from LFQ codes
  sq512_proj   BatchDecoder, 1024 x 512 x 512, LFQ with projections
               (project_out, then dctae_decode_normed)
  config4      _ops.decode from codes on bench.py's config-4 set (1024 ragged
               images, (H, W) ~ U{14..1024}^2, seed 7), the image tables built
               beforehand
Per workload: the call time by events after warm-up, the fp32 and the byte
timings interleaved (one timed group of each per repeat, so clock and thermal
drift hit both alike), median / min / max over the repeats; the stages that
write the caller's images (idct_rows on the FFT path, ipt_to_rgb on the GEMM
path) from the library's timing table for either output type; torch's
`clamp(0, 1).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)` chain alone on
the fp32 output, which the byte call makes unnecessary; and, on the 512 x 512
workloads, the bytes per image the row kernel moves (U' read, RGB written) and
its achieved rate on them.  The byte output is checked equal to the quantised
fp32 output before anything is timed.  Exit status 1, with a line on stderr,
if on any workload the byte call's median exceeds the fp32 call's median plus
the fp32 call's own max - min over the repeats.  Prints one JSON line.

    python tools/decode_u8_time.py [--repeats 7] [--quick]
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
OUT_STAGES = ("idct_rows", "ipt_to_rgb")
U8 = torch.uint8


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


def quantise(x):
    """torch's chain on the device (save_image's; the inner clamp does not change the result)"""
    return x.clamp(0, 1).mul(255).add_(0.5).clamp_(0, 255).to(U8)


def quantise_cpu(x):
    return x.cpu().mul(255).add(0.5).clamp(0, 255).to(U8)


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
    """mean ms per call of the stages that write the images (and the whole table's sum) over reps calls"""
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
        if name.value.decode() in OUT_STAGES and n.value:
            res[name.value.decode()] = round(ms.value / reps, 4)
    ctx.lib.dctae_timing_reset(ctx.h)
    res["all_stages"] = round(total, 4)
    return res


def report(f32_call, u8_call, chain, calls, n_img, rows512):
    ms = interleaved({"f32": f32_call, "u8": u8_call, "torch_chain": chain}, calls)
    r = {"images": n_img, "calls_per_group": calls, "repeats": args.repeats,
         "f32": summary(ms["f32"]), "u8": summary(ms["u8"]), "torch_chain": summary(ms["torch_chain"]),
         "u8_over_f32": round(statistics.median(ms["u8"]) / statistics.median(ms["f32"]), 4),
         "stages_f32_ms": stages(f32_call, 3), "stages_u8_ms": stages(u8_call, 3)}
    if rows512:   # k_idct_rows512: U' (3 x 512 x 448 fp32) read, 3 x 512 x 512 pixels written
        for k, px in (("f32", 4), ("u8", 1)):
            mb = (3 * 512 * 448 * 4 + 3 * 512 * 512 * px) / 1e6
            r[f"idct_rows_MB_per_image_{k}"] = round(mb, 3)
            r[f"idct_rows_TBps_{k}"] = round(mb * 1e6 * n_img / (r[f"stages_{k}_ms"]["idct_rows"] * 1e-3) / 1e12, 3)
    # what has to hold: the byte call's median within the fp32 call's own in-process spread of the fp32 median
    f = r["f32"]
    r["u8_not_slower"] = bool(r["u8"]["median_ms"] <= f["median_ms"] + (f["max_ms"] - f["min_ms"]))
    return r


def main():
    fe, pn, lfq, lfq_p = models()
    div = 8 if args.quick else 1
    res = {"device": torch.cuda.get_device_name(dev), "quick": args.quick}
    B = 1024 // div
    x = _ops.synth_images(B, 512, 512, seed=7, device=dev)
    for name, q in (("sq512_codes", lfq), ("sq512_proj", lfq_p)):
        enc = fe_mod.BatchEncoder(fe, B, 512, 512, pn, q, device=dev)
        packed = {k: v.clone() for k, v in enc(x).items()}
        df, d8 = fe_mod.BatchDecoder(enc, pn, q), fe_mod.BatchDecoder(enc, pn, q, output_dtype=U8)
        want, got = df(packed), d8(packed)
        torch.cuda.synchronize()
        assert torch.equal(got[:8].cpu(), quantise_cpu(want[:8])), "byte output != quantised fp32 output"
        res[name] = report(lambda: df(packed), lambda: d8(packed), lambda: quantise(df.out), 10, B, True)
        del enc, packed, df, d8, want, got
        torch.cuda.empty_cache()
    del x
    hw = np.random.default_rng(7).integers(14, 1025, size=(1024, 2))[:1024 // div]
    imgs = [_ops.synth_images(1, int(h), int(w), seed=7, first_index=i, device=dev)[0] for i, (h, w) in enumerate(hw)]
    batches = []
    for dp, codes in fe.encode_batch(imgs, pn, lfq):
        p = fe.params(dp.key_pad_mask.shape[1])
        a = (p, dp.batched_image_ids, dp.key_pad_mask, dp.patch_positions, dp.patch_channels, dp.patch_sizes,
             dp.original_sizes)
        batches.append((a, dict(codes=codes, norm=pn.state(), lfq=lfq.cfg(), table=_ops.decode_table(*a))))
    del imgs
    torch.cuda.empty_cache()
    state = {}

    def dec(dtype):
        state[dtype] = [_ops.decode(*a, return_flat=True, out_dtype=dtype, **kw)[1] for a, kw in batches]

    dec(torch.float32)
    dec(U8)
    torch.cuda.synchronize()
    for f, g in zip(state[torch.float32], state[U8]):
        assert torch.equal(g[:1 << 22].cpu(), quantise_cpu(f[:1 << 22])), "byte output != quantised fp32 output"
    flats = state[torch.float32]
    res["config4"] = report(lambda: dec(torch.float32), lambda: dec(U8), lambda: [quantise(f) for f in flats], 3,
                            len(hw), False)
    print(json.dumps(res))
    slower = [k for k in ("sq512_codes", "sq512_proj", "config4") if not res[k]["u8_not_slower"]]
    if slower:
        print(f"byte decode slower than the fp32 decode on: {', '.join(slower)}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
