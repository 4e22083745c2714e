"""Time the progressive decode through the transformer
(fe.model_decode_prefixes: the model prefix frames of a batch in one pass of the
decoder per chunk, variable-length attention) against the way the same frames
were obtained before it: the loop of decode_gif.py, one
model.decode_from_codes + fe.postprocess call per frame on a hand-sliced
one-image row.  patch14-l (hidden 1024, 16 heads, 8 + 8 layers, 16 codebooks of
2^13), random init, one process on one GPU, inputs and the loop's sliced rows
resident (the slicing is not timed):
  gif16    16 frames, k = 1 .. 16, of one 512 x 512 image (decode_gif.py's case)
  one512   48 prefixes 64, 128, ..., 3072 of one 512 x 512 image
  ragged16 16 ragged images with the long side at most 448, 8 prefixes each
           (n_i j / 8)
Per workload: the wall time of a call that ends in a device synchronise, the
two ways interleaved (one timed group of each per repeat), median / min / max
over the repeats, and the per-kernel split of the new call from the library's
timing table.  The new call's frames are checked equal, bit for bit, to the
loop's before anything is timed.  No ratio is asserted.  Prints one JSON line.

    python tools/model_prefix_time.py [--repeats 7] [--quick]
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
ap.add_argument("--quick", action="store_true", help="fewer prefixes (a functional check of the tool)")
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)


def models():
    torch.manual_seed(0)
    enc = dict(hidden_size=1024, intermediate_size=4096, num_attention_heads=16, num_hidden_layers=8)
    cfg = pkg.DCTAutoencoderConfig(image_channels=3, patch_size=14, max_patch_h=32, max_patch_w=32,
                                   vq_codebook_size=8192, vq_num_codebooks=16, vq_type="lfq",
                                   encoder_config=enc, decoder_config=enc)
    m = pkg.DCTAutoencoder(cfg)
    tabs = np.load(os.path.join(ROOT, "tests", "golden", "patchnorm_ref.npz"))
    with torch.no_grad():
        m.patchnorm.median.copy_(torch.from_numpy(tabs["median"]))
        m.patchnorm.b.copy_(torch.from_numpy(tabs["b"]))
    m.patchnorm.frozen = True
    return pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072), m.to(dev).eval()


def group_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(ms):
    med = statistics.median(ms)
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "spread": round((max(ms) - min(ms)) / med, 4)}


def stages(fn, reps):
    """mean ms and launches per call of every stage of the library's timing table over reps calls"""
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
        if n.value:
            res[name.value.decode()] = {"ms": round(ms.value / reps, 4), "launches": round(n.value / reps, 1)}
    ctx.lib.dctae_timing_reset(ctx.h)
    return res


def workload(fe, model, imgs, per_of_n):
    ((dp, _),) = fe.encode_batch(imgs, model.patchnorm, return_patches=True)
    meta = dp.shallow_copy()
    codes = model.encode(dp.shallow_copy())[1]
    ids_h, kp_h = meta.batched_image_ids.cpu(), meta.key_pad_mask.cpu()
    places = progressive._places(ids_h.long())
    counts = [int(((ids_h[r] == lid) & ~kp_h[r]).sum()) for r, lid in places]
    per = [per_of_n(n) for n in counts]
    rows = []   # the loop's sliced one-image rows
    for i, (r, lid) in enumerate(places):
        real = ((meta.batched_image_ids[r] == lid) & ~meta.key_pad_mask[r]).nonzero().flatten()
        for k in per[i]:
            sel = real[:k]
            m = sel.numel()
            rows.append((codes[r, sel][None].contiguous(), dict(
                key_pad_mask=torch.zeros(1, m, dtype=torch.bool, device=dev),
                batched_image_ids=torch.zeros(1, m, dtype=torch.long, device=dev),
                patch_channels=meta.patch_channels[r, sel][None].contiguous(),
                patch_positions=meta.patch_positions[r, sel][None].contiguous(),
                patch_sizes=[meta.patch_sizes[i]], original_sizes=[meta.original_sizes[i]])))
    new = lambda: fe.model_decode_prefixes(model, meta, codes, per)                                        # noqa: E731
    loop = lambda: [fe.postprocess(model.decode_from_codes(c, do_inv_norm=True, **kw))[0] for c, kw in rows]  # noqa: E731
    got, want = [f for ims in new() for f in ims], loop()
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a frame differs from the sliced call"
    for fn in (new, loop):
        for _ in range(2):
            fn()
    ms = {"new": [], "loop": []}
    for _ in range(args.repeats):
        ms["new"].append(group_ms(new))
        ms["loop"].append(group_ms(loop))
    res = {"images": len(places), "frames": len(rows), "tokens": sum(c.shape[1] for c, _ in rows),
           "repeats": args.repeats, "new": summary(ms["new"]), "loop": summary(ms["loop"])}
    res["loop_over_new"] = round(res["loop"]["median_ms"] / res["new"]["median_ms"], 3)
    res["new_kernels"] = stages(new, 3)
    res["loop_kernels"] = stages(loop, 3)
    return res


def main():
    fe, model = models()
    res = {"device": torch.cuda.get_device_name(dev), "quick": args.quick, "model": "patch14-l, random init"}
    x = _ops.synth_images(1, 512, 512, seed=7, device=dev)
    res["gif16"] = workload(fe, model, [x[0]], lambda n: list(range(1, 5 if args.quick else 17)))
    step = 12 if args.quick else 1
    res["one512"] = workload(fe, model, [x[0]], lambda n: list(range(64, n + 1, 64))[step - 1::step])
    hw = np.random.default_rng(11).integers(100, 449, size=(16, 2))
    imgs = [_ops.synth_images(1, int(h), int(w), seed=11, first_index=i, device=dev)[0] for i, (h, w) in enumerate(hw)]
    eighths = (4, 8) if args.quick else range(1, 9)
    res["ragged16"] = workload(fe, model, imgs, lambda n: [max(1, n * j // 8) for j in eighths])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
