"""Golden vectors for the progressive decode, produced by running the
REFERENCE's own ``util.image_clip`` and ``DCTAutoencoderFeatureExtractor.postprocess``
in the build container (refload.py).

    python tests/golden/gen_progressive_golden.py   ->  tests/golden/progressive_ref.npz

  clip<i>_in / clip<i>_out   the reference's image_clip on small fp32 arrays
                             (values below 0 and above 1; the last one constant:
                             all NaN).  The numpy mirror the GPU test compares
                             with must equal these bit for bit.
  im<j>_*                    a one-image batch (sizes in SIZES, FE 3, 14, 0.0, 4, 4, 48):
                             patches, key_pad_mask, batched_image_ids,
                             patch_channels, patch_positions, patch_size,
                             original_size, the prefixes ``im<j>_prefixes`` and per
                             prefix i ``im<j>_rgb<i>``: the reference's postprocess of
                             the batch sliced ``[:, :i]`` as decode_gif.py:60-77
                             slices it.

The generator asserts, for every prefix, that the reference's postprocess of the
batch MASKED instead of sliced (key_pad_mask set on the slots from i on) gives
the same pixels bit for bit: the masking definition of a prefix frame is the
reference's slicing.  tests/test_progressive_host.py checks oracle/ref_cpu.py's
postprocess of the masked batches against these pixels.

The archive is written with fixed member timestamps: rerunning the generator
reproduces it byte for byte.  Data only; no reference source is stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import refload  # noqa: E402
from gen_patch_sizes_golden import save_npz  # noqa: E402
from oracle import rng as orng  # noqa: E402

SIZES = [(28, 42), (56, 56)]
FE_ARGS = (3, 14, 0.0, 4, 4, 48)
CLIP_SHAPES = [(3, 1, 1), (3, 5, 7), (3, 14, 14), (3, 31, 17)]


def clip_inputs():
    g = np.random.default_rng(77)
    xs = [(g.standard_normal(s) * 1.5 + 0.4).astype(np.float32) for s in CLIP_SHAPES]
    xs.append(np.full((3, 4, 4), 0.37, dtype=np.float32))
    return xs


def main():
    ref = refload.load()
    torch.set_num_threads(8)
    out = {}
    for i, x in enumerate(clip_inputs()):
        out[f"clip{i}_in"] = x
        out[f"clip{i}_out"] = ref.util.image_clip(torch.from_numpy(x)).numpy()
        assert out[f"clip{i}_out"].dtype == np.float32
    assert np.isnan(out[f"clip{len(CLIP_SHAPES)}_out"]).all()
    proc = ref.fe.DCTAutoencoderFeatureExtractor(*FE_ARGS)
    fields = ("patches", "key_pad_mask", "batched_image_ids", "patch_channels", "patch_positions")
    for j, (x,) in enumerate(orng.synth_images(4242 + j, [s]) for j, s in enumerate(SIZES)):
        it = proc.preprocess(torch.from_numpy(x))
        (batch,) = list(proc.iter_batches(iter([{k: [v] for k, v in it.items()}]), None))
        n = int((~batch.key_pad_mask).sum())
        assert batch.key_pad_mask.shape[0] == 1 and not bool(batch.key_pad_mask[0, :n].any())
        pre = f"im{j}_"
        for f in fields:
            out[pre + f] = getattr(batch, f).numpy()
        out[pre + "patch_size"] = np.array(batch.patch_sizes[0], dtype=np.int32)
        out[pre + "original_size"] = np.array(batch.original_sizes[0], dtype=np.int32)
        prefixes = [1, 2, 3, n // 2, n - 1, n]
        out[pre + "prefixes"] = np.array(prefixes, dtype=np.int32)
        for i in prefixes:
            sliced = batch.shallow_copy()
            for f in fields:
                setattr(sliced, f, getattr(batch, f)[:, :i])
            sliced.attn_mask = None
            masked = batch.shallow_copy()
            masked.key_pad_mask = batch.key_pad_mask.clone()
            masked.key_pad_mask[:, i:] = True
            with torch.no_grad():
                (a,) = proc.postprocess(sliced)
                (b,) = proc.postprocess(masked)
            assert a.dtype == torch.float32 and torch.equal(a, b), (j, i)
            out[f"{pre}rgb{i}"] = a.numpy()
    path = os.path.join(HERE, "progressive_ref.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
