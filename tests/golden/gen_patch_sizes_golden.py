"""Golden vectors for patch sizes other than 14, produced by running the
REFERENCE's own DCTAutoencoderFeatureExtractor.preprocess / iter_batches,
PatchNorm (eval) and LFQ.forward (eval) in the build container (refload.py).

    python tests/golden/gen_patch_sizes_golden.py   ->  tests/golden/patch_sizes_ref.npz

Configurations: CASES below (patch sizes 16, 15, 8, 7, 5, 2, 1; the table of
tests/test_gpu_patch_sizes.py, stored in the archive as ``cases`` /
``case<i>_sizes`` / ``case<i>_cds`` for tests/test_patch_sizes_host.py).
Images are oracle/rng.py's synth_images(100 + P, sizes) and the PatchNorm
tables come from torch.Generator().manual_seed(P), so only outputs are stored:

  per configuration p<P>_   key_pad_mask, batched_image_ids, patch_positions,
                            patch_channels of the packed batch; codes_cd<cd> in
                            full for the first LFQ grouping, codes_cd<cd>_sha
                            (SHA-256 of the int64 codes) for every grouping
  per image p<P>_img<i>_    positions, channels, scores (the reference's own
                            importance scores, captured from its sort call, in
                            emitted order), original_size, patch_size,
                            patches_sha, patches_head / patches_tail (8 tokens)
                            and patches in full for small images

The archive is written with fixed member timestamps: rerunning the generator
reproduces it byte for byte.  Data only; no reference source is stored.
"""
import hashlib
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import refload  # noqa: E402
from oracle import rng as orng  # noqa: E402

# (P, max_patch_h, max_patch_w, image sizes (H, W), LFQ groupings codebook_dim); max_seq_len = 3 mh mw
CASES = [
    (16, 32, 32, [(512, 512), (224, 224), (100, 77), (16, 16), (33, 500)], [16, 8, 1]),
    (15, 32, 32, [(512, 300), (225, 105), (15, 15), (47, 31), (300, 512)], [15, 9, 5]),
    (8, 32, 32, [(224, 224), (97, 64), (8, 8), (30, 300)], [8, 16, 4]),
    (7, 32, 32, [(224, 98), (21, 35), (7, 7), (100, 77), (225, 105)], [7, 1]),
    (5, 6, 9, [(16, 27), (5, 5), (37, 53), (64, 97)], [5]),
    (2, 40, 40, [(97, 64), (2, 2), (7, 12), (80, 80)], [2, 4, 1]),
    (1, 8, 8, [(4, 6), (1, 1), (9, 9), (3, 16)], [1]),
]
FULL_TOKENS_MAX_ELEMS = 8192   # token arrays of at most this many elements are stored in full


def tables(P, mh, mw):
    g = torch.Generator().manual_seed(P)
    median = torch.randn(3, mh, mw, P * P, generator=g) * 0.05
    b = torch.rand(3, mh, mw, P * P, generator=g) * 0.1 + 0.01
    return median, b, torch.ones(3, mh, mw)


def sha(a: np.ndarray) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (reproducible bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


class _SortSpy:
    """Records the tensor of every descending Tensor.sort call: the reference's
    importance scores are local to its _patch_image (sorted at its line 418)."""

    def __enter__(self):
        self.seen = []
        self._orig = torch.Tensor.sort
        spy = self

        def sort(t, *a, **k):
            if k.get("descending"):
                spy.seen.append(t.detach().clone())
            return spy._orig(t, *a, **k)

        torch.Tensor.sort = sort
        return self

    def __exit__(self, *exc):
        torch.Tensor.sort = self._orig


def main():
    ref = refload.load()
    FE = ref.fe.DCTAutoencoderFeatureExtractor
    torch.set_num_threads(8)
    out = {"cases": np.array([(P, mh, mw) for P, mh, mw, _, _ in CASES], dtype=np.int32)}
    for ci, (P, mh, mw, sizes, cds) in enumerate(CASES):
        out[f"case{ci}_sizes"] = np.array(sizes, dtype=np.int32)
        out[f"case{ci}_cds"] = np.array(cds, dtype=np.int32)
        S = 3 * mh * mw
        pre = f"p{P}_"
        proc = FE(3, P, 0.0, mh, mw, S)
        median, b, n = tables(P, mh, mw)
        pn = ref.patchnorm.PatchNorm(mh, mw, P, 3)
        pn.median.data.copy_(median)
        pn.b.data.copy_(b)
        pn.n.data.copy_(n)
        pn.frozen = True
        pn.eval()
        items = []
        for i, x in enumerate(orng.synth_images(100 + P, sizes)):
            with _SortSpy() as spy:
                it = proc.preprocess(torch.from_numpy(x))
            (scores,) = spy.seen
            pt = it["patches"].numpy()
            ranked = scores.sort(descending=True, stable=True).values   # values only: the token order is the reference's
            assert len(ranked) == pt.shape[0]
            ip = f"{pre}img{i}_"
            out[ip + "positions"] = it["positions"].numpy().astype(np.int16)
            out[ip + "channels"] = it["channels"].numpy().astype(np.int8)
            out[ip + "scores"] = ranked.numpy().astype(np.float32)
            out[ip + "original_size"] = np.array(it["original_sizes"], dtype=np.int32)
            out[ip + "patch_size"] = np.array(it["patch_sizes"], dtype=np.int32)
            out[ip + "patches_sha"] = sha(pt)
            out[ip + "patches_head"] = pt[:8]
            out[ip + "patches_tail"] = pt[-8:]
            if pt.size <= FULL_TOKENS_MAX_ELEMS:
                out[ip + "patches"] = pt
            items.append(it)
        (batch,) = list(proc.iter_batches(iter([{k: [it[k] for it in items] for k in items[0]}]), None))
        out[pre + "key_pad_mask"] = batch.key_pad_mask.numpy()
        out[pre + "batched_image_ids"] = batch.batched_image_ids.numpy().astype(np.int16)
        out[pre + "patch_positions"] = batch.patch_positions.numpy().astype(np.int16)
        out[pre + "patch_channels"] = batch.patch_channels.numpy().astype(np.int8)
        with torch.no_grad():
            y = pn(batch.shallow_copy())
        for j, cd in enumerate(cds):
            lfq = ref.lfq.LFQ(dim=P * P, codebook_size=2 ** cd, num_codebooks=P * P // cd).eval()
            with torch.no_grad():
                _, idx, _, _ = lfq(y, mask=~batch.key_pad_mask)
            idx = idx.numpy().astype(np.int64)
            assert idx.min() >= 0 and idx.max() < 2 ** cd
            out[f"{pre}codes_cd{cd}_sha"] = sha(idx)
            if j == 0:
                out[f"{pre}codes_cd{cd}"] = idx.astype(np.uint16 if cd > 8 else np.uint8)
    path = os.path.join(HERE, "patch_sizes_ref.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
