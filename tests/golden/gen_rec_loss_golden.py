"""Golden vectors for the reconstruction terms of the reference's training step
(reference main.py:71, 79-83), produced by running the REFERENCE's own
PatchNorm.inverse_norm (patchnorm.py:167-177), F.l1_loss on the boolean-indexed
patches, autograd and calculate_perplexity in the build container (refload.py).

    python tests/golden/gen_rec_loss_golden.py   ->  tests/golden/rec_loss_ref.npz

The PatchNorm tables are not stored: every case uses the (3, 32, 32, 196)
tables of patchnorm_ref.npz with their last axis cropped or tiled to the case's
PP = patch_size ** 2 (``tables`` below; the tests restate that one line).

Per case (key prefix = the case name): the inputs ``out`` (the model's output),
``tn`` (the normalized target), ``raw`` (the raw target), ``ch``, ``pos``,
``key_pad`` and ``codes``; then, from the reference in fp32 (suffix ``_f32``)
and from the same classes with the module ``.double()`` and float64 inputs
(suffix ``_f64``): ``rec`` and ``unn`` (rec_loss, rec_loss_unnormalized) and
``grad``, the gradient of 0.1 rec + 1.0 unn with respect to ``out``; and
``perplexity`` of ``codes[mask]``.  out = tn + noise with some elements set
exactly equal to tn (sign(0) in d1); raw = the fp32 inverse of tn plus noise,
with some elements set exactly to the fp32 inverse of out (sign(0) in d2).
Data only; no reference source is stored.
"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import refload  # noqa: E402

W = (0.1, 1.0)          # the weights of main.py's objective on the two terms
CODEBOOK = (6, 2)       # codebook_dim, num_codebooks of the perplexity's codes
# name, patch size, (rows, tokens), mask kind
CASES = [
    ("p14", 14, (2, 37), "rand"),
    ("p16", 16, (2, 9), "rand"),
    ("p5", 5, (2, 37), "rand"),
    ("p1", 1, (2, 37), "rand"),
    ("one", 5, (2, 37), "single"),
    ("row", 5, (2, 37), "row"),
    ("none", 5, (2, 37), "none"),
    ("many", 2, (3, 700), "rand"),
]


def tables(PP):
    g = np.load(os.path.join(HERE, "patchnorm_ref.npz"))
    idx = np.arange(PP) % g["median"].shape[-1]
    return torch.from_numpy(g["median"][..., idx].copy()), torch.from_numpy(g["b"][..., idx].copy())


def make_mask(kind, b, n, g):
    """True at real tokens"""
    if kind == "none":
        return torch.zeros(b, n, dtype=torch.bool)
    if kind == "single":
        m = torch.zeros(b, n, dtype=torch.bool)
        m[1, n // 3] = True
        return m
    m = torch.rand(b, n, generator=g) < 0.7
    if kind == "row":
        m[1] = False
    m[0, 0] = True
    return m


def run(ref, pn, out, tn, raw, ch, pos, key_pad):
    out = out.clone().requires_grad_(True)
    mask = ~key_pad
    dp = ref.dct_patches.DCTPatches(patches=out, key_pad_mask=key_pad, attn_mask=None,
                                    batched_image_ids=torch.zeros_like(ch), patch_channels=ch, patch_positions=pos,
                                    patch_sizes=[], original_sizes=[])
    rec = F.l1_loss(out[mask], tn[mask])                       # main.py:71
    un = pn.inverse_norm(dp.shallow_copy())                    # main.py:79 (inv_normalize_)
    unn = F.l1_loss(un[mask], raw[mask])                       # main.py:81-83
    grad, = torch.autograd.grad(W[0] * rec + W[1] * unn, out)
    return {"rec": rec.detach().numpy(), "unn": unn.detach().numpy(), "grad": grad.numpy()}, un.detach()


def main():
    ref = refload.load()
    res = {}
    for ci, (name, P, (b, n), mk) in enumerate(CASES):
        PP = P * P
        g = torch.Generator().manual_seed(300 + ci)
        med, bb = tables(PP)
        pn = ref.patchnorm.PatchNorm(32, 32, P, 3)
        pn.median.data = med
        pn.b.data = bb
        pn.frozen = True
        pn.eval()
        ch = torch.randint(0, 3, (b, n), generator=g)
        pos = torch.randint(0, 32, (b, n, 2), generator=g)
        key_pad = ~make_mask(mk, b, n, g)
        tn = torch.randn(b, n, PP, generator=g).clamp_(-6, 6)
        out = tn + 0.3 * torch.randn(b, n, PP, generator=g)
        same1 = torch.rand(b, n, PP, generator=g) < 0.1
        out[same1] = tn[same1]
        std = bb[ch, pos[..., 0], pos[..., 1]] * 2 ** 0.5 + pn.eps
        raw = (tn * std + med[ch, pos[..., 0], pos[..., 1]]) + 0.3 * std * torch.randn(b, n, PP, generator=g)
        same2 = torch.rand(b, n, PP, generator=g) < 0.1
        raw[same2] = (out * std + med[ch, pos[..., 0], pos[..., 1]])[same2]
        codes = torch.randint(0, 2 ** CODEBOOK[0], (b, n, CODEBOOK[1]), generator=g)
        r32, un = run(ref, pn, out, tn, raw, ch, pos, key_pad)
        assert int(((un - raw) == 0)[~key_pad].sum()) >= int(same2[~key_pad].sum())
        r64, _ = run(ref, copy.deepcopy(pn).double(), out.double(), tn.double(), raw.double(), ch, pos, key_pad)
        for k, v in (("out", out), ("tn", tn), ("raw", raw), ("ch", ch), ("pos", pos), ("key_pad", key_pad),
                     ("codes", codes)):
            res[f"{name}_{k}"] = v.numpy()
        for k, v in r32.items():
            res[f"{name}_{k}_f32"] = v
        for k, v in r64.items():
            res[f"{name}_{k}_f64"] = v
        res[f"{name}_perplexity"] = ref.util.calculate_perplexity(codes[~key_pad], 2 ** CODEBOOK[0]).numpy()
        print(f"{name}: M {int((~key_pad).sum())} rec {float(r64['rec']):.9e} (fp32 dev "
              f"{abs(float(r32['rec']) - float(r64['rec'])):.2e}) unn {float(r64['unn']):.9e} (fp32 dev "
              f"{abs(float(r32['unn']) - float(r64['unn'])):.2e}); d1 == 0 at {int(same1[~key_pad].sum())}, "
              f"d2 == 0 at {int(((un - raw) == 0)[~key_pad].sum())} elements")
    res["names"] = np.array([c[0] for c in CASES])
    res["patch_size"] = np.array([c[1] for c in CASES], dtype=np.int64)
    res["weights"] = np.array(W, dtype=np.float64)
    res["codebook"] = np.array(CODEBOOK, dtype=np.int64)
    path = os.path.join(HERE, "rec_loss_ref.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
