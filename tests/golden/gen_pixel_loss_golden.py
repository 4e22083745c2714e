"""Golden vectors for the pixel loss of the reference's training step (reference
main.py:95-110) and the gradient of FE.postprocess (FE:289-310), produced by
running the REFERENCE's own preprocess, iter_batches, postprocess and autograd
in the build container (refload.py).

    python tests/golden/gen_pixel_loss_golden.py
        ->  tests/golden/pixel_loss_ref.npz              the five small cases
            tests/golden/pixel_loss_ref_sq512.npz        case sq512: inputs and fp32 results
            tests/golden/pixel_loss_ref_sq512_f64.npz    case sq512: float64 results

(three files so that each stays below the 1 MiB limit of a committed file).

Per case (key prefix = the case name): the batch of the reference's
``preprocess`` + ``iter_batches(..., None)`` of ``torch.rand`` images with
sample_patches_beta = 0 -- ``patches``, ``key_pad``, ``ids``, ``pos``, ``ch``,
``patch_sizes``, ``original_sizes`` -- and ``out`` = patches + 0.05 randn, the
perturbed output.  Case ``dup``: slot 1 takes slot 0's position and channel
(the overwritten duplicate of FE:639-643).  The upstream gradient w_i of image
i for the vjp is the fp32 rounding of sum_r a[r, c] u[r, y] v[r, x] evaluated in
float64 (``w{i}_a`` (3, 3), ``w{i}_u`` (3, H), ``w{i}_v`` (3, W); ``upstream``
below, which the tests restate): a full image per case would not fit.

Results, from the reference in fp32 (suffix ``_f32``) and from the float64
oracle (suffix ``_f64``):
  ``loss``      pixel_loss = mean_i F.mse_loss(x_i, x_hat_i), x = postprocess(patches), x_hat = postprocess(out)
  ``grad``      its gradient with respect to ``out``
  ``vjp``       the gradient of sum_i <w_i, x_hat_i> with respect to ``out``
  ``mse``       the per-image terms (float64 only), ``xmax`` max |x_i| (float64 only)
The reference's _transform_image_out casts to fp32 internally (FE:148), so a
.double() run of it is still an fp32 computation; the float64 oracle is composed
from oracle.ref_cpu.revert_patching(per_token_loop=True), the zero pad,
ref_cpu.idct2 and ref_cpu.ipt_to_rgb on double tensors, which keep the dtype.
The colour matrices are the reference's as this host computes them (an fp32
matmul and two fp32 ``.inverse()``); they are the ones recorded in colors.npz
(checked below), which the tests use, because another CPU gives other last bits.
Data only; no reference source is stored.
"""
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
from oracle import ref_cpu  # noqa: E402

# name, patch size, (max_patch_h, max_patch_w), max_seq_len, image sizes
CASES = [
    ("ragged14", 14, (4, 4), 40, [(61, 47), (30, 75), (14, 14)]),
    ("p5", 5, (6, 6), 60, [(23, 31), (9, 5), (40, 12)]),
    ("p16", 16, (2, 2), 12, [(33, 32), (16, 50)]),
    ("p1", 1, (3, 3), 27, [(3, 3), (2, 5)]),
    ("dup", 5, (6, 6), 60, [(23, 31)]),
    ("sq512", 14, (32, 32), 256, [(512, 512)]),
]


def upstream(a, u, v):
    """w[c, y, x] = fp32(sum_r a[r, c] u[r, y] v[r, x]), the sum in float64"""
    return torch.einsum("rc,ry,rx->cyx", a.double(), u.double(), v.double()).float()


def oracle_images(batch, cfg, patches):
    """FE:289-310 on ``patches`` in their own dtype (float64 keeps float64)"""
    b = ref_cpu.Batch(patches=patches, key_pad_mask=batch.key_pad_mask, attn_mask=None,
                      batched_image_ids=batch.batched_image_ids, patch_channels=batch.patch_channels,
                      patch_positions=batch.patch_positions, patch_sizes=batch.patch_sizes,
                      original_sizes=batch.original_sizes)
    out = []
    for img, (h, w) in zip(ref_cpu.revert_patching(b, cfg, per_token_loop=True), batch.original_sizes):
        full = torch.zeros(cfg.channels, h, w, dtype=img.dtype)
        full[:, : img.shape[1], : img.shape[2]] = img
        out.append(ref_cpu.ipt_to_rgb(ref_cpu.idct2(full)))
    return out


def results(decode, patches, out, ws):
    """decode: patches -> list of images.  loss, its gradient, the vjp gradient, per-image mse, max |x|"""
    out = out.clone().requires_grad_(True)
    with torch.no_grad():
        x = decode(patches)
    x_hat = decode(out)
    mses = [F.mse_loss(a, b) for a, b in zip(x, x_hat)]            # main.py:102-104
    loss = sum(mses) / len(x_hat)                                   # main.py:106
    grad, = torch.autograd.grad(loss, out, retain_graph=True)
    vjp, = torch.autograd.grad(sum((w.to(xh.dtype) * xh).sum() for w, xh in zip(ws, x_hat)), out)
    return {"loss": loss.detach().numpy(), "grad": grad.numpy(), "vjp": vjp.numpy(),
            "mse": torch.stack(mses).detach().numpy(), "xmax": torch.stack([a.abs().max() for a in x]).numpy()}


def main():
    ref = refload.load()
    FE = ref.fe.DCTAutoencoderFeatureExtractor
    recorded = np.load(os.path.join(HERE, "colors.npz"))
    for k, v in ref_cpu.color_matrices().items():
        assert np.array_equal(v.numpy(), recorded[k]), f"{k} differs from colors.npz on this host"
    torch.set_num_threads(8)
    files = {"": {}, "_sq512": {}, "_sq512_f64": {}}
    for ci, (name, P, (mh, mw), S, sizes) in enumerate(CASES):
        g = torch.Generator().manual_seed(900 + ci)
        proc = FE(3, P, 0.0, mh, mw, S)
        items = [proc.preprocess(torch.rand(3, h, w, generator=g)) for h, w in sizes]
        (batch,) = list(proc.iter_batches(iter([{k: [it[k] for it in items] for k in items[0]}]), None))
        if name == "dup":
            batch.patch_positions[0, 1] = batch.patch_positions[0, 0]
            batch.patch_channels[0, 1] = batch.patch_channels[0, 0]
        patches = batch.patches.float()
        out = patches + 0.05 * torch.randn(patches.shape, generator=g)
        facs = [(torch.randn(3, 3, generator=g), torch.randn(3, h, generator=g), torch.randn(3, w, generator=g))
                for h, w in batch.original_sizes]
        ws = [upstream(*f) for f in facs]
        cfg = ref_cpu.FEConfig(patch_size=P, max_patch_h=mh, max_patch_w=mw, max_seq_len=S)

        def ref_decode(x):
            dp = batch.shallow_copy()
            dp.patches = x
            return proc.postprocess(dp)
        r32 = results(ref_decode, patches, out, ws)
        o32 = results(lambda x: oracle_images(batch, cfg, x), patches, out, ws)
        for k in ("loss", "grad", "vjp"):
            assert np.array_equal(r32[k], o32[k]), (name, k, "ref_cpu in fp32 differs from the reference")
        r64 = results(lambda x: oracle_images(batch, cfg, x), patches.double(), out.double(), ws)
        small = name != "sq512"
        f_in = files[""] if small else files["_sq512"]
        f_64 = files[""] if small else files["_sq512_f64"]
        for k, v in (("patches", patches), ("out", out), ("key_pad", batch.key_pad_mask),
                     ("ids", batch.batched_image_ids.to(torch.int16)), ("pos", batch.patch_positions.to(torch.int16)),
                     ("ch", batch.patch_channels.to(torch.int8))):
            f_in[f"{name}_{k}"] = v.numpy()
        f_in[f"{name}_patch_sizes"] = np.array(batch.patch_sizes, dtype=np.int32)
        f_in[f"{name}_original_sizes"] = np.array(batch.original_sizes, dtype=np.int32)
        for i, (a, u, v) in enumerate(facs):
            f_in[f"{name}_w{i}_a"], f_in[f"{name}_w{i}_u"], f_in[f"{name}_w{i}_v"] = a.numpy(), u.numpy(), v.numpy()
        for k in ("loss", "grad", "vjp"):
            f_in[f"{name}_{k}_f32"] = r32[k]
        for k, v in r64.items():
            f_64[f"{name}_{k}_f64"] = v
        gm, vm = np.abs(r64["grad"]).max(), np.abs(r64["vjp"]).max()
        print(f"{name}: rows {patches.shape[0]} real tokens {int((~batch.key_pad_mask).sum())} loss "
              f"{float(r64['loss']):.9e} (fp32 rel dev {abs(float(r32['loss']) - float(r64['loss'])) / float(r64['loss']):.2e}) "
              f"grad fp32 dev / max {np.abs(r32['grad'] - r64['grad']).max() / gm:.2e}, "
              f"vjp fp32 dev / max {np.abs(r32['vjp'] - r64['vjp']).max() / vm:.2e}")
    files[""]["names"] = np.array([c[0] for c in CASES])
    files[""]["patch_size"] = np.array([c[1] for c in CASES], dtype=np.int64)
    files[""]["max_patch"] = np.array([c[2] for c in CASES], dtype=np.int64)
    files[""]["max_seq_len"] = np.array([c[3] for c in CASES], dtype=np.int64)
    for suffix, res in files.items():
        path = os.path.join(HERE, f"pixel_loss_ref{suffix}.npz")
        np.savez_compressed(path, **res)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
