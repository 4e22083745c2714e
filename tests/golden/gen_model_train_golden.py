"""Golden vectors for the DCTAutoencoder training step, produced
by running the REFERENCE's own modeling_dct_autoencoder.py / lfq.py /
patchnorm.py in ``.train()`` under torch autograd in the build container
(refload.py; eager attention forced as in gen_model_golden.py).

    python tests/golden/gen_model_train_golden.py  ->  tests/golden/model_train_ref*.npz

Weights, inputs and config are those of model_ref.npz (hidden 128, 2 heads,
2 + 2 layers, 3 rows of 256 tokens with padding and several images per row).
main.py imports wandb / accelerate / bitsandbytes, so its step (main.py:56-93)
and objective (main.py:311-314) are restated below with the reference's own
classes, as gen_rec_loss_golden.py does.

Every gradient is computed with the reference model in float64 and stored as
fp32.  Three cases (key prefix):
  enc.   encoder half: upstream gradient randn(seed SEED_ENC) on the
         pre-quantizer hidden state; ``enc.g.<name>`` for every encoder-side
         parameter and ``enc.g.patches_in``.
  dec.   decoder half: the reference's quantizer output x_q (= project_out of
         the +-1 codes of model_ref.npz's ``codes``) as a leaf, upstream gradient
         randn(seed SEED_DEC) on the decoded patches; ``dec.g.<name>`` for every
         decoder-side parameter and ``dec.g.x_q``.
  step.  the whole step: ``step.loss.<term>`` (four terms and ``total``, the
         weighted sum) and ``step.g.<name>`` for the tensors of STEP_SUBSET.
The yardstick is the same reference in fp32 under
torch.autocast("cpu", dtype=torch.bfloat16) around the model's forward (the
bf16 arrangement of main.py:333-349): ``<case>.dev.<name>`` is the L2 norm of
that run's deviation from the float64 gradient, ``step.dev.loss.<term>`` the
absolute deviation of a loss term.
``adamw.loss``: the reference's total loss before each of 10 steps of
torch.optim.AdamW (fp32, lr ``adamw.lr``) on this fixed batch, and after the
last (11 values).

One npz may not exceed 1 MiB, so the tensors are spread over several files
(``bucket`` below); the tests read all of them into one dict.  Data only; no
reference source is stored.
"""
import glob
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import refload  # noqa: E402

SEED_ENC, SEED_DEC = 7001, 7002
WEIGHTS = dict(rec_loss=0.1, rec_loss_unnormalized=1.0, commit_loss=0.1, entropy_loss=0.1)   # main.py:311-314
STEP_SUBSET = ["encoder.layers.0.self_attn.q_proj.weight", "decoder.layers.1.self_attn.k_proj.bias",
               "encoder.layers.1.mlp.fc1.bias", "encoder.layers.0.layer_norm1.weight",
               "decoder.layers.0.layer_norm2.weight", "to_patch_embedding.0.weight", "vq_model.project_in.weight",
               "vq_model.project_out.bias", "proj_out.1.weight", "encoder_pos_embed_height",
               "decoder_pos_embed_channel"]
LR, STEPS = 3e-4, 10


def bucket(key):
    """file suffix of a stored key: the layers' gradients and the two input gradients get files of their own"""
    for side in ("enc", "dec"):
        for i in range(2):
            if key.startswith(f"{side}.g.{side}oder.layers.{i}."):
                return f"_{side}{i}"
    if key in ("enc.g.patches_in", "dec.g.x_q"):
        return "_" + key.split(".")[-1]
    return ""


def main():
    ref = refload.load()
    m = importlib.import_module("dct_autoencoder.modeling_dct_autoencoder")
    cm = importlib.import_module("dct_autoencoder.configuration_dct_autoencoder")
    g = np.load(os.path.join(HERE, "model_ref.npz"))
    hid, heads, inter, layers, ncb, cbs, S = [int(v) for v in g["cfg"]]
    enc = dict(hidden_size=hid, intermediate_size=inter, num_attention_heads=heads, num_hidden_layers=layers)
    cfg = cm.DCTAutoencoderConfig(image_channels=3, patch_size=14, max_patch_h=32, max_patch_w=32,
                                  vq_codebook_size=cbs, vq_num_codebooks=ncb, vq_type="lfq", encoder_config=enc,
                                  decoder_config=enc)
    cfg.encoder_config._attn_implementation = "eager"
    cfg.decoder_config._attn_implementation = "eager"
    tabs = np.load(os.path.join(HERE, "patchnorm_ref.npz"))
    w = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}
    t = {k: torch.from_numpy(g[k]) for k in ("patches_in", "key_pad_mask", "batched_image_ids", "patch_channels",
                                            "patch_positions", "codes")}
    ids, kp = t["batched_image_ids"], t["key_pad_mask"]
    attn_mask = (ids[:, None, :, None] == ids[:, None, None, :]) & kp[:, None, None, :]   # FE:580-584

    def build(dtype):
        torch.manual_seed(0)
        model = m.DCTAutoencoder(cfg)
        missing, unexpected = model.load_state_dict(w, strict=False)
        assert not unexpected and all(k.startswith("patchnorm.") for k in missing), (missing, unexpected)
        assert model.encoder.layers[0].self_attn.config._attn_implementation == "eager"
        for k in ("median", "b", "n"):
            getattr(model.patchnorm, k).data.copy_(torch.from_numpy(tabs[k]))
        model.patchnorm.frozen = True
        return model.train().to(dtype)

    def patches(x):
        return ref.dct_patches.DCTPatches(patches=x, key_pad_mask=kp, attn_mask=attn_mask, batched_image_ids=ids,
                                          patch_channels=t["patch_channels"], patch_positions=t["patch_positions"],
                                          patch_sizes=[], original_sizes=[])

    def named(model, prefixes):
        return [(n, p) for n, p in model.named_parameters() if p.requires_grad and n.startswith(prefixes)]

    def enc_half(model, dtype, autocast):
        x = t["patches_in"].to(dtype).requires_grad_(True)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            dp = patches(x)
            dp.patches = model.to_patch_embedding(dp.patches)                      # modeling:138-147
            dp = model.add_pos_embedding_encoder_(dp)
            hidden = model.encoder(dp.patches, attention_mask=dp.attn_mask).last_hidden_state
        ps = named(model, ("to_patch_embedding.", "encoder.", "encoder_pos_embed_"))
        up = torch.randn(hidden.shape, generator=torch.Generator().manual_seed(SEED_ENC))
        gs = torch.autograd.grad(hidden, [p for _, p in ps] + [x], up.to(hidden.dtype))
        return {n: v.double() for (n, _), v in zip(ps + [("patches_in", None)], gs)}

    def dec_half(model, dtype, autocast, xq):
        x = xq.to(dtype).requires_grad_(True)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            out = model.decode(patches(x)).patches
        ps = named(model, ("decoder.", "decoder_pos_embed_", "proj_out."))
        up = torch.randn(out.shape, generator=torch.Generator().manual_seed(SEED_DEC))
        gs = torch.autograd.grad(out, [p for _, p in ps] + [x], up.to(out.dtype))
        return {n: v.double() for (n, _), v in zip(ps + [("x_q", None)], gs)}

    def step(model, dtype, autocast):
        """main.py:56-93 and the weighted sum of main.py:311-314"""
        normalized = patches(t["patches_in"].to(dtype))
        with torch.no_grad():
            batch = patches(model.patchnorm.inverse_norm(normalized.shallow_copy()))
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            res = model(normalized.shallow_copy())
        output = res["dct_patches"]
        mask = ~output.key_pad_mask
        terms = dict(entropy_loss=model.entropy_loss(res["distances"], mask=mask),
                     rec_loss=F.l1_loss(output.patches[mask], normalized.patches[mask]))
        un = model.inv_normalize_(output.shallow_copy())
        terms["rec_loss_unnormalized"] = F.l1_loss(un.patches[mask], batch.patches[mask])
        terms["commit_loss"] = res["commit_loss"]
        terms["total"] = sum(wt * terms[k] for k, wt in WEIGHTS.items())
        return terms, res

    res = {}
    m32, m64 = build(torch.float32), build(torch.float64)
    # the quantizer output of the training forward: the +-1 codes of model_ref.npz through project_out
    with torch.no_grad():
        _, r32 = step(m32, torch.float32, False)
        assert torch.equal(r32["codes"], t["codes"])
        xq = m32.vq_model.indices_to_codes(t["codes"])
    for case, fn, extra in (("enc", enc_half, ()), ("dec", dec_half, (xq,))):
        g64 = fn(m64, torch.float64, False, *extra)
        gac = fn(m32, torch.float32, True, *extra)
        for n in g64:
            res[f"{case}.g.{n}"] = g64[n].float().numpy()
            res[f"{case}.dev.{n}"] = np.float64((gac[n] - g64[n]).norm().item())
    for up, seed, shape in (("enc", SEED_ENC, (3, S, hid)), ("dec", SEED_DEC, (3, S, 196))):
        x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
        res[f"{up}.upstream_check"] = np.array([x.double().sum().item(), x[0, 0, 0].item(), x[-1, -1, -1].item()])
    runs = {}
    for tag, model, dtype, ac in (("f64", m64, torch.float64, False), ("ac", m32, torch.float32, True)):
        model.zero_grad()
        terms, _ = step(model, dtype, ac)
        terms["total"].backward()
        runs[tag] = ({k: float(v) for k, v in terms.items()},
                     {n: p.grad.double().clone() for n, p in model.named_parameters() if n in STEP_SUBSET})
        model.zero_grad()
    assert sorted(runs["f64"][1]) == sorted(STEP_SUBSET)
    for k, v in runs["f64"][0].items():
        res[f"step.loss.{k}"] = np.float64(v)
        res[f"step.dev.loss.{k}"] = np.float64(abs(runs["ac"][0][k] - v))
    for n in STEP_SUBSET:
        res[f"step.g.{n}"] = runs["f64"][1][n].float().numpy()
        res[f"step.dev.{n}"] = np.float64((runs["ac"][1][n] - runs["f64"][1][n]).norm().item())
    # ten AdamW steps of the fp32 reference on the fixed batch
    mo = build(torch.float32)
    opt = torch.optim.AdamW(mo.parameters(), lr=LR)
    curve = []
    for _ in range(STEPS):
        opt.zero_grad()
        terms, _ = step(mo, torch.float32, False)
        curve.append(float(terms["total"]))
        terms["total"].backward()
        opt.step()
    with torch.no_grad():
        curve.append(float(step(mo, torch.float32, False)[0]["total"]))
    print("adamw total loss:", " ".join(f"{v:.5f}" for v in curve))
    # the reference's own loss must fall by a clear margin: every step down, 5 % of |loss| in all
    assert all(b < a for a, b in zip(curve, curve[1:])) and curve[0] - curve[-1] >= 0.05 * abs(curve[0]), curve
    res["adamw.loss"] = np.array(curve)
    res["adamw.lr"] = np.float64(LR)
    res["weights"] = np.array([WEIGHTS[k] for k in sorted(WEIGHTS)])
    res["step_subset"] = np.array(STEP_SUBSET)
    for k in sorted(res):
        if ".dev." in k:
            gk = k.replace(".dev.", ".g." if ".loss." not in k else ".")
            ref_n = float(np.linalg.norm(res[gk])) if gk in res else float("nan")
            print(f"{k:70s} {float(res[k]):.4e}  (|ref| {ref_n:.4e})")
    files = {}
    for k, v in res.items():
        files.setdefault(bucket(k), {})[k] = v
    for old in glob.glob(os.path.join(HERE, "model_train_ref*.npz")):
        os.remove(old)
    for suffix, d in files.items():
        path = os.path.join(HERE, f"model_train_ref{suffix}.npz")
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        print("wrote", path, size, "bytes")
        assert size <= 1 << 20, path


if __name__ == "__main__":
    main()
