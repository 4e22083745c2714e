"""Golden vectors for the reference LFQ's TRAINING forward (reference
dct_autoencoder/lfq.py:164-204: straight-through output, commit loss, dense
distance) and its entropy loss (util.py:355-387) with their gradients, produced
by running the REFERENCE's own LFQ class and compute_entropy_loss /
calculate_perplexity in the build container (refload.py).

    python tests/golden/gen_lfq_train_golden.py   ->  tests/golden/lfq_train_ref.npz
                                                      tests/golden/lfq_train_ref_big.npz

(the 2 x 700 token case alone in the second file: its float64 gradients would
take one file past the 1 MiB limit for committed files)

Per case (key prefix = the case name): the input ``x``, ``mask`` and, with
projections, the four projection tensors; then, from the reference in fp32
(suffix ``_f32``) and from a float64 run of the same classes (module
``.double()``; the entropy formula restated below in float64, because the
reference's compute_entropy_loss casts to fp32; suffix ``_f64``):
``entropy``, ``commit``, ``g_entropy`` / ``g_commit`` / ``g_st`` (the gradients
of the entropy loss, the commit loss and ``x_q.sum()`` with respect to x) and,
with projections, ``gw`` / ``gb`` (the gradient of entropy + commit with respect
to project_in's weight / bias); ``avg_probs_f64``; the fp32 run's ``idx`` and
``xq``; ``perplexity`` of the indices.  No dense distance is stored.  Data
only; no reference source is stored.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import refload  # noqa: E402

# name, codebook_dim, num_codebooks, dim (None: no projections), input scale, codebook_scale, (b, n), mask kind
CASES = [
    ("sat", 6, 3, None, 1.0, 1.0, (2, 37), "rand"),
    ("d6", 6, 3, None, 0.01, 1.0, (2, 37), "rand"),
    ("d1", 1, 2, None, 0.01, 1.0, (2, 37), "rand"),
    ("d10", 10, 2, None, 0.003, 1.0, (2, 37), "rand"),
    ("d13", 13, 2, None, 0.004, 1.0, (2, 37), "rand"),
    ("d14", 14, 1, None, 0.004, 1.0, (2, 37), "rand"),
    ("proj", 8, 4, 24, 0.02, 1.0, (2, 37), "rand"),
    ("l", 13, 16, None, 0.01, 1.0, (2, 9), "rand"),
    ("neg", 6, 3, None, 0.01, -0.5, (2, 37), "rand"),
    ("zero", 6, 3, None, 0.01, 0.0, (2, 37), "rand"),
    ("big", 13, 2, None, 0.004, 1.0, (2, 700), "rand"),
    ("one", 6, 3, None, 0.01, 1.0, (2, 37), "single"),
    ("row", 6, 3, None, 0.01, 1.0, (2, 37), "row"),
    ("img", 6, 3, None, 0.01, 1.0, (2, 5, 7), "rand"),
]


def entropy_f64(distance, mask, temperature=0.01, eps=1e-9):
    """util.py:355-387 in the precision of its input; also returns avg_probs"""
    a = distance.reshape(-1, *distance.shape[2:])
    m = mask.reshape(-1).to(a.dtype)
    logits = a / temperature + eps
    lp = torch.log_softmax(logits, dim=-1)
    p = lp.exp()
    M = m.sum()
    avg = (p * m[:, None, None]).sum(0).mean(0) / M
    avg_entropy = -(avg * (avg + eps).log()).sum()
    sample_entropy = -((p * lp).sum(-1) * m[:, None]).sum() / M
    return sample_entropy - avg_entropy, avg


def make_mask(kind, b, n, g):
    if kind == "single":
        m = torch.zeros(b, n, dtype=torch.bool)
        m[1, n // 3] = True
        return m
    m = torch.rand(b, n, generator=g) < 0.7
    if kind == "row":
        m[1] = False
    m[0, 0] = True
    return m


def run(m, x, mask, util, f64):
    x = x.clone().requires_grad_(True)
    xq, idx, commit, dist = m(x, mask=mask)
    if f64:
        ent, avg = entropy_f64(dist, mask)
    else:
        ent, avg = util.compute_entropy_loss(dist, mask), None
    out = {"entropy": ent, "commit": commit}
    out["g_entropy"], = torch.autograd.grad(ent, x, retain_graph=True)
    out["g_commit"], = torch.autograd.grad(commit, x, retain_graph=True)
    out["g_st"], = torch.autograd.grad(xq.sum(), x, retain_graph=True)
    if m.has_projections:
        out["gw"], out["gb"] = torch.autograd.grad(ent + commit, [m.project_in.weight, m.project_in.bias])
    if avg is not None:
        out["avg_probs"] = avg
    return {k: v.detach().numpy() for k, v in out.items()}, idx.detach(), xq.detach()


def main():
    ref = refload.load()
    LFQ = ref.lfq.LFQ
    out = {}
    for ci, (name, cd, ncb, dim, sx, s, bn, mk) in enumerate(CASES):
        g = torch.Generator().manual_seed(100 + ci)
        torch.manual_seed(200 + ci)
        m = LFQ(dim=dim, codebook_size=2 ** cd, num_codebooks=ncb, codebook_scale=s).train()
        feat = dim if dim is not None else cd * ncb
        if len(bn) == 3:   # image form (b, d, h, w)
            b, hh, ww = bn
            x = torch.randn(b, feat, hh, ww, generator=g) * sx
            n = hh * ww
        else:
            b, n = bn
            x = torch.randn(b, n, feat, generator=g) * sx
        mask = make_mask(mk, b, n, g)
        out[f"{name}_x"] = x.numpy()
        out[f"{name}_mask"] = mask.numpy()
        if dim is not None:
            for k, t in (("w_in", m.project_in.weight), ("b_in", m.project_in.bias),
                         ("w_out", m.project_out.weight), ("b_out", m.project_out.bias)):
                out[f"{name}_{k}"] = t.detach().numpy().copy()
        r32, idx, xq = run(m, x, mask, ref.util, False)
        r64, idx64, _ = run(copy.deepcopy(m).double(), x.double(), mask, ref.util, True)
        assert torch.equal(idx, idx64), name
        for k, v in r32.items():
            out[f"{name}_{k}_f32"] = v
        for k, v in r64.items():
            out[f"{name}_{k}_f64"] = v
        out[f"{name}_idx"] = idx.numpy().astype(np.int64)
        out[f"{name}_xq"] = xq.numpy()
        out[f"{name}_perplexity"] = ref.util.calculate_perplexity(idx, 2 ** cd).numpy()
        rel = abs(float(r32["entropy"]) - float(r64["entropy"])) / abs(float(r64["entropy"]))
        ge = r32["g_entropy"].astype(np.float64) + r32["g_commit"].astype(np.float64)
        ge64 = r64["g_entropy"] + r64["g_commit"]
        print(f"{name}: entropy {float(r64['entropy']):+.9e} fp32 rel dev {rel:.2e}; grad dev "
              f"{np.abs(ge - ge64).max() / np.abs(ge64).max():.2e} of max|grad| {np.abs(ge64).max():.3e}")
    out["names"] = np.array([c[0] for c in CASES])
    out["cfg"] = np.array([[c[1], c[2], c[3] or 0] for c in CASES], dtype=np.int64)
    out["scales"] = np.array([c[5] for c in CASES], dtype=np.float64)
    for fname, pick in (("lfq_train_ref.npz", lambda k: not k.startswith("big_")),
                        ("lfq_train_ref_big.npz", lambda k: k.startswith("big_"))):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **{k: v for k, v in out.items() if pick(k)})
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
