"""CPU side of the LFQ training mode: the mathematics the fused kernel rests
on, and the torch-op branches of dct_autoencoder_amd.losses, against the
reference's recorded results (tests/golden/lfq_train_ref.npz,
gen_lfq_train_golden.py)."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

G = golden("lfq_train_ref.npz")
NAMES = [str(n) for n in G["names"] if str(n) != "big"]
CFG = {str(n): (int(c[0]), int(c[1]), int(c[2]) or None, float(s))
       for n, c, s in zip(G["names"], G["cfg"], G["scales"])}
NOPROJ = [n for n in NAMES if CFG[n][2] is None]
FLOOR = 2.0 ** -20


def tokens(name):
    """the case's input as (b, n, c, d) projected features (cases without projections)"""
    cd, ncb, _, _ = CFG[name]
    x = torch.from_numpy(G[f"{name}_x"])
    if x.ndim == 4:
        x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1])
    return x.reshape(*x.shape[:2], ncb, cd)


def factorised_f64(h, mask, s, T=0.01, eps=1e-9):
    """The kernel's formulation in float64: the softmax over the 2^d codes of
    a row is the product over the bits of pi(+1) = sigmoid(-4 s h / T),
    pi(-1) = 1 - pi(+1); dimension 0 is the most significant bit; eps inside
    the softmax is a shift and drops out.  Returns (entropy loss, avg_probs)."""
    b, n, c, d = h.shape
    rows = h.double()[mask].reshape(-1, d)            # the M c masked-in rows
    M = int(mask.sum())
    u = -4.0 * s * rows / T
    pp, pm = torch.sigmoid(u), torch.sigmoid(-u)
    hb = -(torch.xlogy(pp, pp) + torch.xlogy(pm, pm))
    sample_entropy = hb.sum() / M
    hi = (d + 1) // 2

    def group(lo_dim, hi_dim):
        out = torch.ones(rows.shape[0], 1, dtype=torch.float64)
        for dd in range(lo_dim, hi_dim):              # MSB first: each bit doubles the table
            out = torch.stack([out * pm[:, dd, None], out * pp[:, dd, None]], dim=2).reshape(rows.shape[0], -1)
        return out

    A, B = group(0, hi), group(hi, d)
    avg = (A.t() @ B).reshape(-1) / (M * c)
    avg_entropy = -(avg * torch.log(avg + eps)).sum()
    return sample_entropy - avg_entropy, avg


@pytest.mark.parametrize("name", NOPROJ)
def test_factorised_formula_reproduces_float64_reference(name):
    s = CFG[name][3]
    ent, avg = factorised_f64(tokens(name), torch.from_numpy(G[f"{name}_mask"]), s)
    want = float(G[f"{name}_entropy_f64"])
    assert abs(float(ent) - want) <= 1e-12 * max(1.0, abs(want)), (float(ent), want)
    assert np.abs(avg.numpy() - G[f"{name}_avg_probs_f64"]).max() <= 1e-12


@pytest.mark.parametrize("name", NOPROJ)
def test_materialize_is_the_reference_distance(pkg, name):
    cd, ncb, _, s = CFG[name]
    m = pkg.LFQ(codebook_size=2 ** cd, num_codebooks=ncb, codebook_scale=s)
    h = tokens(name)
    dist = pkg.LFQDistance(h, s, cd, ncb)
    want = -2 * torch.einsum("...id,jd->...ij", h, m.codebook)
    assert dist.shape == want.shape and dist.dtype == want.dtype
    assert torch.equal(dist.materialize(), want)


@pytest.mark.parametrize("name", NOPROJ)
def test_dense_branch_on_cpu(pkg, name):
    """compute_entropy_loss on a dense tensor (and on a CPU LFQDistance, which
    materialises) against the fixture, within 4 x the reference's own fp32
    deviation from float64, floored at 2^-20 relative / 2^-20 x max|grad|"""
    cd, ncb, _, s = CFG[name]
    h = tokens(name).requires_grad_(True)
    mask = torch.from_numpy(G[f"{name}_mask"])
    dist = pkg.LFQDistance(h, s, cd, ncb)
    ent = pkg.compute_entropy_loss(dist.materialize(), mask)
    assert torch.equal(ent, pkg.compute_entropy_loss(dist, mask))
    want = float(G[f"{name}_entropy_f64"])
    dev = abs(float(G[f"{name}_entropy_f32"]) - want)
    assert abs(ent.item() - want) <= max(4 * dev, FLOOR * abs(want))
    g, = torch.autograd.grad(ent, h)
    want = G[f"{name}_g_entropy_f64"]
    if want.ndim == 4:
        want = np.transpose(want, (0, 2, 3, 1)).reshape(want.shape[0], -1, want.shape[1])
    dev = np.abs(G[f"{name}_g_entropy_f32"].astype(np.float64) - G[f"{name}_g_entropy_f64"]).max()
    err = np.abs(g.reshape(want.shape).numpy().astype(np.float64) - want).max()
    assert err <= max(4 * dev, FLOOR * np.abs(want).max())


def test_masked_mean(pkg):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 7, 3, generator=g)
    m = torch.rand(5, 7, generator=g) < 0.6
    assert torch.allclose(pkg.masked_mean(x, m), x[m].sum() / m.sum(), rtol=1e-6, atol=0)
    assert torch.allclose(pkg.masked_mean(x, m, dim=0), (x * m[..., None]).sum(0) / m.sum(), rtol=1e-6, atol=1e-7)
    name = "d6"
    h = tokens(name)
    mask = torch.from_numpy(G[f"{name}_mask"])
    q = torch.where(h > 0, 1.0, -1.0)
    commit = pkg.masked_mean((h - q) ** 2, mask, dim=0).sum(0).mean()
    want = float(G[f"{name}_commit_f64"])
    dev = abs(float(G[f"{name}_commit_f32"]) - want)
    assert abs(commit.item() - want) <= max(4 * dev, FLOOR * abs(want))


@pytest.mark.parametrize("name", NAMES)
def test_calculate_perplexity(pkg, name):
    cd = CFG[name][0]
    idx = torch.from_numpy(G[f"{name}_idx"])
    want = float(G[f"{name}_perplexity"])
    assert abs(pkg.calculate_perplexity(idx, 2 ** cd).item() - want) <= FLOOR * want
    # null codes are left out of the histogram
    with_null = torch.cat([idx.flatten(), torch.full((5,), -1, dtype=idx.dtype)])
    assert abs(pkg.calculate_perplexity(with_null, 2 ** cd).item() - want) <= FLOOR * want


def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "dctae.h")) as f:
        text = f.read()
    assert "int dctae_lfq_entropy_forward(" in text and "int dctae_lfq_entropy_backward(" in text
    assert "#define DCTAE_ABI_VERSION 1" in text
