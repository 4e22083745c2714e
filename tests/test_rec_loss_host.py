"""CPU side of the reconstruction losses: the torch-op branch of
dct_autoencoder_amd.losses.reconstruction_losses and masked_perplexity against
the reference's recorded results (tests/golden/rec_loss_ref.npz,
gen_rec_loss_golden.py), the float64 restatement the GPU test's oracle rests on,
and the C ABI's three new entry points."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

G = golden("rec_loss_ref.npz")
NAMES = [str(n) for n in G["names"]]
PSIZE = {str(n): int(p) for n, p in zip(G["names"], G["patch_size"])}
W0, W1 = (float(w) for w in G["weights"])
FLOOR = 2.0 ** -20
SYMBOLS = ("dctae_rec_loss_forward", "dctae_rec_loss_backward", "dctae_norm_inverse_backward")


def tables(PP):
    """patchnorm_ref.npz's (3, 32, 32, 196) tables, last axis cropped or tiled to PP (as the generator)"""
    g = golden("patchnorm_ref.npz")
    idx = np.arange(PP) % g["median"].shape[-1]
    return torch.from_numpy(g["median"][..., idx].copy()), torch.from_numpy(g["b"][..., idx].copy())


def case(pkg, name, device="cpu"):
    P = PSIZE[name]
    med, b = tables(P * P)
    pn = pkg.PatchNorm(32, 32, P, 3)
    pn.median.data.copy_(med)
    pn.b.data.copy_(b)
    pn.frozen = True
    pn = pn.eval().to(device)
    t = {k: torch.from_numpy(G[f"{name}_{k}"]).to(device) for k in ("out", "tn", "raw", "ch", "pos", "key_pad", "codes")}

    def dp(x):
        return pkg.DCTPatches(patches=x, key_pad_mask=t["key_pad"], batched_image_ids=torch.zeros_like(t["ch"]),
                              patch_channels=t["ch"], patch_positions=t["pos"], patch_sizes=[], original_sizes=[])
    return pn, t, dp


def restated_f64(name):
    """main.py:71, 79-83 in float64: both losses and the gradient of W0 rec + W1 unn"""
    P = PSIZE[name]
    med, b = (x.double() for x in tables(P * P))
    out, tn, raw = (torch.from_numpy(G[f"{name}_{k}"]).double() for k in ("out", "tn", "raw"))
    ch, pos, kp = (torch.from_numpy(G[f"{name}_{k}"]) for k in ("ch", "pos", "key_pad"))
    m = (~kp)[..., None].double()
    N = m.sum() * (P * P)
    std = b[ch, pos[..., 0], pos[..., 1]] * 2 ** 0.5 + 1e-6
    d1 = out - tn
    d2 = (out * std + med[ch, pos[..., 0], pos[..., 1]]) - raw
    rec, unn = (d1.abs() * m).sum() / N, (d2.abs() * m).sum() / N
    grad = torch.zeros_like(out) if N == 0 else m * (W0 * torch.sign(d1) + W1 * std * torch.sign(d2)) / N
    return rec, unn, grad


def close_or_both_nan(got, want, tol):
    return (np.isnan(got) and np.isnan(want)) or abs(got - want) <= tol


@pytest.mark.parametrize("name", NAMES)
def test_torch_branch_reproduces_the_reference(pkg, name):
    pn, t, dp = case(pkg, name)
    out = t["out"].clone().requires_grad_(True)
    rec, unn, un = pkg.reconstruction_losses(dp(out), dp(t["tn"]), dp(t["raw"]), pn)
    for key, val in (("rec", rec), ("unn", unn)):
        want = float(G[f"{name}_{key}_f32"])
        assert close_or_both_nan(val.item(), want, FLOOR * abs(want)), (key, val.item(), want)
    grad, = torch.autograd.grad(W0 * rec + W1 * unn, out)
    assert torch.equal(grad, torch.from_numpy(G[f"{name}_grad_f32"]))
    assert torch.all(grad[t["key_pad"]] == 0)
    std = pn.b[t["ch"], t["pos"][..., 0], t["pos"][..., 1]] * 2 ** 0.5 + pn.eps
    assert torch.equal(un, t["out"] * std + pn.median[t["ch"], t["pos"][..., 0], t["pos"][..., 1]])
    assert pkg.reconstruction_losses(dp(out), dp(t["tn"]), dp(t["raw"]), pn, want_unnormalized=False)[2] is None


@pytest.mark.parametrize("name", NAMES)
def test_float64_restatement(name):
    rec, unn, grad = restated_f64(name)
    for key, val in (("rec", rec), ("unn", unn)):
        assert close_or_both_nan(float(val), float(G[f"{name}_{key}_f64"]), 1e-12)
    assert np.abs(grad.numpy() - G[f"{name}_grad_f64"]).max() <= 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_masked_perplexity(pkg, name):
    codes, mask = torch.from_numpy(G[f"{name}_codes"]), ~torch.from_numpy(G[f"{name}_key_pad"])
    want = float(G[f"{name}_perplexity"])
    got = pkg.masked_perplexity(codes, mask, 2 ** int(G["codebook"][0])).item()
    assert close_or_both_nan(got, want, FLOOR * abs(want)), (got, want)


def test_step_losses_on_cpu(pkg):
    """the dict of main.py:85-93 from a dense-distance result, torch ops throughout"""
    name = "p5"
    pn, t, dp = case(pkg, name)
    out = t["out"].clone().requires_grad_(True)
    cd, ncb = (int(v) for v in G["codebook"])
    h = (torch.randn(*t["ch"].shape, ncb, cd, generator=torch.Generator().manual_seed(1)) * 0.01).requires_grad_(True)
    res = dict(dct_patches=dp(out), codes=t["codes"], commit_loss=(h ** 2).mean(),
               distances=pkg.LFQDistance(h, 1.0, cd, ncb))
    d = pkg.step_losses(res, dp(t["raw"]), dp(t["tn"]), pn, 2 ** cd)
    assert set(d) == {"rec_patches", "rec_patches_unnormalized", "rec_loss", "rec_loss_unnormalized", "perplexity",
                      "commit_loss", "entropy_loss"}
    assert abs(d["rec_loss"].item() - float(G[f"{name}_rec_f32"])) <= FLOOR
    assert isinstance(d["rec_patches_unnormalized"], pkg.DCTPatches) and d["rec_patches"].patches is out
    sum(v for k, v in d.items() if "loss" in k).backward()
    assert out.grad.abs().sum() > 0 and h.grad.abs().sum() > 0
    assert pkg.step_losses(res, dp(t["raw"]), dp(t["tn"]), pn, 2 ** cd, training=False)["entropy_loss"] == 0.0


def test_header_declares_and_library_exports_the_entry_points(pkg):
    with open(os.path.join(ROOT, "include", "dctae.h")) as f:
        text = f.read()
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert f"int {s}(" in text
        assert getattr(lib, s).restype is not None
    assert "#define DCTAE_ABI_VERSION 1" in text and lib.dctae_abi_version() == 1
