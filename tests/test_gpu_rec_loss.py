"""The fused reconstruction losses (dctae_rec_loss_forward / _backward) and the
differentiable PatchNorm.inverse_norm (dctae_norm_inverse_backward) against the
reference's own run of main.py:71, 79-83, recorded in
tests/golden/rec_loss_ref.npz (gen_rec_loss_golden.py).

Losses: oracle the fixture's float64 run; allowance 4 x the reference's own fp32
deviation from float64 in that case, floored at 2^-20 relative (the allowance
of test_gpu_lfq_train.py: the kernel sums in another order than torch).
Gradient: against the reference's fp32 gradient.  d1 and d2 are the same
separately rounded fp32 operations in the kernel and in torch, so the signs
must agree everywhere; an element is term1 + term2 = W0 sign(d1) / N +
W1 std sign(d2) / N with at most three roundings per term, so it must be within
4 x 2^-24 x (|term1| + |term2|).  Gradients at padded tokens are exact zeros.

Kernel geometry (dctae_rec_loss.hip): blocks of 256 threads, a thread takes one
unit (a float4 where PP % 4 == 0, else a float) per step, a block at least 256
units; up to 2048 blocks, whose partial sums one block adds, thread t taking
the partials t, t + 256, ...  The fixture's largest case ("many", 2100 tokens
of 4 floats) runs 9 blocks; test_many_blocks (2 x 3072 tokens of 196 floats:
1176 blocks) is the one in which that strided loop takes more than one step.
Its oracle is the same formula in torch on the device, fp32 and float64.
Run on an MI355X.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from test_rec_loss_host import FLOOR, G, NAMES, PSIZE, W0, W1, case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ops():
    from dct_autoencoder_amd import _ops
    return _ops


def fused(pkg, pn, t, dp, out, want_unnormalized=True):
    return pkg.reconstruction_losses(dp(out), dp(t["tn"]), dp(t["raw"]), pn, want_unnormalized)


def std_of(pn, t):
    """b * sqrt(2) + eps gathered per token with torch's fp32 ops (patchnorm.py:175)"""
    return pn.b[t["ch"], t["pos"][..., 0], t["pos"][..., 1]] * 2 ** 0.5 + pn.eps


def check_losses(name, got, f32, f64):
    for key, val, a, b in zip(("rec_loss", "rec_loss_unnormalized"), got, f32, f64):
        if np.isnan(b):
            assert np.isnan(val), (name, key, val)
            continue
        dev = abs(a - b)
        tol = max(4.0 * dev, FLOOR * abs(b))
        print(f"{name} {key}: kernel dev {abs(val - b):.3e} reference fp32 dev {dev:.3e} allowance {tol:.3e}")
        assert abs(val - b) <= tol, f"{name} {key}: {abs(val - b):.3e} > {tol:.3e}"


def check_grad(name, got, want, std, key_pad, n_real):
    """got / want: fp32 gradients of W0 rec + W1 unn; std (.., PP) fp32"""
    got, want = got.double().cpu(), want.double().cpu()
    mism = int((torch.sign(got) != torch.sign(want)).sum())
    N = max(n_real, 1) * got.shape[-1]
    bound = 4 * 2.0 ** -24 * (abs(W0) / N + abs(W1) * std.double().cpu() / N)
    excess = ((got - want).abs() - bound).max().item()
    worst = ((got - want).abs() / bound).max().item()
    print(f"{name} grad: sign mismatches {mism} of {got.numel()}, max |diff| {(got - want).abs().max().item():.3e}, "
          f"worst diff / bound {worst:.3f}, elements that differ {int((got != want).sum())}")
    assert mism == 0
    assert excess <= 0
    assert torch.all(got[key_pad.cpu()] == 0), "gradient at padded tokens must be exactly zero"


@pytest.mark.parametrize("name", NAMES)
def test_losses_and_gradient(pkg, name):
    pn, t, dp = case(pkg, name, DEV)
    out = t["out"].clone().requires_grad_(True)
    rec, unn, un = fused(pkg, pn, t, dp, out)
    assert rec.dtype == torch.float32 and rec.ndim == 0 and unn.ndim == 0 and un.shape == out.shape
    check_losses(name, (rec.item(), unn.item()), [float(G[f"{name}_{k}_f32"]) for k in ("rec", "unn")],
                 [float(G[f"{name}_{k}_f64"]) for k in ("rec", "unn")])
    grad, = torch.autograd.grad(W0 * rec + W1 * unn, out)
    n_real = int((~t["key_pad"]).sum())
    check_grad(name, grad, torch.from_numpy(G[f"{name}_grad_f32"]), std_of(pn, t), t["key_pad"], n_real)
    sc, _ = ops().rec_loss_forward(t["out"], t["tn"], t["raw"], t["ch"], t["pos"], t["key_pad"], pn.state(),
                                   pn._params(), want_unnorm=False)
    assert sc[2].item() == n_real and torch.equal(sc[:2].nan_to_num(-1), torch.stack([rec, unn]).detach().nan_to_num(-1))
    ops().check_device_errors(out.device)


@pytest.mark.parametrize("name", NAMES)
def test_unnormalized_patches_are_inverse_norm(pkg, name):
    pn, t, dp = case(pkg, name, DEV)
    want = pn.inverse_norm(dp(t["out"]))
    assert want.grad_fn is None
    _, _, un = fused(pkg, pn, t, dp, t["out"].clone().requires_grad_(True))
    assert torch.equal(un.detach().view(torch.int32), want.view(torch.int32))
    assert fused(pkg, pn, t, dp, t["out"], want_unnormalized=False)[2] is None


@pytest.mark.parametrize("name", NAMES)
def test_inverse_norm_is_differentiable(pkg, name):
    """the test that fails without the feature: inverse_norm of a tensor that
    requires grad had no grad_fn"""
    pn, t, dp = case(pkg, name, DEV)
    x = t["out"].clone().requires_grad_(True)
    y = pn.inverse_norm(dp(x))
    assert y.grad_fn is not None
    assert torch.equal(y.detach().view(torch.int32), pn.inverse_norm(dp(t["out"])).view(torch.int32))
    y.sum().backward()
    assert torch.equal(x.grad, std_of(pn, t))
    up = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    g, = torch.autograd.grad((pn.inverse_norm(dp(x)) * up).sum(), x)
    assert torch.equal(g, up * std_of(pn, t))


def test_padding_values_are_never_read(pkg):
    name = "p5"
    pn, t, dp = case(pkg, name, DEV)
    base = fused(pkg, pn, t, dp, t["out"])
    poisoned = dict(t)
    for k in ("tn", "raw"):
        poisoned[k] = t[k].clone()
        poisoned[k][t["key_pad"]] = float("nan")
    out = t["out"].clone().requires_grad_(True)
    rec, unn, _ = fused(pkg, pn, poisoned, dp, out)
    assert torch.isfinite(rec) and torch.isfinite(unn) and torch.equal(rec, base[0]) and torch.equal(unn, base[1])
    g, = torch.autograd.grad(rec + unn, out)
    assert torch.isfinite(g).all() and torch.all(g[t["key_pad"]] == 0)
    r, s = torch.nonzero(~t["key_pad"])[0].tolist()
    for k in ("tn", "raw"):
        bad = dict(t)
        bad[k] = t[k].clone()
        bad[k][r, s, 3] = float("nan")
        rec, unn, _ = fused(pkg, pn, bad, dp, t["out"])
        assert torch.isnan(rec) == (k == "tn") and torch.isnan(unn) == (k == "raw")
    bad_out = t["out"].clone()
    bad_out[r, s, 3] = float("nan")
    rec, unn, _ = fused(pkg, pn, t, dp, bad_out)
    assert torch.isnan(rec) and torch.isnan(unn)


def test_bad_index_raises(pkg):
    name = "p5"
    pn, t, dp = case(pkg, name, DEV)
    r, s = torch.nonzero(~t["key_pad"])[0].tolist()
    bad = dict(t)
    bad["pos"] = t["pos"].clone()
    bad["pos"][r, s, 1] = 32          # one past max_patch_w

    def dp_bad(x):
        d = dp(x)
        d.patch_positions = bad["pos"]
        return d
    out = t["out"].clone().requires_grad_(True)
    rec, unn, un = pkg.reconstruction_losses(dp_bad(out), dp_bad(t["tn"]), dp_bad(t["raw"]), pn)
    assert torch.isnan(rec) and torch.isnan(unn) and torch.isnan(un[r, s]).all()
    with pytest.raises(Exception, match="out of range"):
        ops().check_device_errors(out.device)
    # the backward runs on autograd's thread, which has a context (and an error flag) of its own:
    # what shows here is the NaN gradient of that token
    g, = torch.autograd.grad(rec + unn, out)
    assert torch.isnan(g[r, s]).all()
    sc, _ = ops().rec_loss_forward(t["out"], t["tn"], t["raw"], t["ch"], t["pos"], t["key_pad"], pn.state(),
                                   pn._params(), want_unnorm=False)
    ops().rec_loss_backward(t["out"], t["tn"], t["raw"], t["ch"], bad["pos"], t["key_pad"], pn.state(), pn._params(),
                            sc, torch.ones(2, device=DEV))
    with pytest.raises(Exception, match="out of range"):
        ops().check_device_errors(out.device)
    # a bad index on a padded token is not looked at unless the unnormalized patches are wanted
    rp, sp = torch.nonzero(t["key_pad"])[0].tolist()
    bad["pos"] = t["pos"].clone()
    bad["pos"][rp, sp, 0] = -1
    rec, unn, _ = pkg.reconstruction_losses(dp_bad(t["out"]), dp_bad(t["tn"]), dp_bad(t["raw"]), pn,
                                            want_unnormalized=False)
    ops().check_device_errors(out.device)
    assert torch.isfinite(rec) and torch.isfinite(unn)


@pytest.mark.parametrize("poison", [0, 1])
@pytest.mark.parametrize("name", ["p14", "p5", "many"])
def test_bit_identical_runs(pkg, name, poison):
    pn, t, dp = case(pkg, name, DEV)
    ops().set_option("ws_poison", poison)
    try:
        runs = []
        for _ in range(2):
            out = t["out"].clone().requires_grad_(True)
            rec, unn, un = fused(pkg, pn, t, dp, out)
            g, = torch.autograd.grad(W0 * rec + W1 * unn, out)
            runs.append((rec.detach().clone(), unn.detach().clone(), un.detach().clone(), g.clone()))
    finally:
        ops().set_option("ws_poison", 0)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert torch.isfinite(runs[0][0]) and torch.isfinite(runs[0][1])


@pytest.mark.parametrize("name", ["p14", "p5", "row"])
def test_upstream_gradient_of_unnormalized_patches(pkg, name):
    """(unnorm * w).sum() + rec: the fused backward with unnorm's upstream
    gradient against torch ops on the same device tensors.  An element is
    w std + sign(d1) / N, a product and a quotient rounded once on either side
    and their sum: within 4 x 2^-24 x (|w std| + 1 / N)."""
    pn, t, dp = case(pkg, name, DEV)
    mask = ~t["key_pad"]
    w = torch.randn(t["out"].shape, generator=torch.Generator().manual_seed(7)).to(DEV)
    a = t["out"].clone().requires_grad_(True)
    rec, _, un = fused(pkg, pn, t, dp, a)
    ga, = torch.autograd.grad((un * w).sum() + rec, a)
    b = t["out"].clone().requires_grad_(True)
    std = std_of(pn, t)
    un_t = b * std + pn.median[t["ch"], t["pos"][..., 0], t["pos"][..., 1]]
    rec_t = F.l1_loss(b[mask], t["tn"][mask])
    gb, = torch.autograd.grad((un_t * w).sum() + rec_t, b)
    assert torch.equal(un.detach(), un_t.detach())
    assert abs(rec.item() - rec_t.item()) <= 4 * FLOOR * abs(rec_t.item())
    N = int(mask.sum()) * a.shape[-1]
    bound = 4 * 2.0 ** -24 * ((w * std).abs().double() + 1.0 / N)
    diff = (ga.double() - gb.double()).abs()
    print(f"{name} upstream: max |diff| {diff.max().item():.3e}, worst diff / bound {(diff / bound).max().item():.3f}")
    assert torch.all(diff <= bound)
    assert torch.equal(ga[t["key_pad"]], (w * std)[t["key_pad"]])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_outputs_are_upcast(pkg, dtype):
    name = "p5"
    pn, t, dp = case(pkg, name, DEV)
    o16 = t["out"].to(dtype).requires_grad_(True)
    o32 = o16.detach().float().requires_grad_(True)
    r16, r32 = fused(pkg, pn, t, dp, o16), fused(pkg, pn, t, dp, o32)
    assert r16[0].dtype == torch.float32 and r16[2].dtype == torch.float32
    assert all(torch.equal(a, b) for a, b in zip(r16, r32))
    g16, = torch.autograd.grad(r16[0] + r16[1], o16)
    g32, = torch.autograd.grad(r32[0] + r32[1], o32)
    assert g16.dtype == dtype and torch.equal(g16, g32.to(dtype))


def test_step_losses(pkg):
    """the dict of main.py:85-93 on a training-mode LFQ's output (6 bits x 3
    codebooks, projected to the 25-float tokens of the case "p5")"""
    name = "p5"
    pn, t, dp = case(pkg, name, DEV)
    mask = ~t["key_pad"]
    torch.manual_seed(11)
    lfq = pkg.LFQ(dim=25, codebook_size=2 ** 6, num_codebooks=3).to(DEV).train()
    x = t["tn"].clone().requires_grad_(True)
    xq, idx, commit, dist = lfq(x, mask=mask)
    res = dict(dct_patches=dp(xq), codes=idx, commit_loss=commit, distances=dist)
    d = pkg.step_losses(res, dp(t["raw"]), dp(t["tn"]), pn, 2 ** 6)
    assert set(d) == {"rec_patches", "rec_patches_unnormalized", "rec_loss", "rec_loss_unnormalized", "perplexity",
                      "commit_loss", "entropy_loss"}
    assert d["rec_patches"].patches is xq and isinstance(d["rec_patches_unnormalized"], pkg.DCTPatches)
    assert torch.equal(d["rec_patches_unnormalized"].patches.detach(), pn.inverse_norm(dp(xq.detach())))
    assert torch.equal(d["entropy_loss"], pkg.compute_entropy_loss(dist, mask))
    want = pkg.calculate_perplexity(idx[mask], 2 ** 6)
    assert abs(d["perplexity"].item() - want.item()) <= FLOOR * want.item() and not d["perplexity"].requires_grad
    losses = [v for k, v in d.items() if "loss" in k]
    assert len(losses) == 4 and all(torch.isfinite(v) for v in losses)
    sum(losses).backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad[mask].abs().sum() > 0
    assert all(p.grad is not None and p.grad.abs().sum() > 0 for p in (lfq.project_in.weight, lfq.project_out.weight))
    ev = pkg.step_losses(res, dp(t["raw"]), dp(t["tn"]), pn, 2 ** 6, training=False)
    assert ev["entropy_loss"] == 0.0


def test_many_blocks(pkg):
    """2 x 3072 tokens of 196 floats, about 10 % padding: 1176 blocks, so the
    finishing block's threads each add several partials.  Oracle: the reference
    formula with torch ops on the device, in fp32 (the gradient, and the
    yardstick of the loss allowance) and in float64 (the losses)."""
    g = torch.Generator().manual_seed(21)
    R, S, P = 2, 3072, 14
    PP = P * P
    tabs = golden("patchnorm_ref.npz")
    pn = pkg.PatchNorm(32, 32, P, 3)
    pn.median.data.copy_(torch.from_numpy(tabs["median"]))
    pn.b.data.copy_(torch.from_numpy(tabs["b"]))
    pn.frozen = True
    pn = pn.eval().to(DEV)
    t = {"ch": torch.randint(0, 3, (R, S), generator=g).to(DEV), "pos": torch.randint(0, 32, (R, S, 2), generator=g).to(DEV),
         "key_pad": (torch.rand(R, S, generator=g) < 0.1).to(DEV), "tn": torch.randn(R, S, PP, generator=g).to(DEV)}
    t["out"] = t["tn"] + 0.3 * torch.randn(R, S, PP, generator=g).to(DEV)
    std = std_of(pn, t)
    med = pn.median[t["ch"], t["pos"][..., 0], t["pos"][..., 1]]
    t["raw"] = (t["tn"] * std + med) + 0.3 * std * torch.randn(R, S, PP, generator=g).to(DEV)
    mask = ~t["key_pad"]

    def dp(x):
        return pkg.DCTPatches(patches=x, key_pad_mask=t["key_pad"], batched_image_ids=torch.zeros_like(t["ch"]),
                              patch_channels=t["ch"], patch_positions=t["pos"], patch_sizes=[], original_sizes=[])

    def torch_ops(dtype):
        o = t["out"].to(dtype).requires_grad_(True)
        s = pn.b.to(dtype)[t["ch"], t["pos"][..., 0], t["pos"][..., 1]] * 2 ** 0.5 + pn.eps
        un = o * s + pn.median.to(dtype)[t["ch"], t["pos"][..., 0], t["pos"][..., 1]]
        rec, unn = F.l1_loss(o[mask], t["tn"].to(dtype)[mask]), F.l1_loss(un[mask], t["raw"].to(dtype)[mask])
        gr, = torch.autograd.grad(W0 * rec + W1 * unn, o)
        return rec.item(), unn.item(), gr
    r32, u32, g32 = torch_ops(torch.float32)
    r64, u64, _ = torch_ops(torch.float64)
    out = t["out"].clone().requires_grad_(True)
    rec, unn, un = fused(pkg, pn, t, dp, out)
    check_losses("6144 tokens", (rec.item(), unn.item()), (r32, u32), (r64, u64))
    grad, = torch.autograd.grad(W0 * rec + W1 * unn, out)
    check_grad("6144 tokens", grad, g32, std, t["key_pad"], int(mask.sum()))
    assert torch.equal(un.detach(), pn.inverse_norm(dp(t["out"])))
