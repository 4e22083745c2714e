"""LFQ training mode on the fused HIP losses (dctae_lfq_entropy_forward /
_backward) against the reference's own LFQ.forward (training) and
compute_entropy_loss, recorded in tests/golden/lfq_train_ref.npz and
lfq_train_ref_big.npz (gen_lfq_train_golden.py).

Oracle: the fixture's float64 run.  Allowance per quantity and case: 4 x the
reference's own fp32 deviation from float64 in that case (read from the
fixture), with a floor of 2^-20 relative for the two losses and 2^-20 x
max|grad| for the gradients.  The factor 4: the kernel sums in another order
than torch, and the reference's own rounding is the only yardstick there is.
avg_probs has no fp32 run in the fixture; its allowance, measured against max
avg_probs, is (d + 2) x 2^-22: each of the d factors of a code's probability
carries up to four fp32 roundings (the scaled logit, its division by the
temperature, exp, the reciprocal), 2^-24 each, and the fp32 MFMA accumulation
and the mean add the rest.

Tile constants (dctae_lfq_entropy.hip): 32 rows ((token, codebook) pairs) per
chunk, at least 4 chunks per block.  The case "big" (2 x 700 tokens x 2
codebooks = 2800 rows = 88 chunks) runs 22 blocks of 4 chunks each; "l" (288
rows = 9 chunks) runs 3 blocks of 4 / 4 / 1 chunks; the 2 x 37 token cases run
2 blocks (e.g. 222 rows = 7 chunks: 4 + 3).  "d14" is the only case whose
histogram is a full 128 x 128 tile; d = 15 / 16 (2 / 4 tiles per row block) are
covered by test_wide_codebooks against the dense branch.
Run on an MI355X.
"""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = dict(golden("lfq_train_ref.npz"))
G.update(golden("lfq_train_ref_big.npz"))
NAMES = [str(n) for n in G["names"]]
CFG = {n: (int(c[0]), int(c[1]), int(c[2]) or None, float(s)) for n, c, s in zip(NAMES, G["cfg"], G["scales"])}
FLOOR = 2.0 ** -20


def build(pkg, name):
    cd, ncb, dim, s = CFG[name]
    m = pkg.LFQ(dim=dim, codebook_size=2 ** cd, num_codebooks=ncb, codebook_scale=s)
    if dim is not None:
        with torch.no_grad():
            for k, p in (("w_in", m.project_in.weight), ("b_in", m.project_in.bias),
                         ("w_out", m.project_out.weight), ("b_out", m.project_out.bias)):
                p.copy_(torch.from_numpy(G[f"{name}_{k}"]))
    return m.to(DEV)


def run(pkg, name):
    m = build(pkg, name).train()
    x = torch.from_numpy(G[f"{name}_x"]).to(DEV).requires_grad_(True)
    mask = torch.from_numpy(G[f"{name}_mask"]).to(DEV)
    xq, idx, commit, dist = m(x, mask=mask)
    ent = pkg.compute_entropy_loss(dist, mask)
    return m, x, mask, xq, idx, commit, dist, ent


def allow(name, key, scale):
    """4 x the reference's fp32 deviation from float64, floored at 2^-20 x scale"""
    dev = np.abs(G[f"{name}_{key}_f32"].astype(np.float64) - G[f"{name}_{key}_f64"]).max()
    return max(4.0 * dev, FLOOR * scale), dev


def check(name, what, got, want, tol, ref_dev):
    err = float(np.abs(np.asarray(got, dtype=np.float64) - want).max())
    print(f"{name} {what}: kernel dev {err:.3e} reference fp32 dev {ref_dev:.3e} allowance {tol:.3e}")
    assert err <= tol, f"{name} {what}: {err:.3e} > {tol:.3e}"


def mask_rows(name, x):
    """the input's mask, broadcast to x's shape (image form: (b, d, h, w))"""
    mk = torch.from_numpy(G[f"{name}_mask"])
    if x.ndim == 4:
        return mk.view(x.shape[0], 1, *x.shape[2:]).expand_as(x)
    return mk[..., None].expand_as(x)


@pytest.mark.parametrize("name", NAMES)
def test_losses_and_outputs(pkg, name):
    cd = CFG[name][0]
    m, x, mask, xq, idx, commit, dist, ent = run(pkg, name)
    assert dist.shape == (*dist.h.shape[:3], 2 ** cd) and dist.dtype == torch.float32
    assert ent.dtype == torch.float32 and ent.ndim == 0 and commit.ndim == 0
    for key, val in (("entropy", ent), ("commit", commit)):
        want = float(G[f"{name}_{key}_f64"])
        tol, dev = allow(name, key, abs(want))
        check(name, key, val.item(), want, tol, dev)
    from dct_autoencoder_amd import losses
    avg, sc = losses.fused_losses(dist, mask)
    want = G[f"{name}_avg_probs_f64"]
    check(name, "avg_probs", avg.cpu().numpy(), want, (cd + 2) * 2.0 ** -22 * want.max(), float("nan"))
    assert sc[4].item() == float(G[f"{name}_mask"].sum())
    assert torch.equal(idx.cpu(), torch.from_numpy(G[f"{name}_idx"]))
    # perplexity = 2^H: the fixture's H (bits) was summed on a CPU, this one on the GPU in
    # another order; each term p log2 p carries three roundings (division, log2, product)
    # and each reduction about log2(n) more on partial sums <= H: 8 x 2^-24 x H on H
    ppl = pkg.calculate_perplexity(idx, 2 ** cd)
    H = np.log2(float(G[f"{name}_perplexity"]))
    assert abs(np.log2(ppl.item()) - H) <= 8 * 2.0 ** -24 * max(H, 1.0)


@pytest.mark.parametrize("name", NAMES)
def test_gradients(pkg, name):
    m, x, mask, xq, idx, commit, dist, ent = run(pkg, name)
    params = [m.project_in.weight, m.project_in.bias] if m.has_projections else []
    gx, *gp = torch.autograd.grad(ent + commit, [x] + params, retain_graph=True)
    want = G[f"{name}_g_entropy_f64"] + G[f"{name}_g_commit_f64"]
    ref32 = G[f"{name}_g_entropy_f32"].astype(np.float64) + G[f"{name}_g_commit_f32"].astype(np.float64)
    dev = np.abs(ref32 - want).max()
    check(name, "grad", gx.cpu().numpy(), want, max(4.0 * dev, FLOOR * np.abs(want).max()), dev)
    assert torch.all(gx.cpu()[~mask_rows(name, gx)] == 0), "gradient at masked-out tokens must be exactly zero"
    gst, = torch.autograd.grad(xq.sum(), x)
    want = G[f"{name}_g_st_f64"]
    tol, dev = allow(name, "g_st", np.abs(want).max())
    check(name, "straight-through grad", gst.cpu().numpy(), want, tol, dev)
    for key, g in zip(("gw", "gb"), gp):
        want = G[f"{name}_{key}_f64"]
        tol, dev = allow(name, key, np.abs(want).max())
        check(name, key, g.cpu().numpy(), want, tol, dev)


@pytest.mark.parametrize("name", NAMES)
def test_fused_agrees_with_dense_branch(pkg, name):
    m, x, mask, xq, idx, commit, dist, ent = run(pkg, name)
    dense = pkg.compute_entropy_loss(dist.materialize(), mask)
    want = float(G[f"{name}_entropy_f64"])
    tol, dev = allow(name, "entropy", abs(want))
    check(name, "fused - dense", ent.item(), dense.item(), tol, dev)
    g_f, = torch.autograd.grad(ent, x, retain_graph=True)
    g_d, = torch.autograd.grad(dense, x)
    want = G[f"{name}_g_entropy_f64"]
    tol, dev = allow(name, "g_entropy", np.abs(want).max())
    check(name, "fused - dense grad", g_f.cpu().numpy(), g_d.cpu().numpy().astype(np.float64), tol, dev)


@pytest.mark.parametrize("name", ["d13", "big", "proj"])
def test_bit_identical_runs(pkg, name):
    outs = []
    for _ in range(2):
        m, x, mask, xq, idx, commit, dist, ent = run(pkg, name)
        g, = torch.autograd.grad(ent + commit, x)
        outs.append((ent.detach().clone(), commit.detach().clone(), g.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_padding_values_are_never_read(pkg):
    """deliberate deviation: a NaN in a masked-out token leaves the losses
    alone (the reference's mask multiplication would turn them NaN); a NaN in
    a masked-in token gives NaN; an all-False mask gives NaN"""
    name = "d6"
    m = build(pkg, name).train()
    x0 = torch.from_numpy(G[f"{name}_x"]).to(DEV)
    mask = torch.from_numpy(G[f"{name}_mask"]).to(DEV)
    _, _, c0, d0 = m(x0, mask=mask)
    e0 = pkg.compute_entropy_loss(d0, mask)
    x1 = x0.clone()
    x1[~mask] = float("nan")
    x1.requires_grad_(True)
    _, _, c1, d1 = m(x1, mask=mask)
    e1 = pkg.compute_entropy_loss(d1, mask)
    assert torch.equal(e0, e1) and torch.equal(c0, c1)
    g, = torch.autograd.grad(e1 + c1, x1)
    assert torch.all(g[~mask] == 0) and torch.isfinite(g[mask]).all()
    x2 = x0.clone()
    b, n = torch.nonzero(mask)[0].tolist()
    x2[b, n, 0] = float("nan")
    _, _, c2, d2 = m(x2, mask=mask)
    assert torch.isnan(pkg.compute_entropy_loss(d2, mask)) and torch.isnan(c2)
    none = torch.zeros_like(mask)
    _, _, c3, d3 = m(x0, mask=none)
    assert torch.isnan(pkg.compute_entropy_loss(d3, none)) and torch.isnan(c3)


@pytest.mark.parametrize("cd", [15, 16])
def test_wide_codebooks(pkg, cd):
    """2 / 4 histogram tiles per row block and the backward's large LDS form,
    against the package's dense branch.  Allowance: 2^-20 relative on the loss,
    and on the gradient the largest fp32 deviation the reference itself shows
    in the fixture's unsaturated cases (2e-5 of max|grad|, the issue's figure)."""
    g = torch.Generator().manual_seed(cd)
    m = pkg.LFQ(codebook_size=2 ** cd, num_codebooks=1).to(DEV).train()
    x = (torch.randn(2, 19, cd, generator=g) * 0.004).to(DEV).requires_grad_(True)
    mask = (torch.rand(2, 19, generator=g) < 0.7).to(DEV)
    _, _, commit, dist = m(x, mask=mask)
    ent = pkg.compute_entropy_loss(dist, mask)
    dense = pkg.compute_entropy_loss(dist.materialize(), mask)
    assert abs(ent.item() - dense.item()) <= 4 * FLOOR * abs(dense.item())
    g_f, = torch.autograd.grad(ent, x, retain_graph=True)
    g_d, = torch.autograd.grad(dense, x)
    assert (g_f - g_d).abs().max().item() <= 2e-5 * g_d.abs().max().item()


def test_model_entropy_loss(pkg):
    enc = dict(hidden_size=64, intermediate_size=128, num_attention_heads=1, num_hidden_layers=1)
    model = pkg.DCTAutoencoder(pkg.DCTAutoencoderConfig(vq_codebook_size=2 ** 6, vq_num_codebooks=3,
                                                         encoder_config=enc, decoder_config=enc))
    m, x, mask, xq, idx, commit, dist, ent = run(pkg, "d6")
    assert torch.equal(model.entropy_loss(dist, mask), ent)
    dense = dist.materialize().detach()
    assert torch.equal(model.entropy_loss(dense, mask), pkg.compute_entropy_loss(dense, mask))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_features_are_upcast(pkg, dtype):
    """non-fp32 features: the kernel sees their exact fp32 values; losses and
    gradient come back in the features' dtype"""
    name = "d6"
    mask = torch.from_numpy(G[f"{name}_mask"]).to(DEV)
    x16 = torch.from_numpy(G[f"{name}_x"]).to(DEV).to(dtype).requires_grad_(True)
    x32 = x16.detach().float().requires_grad_(True)
    m16, m32 = build(pkg, name).to(dtype).train(), build(pkg, name).train()
    xq16, idx16, c16, d16 = m16(x16, mask=mask)
    xq32, idx32, c32, d32 = m32(x32, mask=mask)
    e16, e32 = pkg.compute_entropy_loss(d16, mask), pkg.compute_entropy_loss(d32, mask)
    assert d16.dtype == dtype and e16.dtype == dtype and c16.dtype == dtype and xq16.dtype == dtype
    assert torch.equal(idx16, idx32) and torch.equal(xq16.float(), xq32)
    assert torch.equal(e16, e32.to(dtype)) and torch.equal(c16, c32.to(dtype))
    g16, = torch.autograd.grad(e16.float() + c16.float(), x16)
    g32, = torch.autograd.grad(e32 + c32, x32)
    # both gradients are rounded to the dtype and autograd's sum once more: three roundings of at most max|g|
    eps = torch.finfo(dtype).eps
    assert g16.dtype == dtype and (g16.float() - g32).abs().max().item() <= 3 * eps * g32.abs().max().item()


@pytest.mark.parametrize("n,K,D", [(37, 13, 300), (16, 32, 24), (1, 1, 1), (49, 208, 196)])
def test_project_out_summation_order(pkg, n, K, D):
    """dctae_linear_ordered (project_out of the training forward): every output
    is its terms added in index order from 0, the bias last.  With +-1 inputs
    the products are exact, so a float32 loop on the CPU is the oracle bit for
    bit; n off the 16-token tile, D past one pass of the block's 256 threads.
    Gradients are those of F.linear."""
    from dct_autoencoder_amd import _ops
    from dct_autoencoder_amd.lfq import _OrderedLinear
    g = torch.Generator().manual_seed(n + K + D)
    x = torch.where(torch.rand(n, K, generator=g) < 0.5, -1.0, 1.0)
    w, b = torch.randn(D, K, generator=g), torch.randn(D, generator=g)
    want = np.zeros((n, D), np.float32)
    for k in range(K):
        want = want + x.numpy()[:, k, None] * w.numpy()[None, :, k]
    want = want + b.numpy()[None]
    assert want.dtype == np.float32
    got = _ops.linear_ordered(x.to(DEV), w.to(DEV), b.to(DEV))
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    xs = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
    ys = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
    up = torch.randn(n, D, generator=g).to(DEV)
    ga = torch.autograd.grad((_OrderedLinear.apply(*xs) * up).sum(), xs)
    gb = torch.autograd.grad((torch.nn.functional.linear(*ys) * up).sum(), ys)
    for a, c in zip(ga, gb):
        assert (a - c).abs().max().item() <= 2.0 ** -20 * max(c.abs().max().item(), 1.0) * max(n, D, K) ** 0.5


def test_unsupported_codebook_dim(pkg):
    m = pkg.LFQ(codebook_size=2 ** 17).to(DEV).train()
    x = torch.zeros(1, 4, 17, device=DEV)
    with pytest.raises(NotImplementedError):
        m(x, mask=torch.ones(1, 4, dtype=torch.bool, device=DEV))


@pytest.mark.parametrize("name", ["d6", "proj"])
def test_eval_is_unchanged(pkg, name):
    m = build(pkg, name).eval()
    x = torch.from_numpy(G[f"{name}_x"]).to(DEV)
    mask = torch.from_numpy(G[f"{name}_mask"]).to(DEV)
    q, idx, commit, dist = m(x, mask=mask)
    assert commit is m.zero and dist is m.zero
    assert torch.equal(idx.cpu(), torch.from_numpy(G[f"{name}_idx"]))


@pytest.mark.parametrize("name", NAMES)
def test_xq_bit_exact(pkg, name):
    """x_q bit for bit against the reference's.  Without projections x_q is
    the exact +-s codes.  With them it is project_out of those codes, a 32-term
    fp32 dot product per element: the training forward sums it in index order,
    bias last (dctae_linear_ordered), as the CPU GEMM behind the fixture does; a
    GPU GEMM library's order differed in 1153 of 1776 elements, by up to 3e-7."""
    m, x, mask, xq, idx, commit, dist, ent = run(pkg, name)
    want = torch.from_numpy(G[f"{name}_xq"])
    got = xq.detach().cpu()
    print(f"{name} x_q: max |diff| {(got - want).abs().max().item():.3e}, "
          f"{int((got != want).sum())} of {want.numel()} elements differ")
    assert torch.equal(got, want)
