"""dctae_decode_backward and dctae_pixel_loss_forward at the shapes the six
recorded fixtures of test_gpu_pixel_loss.py do not reach: the cases of
oracle/decode_cases.py (what each is there for is listed there and asserted by
arithmetic in test_pixel_loss_shapes_host.py), through the public API
(proc.postprocess, pkg.pixel_loss, torch.autograd.grad).

Oracle: oracle.decode_cases.oracle_results on float64 tensors, run here on the
CPU; its own fp32 run is the yardstick.  test_pixel_loss_host.py pins that
recipe to the reference's recorded losses and gradients.  Both sides use the
recorded colour matrices (the reference_colour_matrices fixture of
test_gpu_pixel_loss.py).  The allowances are those of test_gpu_pixel_loss.py
(its docstring), unchanged: the images 1e-5 + 1e-5 |x| (test_gpu_parity
_rgb_close); per image over its tokens, the vjp and (c) the loss gradient
max(4 x the oracle's fp32 deviation, 2e-6 x max |g_f64|); the loss (a) 2^-20
relative against float64 of its own images and (b) the rule of test_pixel_loss;
(d) the fused backward against autograd through the differentiable postprocess
within 1e-5 x max |g| per image.  On the CPU the fp32 yardstick of the vjp is
2-8e-7 of max |g|, so the 2e-6 floor decides nearly everywhere; that of (c) is
1e-4 - 1e-3 (the cancellation in x_hat - x), so (d) and the vjp are the sharp checks.

Measured on an MI355X: the module's 43 tests take 7.7 s, CPU oracle included
(the slowest, test_forward[many300], 1.0 s); the worst share of an allowance is
0.47 for the vjp (mixed512) and 0.71 for the loss gradient (many72), the fused
backward is within 5.0e-7 of max |g| of the generic one.  Every case's figures
are in DESIGN.md 4g.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import decode_cases as D
from test_gpu_pixel_loss import (DEV, FLOOR, _table_and_flats, bit_identical_runs, check_per_image, ops,
                                 reference_colour_matrices)  # noqa: F401  (the autouse fixture serves this module too)

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


def extractor(pkg, cfg):
    return pkg.DCTAutoencoderFeatureExtractor(3, cfg.patch_size, 0.0, cfg.max_patch_h, cfg.max_patch_w,
                                              cfg.max_seq_len)


def on_device(pkg, batch, **tensors):
    """the batch's index tensors and ``tensors`` on the device, a DCTPatches factory over them"""
    t = {"key_pad": batch.key_pad_mask, "ids": batch.batched_image_ids, "pos": batch.patch_positions,
         "ch": batch.patch_channels, **tensors}
    t = {k: v.to(DEV) for k, v in t.items()}
    psizes = [tuple(int(v) for v in s) for s in batch.patch_sizes]
    sizes = [tuple(int(v) for v in s) for s in batch.original_sizes]

    def dp(x):
        return pkg.DCTPatches(patches=x, key_pad_mask=t["key_pad"], batched_image_ids=t["ids"],
                              patch_channels=t["ch"], patch_positions=t["pos"], patch_sizes=psizes,
                              original_sizes=sizes)
    return t, dp


def case(pkg, name):
    """the case, proc, a DCTPatches factory over its batch, its tensors on the device, the upstream images"""
    c = D.build(name)
    t, dp = on_device(pkg, c.batch, patches=c.batch.patches, out=c.out)
    return c, extractor(pkg, c.cfg), dp, t, [w.to(DEV) for w in c.ws]


def same_bits(a, b):
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


@pytest.mark.parametrize("name", D.NAMES)
def test_forward(pkg, name):
    c, proc, dp, t, _ = case(pkg, name)
    r64 = D.results(name, F64)
    want = proc.postprocess(dp(t["out"]))
    got = proc.postprocess(dp(t["out"].clone().requires_grad_(True)))
    _, x_hat, x = pkg.pixel_loss(dp(t["out"].clone().requires_grad_(True)), dp(t["patches"]), proc)
    target = proc.postprocess(dp(t["patches"]))
    assert len(got) == len(want) == len(x_hat) == len(x) == len(c.sizes)
    worst = 0.0
    for i, hw in enumerate(c.sizes):
        assert want[i].shape == (3, *hw) and got[i].grad_fn is not None and want[i].grad_fn is None
        assert same_bits(got[i], want[i]) and same_bits(x_hat[i], want[i]) and same_bits(x[i], target[i])
        for a, b in ((want[i], r64["x_hat"][i]), (target[i], r64["x"][i])):
            d = (a.double().cpu() - b).abs()
            worst = max(worst, float((d / (1e-5 + 1e-5 * b.abs())).max()))
            assert torch.all(d <= 1e-5 + 1e-5 * b.abs()), f"{name} image {i}: max |dev| {float(d.max()):.3e}"
        if i in c.zero_images:
            assert torch.all(want[i] == 0)
    print(f"{name} forward: worst |dev| / (1e-5 + 1e-5 |x|) {worst:.3f}")
    ops().check_device_errors(t["out"].device)


@pytest.mark.parametrize("name", D.NAMES)
def test_vjp(pkg, name):
    c, proc, dp, t, ws = case(pkg, name)
    out = t["out"].clone().requires_grad_(True)
    imgs = proc.postprocess(dp(out))
    g, = torch.autograd.grad(sum((w * im).sum() for w, im in zip(ws, imgs)), out)
    assert g.dtype == torch.float32 and g.shape == out.shape
    check_per_image(name, "vjp", g, D.results(name, F32)["vjp"], D.results(name, F64)["vjp"], c.img.numpy(), 2e-6)
    structure(c, t, g)
    ops().check_device_errors(out.device)


def structure(c, t, g):
    """exact zeros at every padded slot (removed tokens included) and on an all-zero image, finite
    everywhere, non-zero at every other real token"""
    assert torch.isfinite(g).all()
    assert torch.all(g[t["key_pad"]] == 0), "gradient at padded tokens must be exactly zero"
    img = c.img.to(DEV)
    assert torch.equal(img < 0, t["key_pad"])
    hit = g.abs().amax(-1) > 0
    for i in range(len(c.sizes)):
        if i in c.zero_images:
            assert not hit[img == i].any(), f"image {i} is all zero: its gradient is defined as zero"
        else:
            assert hit[img == i].all(), f"image {i}: a real token without gradient"


@pytest.mark.parametrize("name", D.NAMES)
def test_pixel_loss(pkg, name):
    c, proc, dp, t, _ = case(pkg, name)
    r32, r64 = D.results(name, F32), D.results(name, F64)
    out = t["out"].clone().requires_grad_(True)
    loss, x_hat, x = pkg.pixel_loss(dp(out), dp(t["patches"]), proc)
    assert loss.dtype == torch.float32 and loss.ndim == 0 and loss.requires_grad
    assert all(im.dtype == torch.float32 and not im.requires_grad for im in x_hat + x)
    # (a) the fused reduction against torch's float64 on the same images
    mses = torch.stack([F.mse_loss(a.double(), b.double()) for a, b in zip(x, x_hat)])
    same = mses.mean().item()
    print(f"{name} loss {loss.item():.9e}: |fused - float64 of its own images| / value {abs(loss.item() - same) / same:.3e}")
    assert abs(loss.item() - same) <= FLOOR * same
    sc = ops().pixel_loss_forward(*_table_and_flats(pkg, proc, dp, t))
    assert sc.shape == (1 + len(c.sizes),) and torch.equal(sc[0], loss.detach())
    assert torch.all((sc[1:].double() - mses).abs() <= FLOOR * mses)
    # (b) against the oracle's float64 loss
    l32, l64 = float(r32["loss"]), float(r64["loss"])
    eps = 1e-5 * np.maximum(1.0, r64["xmax"])
    tol = max(4.0 * abs(l32 - l64), float(np.mean(2 * eps * np.sqrt(r64["mse"]) + eps ** 2)))
    print(f"{name} loss: kernel dev {abs(loss.item() - l64):.3e} reference fp32 dev {abs(l32 - l64):.3e} "
          f"allowance {tol:.3e}")
    assert abs(loss.item() - l64) <= tol
    # (c) the gradient against the oracle's float64 gradient
    g, = torch.autograd.grad(loss, out)
    check_per_image(name, "pixel-loss grad", g, r32["grad"], r64["grad"], c.img.numpy(), 2e-6)
    structure(c, t, g)
    # (d) the fused backward against the generic route
    o2 = t["out"].clone().requires_grad_(True)
    xh2 = proc.postprocess(dp(o2))
    x2 = proc.postprocess(dp(t["patches"]))
    g2, = torch.autograd.grad(sum(F.mse_loss(a, b) for a, b in zip(x2, xh2)) / len(xh2), o2)
    img = c.img.to(DEV)
    worst = 0.0
    for i in range(len(x2)):
        sel = img == i
        d, m = (g[sel] - g2[sel]).abs().max().item(), g2[sel].abs().max().item()
        worst = max(worst, d / m if m else 0.0)
        assert d <= 1e-5 * m, f"{name} image {i}: fused vs generic backward {d:.3e}, allowance {1e-5 * m:.3e}"
    print(f"{name}: fused vs generic backward, worst image {worst:.3e} of max |g| (allowance 1e-5)")
    ops().check_device_errors(out.device)


@pytest.mark.parametrize("name", ["mid", "mixed512"])
def test_partial_upstream(pkg, name):
    """a loss on image 1 alone: the other images' gradients reach the backward as None and their
    slots of the flat upstream buffer stay zero"""
    c, proc, dp, t, ws = case(pkg, name)

    def vjp(weights, direct=None):
        out = t["out"].clone().requires_grad_(True)
        imgs = proc.postprocess(dp(out))
        if direct is not None:
            return torch.autograd.grad(imgs[1], out, grad_outputs=direct)[0]
        return torch.autograd.grad(sum((w * im).sum() for w, im in weights(imgs)), out)[0]
    alone = vjp(lambda imgs: [(ws[1], imgs[1])])
    zeros = vjp(lambda imgs: [(w if i == 1 else torch.zeros_like(w), im) for i, (w, im) in enumerate(zip(ws, imgs))])
    assert same_bits(alone, zeros)
    img = c.img.to(DEV)
    assert torch.all(alone[img != 1] == 0) and torch.all(alone[img == 1].abs().amax(-1) > 0)
    strided = ws[1].transpose(1, 2).contiguous().transpose(1, 2)
    assert not strided.is_contiguous() and torch.equal(strided, ws[1])
    assert same_bits(vjp(None, direct=strided), alone)
    ops().check_device_errors(alone.device)


@pytest.mark.parametrize("poison", [0, 1])
@pytest.mark.parametrize("name", ["mid", "caps", "many72"])
def test_bit_identical_runs(pkg, name, poison):
    c, proc, dp, t, _ = case(pkg, name)
    g, d2 = bit_identical_runs(pkg, proc, dp, t, poison)
    assert torch.isfinite(g).all() and torch.isfinite(d2).all()


GATHER_BLOCKS, GATHER_THREADS = 16384, 256    # the grid cap of k_gather_tokens (dctae_decode_bwd.hip)


@pytest.mark.parametrize("name", list(D.GRID_CAP))
def test_gather_grid_cap(pkg, name):
    """R rows of which only the first and the last hold tokens: the last row's units belong to the
    second iteration of the gather's grid-stride loop (its ``t += dt; q += dq`` carry)"""
    small, big, out2, outR, factors = D.grid_cap_case(name)
    cfg = D.config(name)
    proc = extractor(pkg, cfg)
    R, S, PP = outR.shape
    U = PP // 4 if PP % 4 == 0 else PP           # units per token: float4 where P * P allows
    step = GATHER_BLOCKS * GATHER_THREADS
    assert R * S * U > step
    assert (R - 1) * S >= -(-step // U), "the last row is not owned by the second iteration"
    ws = [D.upstream(*f).to(DEV) for f in factors]
    n = len(ws)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()

    def run(batch, out, where):
        t, dp = on_device(pkg, batch)
        x = out.to(DEV).requires_grad_(True)
        imgs = proc.postprocess(dp(x))
        assert len(imgs) == len(batch.original_sizes)
        g, = torch.autograd.grad(sum((w * imgs[j]).sum() for w, j in zip(ws, where)), x)
        return g.cpu()
    gR = run(big, outR, [0] + [R - 2 + i for i in range(1, n)])
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"{name}: {R * S} tokens, {R * S * U} units, peak device memory {peak / 1e6:.0f} MB")
    assert peak < 200e6
    g2 = run(small, out2, list(range(n)))
    assert same_bits(gR[0], g2[0]) and same_bits(gR[R - 1], g2[1])
    assert torch.all(gR[1:R - 1] == 0)
    real = ~small.key_pad_mask
    assert torch.all(g2[real].abs().amax(-1) > 0) and torch.all(g2[~real] == 0)
    ops().check_device_errors(torch.device(DEV, torch.cuda.current_device()))
