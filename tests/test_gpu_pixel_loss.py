"""The differentiable postprocess (dctae_decode_backward) and the fused pixel
loss (dctae_pixel_loss_forward) against the reference's own run of
FE.postprocess and main.py:95-110 under autograd, recorded in
tests/golden/pixel_loss_ref*.npz (gen_pixel_loss_golden.py).

Oracle: the fixture's float64 entries.  Allowances, per image over that
image's tokens (deviations are max |difference|):
  vjp gradient   max(4 x the reference's own fp32 deviation from float64,
                 2e-6 x max |g_f64|): the factor 4 is the project's convention
                 (test_gpu_rec_loss, test_gpu_lfq_train), the floor its
                 DCT-coefficient tolerance (test_gpu_parity);
  loss           (a) against mean_i mse in float64 of the images the call
                 returns: 2^-20 relative, the floor for a re-ordered sum;
                 (b) against the fixture: max(4 x reference fp32 deviation,
                 mean_i(2 e sqrt(mse_i) + e^2)), e = 1e-5 max(1, max |x_i|), the
                 accepted RGB error (test_gpu_parity _rgb_close) through the square;
  loss gradient  (c) max(4 x reference fp32 deviation, 2e-6 x max |g_f64|);
                 (d) the fused backward against autograd through
                 sum_i F.mse_loss / n on the differentiable postprocess:
                 1e-5 x max |g| per image (a wrong per-image or n_img scale).
Run on an MI355X.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from test_pixel_loss_host import CFG, G, NAMES, token_image, upstream

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 2.0 ** -20


def ops():
    from dct_autoencoder_amd import _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def reference_colour_matrices(pkg):
    """The fixture was recorded with the reference's colour matrices as the
    recording host computed them (tests/golden/colors.npz: rgb2lms is an fp32
    matmul, lms2rgb and ipt2lms fp32 ``.inverse()``).  ``color.matrices()``
    recomputes them on whatever host it runs on, and another CPU gives other
    last bits: measured on an MI355X host, the same float64 recipe then differs
    from the recorded one by 5.8e-5 on ragged14's vjp (max |g| 30), more than
    the whole allowance.  The matrices are a parameter of the library
    (dctae_set_color_matrices), so for this module every context -- this
    thread's, autograd's, and any created meanwhile -- gets the recorded ones."""
    from dct_autoencoder_amd import _lib, color
    g = golden("colors.npz")
    recorded = {k: torch.from_numpy(g[k].copy()) for k in ("rgb2lms", "lms2ipt", "ipt2lms", "lms2rgb")}
    original = color.matrices

    def install(m):
        keep = [m[k].contiguous().float().cpu() for k in ("rgb2lms", "lms2ipt", "ipt2lms", "lms2rgb")]
        for ctx in list(_lib._ctx_by_key.values()):
            ctx.check(ctx.lib.dctae_set_color_matrices(ctx.h, *[C.c_void_p(t.data_ptr()) for t in keep]))
    torch.cuda.synchronize()
    color.matrices = lambda: recorded
    install(recorded)
    yield
    torch.cuda.synchronize()
    color.matrices = original
    install(original())


def case(pkg, name):
    """proc, a DCTPatches factory over the recorded batch, its tensors on the device, the upstream images"""
    P, mh, mw, S = CFG[name]
    proc = pkg.DCTAutoencoderFeatureExtractor(3, P, 0.0, mh, mw, S)
    t = {k: torch.from_numpy(G[f"{name}_{k}"]).to(DEV) for k in ("patches", "out", "key_pad", "ids", "pos", "ch")}
    t["ids"], t["pos"], t["ch"] = t["ids"].long(), t["pos"].long(), t["ch"].long()
    sizes = [tuple(int(v) for v in s) for s in G[f"{name}_original_sizes"]]
    psizes = [tuple(int(v) for v in s) for s in G[f"{name}_patch_sizes"]]

    def dp(x):
        return pkg.DCTPatches(patches=x, key_pad_mask=t["key_pad"], batched_image_ids=t["ids"],
                              patch_channels=t["ch"], patch_positions=t["pos"], patch_sizes=psizes,
                              original_sizes=sizes)
    ws = [upstream(*(torch.from_numpy(G[f"{name}_w{i}_{k}"]) for k in "auv")).to(DEV) for i in range(len(sizes))]
    return proc, dp, t, ws


def check_per_image(name, what, got, g32, g64, img, floor_rel):
    """got: fp32 gradient (R, S, PP) against the float64 oracle g64, image by image (img: the image
    of every slot, -1 at padding); g32 is the oracle's own fp32 run, the yardstick.  Returns
    (dev, ref, allowance, max |g|) of every image."""
    got = got.detach().double().cpu().numpy()
    g32, g64, img = np.asarray(g32, dtype=np.float64), np.asarray(g64), np.asarray(img)
    rows = []
    for i in range(int(img.max()) + 1):
        sel = img == i
        dev, ref = np.abs(got[sel] - g64[sel]).max(), np.abs(g32[sel] - g64[sel]).max()
        tol = max(4.0 * ref, floor_rel * np.abs(g64[sel]).max())
        print(f"{name} {what} image {i}: kernel dev {dev:.3e} reference fp32 dev {ref:.3e} allowance {tol:.3e} "
              f"(max |g| {np.abs(g64[sel]).max():.3e})")
        assert dev <= tol, f"{name} {what} image {i}: {dev:.3e} > {tol:.3e}"
        rows.append((dev, ref, tol, np.abs(g64[sel]).max()))
    return rows


def check_fixture(name, what, got, key, floor_rel):
    """check_per_image against the recorded entries ``key`` of the fixture"""
    check_per_image(name, what, got, G[f"{name}_{key}_f32"], G[f"{name}_{key}_f64"], token_image(name).numpy(),
                    floor_rel)


def step_setup(pkg):
    """ragged14 as a training step: PatchNorm tables cropped to the 4 x 4 grid, a
    training-mode LFQ (6 bits x 3 codebooks, projected) as the model's output"""
    name = "ragged14"
    proc, dp, t, _ = case(pkg, name)
    P, mh, mw, _ = CFG[name]
    tabs = golden("patchnorm_ref.npz")
    pn = pkg.PatchNorm(mh, mw, P, 3)
    pn.median.data.copy_(torch.from_numpy(tabs["median"][:, :mh, :mw].copy()))
    pn.b.data.copy_(torch.from_numpy(tabs["b"][:, :mh, :mw].copy()))
    pn.frozen = True
    pn = pn.eval().to(DEV)
    tn = pn(dp(t["patches"]))
    torch.manual_seed(11)
    lfq = pkg.LFQ(dim=P * P, codebook_size=2 ** 6, num_codebooks=3).to(DEV).train()
    x = tn.clone().requires_grad_(True)
    xq, idx, commit, dist = lfq(x, mask=~t["key_pad"])
    res = dict(dct_patches=dp(xq), codes=idx, commit_loss=commit, distances=dist)
    return proc, dp, t, pn, tn, res


def test_feature_is_there(pkg):
    """the test that fails without the feature"""
    proc, dp, t, _ = case(pkg, "p5")
    x = t["out"].clone().requires_grad_(True)
    imgs = proc.postprocess(dp(x))
    assert all(im.grad_fn is not None and im.dtype == torch.float32 for im in imgs)
    with torch.no_grad():
        assert all(im.grad_fn is None for im in proc.postprocess(dp(x)))
    assert callable(pkg.pixel_loss)
    proc, dp, t, pn, tn, res = step_setup(pkg)
    d = pkg.step_losses(res, dp(t["patches"]), dp(tn), pn, 2 ** 6, decode_pixels=True, proc=proc)
    assert set(d) == {"rec_patches", "rec_patches_unnormalized", "rec_loss", "rec_loss_unnormalized", "perplexity",
                      "commit_loss", "entropy_loss", "x_hat", "pixel_loss", "x"}
    assert d["pixel_loss"].requires_grad and d["pixel_loss"].ndim == 0 and d["pixel_loss"].dtype == torch.float32
    assert len(d["x_hat"]) == len(d["x"]) == 3 and d["x"][0].shape == (3, 61, 47) and not d["x"][0].requires_grad
    assert set(pkg.step_losses(res, dp(t["patches"]), dp(tn), pn, 2 ** 6)) == set(d) - {"x_hat", "pixel_loss", "x"}
    with pytest.raises(ValueError):
        pkg.step_losses(res, dp(t["patches"]), dp(tn), pn, 2 ** 6, decode_pixels=True)


@pytest.mark.parametrize("name", NAMES)
def test_forward_is_untouched(pkg, name):
    proc, dp, t, _ = case(pkg, name)
    want = proc.postprocess(dp(t["out"]))
    got = proc.postprocess(dp(t["out"].clone().requires_grad_(True)))
    assert len(got) == len(want) == len(G[f"{name}_original_sizes"])
    for a, b in zip(got, want):
        assert a.grad_fn is not None and b.grad_fn is None
        assert torch.equal(a.detach().view(torch.int32), b.view(torch.int32))
    _, x_hat, x = pkg.pixel_loss(dp(t["out"].clone().requires_grad_(True)), dp(t["patches"]), proc)
    for a, b in zip(x_hat, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for a, b in zip(x, proc.postprocess(dp(t["patches"]))):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", NAMES)
def test_vjp_against_the_reference(pkg, name):
    proc, dp, t, ws = case(pkg, name)
    out = t["out"].clone().requires_grad_(True)
    imgs = proc.postprocess(dp(out))
    g, = torch.autograd.grad(sum((w * im).sum() for w, im in zip(ws, imgs)), out)
    assert g.dtype == torch.float32 and g.shape == out.shape
    check_fixture(name, "vjp", g, "vjp", 2e-6)
    assert torch.all(g[t["key_pad"]] == 0), "gradient at padded tokens must be exactly zero"
    ops().check_device_errors(out.device)


@pytest.mark.parametrize("name", NAMES)
def test_pixel_loss(pkg, name):
    proc, dp, t, _ = case(pkg, name)
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
    assert torch.equal(sc[0], loss.detach()) and torch.all((sc[1:].double() - mses).abs() <= FLOOR * mses)
    # (b) against the reference's float64 loss
    l32, l64 = float(G[f"{name}_loss_f32"]), float(G[f"{name}_loss_f64"])
    eps = 1e-5 * np.maximum(1.0, G[f"{name}_xmax_f64"])
    tol = max(4.0 * abs(l32 - l64), float(np.mean(2 * eps * np.sqrt(G[f"{name}_mse_f64"]) + eps ** 2)))
    print(f"{name} loss: kernel dev {abs(loss.item() - l64):.3e} reference fp32 dev {abs(l32 - l64):.3e} "
          f"allowance {tol:.3e}")
    assert abs(loss.item() - l64) <= tol
    # (c) the gradient against the reference's float64 gradient
    g, = torch.autograd.grad(loss, out)
    check_fixture(name, "pixel-loss grad", g, "grad", 2e-6)
    # (d) the fused backward against the generic route
    o2 = t["out"].clone().requires_grad_(True)
    xh2 = proc.postprocess(dp(o2))
    x2 = proc.postprocess(dp(t["patches"]))
    g2, = torch.autograd.grad(sum(F.mse_loss(a, b) for a, b in zip(x2, xh2)) / len(xh2), o2)
    img = token_image(name).to(DEV)
    for i in range(len(x2)):
        sel = img == i
        d, m = (g[sel] - g2[sel]).abs().max().item(), g2[sel].abs().max().item()
        print(f"{name} image {i}: fused vs generic backward {d:.3e}, allowance {1e-5 * m:.3e}")
        assert d <= 1e-5 * m
    ops().check_device_errors(out.device)


def _table_and_flats(pkg, proc, dp, t):
    """the image table of the batch and the flat decodes of out / patches (the library calls alone)"""
    d = dp(t["out"])
    p = proc.params(t["out"].shape[1])
    tab = ops().decode_table(p, d.batched_image_ids, d.key_pad_mask, d.patch_positions, d.patch_channels,
                             d.patch_sizes, d.original_sizes)
    flats = [ops().decode(p, tab.ids, tab.key_pad, tab.pos, tab.ch, None, None, patches=x, table=tab,
                          return_flat=True)[1] for x in (t["out"], t["patches"])]
    return tab, flats[0], flats[1]


@pytest.mark.parametrize("name", NAMES)
def test_structure(pkg, name):
    proc, dp, t, ws = case(pkg, name)
    out = t["out"].clone().requires_grad_(True)
    loss, _, _ = pkg.pixel_loss(dp(out), dp(t["patches"]), proc)
    g, = torch.autograd.grad(loss, out)
    assert torch.isfinite(g).all() and torch.all(g[t["key_pad"]] == 0)
    real = g[~t["key_pad"]].abs().amax(-1) > 0
    if name == "dup":
        # slot 0 and slot 1 share a place: the later one wins the forward and takes the gradient
        assert torch.equal(t["pos"][0, 0], t["pos"][0, 1]) and t["ch"][0, 0] == t["ch"][0, 1]
        assert torch.all(g[0, 0] == 0) and g[0, 1].abs().max() > 0 and torch.all(real[1:])
        imgs = proc.postprocess(dp(out))
        v, = torch.autograd.grad(sum((w * im).sum() for w, im in zip(ws, imgs)), out)
        assert torch.all(v[0, 0] == 0) and v[0, 1].abs().max() > 0
    else:
        assert torch.all(real)
    ops().check_device_errors(out.device)


def bit_identical_runs(pkg, proc, dp, t, poison):
    """two runs through autograd (whose thread has a context of its own) and through the
    library calls on this thread, where the option is set"""
    ops().set_option("ws_poison", poison)
    try:
        runs = []
        for _ in range(2):
            out = t["out"].clone().requires_grad_(True)
            loss, _, _ = pkg.pixel_loss(dp(out), dp(t["patches"]), proc)
            g, = torch.autograd.grad(loss, out)
            tab, fh, fx = _table_and_flats(pkg, proc, dp, t)
            sc = ops().pixel_loss_forward(tab, fh, fx)
            p = proc.params(out.shape[1])
            d1 = ops().decode_backward(p, tab, t["out"], rgb_hat=fh, rgb=fx, g=torch.ones((), device=DEV))
            d2 = ops().decode_backward(p, tab, t["out"], grad_rgb=fh)
            runs.append((loss.detach().clone(), g.clone(), sc.clone(), d1.clone(), d2.clone()))
    finally:
        ops().set_option("ws_poison", 0)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    loss, g, sc, d1, d2 = runs[0]
    assert torch.isfinite(loss) and torch.equal(sc[0], loss) and torch.equal(d1, g)
    return g, d2


@pytest.mark.parametrize("poison", [0, 1])
@pytest.mark.parametrize("name", ["ragged14", "p5", "sq512"])
def test_bit_identical_runs(pkg, name, poison):
    proc, dp, t, _ = case(pkg, name)
    bit_identical_runs(pkg, proc, dp, t, poison)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_patches_are_upcast(pkg, dtype):
    proc, dp, t, ws = case(pkg, "p5")
    o16 = t["out"].to(dtype).requires_grad_(True)
    o32 = o16.detach().float().requires_grad_(True)
    l16, l32 = (pkg.pixel_loss(dp(o), dp(t["patches"]), proc)[0] for o in (o16, o32))
    assert l16.dtype == torch.float32 and torch.equal(l16, l32)
    g16, = torch.autograd.grad(l16, o16)
    g32, = torch.autograd.grad(l32, o32)
    assert g16.dtype == dtype and torch.equal(g16, g32.to(dtype))
    i16, i32 = proc.postprocess(dp(o16)), proc.postprocess(dp(o32))
    assert all(a.dtype == torch.float32 and torch.equal(a, b) for a, b in zip(i16, i32))
    v16, = torch.autograd.grad(sum((w * im).sum() for w, im in zip(ws, i16)), o16)
    v32, = torch.autograd.grad(sum((w * im).sum() for w, im in zip(ws, i32)), o32)
    assert v16.dtype == dtype and torch.equal(v16, v32.to(dtype))


def test_staged_hooks_carry_no_grad(pkg):
    proc, dp, t, _ = case(pkg, "p5")
    proc._transform_image_out = lambda x: x
    imgs = proc.postprocess(dp(t["out"].clone().requires_grad_(True)))
    assert all(im.grad_fn is None for im in imgs)


def test_step_chain(pkg):
    """pixel_loss of step_losses reaches the model's output through the
    rec-loss backward's grad_unnorm input: (0 + g_unnorm) std + 0, the same
    product as inverse_norm's own backward, so the two routes agree to
    4 x 2^-24 x |value| (they are in fact the same fp32 operations)."""
    proc, dp, t, pn, tn, res = step_setup(pkg)
    xq = res["dct_patches"].patches
    d = pkg.step_losses(res, dp(t["patches"]), dp(tn), pn, 2 ** 6, decode_pixels=True, proc=proc)
    ga, = torch.autograd.grad(d["pixel_loss"], xq, retain_graph=True)
    o = xq.detach().clone().requires_grad_(True)
    with torch.no_grad():
        target = pn.inverse_norm(dp(tn))
    direct, x_hat, x = pkg.pixel_loss(dp(pn.inverse_norm(dp(o))), dp(target), proc)
    gb, = torch.autograd.grad(direct, o)
    assert torch.equal(d["pixel_loss"].detach(), direct.detach())
    assert all(torch.equal(a, b) for a, b in zip(d["x_hat"] + d["x"], x_hat + x))
    diff = (ga.double() - gb.double()).abs()
    print(f"step chain: max |diff| {diff.max().item():.3e}, max |g| {gb.abs().max().item():.3e}")
    assert gb[~t["key_pad"]].abs().max() > 0 and torch.all(diff <= 4 * 2.0 ** -24 * gb.double().abs())
    assert torch.all(ga[t["key_pad"]] == 0)
    # every loss of the step together still backpropagates
    total = sum(v for k, v in d.items() if "loss" in k)
    gt, = torch.autograd.grad(total, xq)
    assert torch.isfinite(total) and torch.isfinite(gt).all()


def _stage_names(ctx, fn):
    ctx.lib.dctae_timing_reset(ctx.h)
    ctx.lib.dctae_set_timing(ctx.h, 1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ctx.lib.dctae_set_timing(ctx.h, 0)
    ctx.lib.dctae_timing_collect(ctx.h)
    names = {}
    for i in range(256):
        name, ms, n = C.c_char_p(), C.c_double(), C.c_int64()
        if ctx.lib.dctae_timing_get(ctx.h, i, C.byref(name), C.byref(ms), C.byref(n)) != 0:
            break
        names[name.value.decode()] = int(n.value)
    ctx.lib.dctae_timing_reset(ctx.h)
    return names


def test_sq512_takes_the_fft_decode(pkg):
    from dct_autoencoder_amd import _lib
    proc, dp, t, _ = case(pkg, "sq512")
    ctx = _lib.context(torch.device(DEV, torch.cuda.current_device()))
    names = _stage_names(ctx, lambda: proc.postprocess(dp(t["out"].clone().requires_grad_(True))))
    assert names.get("idct_rows", 0) >= 1 and "scatter_tokens" not in names and "ipt_to_rgb" not in names, names
    names = _stage_names(ctx, lambda: pkg.pixel_loss(dp(t["out"].clone().requires_grad_(True)), dp(t["patches"]), proc))
    assert names.get("idct_rows", 0) == 2 and names.get("pixel_loss_forward", 0) == 1 and "scatter_tokens" not in names
    # the backward, called on this thread: the recompute and the adjoint stages
    tab, fh, fx = _table_and_flats(pkg, proc, dp, t)
    names = _stage_names(ctx, lambda: ops().decode_backward(proc.params(t["out"].shape[1]), tab, t["out"], grad_rgb=fh))
    assert all(names.get(k, 0) == 1 for k in ("bwd_recompute_ipt", "color_bwd", "dct_rows_bwd", "dct_cols_bwd",
                                              "gather_tokens")), names
