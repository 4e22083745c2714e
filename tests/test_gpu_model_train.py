"""GPU tests of the DCTAutoencoder training step.

Operator tests compare each backward kernel with torch autograd on bf16-exact
inputs: fp32 outputs differ from torch by summation order only (1e-4 of
max|ref|, the forward tests' fp32 bound), bf16 outputs by one rounding (8e-3).
The attention gradients follow the project's 4 x yardstick rule: the distance
to the float64 gradient may be four times that of the same formula under torch
bf16 autocast (computed here), or one bf16 rounding (2^-8) of the gradient's
norm, whichever is larger.

Model tests run whole training steps on the reference's golden weights and
inputs (tests/golden/model_ref.npz): run-to-run bit identity, finite nonzero
gradients on every parameter, eval after train unchanged."""
import copy
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_model as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))
LIN_F32, LIN_BF16, LIN_F32_RESIDUAL = 0, 1, 3


def _T(pkg):
    from importlib import import_module
    return import_module("dct_autoencoder_amd.model_train")


def _bf(x):
    return x.to(torch.bfloat16)


def _bits(x, kp=None):
    """bf16 bit patterns of x (M, K), zero-padded to kp columns."""
    b = _bf(x)
    if kp is not None and kp != x.shape[1]:
        out = torch.zeros(x.shape[0], kp, dtype=torch.bfloat16, device=x.device)
        out[:, :x.shape[1]] = b
        b = out
    return b.view(torch.int16).contiguous()


def _close(got, ref, tol):
    err = (got - ref).abs().max().item()
    assert err <= tol * ref.abs().max().item() + 1e-6, (err, ref.abs().max().item())


# ---------------------------------------------------------------- linear
@pytest.mark.parametrize("m,n,k", [(77, 52, 128), (300, 200, 192), (2304, 200, 192), (130, 196, 128)])
def test_linear_backward(pkg, m, n, k):
    """dX = dY W (f32, residual and bf16 epilogues), dW = dY^T X with the token
    tail of the reduction contributing zeros, db = colsum(dY) from f32 and bf16."""
    T = _T(pkg)
    g = torch.Generator().manual_seed(m + n + k)
    x = _bf(torch.randn(m, k, generator=g)).float().to(DEV)
    w = _bf(torch.randn(n, k, generator=g) / k ** 0.5).float().to(DEV)
    dy = _bf(torch.randn(m, n, generator=g)).float().to(DEV)
    np_ = T.pad64(n)
    dyb, xb, wt = _bits(dy, np_), _bits(x), _bits(w.t().contiguous(), np_)
    assert torch.equal(T.to_bf16(dy, np_), dyb)
    dx_ref, dw_ref, db_ref = dy @ w, dy.t() @ x, dy.sum(0)
    dx = T.linear_dx(dyb, wt, k, LIN_F32, torch.empty(m, k, device=DEV))
    base = torch.randn(m, k, generator=g).to(DEV)
    dx_acc = T.linear_dx(dyb, wt, k, LIN_F32_RESIDUAL, base.clone())
    dx_b = T.linear_dx(dyb, wt, k, LIN_BF16, torch.empty(m, k, dtype=torch.int16, device=DEV))
    dw = T.linear_dw(dyb, n, xb, k)
    db, db_b = T.colsum(dy, n), T.colsum(dyb, n)
    torch.cuda.synchronize()
    _close(dx, dx_ref, 1e-4)
    _close(dx_acc, base + dx_ref, 1e-4)
    _close(dx_b.view(torch.bfloat16).float(), dx_ref, 8e-3)
    assert dw.shape == (n, k)
    _close(dw, dw_ref, 1e-4)
    _close(db, db_ref, 1e-4)
    _close(db_b, db_ref, 1e-4)


def test_transpose_pack_zero_tail(pkg):
    T = _T(pkg)
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-30000, 30000, (130, 200), generator=g, dtype=torch.int16).to(DEV)
    out = T.transpose_pack(x, 196)
    torch.cuda.synchronize()
    assert out.shape == (196, 192)
    assert torch.equal(out[:, :130], x[:, :196].t()) and not out[:, 130:].any()


# ---------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("d", [128, 1024])
def test_layernorm_backward_and_embed_norm_form(pkg, d):
    T = _T(pkg)
    m = 333
    g = torch.Generator().manual_seed(d)
    x = (torch.randn(m, d, generator=g) * 3 + 1).to(DEV).requires_grad_(True)
    gam = torch.randn(d, generator=g).to(DEV).requires_grad_(True)
    bet = torch.randn(d, generator=g).to(DEV).requires_grad_(True)
    dy = torch.randn(m, d, generator=g).to(DEV)
    for eps in (1e-5, 1e-4):   # layer_norm1/2; to_patch_embedding[1] / proj_out[0]
        dx_ref, dg_ref, db_ref = torch.autograd.grad(F.layer_norm(x, (d,), gam, bet, eps), (x, gam, bet), dy)
        dx = torch.empty(m, d, device=DEV)
        dg, db = T.layernorm_bwd(x.detach(), gam.detach(), eps, dy, dx, False)
        base = torch.randn(m, d, generator=g).to(DEV)
        acc = base.clone()
        dg2, db2 = T.layernorm_bwd(x.detach(), gam.detach(), eps, dy, acc, True)
        torch.cuda.synchronize()
        _close(dx, dx_ref, 1e-4)
        _close(acc, base + dx_ref, 1e-4)
        _close(dg, dg_ref, 1e-4)
        _close(db, db_ref, 1e-4)
        assert torch.equal(dg, dg2) and torch.equal(db, db2)
    # embed_norm: LayerNorm (eps 1e-4) + position terms; the tables' gradients
    ph, pw, pc = (torch.randn(n, d, generator=g).to(DEV).requires_grad_(True) for n in (32, 32, 3))
    ch = torch.randint(0, 3, (m,), generator=g).to(DEV)
    pos = torch.randint(0, 32, (m, 2), generator=g).to(DEV)
    y = F.layer_norm(x, (d,), gam, bet, 1e-4) + ph[pos[:, 0]] + pw[pos[:, 1]] + pc[ch]
    refs = torch.autograd.grad(y, (ph, pw, pc), dy)
    got = (T.pos_grad(dy, pos[:, 0], 32), T.pos_grad(dy, pos[:, 1], 32), T.pos_grad(dy, ch, 3))
    torch.cuda.synchronize()
    for a, b in zip(got, refs):
        _close(a, b, 1e-4)


# ---------------------------------------------------------------- quick_gelu
def test_quick_gelu_forward_backward(pkg):
    T = _T(pkg)
    m, n = 130, 200
    g = torch.Generator().manual_seed(9)
    pre = _bf(torch.randn(m, n, generator=g) * 2).float().to(DEV)
    df = _bf(torch.randn(m, n, generator=g)).float().to(DEV)
    pb, dfb = _bits(pre, 256), _bits(df, 256)
    f = T.qgelu(pb, n, torch.zeros(m, 256, dtype=torch.int16, device=DEV))
    dp = T.qgelu_bwd(dfb, pb, n, torch.zeros(m, 256, dtype=torch.int16, device=DEV))
    torch.cuda.synchronize()
    sg = torch.sigmoid(1.702 * pre)
    _close(f.view(torch.bfloat16).float()[:, :n], pre * sg, 8e-3)
    _close(dp.view(torch.bfloat16).float()[:, :n], df * sg * (1 + 1.702 * pre * (1 - sg)), 8e-3)
    assert not f[:, n:].any() and not dp[:, n:].any()


# ---------------------------------------------------------------- attention
def _packing(r, s, seed):
    """ids / key_pad of r rows: a few images per row, then padding."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(r, s, dtype=torch.long)
    kp = torch.zeros(r, s, dtype=torch.bool)
    for i in range(r):
        n = int(torch.randint(s // 2, s, (1,), generator=g))
        cuts = sorted(torch.randint(1, n, (2,), generator=g).tolist())
        ids[i, cuts[0]:cuts[1]] = 1
        ids[i, cuts[1]:n] = 2
        kp[i, n:] = True
    return ids, kp


def _attn_torch(qkv, d_out, bias, r, s, heads, dtype, autocast):
    """(lse, dqkv) of softmax(q k^T / 8 + bias) v by torch autograd."""
    d = 64 * heads
    x = qkv.to(dtype).requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        q, k, v = (x[:, i * d:(i + 1) * d].view(r, s, heads, 64).transpose(1, 2) for i in range(3))
        logits = q @ k.transpose(-1, -2) * 0.125 + bias.to(dtype)
        o = (torch.softmax(logits, -1) @ v).transpose(1, 2).reshape(r * s, d)
    g, = torch.autograd.grad(o, x, d_out.to(o.dtype))
    return torch.logsumexp(logits.detach().double(), -1), g.double()


@pytest.mark.parametrize("r,s,heads", [(2, 200, 2), (2, 320, 2), (3, 256, 1), (1, 1100, 1)])
def test_attention_lse_and_backward(pkg, r, s, heads):
    T = _T(pkg)
    d = 64 * heads
    g = torch.Generator().manual_seed(r * s + heads)
    qkv = _bf(torch.randn(r * s, 3 * d, generator=g)).float()
    d_out = _bf(torch.randn(r * s, d, generator=g)).float()
    ids, kp = _packing(r, s, s)
    bias = R.attn_bias(ids, kp)
    lse64, g64 = _attn_torch(qkv, d_out, bias, r, s, heads, torch.float64, False)
    _, gac = _attn_torch(qkv, d_out, bias, r, s, heads, torch.float32, True)
    qb, dob = _bits(qkv).to(DEV), _bits(d_out).to(DEV)
    idd, kpd = ids.to(DEV), kp.to(torch.uint8).to(DEV)
    out, lse = T.attention_lse(qb, idd, kpd, r, s, heads)
    ctx = T._c(qb)
    ref_out = torch.empty_like(out)   # the eval entry point gives the same output
    P = T._lib.ptr
    ctx.check(ctx.lib.dctae_model_attention(ctx.h, r, s, heads, 64, P(qb), P(idd), P(kpd), P(ref_out), d, T._st(qb)),
              "attention")
    dqkv = T.attention_bwd(qb, idd, kpd, out, dob, lse, r, s, heads)
    torch.cuda.synchronize()
    assert torch.equal(out, ref_out)
    lse_err = (lse.cpu().double() * math.log(2.0) - lse64).abs().max().item()
    print(f"lse max err {lse_err:.3g}")
    assert lse_err <= 1e-4
    got = dqkv.view(torch.bfloat16).double().cpu()
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * d, (i + 1) * d)
        ours = (got[:, sl] - g64[:, sl]).norm().item()
        yard = (gac[:, sl] - g64[:, sl]).norm().item()
        gn = g64[:, sl].norm().item()
        print(f"{name}: ours {ours:.4g} yardstick {yard:.4g} |g| {gn:.4g}")
        assert ours <= max(4 * yard, 2 ** -8 * gn)


# ---------------------------------------------------------------- position tables
def test_pos_grad_is_the_token_ordered_sum(pkg):
    T = _T(pkg)
    m, d = 777, 192
    g = torch.Generator().manual_seed(3)
    x = torch.randn(m, d, generator=g)
    pos = torch.randint(0, 32, (m, 2), generator=g)
    for col, rows in ((0, 32), (1, 40)):   # rows 32 .. 39 have no token: zeros
        got = T.pos_grad(x.to(DEV), pos.to(DEV)[:, col], rows)
        torch.cuda.synchronize()
        ref = torch.zeros(rows, d)
        for t in range(m):   # fp32, tokens in order
            ref[pos[t, col]] += x[t]
        assert torch.equal(got.cpu(), ref)


# ---------------------------------------------------------------- model
@pytest.fixture(scope="module")
def golden(pkg):
    d = np.load(os.path.join(HERE, "golden", "model_ref.npz"))
    w = {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w.")}
    hid, heads, inter, layers, ncb, cbs, s = [int(v) for v in d["cfg"]]
    enc = dict(hidden_size=hid, intermediate_size=inter, num_attention_heads=heads, num_hidden_layers=layers)
    cfg = pkg.DCTAutoencoderConfig(image_channels=3, patch_size=14, max_patch_h=32, max_patch_w=32,
                                   vq_codebook_size=cbs, vq_num_codebooks=ncb, vq_type="lfq", encoder_config=enc,
                                   decoder_config=enc)
    tabs = np.load(os.path.join(HERE, "golden", "patchnorm_ref.npz"))

    def make():
        m = pkg.DCTAutoencoder(cfg)
        m.load_state_dict(w, strict=False)
        m.patchnorm.median.data.copy_(torch.from_numpy(tabs["median"]))
        m.patchnorm.b.data.copy_(torch.from_numpy(tabs["b"]))
        m.patchnorm.frozen = True
        return m.to(DEV)

    t = {k: torch.from_numpy(d[k]).to(DEV) for k in d.files if not k.startswith("w.") and k != "cfg"}
    return make, t, cbs


def _dp(pkg, t, patches):
    return pkg.DCTPatches(patches=patches, key_pad_mask=t["key_pad_mask"], batched_image_ids=t["batched_image_ids"],
                          patch_channels=t["patch_channels"], patch_positions=t["patch_positions"], patch_sizes=[],
                          original_sizes=[])


WEIGHTS = dict(rec_loss=0.1, rec_loss_unnormalized=1.0, commit_loss=0.1, entropy_loss=0.1)   # main.py:311-314


def _step(pkg, m, t, cbs):
    """One training step's losses (main.py:56-93 through step_losses) and their weighted sum."""
    from importlib import import_module
    losses = import_module("dct_autoencoder_amd.losses")
    normalized = _dp(pkg, t, t["patches_in"])
    with torch.no_grad():
        raw = _dp(pkg, t, m.patchnorm.inverse_norm(_dp(pkg, t, t["patches_in"].clone())))
    res = m(normalized.shallow_copy())
    out = losses.step_losses(res, raw, normalized, m.patchnorm, cbs)
    total = sum(w * out[k] for k, w in WEIGHTS.items())
    return out, total


def test_train_step_is_deterministic_and_reaches_every_parameter(pkg, golden):
    make, t, cbs = golden
    runs = []
    for _ in range(2):
        m = make().train()
        out, total = _step(pkg, m, t, cbs)
        total.backward()
        torch.cuda.synchronize()
        runs.append(({k: out[k].detach().clone() for k in WEIGHTS}, {n: p.grad.clone() for n, p in m.named_parameters() if p.requires_grad}))
    (l0, g0), (l1, g1) = runs
    for k in WEIGHTS:
        assert torch.isfinite(l0[k]) and torch.equal(l0[k], l1[k]), k
    names = [n for n, p in make().named_parameters() if p.requires_grad]
    assert sorted(g0) == sorted(names)
    for n in names:
        assert torch.isfinite(g0[n]).all(), n
        assert torch.equal(g0[n], g1[n]), n
        # k_proj.bias: analytically zero (softmax shift invariance); rounding noise at most
        if not n.endswith("k_proj.bias"):
            assert g0[n].abs().max().item() > 0, n


def test_eval_after_train_is_bit_identical(pkg, golden):
    make, t, cbs = golden
    fresh = make().eval()
    ref = fresh(_dp(pkg, t, t["patches_in"].clone()))
    m = make().train()
    _step(pkg, m, t, cbs)[1].backward()
    m.eval()
    out = m(_dp(pkg, t, t["patches_in"].clone()))
    torch.cuda.synchronize()
    assert not out["dct_patches"].patches.requires_grad
    assert torch.equal(out["codes"], ref["codes"])
    assert torch.equal(out["dct_patches"].patches, ref["dct_patches"].patches)


def test_decode_from_codes_in_training_reaches_project_out(pkg, golden):
    make, t, cbs = golden
    m = make().train()
    kw = dict(key_pad_mask=t["key_pad_mask"], batched_image_ids=t["batched_image_ids"],
              patch_channels=t["patch_channels"], patch_positions=t["patch_positions"], patch_sizes=[], original_sizes=[])
    out = m.decode_from_codes(t["codes"], **kw).patches
    ref = m.eval().decode_from_codes(t["codes"], **kw).patches
    assert out.requires_grad and not ref.requires_grad
    _close(out.detach(), ref, 3e-2)   # the forward test's bf16 bound: eval packs project_out in bf16, training keeps it fp32
    out.square().mean().backward()
    torch.cuda.synchronize()
    for n in ("vq_model.project_out.weight", "vq_model.project_out.bias", "decoder.layers.0.mlp.fc1.weight",
              "proj_out.1.weight"):
        g = dict(m.named_parameters())[n].grad
        assert g is not None and torch.isfinite(g).all() and g.abs().max().item() > 0, n
    assert m.to_patch_embedding[0].weight.grad is None


def test_training_refusals(pkg, golden):
    make, t, cbs = golden
    m = make().train()
    with pytest.raises(NotImplementedError):
        copy.deepcopy(m).half().encode(None)
    m2 = copy.deepcopy(m)
    m2.config.encoder_config.attention_dropout = 0.1
    with pytest.raises(NotImplementedError):
        m2.encode(None)


# ---------------------------------------------------------------- model against the reference (fixture)
SEED_ENC, SEED_DEC = 7001, 7002


@pytest.fixture(scope="module")
def fx():
    import glob
    out = {}
    for path in sorted(glob.glob(os.path.join(HERE, "golden", "model_train_ref*.npz"))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def _allowance(fx, case, got, label):
    """||ours - float64||_2 <= max(4 x the bf16-autocast reference's deviation, 2^-8 ||g||_2) for every
    stored tensor of the case; prints the table."""
    bad = []
    print(f"\n{label}: tensor, ours, yardstick (reference under bf16 autocast), |g|")
    for n, g in got.items():
        ref = torch.from_numpy(fx[f"{case}.g.{n}"]).double()
        ours = (g.detach().double().cpu().reshape(ref.shape) - ref).norm().item()
        yard, gn = float(fx[f"{case}.dev.{n}"]), ref.norm().item()
        ok = ours <= max(4 * yard, 2 ** -8 * gn)
        print(f"  {n:52s} {ours:.4e} {yard:.4e} {gn:.4e}{'' if ok else '   <-- over'}")
        if not ok:
            bad.append(n)
    assert not bad, bad


def test_encoder_half_gradients_vs_reference(pkg, golden, fx):
    make, t, cbs = golden
    m = make().train()
    x = t["patches_in"].clone().requires_grad_(True)
    h = m._encode_hidden(_dp(pkg, t, x))
    up = torch.randn(3, 256, 128, generator=torch.Generator().manual_seed(SEED_ENC))
    names = [k[len("enc.g."):] for k in fx if k.startswith("enc.g.")]
    params = dict(m.named_parameters())
    leaves = [x if n == "patches_in" else params[n] for n in names]
    grads = torch.autograd.grad(h, leaves, up.reshape(-1, 128).to(DEV))
    torch.cuda.synchronize()
    _allowance(fx, "enc", dict(zip(names, grads)), "encoder half")


def test_decoder_half_gradients_vs_reference(pkg, golden, fx):
    make, t, cbs = golden
    m = make().train()
    with torch.no_grad():   # the reference's quantizer output: project_out of the +-1 codes
        xq = m.vq_model.indices_to_codes(t["codes"]).float()
    x = xq.clone().requires_grad_(True)
    out = m.decode(_dp(pkg, t, x)).patches
    up = torch.randn(3, 256, 196, generator=torch.Generator().manual_seed(SEED_DEC))
    names = [k[len("dec.g."):] for k in fx if k.startswith("dec.g.")]
    params = dict(m.named_parameters())
    leaves = [x if n == "x_q" else params[n] for n in names]
    grads = torch.autograd.grad(out, leaves, up.to(DEV))
    torch.cuda.synchronize()
    _allowance(fx, "dec", dict(zip(names, grads)), "decoder half")


def test_whole_step_vs_reference(pkg, golden, fx):
    make, t, cbs = golden
    m = make().train()
    out, total = _step(pkg, m, t, cbs)
    total.backward()
    torch.cuda.synchronize()
    terms = dict(out, total=total)
    bad = []
    print("\nwhole step: loss term, ours, reference float64, deviation, yardstick")
    for k in list(WEIGHTS) + ["total"]:
        ref, yard = float(fx[f"step.loss.{k}"]), float(fx[f"step.dev.loss.{k}"])
        ours = terms[k].detach().item()
        dev = abs(ours - ref)
        print(f"  {k:24s} {ours:.6f} {ref:.6f} {dev:.3e} {yard:.3e}")
        if not dev <= 4 * yard:
            bad.append(k)
    assert not bad, bad
    params = dict(m.named_parameters())
    _allowance(fx, "step", {n: params[n].grad for n in fx["step_subset"].tolist()}, "whole step")


def test_ten_adamw_steps_lower_the_loss(pkg, golden, fx):
    make, t, cbs = golden
    m = make().train()
    opt = torch.optim.AdamW(m.parameters(), lr=float(fx["adamw.lr"]))
    curve = []
    for _ in range(10):
        opt.zero_grad()
        _, total = _step(pkg, m, t, cbs)
        curve.append(total.item())
        total.backward()
        opt.step()
    with torch.no_grad():
        curve.append(_step(pkg, m, t, cbs)[1].item())
    ref = fx["adamw.loss"]
    print("total loss, ours     :", " ".join(f"{v:.4f}" for v in curve))
    print("total loss, reference:", " ".join(f"{v:.4f}" for v in ref))
    assert curve[0] - curve[-1] >= 0.5 * (ref[0] - ref[-1])
