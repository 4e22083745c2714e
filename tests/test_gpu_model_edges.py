"""GPU tests of the transformer kernels (dctae_model.hip, dctae_model_bwd.hip)
at the shapes and logits the operator tests of test_gpu_model.py and
test_gpu_model_train.py do not reach ("Edge cases").

Every reference is computed here in float64 on the CPU from the very bf16-exact
or fp32 inputs the kernel gets.  Bounds:
  * attention forward, elementwise: 2^-7 sum_j p |v| + 1e-6 (P is rounded to
    bf16 before P V and the output once more: 2^-8 sum p |v|, doubled);
    log-sum-exp 1e-4; gradients by the project's rule, max(4 x the deviation of
    the same formula under torch bf16 autocast, 2^-8 ||g||), per tensor and per
    query row of dq.  Where the gradient is zero (one key: dq = dk = 0 and the
    yardstick's deviation is 0 too) that rule allows nothing, which an fp32
    log-sum-exp cannot meet (1.5e-6 measured at S = 1), so the allowance has a
    third term, the first-order cost of half-ulp errors of logit and lse
    (oracle/attn_edges.py _fp32_floor): about a tenth of the 2^-8 term or less
    from S = 31 on.  tests/test_model_edges_host.py shows that the arithmetic
    the kernels intend meets these with room (worst ratios 0.75, 0.23 and, per
    dq row, 0.31: the per-row rule needs no widening, factor 1).
  * bf16 outputs of one rounding, elementwise: 2^-8 |ref| (+ 1e-5 max|ref| for
    LayerNorm, whose fp32 statistics carry the row's scale).
  * fp32 outputs: 1e-4 max|ref| (summation order only).
  * LayerNorm rows of zero variance or of mean 1000 cancel in fp32, so 1e-4
    cannot be derived for them: they, and the column sums they feed, are held to
    the yardstick rule against torch's own fp32 CPU LayerNorm.
"""
import ctypes as C
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from oracle import attn_edges as E
from oracle import ref_model as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LIN_F32, LIN_BF16 = 0, 1
SENT = 0x5A5A   # guard pattern of int16 buffers (bf16 2.4e16)


def _T(pkg):
    from importlib import import_module
    return import_module("dct_autoencoder_amd.model_train")


def _bits(x):
    """int16 bit patterns of the bf16 rounding of x."""
    return x.to(torch.bfloat16).view(torch.int16).contiguous()


def _bf(x):
    return x.to(torch.bfloat16).float()


def _unbits(x):
    return x.view(torch.bfloat16).double().cpu()


def _wide(rows, cols, extra, dtype, fill, col0=0):
    """A (rows, cols) view at column col0 of a (rows + 1, cols + extra) buffer filled with `fill`:
    returns (buffer, view); the buffer outside the view is the guard."""
    buf = torch.full((rows + 1, cols + extra), fill, dtype=dtype, device=DEV)
    return buf, buf[:rows, col0:col0 + cols]


def _guard_intact(buf, rows, cols, fill, col0=0):
    g = buf.clone()
    g[:rows, col0:col0 + cols] = fill
    if isinstance(fill, float) and math.isnan(fill):
        return bool(torch.isnan(g).all())
    return bool((g == fill).all())


# ---------------------------------------------------------------- attention
def _attention(T, c, r, s, heads, extra=0):
    """Forward (eval and LSE entry points) and backward of one case through the C ABI, every output in
    a guarded buffer (out and d_out as column slices when extra > 0).  Returns the outputs on the CPU."""
    L = T._lib
    d, m = 64 * heads, r * s
    qb = _bits(c.qkv).to(DEV)
    idd, kpd = c.ids.to(DEV), c.kp.to(torch.uint8).to(DEV)
    ctx, st = T._c(qb), T._st(qb)
    col0 = 64 if extra else 0
    obuf0, out0 = _wide(m, d, extra, torch.int16, SENT, col0)
    obuf, out = _wide(m, d, extra, torch.int16, SENT, col0)
    dobuf, dob = _wide(m, d, extra, torch.int16, SENT, col0)
    dob.copy_(_bits(c.d_out).to(DEV))
    lbuf, lse = _wide(r * heads, s, 0, torch.float32, math.nan)
    dbuf, delta = _wide(r * heads, s, 0, torch.float32, math.nan)
    gbuf, dqkv = _wide(m, 3 * d, 0, torch.int16, SENT)
    P = L.ptr
    ctx.check(ctx.lib.dctae_model_attention(ctx.h, r, s, heads, 64, P(qb), P(idd), P(kpd), P(out0), out0.stride(0), st),
              "attention")
    ctx.check(ctx.lib.dctae_model_attention_lse(ctx.h, r, s, heads, 64, P(qb), P(idd), P(kpd), P(out), out.stride(0),
                                                P(lse), st), "attention_lse")
    ctx.check(ctx.lib.dctae_model_attention_bwd(ctx.h, r, s, heads, 64, P(qb), P(idd), P(kpd), P(out), out.stride(0),
                                                P(dob), dob.stride(0), P(lse), P(delta), P(dqkv), st), "attention_bwd")
    torch.cuda.synchronize()
    assert _guard_intact(obuf0, m, d, SENT, col0) and _guard_intact(obuf, m, d, SENT, col0), "out guard"
    assert _guard_intact(dobuf, m, d, SENT, col0), "d_out is an input"
    assert _guard_intact(lbuf, r * heads, s, math.nan) and _guard_intact(dbuf, r * heads, s, math.nan), "lse / delta guard"
    assert _guard_intact(gbuf, m, 3 * d, SENT), "dqkv guard"
    return dict(out0=out0.cpu(), out=out.cpu(), lse=lse.cpu().view(r, heads, s), delta=delta.cpu(), dqkv=dqkv.cpu())


def _same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int16) if a[k].dtype != torch.float32 else a[k].view(torch.int32),
                           b[k].view(torch.int16) if b[k].dtype != torch.float32 else b[k].view(torch.int32)) for k in a)


@pytest.mark.parametrize("mask", E.MASKS)
@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("r,s,heads", E.SHAPES)
def test_attention_edges(pkg, r, s, heads, kind, mask):
    """Forward output elementwise, LSE, gradients (whole tensors and every dq row), guards, run-to-run
    bit identity.  Per-row dq rule: not widened (factor 1; the CPU emulation's worst row is at 0.31)."""
    T = _T(pkg)
    c = E.case(kind, mask, r, s, heads)
    got = _attention(T, c, r, s, heads)
    again = _attention(T, c, r, s, heads)
    assert torch.equal(got["out"], got["out0"]), "LSE and eval entry points differ"
    assert torch.isfinite(got["lse"]).all() and torch.isfinite(got["delta"]).all(), "a (row, head, query) was not written"
    fwd = E.forward_ratio(_unbits(got["out"]), c.ref)
    lse = E.lse_error(got["lse"], c.ref)
    gr = E.grad_ratios(_unbits(got["dqkv"]), c.ref, 64 * heads)
    print(f"forward error / bound {fwd:.3f}  lse error {lse:.3g}  gradient deviation / allowance "
          + "  ".join(f"{k} {v:.3f}" for k, v in gr.items()))
    assert fwd <= 1.0
    assert lse <= 1e-4
    assert max(gr.values()) <= 1.0, gr
    assert _same_bits(got, again), "two runs differ"


def test_attention_strided_out_and_d_out(pkg):
    T = _T(pkg)
    r, s, heads = 2, 200, 3
    c = E.case("slow", "scatter", r, s, heads)
    flat, wide = _attention(T, c, r, s, heads), _attention(T, c, r, s, heads, extra=64)
    assert _same_bits(flat, wide)


# ---------------------------------------------------------------- LayerNorm
def _ln_inputs(m, d, seed):
    """x = 3 randn + 1; from 5 rows on, row 1 is constant (zero variance) and row 3 is 1000 + randn."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, d, generator=g) * 3 + 1
    special = []
    if m >= 5:
        x[1] = 0.7
        x[3] = 1000 + torch.randn(d, generator=g)
        special = [1, 3]
    return x, torch.randn(d, generator=g), torch.randn(d, generator=g), special, g


def _rows_check(label, got, ref, yard, special, tol):
    """Normal rows: |got - ref| <= tol(ref, max|ref| over them) elementwise.  Special rows: the yardstick
    rule, ||got - ref||_2 <= max(4 ||yard - ref||_2, 2^-8 ||ref||_2) per row; prints both deviations."""
    got, ref, yard = got.double().cpu(), ref.double(), yard.double()
    normal = torch.ones(ref.shape[0], dtype=torch.bool)
    if special:
        normal[special] = False
    scale = ref[normal].abs().max()
    err = (got[normal] - ref[normal]).abs()
    bound = tol(ref[normal].abs(), scale)
    worst = (err / bound).max().item()
    assert worst <= 1.0, (label, worst)
    for i in special:
        ours, yd, rn = (got[i] - ref[i]).norm().item(), (yard[i] - ref[i]).norm().item(), ref[i].norm().item()
        print(f"  {label} special row {i}: ours {ours:.3e} yardstick {yd:.3e} |ref| {rn:.3e}")
        assert ours <= max(4 * yd, 2.0 ** -8 * rn), (label, i, ours, yd, rn)


def _bf16_tol(a, scale):
    return 2.0 ** -8 * a + 1e-5 * scale


def _f32_tol(a, scale):
    return 1e-4 * scale + 0 * a


def _ln_fwd(T, x, gam, bet, eps, out):
    ctx = T._c(x)
    m, d = x.shape
    P = T._lib.ptr
    ctx.check(ctx.lib.dctae_model_layernorm(ctx.h, m, d, P(x), x.stride(0), P(gam), P(bet), C.c_float(eps), P(out),
                                            out.stride(0), T._st(x)), "layernorm")


LN_FWD = [(d, m) for d in (25, 64, 100, 192, 256, 512, 768, 2048, 3072, 4096) for m in ((1, 5, 333) if d <= 768 else (1, 5))]


@pytest.mark.parametrize("d,m", LN_FWD)
def test_layernorm_forward_dispatch(pkg, d, m):
    """bf16 LayerNorm over launch_layernorm's vector (D % 256 == 0, p4 1 .. 16) and scalar (PER 2 .. 64)
    instantiations, the vector-to-scalar fallbacks (D = 768 and 3072; at D = 256 a base pointer aligned
    to 4 bytes only), and row strides != D in padded buffers whose padding must survive."""
    T = _T(pkg)
    x, gam, bet, special, _ = _ln_inputs(m, d, 11 * d + m)
    eps = 1e-5
    ref = F.layer_norm(x.double(), (d,), gam.double(), bet.double(), eps)
    yard = F.layer_norm(x, (d,), gam, bet, eps)
    xd, gd, bd = x.to(DEV), gam.to(DEV), bet.to(DEV)
    runs = {}
    obuf, out = _wide(m, d, 0, torch.int16, SENT)
    _ln_fwd(T, xd, gd, bd, eps, out)
    runs["contiguous"] = (obuf, out, 0)
    xbuf, xs = _wide(m, d, 4, torch.float32, 77.0)
    xs.copy_(xd)
    obuf2, out2 = _wide(m, d, 8, torch.int16, SENT)
    _ln_fwd(T, xs, gd, bd, eps, out2)
    runs["ldx = D + 4, ldo = D + 8"] = (obuf2, out2, 8)
    if d == 256:
        flat = torch.empty(m * d + 1, device=DEV)
        xo = flat[1:].view(m, d)
        xo.copy_(xd)
        assert xo.data_ptr() % 16 == 4
        obuf3, out3 = _wide(m, d, 0, torch.int16, SENT)
        _ln_fwd(T, xo, gd, bd, eps, out3)
        runs["x offset by one float"] = (obuf3, out3, 0)
    torch.cuda.synchronize()
    assert _guard_intact(xbuf, m, d, 77.0)
    for label, (buf, o, extra) in runs.items():
        assert _guard_intact(buf, m, d, SENT), label
        _rows_check(f"D={d} M={m} {label}", _unbits(o.contiguous()), ref, _bf(yard), special, _bf16_tol)


@pytest.mark.parametrize("d", [25, 100, 192, 256, 768])
def test_embed_norm_widths(pkg, d):
    """LayerNorm (eps 1e-4) + position terms, fp32 out: always the scalar kernel, PER 2 .. 16, ragged D."""
    T = _T(pkg)
    m = 333
    x, gam, bet, special, g = _ln_inputs(m, d, 13 * d)
    ph, pw, pc = (torch.randn(n, d, generator=g) for n in (32, 32, 3))
    ch = torch.randint(0, 3, (m,), generator=g)
    pos = torch.randint(0, 32, (m, 2), generator=g)

    def f(t):
        add = ph.to(t)[pos[:, 0]] + pw.to(t)[pos[:, 1]] + pc.to(t)[ch]
        return F.layer_norm(x.to(t), (d,), gam.to(t), bet.to(t), 1e-4) + add

    ref, yard = f(torch.float64), f(torch.float32)
    dev = [t.to(DEV) for t in (x, gam, bet, ph, pw, pc, ch, pos)]
    obuf, out = _wide(m, d, 4, torch.float32, math.nan)
    ctx, P = T._c(dev[0]), T._lib.ptr
    ctx.check(ctx.lib.dctae_model_embed_norm(ctx.h, m, d, P(dev[0]), d, P(dev[1]), P(dev[2]), C.c_float(1e-4), P(dev[3]),
                                             P(dev[4]), P(dev[5]), P(dev[6]), P(dev[7]), P(out), out.stride(0),
                                             T._st(dev[0])), "embed_norm")
    torch.cuda.synchronize()
    assert _guard_intact(obuf, m, d, math.nan)
    _rows_check(f"embed_norm D={d}", out.cpu(), ref, yard, special, _f32_tol)


def _ln_bwd(T, x, gam, eps, dy, dx, accumulate):
    """dctae_model_layernorm_bwd with the tensors' own row strides; returns (dgamma, dbeta)."""
    ctx, P = T._c(x), T._lib.ptr
    m, d = x.shape
    parts = torch.empty(2, (m + T.LN_RPW - 1) // T.LN_RPW, d, device=x.device)
    ctx.check(ctx.lib.dctae_model_layernorm_bwd(ctx.h, m, d, P(x), x.stride(0), P(gam), C.c_float(eps), P(dy),
                                                dy.stride(0), P(dx), dx.stride(0), int(accumulate), P(parts[0]),
                                                P(parts[1]), T._st(x)), "layernorm_bwd")
    return T.colsum(parts[0], d), T.colsum(parts[1], d)


@pytest.mark.parametrize("m", [1, 7, 8, 9, 333])
@pytest.mark.parametrize("d", [25, 64, 100, 192, 320, 768, 1100, 2048])
def test_layernorm_backward_dispatch(pkg, d, m):
    """k_ln_bwd's five instantiations (PER 2, 4, 8, 16, 32) with ragged D, the LN_RPW = 8 row tail on
    both sides, accumulate 0 / 1, and row strides != D on x, dy and dx."""
    T = _T(pkg)
    x, gam, _, special, g = _ln_inputs(m, d, 17 * d + m)
    dy = torch.randn(m, d, generator=g)
    base = torch.randn(m, d, generator=g)
    eps = 1e-5

    def grads(t):
        xx, gg, bb = x.to(t).requires_grad_(True), gam.to(t).requires_grad_(True), torch.zeros(d, dtype=t, requires_grad=True)
        return torch.autograd.grad(F.layer_norm(xx, (d,), gg, bb, eps), (xx, gg, bb), dy.to(t))

    ref, yard = grads(torch.float64), grads(torch.float32)
    xd, gd, dyd, based = x.to(DEV), gam.to(DEV), dy.to(DEV), base.to(DEV)
    dx0 = torch.empty(m, d, device=DEV)
    dg0, db0 = _ln_bwd(T, xd, gd, eps, dyd, dx0, False)
    dx1 = based.clone()
    dg1, db1 = _ln_bwd(T, xd, gd, eps, dyd, dx1, True)
    xbuf, xs = _wide(m, d, 4, torch.float32, 77.0)
    ybuf, ys = _wide(m, d, 8, torch.float32, 77.0)
    dbuf, ds = _wide(m, d, 12, torch.float32, 77.0)
    xs.copy_(xd), ys.copy_(dyd), ds.copy_(based)
    dg2, db2 = _ln_bwd(T, xs, gd, eps, ys, ds, True)
    torch.cuda.synchronize()
    assert all(_guard_intact(b, m, d, 77.0) for b in (xbuf, ybuf, dbuf))
    assert torch.equal(ds, dx1), "strided run differs from the contiguous one"
    for a, b in ((dg1, dg0), (dg2, dg0), (db1, db0), (db2, db0)):
        assert torch.equal(a, b)
    label = f"ln_bwd D={d} M={m}"
    _rows_check(label + " dx", dx0, ref[0], yard[0], special, _f32_tol)
    _rows_check(label + " dx accumulated", dx1, base.double() + ref[0], base + yard[0], special, _f32_tol)
    for name, got, r64, y32 in (("dgamma", dg0, ref[1], yard[1]), ("dbeta", db0, ref[2], yard[2])):
        err = (got.double().cpu() - r64).abs().max().item()
        yd = (y32.double() - r64).abs().max().item()
        # the special rows are summed into every column: 1e-4, or 4 x what they cost torch's fp32 sum
        allow = max(1e-4 * r64.abs().max().item(), 4 * yd if special else 0.0)
        print(f"  {label} {name}: ours {err:.3e} yardstick {yd:.3e} max|ref| {r64.abs().max().item():.3e}")
        assert err <= allow, (name, err, allow)


def test_layernorm_backward_refuses_2049(pkg):
    T = _T(pkg)
    x = torch.zeros(2, 2049, device=DEV)
    with pytest.raises(AssertionError, match="D <= 2048"):
        _ln_bwd(T, x, torch.ones(2049, device=DEV), 1e-5, x, torch.empty_like(x), False)


# ---------------------------------------------------------------- small operators
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("m", [1, 4, 256, 257, 320])
def test_colsum_stages_and_tails(pkg, m, bf16):
    """One stage up to 256 rows, two from 257 (64-row chunks, the last one partial), 1 .. 200 columns in
    64-column blocks, ldx > N; fixed order: two runs are bit-equal."""
    T = _T(pkg)
    g = torch.Generator().manual_seed(m)
    for n in (1, 65, 200):
        x = torch.randn(m, n + 3, generator=g)
        xd = (_bits(x) if bf16 else x).to(DEV)[:, :n]
        ref = (_bf(x) if bf16 else x)[:, :n].double().sum(0)
        a, b = T.colsum(xd, n), T.colsum(xd, n)
        torch.cuda.synchronize()
        assert xd.stride(0) == n + 3 and torch.equal(a, b)
        assert (a.double().cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


@pytest.mark.parametrize("m", [1, 63, 64, 65])
def test_transpose_pack_shapes(pkg, m):
    T = _T(pkg)
    g = torch.Generator().manual_seed(m)
    for c in (1, 64, 100):
        x = torch.randint(-30000, 30000, (m, c + 5), generator=g, dtype=torch.int16).to(DEV)
        out = T.transpose_pack(x[:, :c], c)
        torch.cuda.synchronize()
        assert out.shape == (c, T.pad64(m))
        assert torch.equal(out[:, :m], x[:, :c].t()) and not out[:, m:].any()


BF16_MAX = 3.3895313892515355e38


def test_quick_gelu_extremes_and_strides(pkg):
    """M N = 259 (a partial last block), input and output strides differ, and the inputs hold +-0, +-30,
    +-88 and the largest finite bf16 of both signs: finite wherever the float64 value is, and within one
    bf16 rounding of it elementwise (2^-8 |ref| + 1e-30)."""
    T = _T(pkg)
    m, n = 7, 37
    g = torch.Generator().manual_seed(21)
    pre = _bf(torch.randn(m, n, generator=g) * 2)
    df = _bf(torch.randn(m, n, generator=g))
    pre[0, :8] = torch.tensor([0.0, -0.0, 30.0, -30.0, 88.0, -88.0, BF16_MAX, -BF16_MAX])
    pre[m - 1, n - 4:] = torch.tensor([BF16_MAX, -BF16_MAX, 88.0, -88.0])
    assert torch.equal(_bf(pre), pre) and torch.isfinite(pre).all()
    x64, d64 = pre.double(), df.double()
    sg = torch.sigmoid(1.702 * x64)
    refs = (x64 * sg, d64 * (sg * (1 + 1.702 * x64 * (1 - sg))))
    assert all(torch.isfinite(t).all() for t in refs)
    pbuf, pv = _wide(m, n, 3, torch.int16, SENT)
    fbuf, fv = _wide(m, n, 5, torch.int16, SENT)
    pv.copy_(_bits(pre).to(DEV)), fv.copy_(_bits(df).to(DEV))
    obuf, ov = _wide(m, n, 11, torch.int16, SENT)
    bbuf, bv = _wide(m, n, 27, torch.int16, SENT)
    T.qgelu(pv, n, ov)
    T.qgelu_bwd(fv, pv, n, bv)
    torch.cuda.synchronize()
    for name, buf, view, ref in (("qgelu", obuf, ov, refs[0]), ("qgelu_bwd", bbuf, bv, refs[1])):
        assert _guard_intact(buf, m, n, SENT), name
        got = _unbits(view.contiguous())
        assert torch.isfinite(got).all(), (name, pre[~torch.isfinite(got)])
        ratio = ((got - ref).abs() / (2.0 ** -8 * ref.abs() + 1e-30)).max().item()
        print(f"  {name}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0, name


@pytest.mark.parametrize("m", [1, 63, 65])
def test_linear_dw_short_reductions(pkg, m):
    """dW = dY^T X with 1, 63 and 65 tokens: the packs' zero tail is most or all of the reduction."""
    T = _T(pkg)
    n, k = 52, 128
    g = torch.Generator().manual_seed(m)
    x, dy = _bf(torch.randn(m, k, generator=g)), _bf(torch.randn(m, n, generator=g))
    dyb = torch.zeros(m, T.pad64(n), dtype=torch.int16)
    dyb[:, :n] = _bits(dy)
    dw = T.linear_dw(dyb.to(DEV), n, _bits(x).to(DEV), k)
    torch.cuda.synchronize()
    ref = dy.double().t() @ x.double()
    assert dw.shape == (n, k)
    assert (dw.double().cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + 1e-6


@pytest.mark.parametrize("k", [100, 200])
def test_linear_dx_ragged_width(pkg, k):
    """dX with 100 and 200 output columns (patch 10's P^2; one full 128-column tile plus a ragged one)."""
    T = _T(pkg)
    m, n = 130, 192
    g = torch.Generator().manual_seed(k)
    w = _bf(torch.randn(n, k, generator=g) / n ** 0.5)
    dy = _bf(torch.randn(m, n, generator=g))
    dyb, wt = _bits(dy).to(DEV), _bits(w.t().contiguous()).to(DEV)
    ref = dy.double() @ w.double()
    dx = T.linear_dx(dyb, wt, k, LIN_F32, torch.empty(m, k, device=DEV))
    bbuf, bv = _wide(m, k, T.pad64(k) - k, torch.int16, SENT)
    T.linear_dx(dyb, wt, k, LIN_BF16, bv)
    torch.cuda.synchronize()
    scale = ref.abs().max().item()
    assert (dx.double().cpu() - ref).abs().max().item() <= 1e-4 * scale + 1e-6
    assert (_unbits(bv.contiguous()) - ref).abs().max().item() <= 8e-3 * scale + 1e-6
    assert _guard_intact(bbuf, m, k, SENT)


# ---------------------------------------------------------------- whole model, two more configurations
CONFIGS = {
    # projections (8 codebooks of 2^8: 64 != 192), patch 10, ragged S, pad keys of every image anywhere
    "A": dict(hidden=192, heads=3, inter=200, enc_layers=2, dec_layers=1, patch=10, ncb=8, cbs=2 ** 8, r=2, s=200,
              mask="scatter"),
    # 16 codebooks of 2^16 = 256: no projections; one row all pad, S = 65 (one full key block and one key)
    "B": dict(hidden=256, heads=4, inter=512, enc_layers=1, dec_layers=1, patch=16, ncb=16, cbs=2 ** 16, r=3, s=65,
              mask="allpad"),
}
SEED_ENC, SEED_DEC = 7001, 7002


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def model_case(pkg, request):
    """The model with seeded random weights, its batch, and the float64 / bf16-autocast runs of
    oracle/ref_model.py on the same weights, computed once per configuration."""
    c = CONFIGS[request.param]
    cbd = int(math.log2(c["cbs"]))
    torch.manual_seed(100 + ord(request.param))
    side = lambda layers: dict(hidden_size=c["hidden"], intermediate_size=c["inter"], num_attention_heads=c["heads"],
                               num_hidden_layers=layers)
    cfg = pkg.DCTAutoencoderConfig(image_channels=3, patch_size=c["patch"], max_patch_h=32, max_patch_w=32,
                                   vq_codebook_size=c["cbs"], vq_num_codebooks=c["ncb"], vq_type="lfq",
                                   encoder_config=side(c["enc_layers"]), decoder_config=side(c["dec_layers"]))
    m = pkg.DCTAutoencoder(cfg)
    w32 = {k: v.detach().clone().float() for k, v in m.state_dict().items() if v.is_floating_point()}
    g = torch.Generator().manual_seed(5)
    r, s, pd = c["r"], c["s"], c["patch"] ** 2
    ids, kp = E.mask(c["mask"], r, s, g)
    t = dict(patches=torch.randn(r, s, pd, generator=g), ids=ids, kp=kp, ch=torch.randint(0, 3, (r, s), generator=g),
             pos=torch.randint(0, 32, (r, s, 2), generator=g),
             codes=torch.randint(0, c["cbs"], (r, s, c["ncb"]), generator=g))
    up_enc = torch.randn(r, s, c["hidden"], generator=torch.Generator().manual_seed(SEED_ENC))
    up_dec = torch.randn(r, s, pd, generator=torch.Generator().manual_seed(SEED_DEC))
    enc_names = [n for n in w32 if n.startswith(("to_patch_embedding.", "encoder.", "encoder_pos_embed_"))]
    dec_names = [n for n in w32 if n.startswith(("decoder.", "decoder_pos_embed_", "proj_out."))]

    with torch.no_grad():   # the training decoder half's leaf: project_out of the +-1 codes, as the fixture's x_q
        xq0 = R.codes_to_features(w32, t["codes"], c["ncb"], cbd)
    bits = (t["codes"][..., None] & 2 ** torch.arange(cbd - 1, -1, -1)) != 0

    def run(dtype, autocast):
        w = {k: v.to(dtype).requires_grad_(k in enc_names or k in dec_names) for k, v in w32.items()}
        x = t["patches"].to(dtype).requires_grad_(True)
        xq = xq0.to(dtype).requires_grad_(True)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            hidden = R.encode(w, x, ids, kp, t["ch"], t["pos"], c["heads"], c["enc_layers"], c["ncb"], cbd)[0]
            dec = R.decode(w, xq, ids, kp, t["ch"], t["pos"], c["heads"], c["dec_layers"])
            with torch.no_grad():   # eval: decode_from_codes, project_out included
                q = (bits.to(dtype) * 2 - 1).reshape(r, s, c["ncb"] * cbd)
                if "vq_model.project_out.weight" in w:
                    q = F.linear(q, w["vq_model.project_out.weight"], w["vq_model.project_out.bias"])
                decoded = R.decode(w, q, ids, kp, t["ch"], t["pos"], c["heads"], c["dec_layers"])
        ge = torch.autograd.grad(hidden, [w[n] for n in enc_names] + [x], up_enc.to(hidden.dtype))
        gd = torch.autograd.grad(dec, [w[n] for n in dec_names] + [xq], up_dec.to(dec.dtype))
        return dict(hidden=hidden.detach().double(), decoded=decoded.double(),
                    enc=dict(zip(enc_names + ["patches_in"], (v.double() for v in ge))),
                    dec=dict(zip(dec_names + ["x_q"], (v.double() for v in gd))))

    def dp(patches):
        return pkg.DCTPatches(patches=patches, key_pad_mask=kp.to(DEV), batched_image_ids=ids.to(DEV),
                              patch_channels=t["ch"].to(DEV), patch_positions=t["pos"].to(DEV), patch_sizes=[],
                              original_sizes=[])

    return SimpleNamespace(name=request.param, model=m.to(DEV), t=t, dp=dp, xq=xq0, ref=run(torch.float64, False),
                           yard=run(torch.float32, True), up_enc=up_enc, up_dec=up_dec, hidden=c["hidden"])


def _yardstick_table(label, got, ref, yard):
    """||ours - float64||_2 <= max(4 x the bf16-autocast reference's deviation, 2^-8 ||ref||_2) per tensor."""
    bad = []
    print(f"\n{label}: tensor, ours, yardstick (reference under bf16 autocast), |ref|")
    for n, g in got.items():
        r64 = ref[n]
        ours = (g.detach().double().cpu().reshape(r64.shape) - r64).norm().item()
        yd, rn = (yard[n] - r64).norm().item(), r64.norm().item()
        ok = ours <= max(4 * yd, 2.0 ** -8 * rn)
        print(f"  {n:52s} {ours:.4e} {yd:.4e} {rn:.4e}{'' if ok else '   <-- over'}")
        if not ok:
            bad.append(n)
    assert not bad, bad


def test_model_eval_vs_reference(pkg, model_case):
    """Pre-quantiser hidden state and decode of fixed +-1 codes.  Codes are not compared: a sign flip of
    a feature near zero is not an error."""
    mc = model_case
    m = mc.model.eval()
    seen = []
    inner = m._lfq
    m._lfq = lambda h: (seen.append(h.clone()), inner(h))[1]
    try:
        m.encode(mc.dp(mc.t["patches"].to(DEV)))
    finally:
        del m._lfq
    kw = dict(key_pad_mask=mc.t["kp"].to(DEV), batched_image_ids=mc.t["ids"].to(DEV), patch_channels=mc.t["ch"].to(DEV),
              patch_positions=mc.t["pos"].to(DEV), patch_sizes=[], original_sizes=[])
    dec = m.decode_from_codes(mc.t["codes"].to(DEV), **kw).patches
    torch.cuda.synchronize()
    _yardstick_table(f"config {mc.name} eval", dict(hidden=seen[0], decoded=dec), mc.ref, mc.yard)


def _train_grads(pkg, mc):
    m = mc.model.train()
    params = dict(m.named_parameters())
    x = mc.t["patches"].to(DEV).requires_grad_(True)
    h = m._encode_hidden(mc.dp(x))
    names = list(mc.ref["enc"])
    ge = torch.autograd.grad(h, [x if n == "patches_in" else params[n] for n in names],
                             mc.up_enc.reshape(-1, mc.hidden).to(DEV))
    xq = mc.xq.to(DEV).requires_grad_(True)
    out = m.decode(mc.dp(xq)).patches
    dnames = list(mc.ref["dec"])
    gd = torch.autograd.grad(out, [xq if n == "x_q" else params[n] for n in dnames], mc.up_dec.to(DEV))
    torch.cuda.synchronize()
    return dict(zip(names, ge)), dict(zip(dnames, gd))


def test_model_train_gradients_vs_reference(pkg, model_case):
    """Random-upstream encoder-half and decoder-half gradients of every parameter and the input, as
    test_encoder_half_gradients_vs_reference does at the fixture's configuration; two runs bit-identical."""
    mc = model_case
    ge, gd = _train_grads(pkg, mc)
    ge2, gd2 = _train_grads(pkg, mc)
    for a, b in ((ge, ge2), (gd, gd2)):
        for n in a:
            assert torch.equal(a[n], b[n]), n
    _yardstick_table(f"config {mc.name} encoder half", ge, mc.ref["enc"], mc.yard["enc"])
    _yardstick_table(f"config {mc.name} decoder half", gd, mc.ref["dec"], mc.yard["dec"])


def test_training_refuses_a_width_the_layernorm_backward_cannot_take(pkg):
    """hidden 2112 (33 heads): LayerNorm forward takes it (D <= 4096), its backward does not
    (D <= 2048).  Refused before the input is looked at; .eval() is not affected."""
    side = dict(hidden_size=2112, intermediate_size=64, num_attention_heads=33, num_hidden_layers=1)
    m = pkg.DCTAutoencoder(pkg.DCTAutoencoderConfig(patch_size=8, vq_codebook_size=2 ** 8, vq_num_codebooks=8,
                                                    encoder_config=side, decoder_config=side)).to(DEV).train()
    for call in (lambda: m.encode(None), lambda: m.decode(None), lambda: m(None)):
        with pytest.raises(NotImplementedError, match="LayerNorm backward"):
            call()
    m.eval()
    m._check_mode()
