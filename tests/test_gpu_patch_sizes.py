"""GPU parity at patch sizes other than 14: dctae_encode / dctae_decode /
dctae_spectrum_tokens / dctae_patch_spectrum against the CPU oracle at
P in {16, 15, 8, 7, 5, 2, 1}.  Run on an MI355X: pytest -m gpu.

The oracle is pinned to the reference at these patch sizes by
tests/test_patch_sizes_host.py (tests/golden/patch_sizes_ref.npz).

What P != 14 reaches: the runtime-P tile epilogue and the
generic token epilogue with idle lanes / all 16 lanes live / codes spanning
tile rows, odd kept corners in the parity-split GEMMs and the parity-planar
layout, the scalar token gather, sides 512 and 224 off the specialised plans,
256 codebooks in the pad-token path, score ties and the bitonic sort.

Tolerances are the project's existing ones (tests/test_gpu_parity.py):
  * masks, ids, positions, channels, pad codes, PatchNorm / LFQ given
    identical input: bit-exact;
  * DCT coefficients: |gpu - oracle| <= 2e-6 * max|Y| + 1e-6 per image;
  * codes: a code may differ only where an element of its group lies within
    2 d + 1e-7 of the median (d = that image's measured token difference), at
    most max(2, n_codes // 10000) such flips.  The fp32 oracle against a
    float64 DCT flips 0 of these configurations' 2,336,793 sign bits (worst
    relative token error 1.4e-7), so the reference alone sits far inside;
  * decode RGB: 1e-5 absolute + 1e-5 relative.
"""
import ctypes as C
import functools
from importlib import import_module
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu, rng

pytestmark = pytest.mark.gpu
DEV = "cuda"

# P -> (max_patch_h, max_patch_w, image sizes (H, W), LFQ groupings codebook_dim); max_seq_len = 3 mh mw
CASES = {
    16: (32, 32, [(512, 512), (224, 224), (100, 77), (16, 16), (33, 500)], [16, 8, 1]),
    15: (32, 32, [(512, 300), (225, 105), (15, 15), (47, 31), (300, 512)], [15, 9, 5]),
    8: (32, 32, [(224, 224), (97, 64), (8, 8), (30, 300)], [8, 16, 4]),
    7: (32, 32, [(224, 98), (21, 35), (7, 7), (100, 77), (225, 105)], [7, 1]),
    5: (6, 9, [(16, 27), (5, 5), (37, 53), (64, 97)], [5]),
    2: (40, 40, [(97, 64), (2, 2), (7, 12), (80, 80)], [2, 4, 1]),
    1: (8, 8, [(4, 6), (1, 1), (9, 9), (3, 16)], [1]),
}
ALL_P = list(CASES)
P_CD = [(P, cd) for P in CASES for cd in CASES[P][3]]
OPTION_DEFAULTS = {"tperm": 1, "gemm_dma": 1, "cols_dma": 1, "sort_kernel": 2, "xcd_order": 1, "rows_fused": 1,
                   "gemm_h2": 1, "gemm_x3": 1, "fft_generic": 0, "fft_odd": 0, "bluestein": 0}


def _ops():
    return import_module("dct_autoencoder_amd._ops")


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
    """A device fault poisons the process: end the run there instead of
    launching the remaining cases onto a faulted device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # pragma: no cover
        pytest.exit(f"GPU fault, stopping: {e}", returncode=3)


# ---------------------------------------------------------------------------
# the oracle side: computed once per configuration, shared, never modified
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(P, extra_seq=0):
    mh, mw, sizes, cds = CASES[P]
    S = 3 * mh * mw + extra_seq
    cfg = ref_cpu.FEConfig(patch_size=P, max_patch_h=mh, max_patch_w=mw, max_seq_len=S)
    g = torch.Generator().manual_seed(P)
    median = torch.randn(3, mh, mw, P * P, generator=g) * 0.05
    b = torch.rand(3, mh, mw, P * P, generator=g) * 0.1 + 0.01
    tabs = ref_cpu.NormTables(torch.ones(3, mh, mw), median, b)
    imgs = [torch.from_numpy(x) for x in rng.synth_images(100 + P, sizes)]
    spectra, scored, items = [], [], []
    for x in imgs:
        y = ref_cpu.transform_image_in(x)
        ch, cw = ref_cpu.crop_dims(y.shape[1], y.shape[2], P)
        y = y[:, :ch, :cw].contiguous()
        spectra.append(y)
        scored.append(ref_cpu.patch_scores(y, cfg))
        items.append(ref_cpu.preprocess(x, cfg))
    return SimpleNamespace(P=P, mh=mh, mw=mw, S=S, sizes=sizes, cds=cds, cfg=cfg, tabs=tabs, imgs=imgs,
                           spectra=spectra, scored=scored, items=items)


def _lcfg(P, cd):
    return ref_cpu.LFQConfig(dim=P * P, codebook_size=2 ** cd, num_codebooks=P * P // cd)


@functools.lru_cache(maxsize=None)
def _oracle_encode(P, cd, extra_seq=0):
    c = _case(P, extra_seq)
    ((ob, oidx),) = ref_cpu.encode(c.imgs, c.cfg, c.tabs, _lcfg(P, cd))
    return ob, oidx


# ---------------------------------------------------------------------------
# the GPU side
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(pkg):
    """Factory of the per-configuration GPU objects (built once each)."""
    cache = {}

    def get(P, extra_seq=0):
        if (P, extra_seq) not in cache:
            c = _case(P, extra_seq)
            pn = pkg.PatchNorm(c.mh, c.mw, P, 3).to(DEV)
            pn.median.data.copy_(c.tabs.median)
            pn.b.data.copy_(c.tabs.b)
            pn.n.data.copy_(c.tabs.n)
            pn.frozen = True
            pn.eval()
            cache[(P, extra_seq)] = SimpleNamespace(
                fe=pkg.DCTAutoencoderFeatureExtractor(3, P, 0.0, c.mh, c.mw, c.S), pn=pn,
                imgs=[x.to(DEV) for x in c.imgs],
                lfq=lambda cd: pkg.LFQ(dim=P * P, codebook_size=2 ** cd, num_codebooks=P * P // cd).to(DEV).eval())
        return cache[(P, extra_seq)]

    return get


def _key(c, p):
    return (int(c), int(p[0]), int(p[1]))


def _image_slots(kp, ids):
    """(row, image id, token index tensor) in the reference's image enumeration order."""
    out = []
    for r in range(kp.shape[0]):
        for im in torch.unique(ids[r][~kp[r]]).tolist():
            out.append((r, im, torch.nonzero((~kp[r]) & (ids[r] == im)).flatten()))
    return out


def _encode_vs_oracle(g, P, cd, tag, ties=False):
    """tests/test_gpu_parity.py's _encode_vs_oracle for any patch size and LFQ
    grouping (the guard band grouped by (num_codebooks, codebook_dim)), plus
    the tie contract on the GPU's own scores.  Returns (worst token error /
    max|Y|, guard-band flips, codes compared)."""
    c = _case(P)
    ncb = P * P // cd
    ((dp, codes),) = g.fe.encode_batch(g.imgs, g.pn, g.lfq(cd), return_raw=True, return_scores=True)
    raw, codes, sc = dp.patches.cpu(), codes.cpu(), dp._data["scores"].cpu()
    kp, ids, pos, ch = (dp.key_pad_mask.cpu(), dp.batched_image_ids.cpu(), dp.patch_positions.cpu(),
                        dp.patch_channels.cpu())
    ob, oidx = _oracle_encode(P, cd)
    assert codes.shape == oidx.shape == (*kp.shape, ncb) and codes.dtype == torch.long
    # packing metadata: bit-exact
    assert torch.equal(kp, ob.key_pad_mask)
    assert torch.equal(ids, ob.batched_image_ids)
    # pad tokens: exact (zeros normalised at c = h = w = 0)
    assert torch.equal(codes[kp], oidx[kp])
    assert torch.all(pos[kp] == 0) and torch.all(ch[kp] == 0)
    flips, n_codes, worst, n_ties = 0, 0, 0.0, 0
    slots = _image_slots(kp, ids)
    assert len(slots) == len(c.items)
    for (r, im, tj), it, (H, W) in zip(slots, c.items, c.sizes):
        gkeys = [_key(cc, p) for p, cc in zip(pos[r, tj].tolist(), ch[r, tj].tolist())]
        okeys = [_key(cc, p) for p, cc in zip(it["positions"].tolist(), it["channels"].tolist())]
        assert sorted(gkeys) == sorted(okeys)
        omap = {k: j for j, k in enumerate(okeys)}
        oj = torch.tensor([omap[k] for k in gkeys])
        toks_o = it["patches"][oj]
        d = (raw[r, tj] - toks_o).abs().max().item()
        ymax = toks_o.abs().max().item()
        worst = max(worst, d / ymax if ymax > 0 else 0.0)
        assert d <= 2e-6 * ymax + 1e-6, (d, ymax)
        # oracle codes of the same tokens (oracle row r holds the same image at its own order)
        osel = torch.nonzero((~ob.key_pad_mask[r]) & (ob.batched_image_ids[r] == im)).flatten()
        ok = {_key(cc, p): j for j, (p, cc) in zip(osel.tolist(), zip(ob.patch_positions[r, osel].tolist(),
                                                                      ob.patch_channels[r, osel].tolist()))}
        oc = oidx[r, torch.tensor([ok[k] for k in gkeys])]
        gc = codes[r, tj]
        diff = gc != oc
        if diff.any():
            med = c.tabs.median[ch[r, tj], pos[r, tj, 0], pos[r, tj, 1]]
            near = ((toks_o - med).abs() <= 2 * d + 1e-7).view(-1, ncb, cd).any(-1)
            assert torch.all(near[diff]), "code mismatch outside the guard band"
            flips += int(diff.sum())
        n_codes += gc.numel()
        # the order contract on the GPU's own scores: non-increasing, and
        # flat index (h qw + w) 3 + c ascending wherever two neighbours tie
        s = sc[r, tj]
        assert torch.all(s[1:] <= s[:-1])
        qw = min(W // P, c.mw)
        flat = (pos[r, tj, 0] * qw + pos[r, tj, 1]) * 3 + ch[r, tj]
        tied = s[1:].view(torch.int32) == s[:-1].view(torch.int32)
        assert torch.all(flat[1:][tied] > flat[:-1][tied]), "equal scores out of flat-index order"
        n_ties += int(tied.sum())
    print(f"[P={P} cd={cd} {tag}] worst token error / max|Y| {worst:.3g}; code mismatches inside the guard band: "
          f"{flips} / {n_codes}; tied neighbours {n_ties}")
    assert flips <= max(2, n_codes // 10000)
    if ties:
        o_ties = sum(len(s[3]) - len(torch.unique(s[3])) for s in c.scored)
        assert o_ties > 0, "this configuration is there for its score ties"
    return worst, flips, n_codes


@pytest.mark.parametrize("P,cd", P_CD)
def test_encode_vs_oracle(gpu, P, cd):
    _encode_vs_oracle(gpu(P), P, cd, "default", ties=(P == 2))


@pytest.mark.parametrize("P", ALL_P)
def test_normalised_patches_and_threshold_bits(gpu, P):
    """Codes from the exact thresholds (codes-only encode) equal the codes of
    the encode that returns the PatchNorm output, and that output equals
    PatchNorm.forward (patchnorm.py:157-165, the oracle's) of the GPU's own
    raw tokens bit for bit, pads included."""
    c, g = _case(P), gpu(P)
    cd = c.cds[0]
    lfq = g.lfq(cd)
    ((dp_a, c_a),) = g.fe.encode_batch(g.imgs, g.pn, lfq)
    ((dp_n, c_n),) = g.fe.encode_batch(g.imgs, g.pn, lfq, return_patches=True, return_raw=True)
    assert dp_a.patches.shape[-1] == 0
    assert torch.equal(c_a, c_n)
    assert torch.equal(dp_a.patch_positions, dp_n.patch_positions)
    assert torch.equal(dp_a.patch_channels, dp_n.patch_channels)
    raw = dp_n._data["raw_patches"].cpu()
    pos, ch = dp_n.patch_positions.cpu(), dp_n.patch_channels.cpu()
    ref = ref_cpu.norm_forward_eval(c.tabs, raw, ch, pos[..., 0], pos[..., 1])
    got = dp_n.patches.cpu()
    assert got.shape == ref.shape == (*ch.shape, P * P)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    _, idx = ref_cpu.lfq_forward(got, _lcfg(P, cd))
    assert torch.equal(idx.long(), c_n.cpu())


@pytest.mark.parametrize("P", ALL_P)
def test_preprocess_and_patch_image(gpu, P):
    """fe.preprocess against the oracle's tokens and order (as
    test_preprocess_tokens_and_order), and fe._patch_image
    (dctae_patch_spectrum) on the oracle's cropped spectrum: identical input,
    so tokens, positions, channels and order equal the oracle's exactly, and
    the fused preprocess's within the coefficient tolerance."""
    c, g = _case(P), gpu(P)
    for x, y, (toks, pos, ch, scores), it in zip(g.imgs, c.spectra, c.scored, c.items):
        out = g.fe.preprocess(x)
        omap = {_key(cc, p): i for i, (p, cc) in enumerate(zip(pos.tolist(), ch.tolist()))}
        gp, gpos, gch = out["patches"].cpu(), out["positions"].cpu(), out["channels"].cpu()
        assert gp.shape == (len(omap), P * P) and out["positions"].dtype == torch.long
        assert out["original_sizes"] == it["original_sizes"] and tuple(out["patch_sizes"]) == tuple(it["patch_sizes"])
        idx = torch.tensor([omap[_key(cc, p)] for p, cc in zip(gpos.tolist(), gch.tolist())])
        assert len(set(idx.tolist())) == len(idx)
        ymax = float(toks.abs().max())
        err = float((gp - toks[idx]).abs().max())
        assert err <= 2e-6 * ymax, (err, ymax)
        # the GPU order is non-increasing in the oracle's scores up to the coefficient error
        s = scores[idx]
        assert torch.all(s[1:] <= s[:-1] + 0.1 * 4 * err + 1e-6)
        pt, ppos, pch = g.fe._patch_image(y.to(DEV))
        assert torch.equal(ppos.cpu(), it["positions"]) and torch.equal(pch.cpu(), it["channels"])
        assert torch.equal(pt.cpu().view(torch.int32), it["patches"].view(torch.int32))
        pmap = {_key(cc, p): i for i, (p, cc) in enumerate(zip(ppos.tolist(), pch.tolist()))}
        pj = torch.tensor([pmap[_key(cc, p)] for p, cc in zip(gpos.tolist(), gch.tolist())])
        assert float((gp - pt.cpu()[pj]).abs().max()) <= 2e-6 * ymax


def _with_options(opts, fn):
    ops = _ops()
    try:
        for k, v in opts.items():
            ops.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            ops.set_option(k, OPTION_DEFAULTS[k])


BIT_IDENTICAL = [{"tperm": 0}, {"gemm_dma": 0}, {"cols_dma": 0}, {"sort_kernel": 1}, {"xcd_order": 0},
                 {"rows_fused": 0}, {"rows_fused": 0, "gemm_dma": 0}]


@pytest.mark.parametrize("P", [16, 15, 7])
def test_option_paths_bit_identical(gpu, P):
    """The options include/dctae.h documents as bit-identical stay so at this
    patch size, each flipped alone against the default: tperm, gemm_dma,
    cols_dma, sort_kernel 2 -> 1, xcd_order; rows_fused 1 -> 0 too (the inputs
    are [0, 1] RGB: no fix-up), and gemm_dma under rows_fused = 0, where the
    row GEMM it switches actually runs."""
    c, g = _case(P), gpu(P)
    lfq = g.lfq(c.cds[0])

    def run():
        ((dp, codes),) = g.fe.encode_batch(g.imgs, g.pn, lfq, return_raw=True, return_scores=True)
        torch.cuda.synchronize()
        return dp, codes

    d0, c0 = run()
    for opts in BIT_IDENTICAL:
        d1, c1 = _with_options(opts, run)
        assert torch.equal(c0, c1), opts
        assert torch.equal(d0.patches.view(torch.int32), d1.patches.view(torch.int32)), opts
        assert torch.equal(d0._data["scores"].view(torch.int32), d1._data["scores"].view(torch.int32)), opts
        for f in ("key_pad_mask", "batched_image_ids", "patch_channels", "patch_positions"):
            assert torch.equal(getattr(d0, f), getattr(d1, f)), (opts, f)


TRANSFORMS = {"x3": {"gemm_h2": 0}, "f32": {"gemm_x3": 0}, "fft": {"fft_generic": 1},
              "fft_odd": {"fft_generic": 1, "fft_odd": 1}, "bluestein": {"bluestein": 1}}


@pytest.mark.parametrize("variant", list(TRANSFORMS))
@pytest.mark.parametrize("P", [16, 15, 7])
def test_alternative_transforms_vs_oracle(gpu, P, variant):
    """The other evaluations of the DCT (split-bf16 GEMM, fp32 GEMM, the
    generic FFT kernels with KS = P strips on the 7-smooth sides 512 / 224 /
    225 / 105, the odd-side FFT form, Bluestein) meet the default's oracle
    tolerances at this patch size."""
    _with_options(TRANSFORMS[variant], lambda: _encode_vs_oracle(gpu(P), P, CASES[P][3][0], variant))


def _rgb_close(a, b, atol=1e-5, rtol=1e-5):
    d = (a - b).abs()
    return bool(torch.all(d <= atol + rtol * b.abs())), float(d.max())


@pytest.mark.parametrize("P", ALL_P)
def test_decode_vs_oracle(pkg, gpu, P):
    """decode_batch of the oracle's codes against the oracle's decode, and
    postprocess of the oracle's raw patches against ref_cpu.postprocess.
    P = 15 runs at max_seq_len 3 mh mw + 1, so its rows carry padding and the
    token count is odd (as test_decode_odd_seq_len_vs_oracle)."""
    extra = 1 if P == 15 else 0
    c, g = _case(P, extra), gpu(P, extra)
    cd = c.cds[0]
    ob, oidx = _oracle_encode(P, cd, extra)
    if extra:
        assert ob.key_pad_mask.any(-1).all() and ob.key_pad_mask.numel() % 4 != 0

    def dp_of(patches):
        return pkg.DCTPatches(patches.to(DEV), ob.key_pad_mask.to(DEV), None, ob.batched_image_ids.to(DEV),
                              ob.patch_channels.to(DEV), ob.patch_positions.to(DEV), list(ob.patch_sizes),
                              list(ob.original_sizes))

    imgs = g.fe.decode_batch(dp_of(torch.zeros(*oidx.shape[:2], 0)), oidx.to(DEV), g.pn, g.lfq(cd))
    _ops().check_device_errors(torch.device(DEV, torch.cuda.current_device()))
    y = ref_cpu.lfq_indices_to_codes(oidx, _lcfg(P, cd))
    xin = ref_cpu.norm_inverse(c.tabs, y, ob.patch_channels, ob.h_indices, ob.w_indices)
    refs = ref_cpu.postprocess(ref_cpu.Batch(xin, ob.key_pad_mask, None, ob.batched_image_ids, ob.patch_channels,
                                             ob.patch_positions, ob.patch_sizes, ob.original_sizes), c.cfg)
    assert len(imgs) == len(refs) == len(c.imgs)
    worst = 0.0
    for a, r in zip(imgs, refs):
        assert a.shape == r.shape
        ok, dmax = _rgb_close(a.cpu(), r)
        worst = max(worst, dmax)
        assert ok, ("decode_batch", dmax, float(r.abs().max()))
    # postprocess of raw (un-normalised) tokens: the oracle's packed batch of its own tokens
    rb = list(ref_cpu.iter_batches(iter([{k: [it[k] for it in c.items] for k in c.items[0]}]), c.cfg, None,
                                   build_attn_mask=False))[0]
    assert torch.equal(rb.key_pad_mask, ob.key_pad_mask)
    outs = g.fe.postprocess(dp_of(rb.patches))
    refs2 = ref_cpu.postprocess(rb, c.cfg)
    worst2 = 0.0
    for a, r in zip(outs, refs2):
        ok, dmax = _rgb_close(a.cpu(), r)
        worst2 = max(worst2, dmax)
        assert ok, ("postprocess", dmax, float(r.abs().max()))
    print(f"[P={P}] decode_batch worst |rgb - oracle| {worst:.3g}; postprocess {worst2:.3g}")


@pytest.mark.parametrize("P", ALL_P)
def test_roundtrip_dct_idct(gpu, P):
    """The transform-in / transform-out hooks (dctae_dct2) on this
    configuration's images, on the context that cached the P-specific plans:
    spectrum within 2e-6 max|Y| of the oracle, RGB back within 1e-5 + 1e-5 |x|."""
    c, g = _case(P), gpu(P)
    g.fe.encode_batch(g.imgs, g.pn, g.lfq(c.cds[0]))
    for x in c.imgs:
        y = g.fe._transform_image_in(x.to(DEV))
        y_o = ref_cpu.transform_image_in(x)
        assert y.shape == y_o.shape
        d = (y.cpu() - y_o).abs().max().item()
        assert d <= 2e-6 * y_o.abs().max().item(), (tuple(x.shape), d)
        back = g.fe._transform_image_out(y)
        diff = (back.cpu() - x).abs()
        assert torch.all(diff <= 1e-5 + 1e-5 * x.abs()), (tuple(x.shape), diff.max().item())


def _kernel_names(ctx, fn):
    """Stage names of the library's per-kernel timing table for one call of fn."""
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


def test_specialised_paths_decline(pkg, gpu):
    """A 512 x 512 image at P = 16 launches none of the compile-time-plan
    kernels.  The timing table names stages: every FFT row / column kernel of
    the encode (k_rows512pk, k_cols512b, k_fft_cols7, the 224 plan kernels,
    the generic ones) is timed as fft_rows / fft_cols, and the FFT decode
    (k_idct_cols512b, k_idct_rows512) is the one decode without the
    scatter_tokens and ipt_to_rgb stages.  The same calls at P = 14 do take
    those paths, so the names tell them apart."""
    lib = import_module("dct_autoencoder_amd._lib")
    ctx = lib.context(torch.device(DEV, torch.cuda.current_device()))

    def names_at(P, fe, pn, lfq, x):
        out = {}

        def enc():
            out["enc"] = fe.encode_batch(x, pn, lfq)[0]

        e = _kernel_names(ctx, enc)
        dp, codes = out["enc"]
        d = _kernel_names(ctx, lambda: fe.decode_batch(dp, codes, pn, lfq))
        return e, d

    g = gpu(16)
    x = g.imgs[0][None]
    assert tuple(x.shape) == (1, 3, 512, 512)
    e16, d16 = names_at(16, g.fe, g.pn, g.lfq(16), x)
    assert "fft_rows" not in e16 and "fft_cols" not in e16, e16
    assert "gemm_cols" in e16 and "tile_epilogue" in e16 and ("rows_fused" in e16 or "gemm_rows" in e16), e16
    assert "scatter_tokens" in d16 and "ipt_to_rgb" in d16, d16
    # 224 x 224 (k_rows224p / k_cols224 at P = 14): the GEMM DCT too
    e224, d224 = names_at(16, g.fe, g.pn, g.lfq(16), g.imgs[1][None])
    assert "fft_rows" not in e224 and "fft_cols" not in e224 and "gemm_cols" in e224, e224
    assert "scatter_tokens" in d224, d224
    # the control: P = 14 on the same image takes the specialised paths
    pn14 = pkg.PatchNorm(32, 32, 14, 3).to(DEV)
    pn14.b.data.fill_(0.05)
    pn14.frozen = True
    pn14.eval()
    fe14 = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
    lfq14 = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).to(DEV).eval()
    e14, d14 = names_at(14, fe14, pn14, lfq14, x)
    assert "fft_rows" in e14 and "fft_cols" in e14 and "gemm_cols" not in e14, e14
    assert "scatter_tokens" not in d14 and "idct_cols" in d14, d14
    e14, _ = names_at(14, fe14, pn14, lfq14, g.imgs[1][None])
    assert "fft_rows" in e14 and "fft_cols" in e14 and "gemm_cols" not in e14, e14


@pytest.mark.parametrize("P", [0, 17])
def test_patch_size_outside_1_16_is_rejected(pkg, P):
    """include/dctae.h: patch_size 1..16; check_cfg answers DCTAE_EUNSUP outside it."""
    fe = pkg.DCTAutoencoderFeatureExtractor(3, P, 0.0, 4, 4, 48)
    x = torch.rand(3, 40, 40, device=DEV)
    desc, dev, keep = _ops().image_set([x])
    plan = SimpleNamespace(row=[0], col=[0], k=[1], local_id=[0], row_len=[1])
    with pytest.raises(Exception, match=r"patch_size must be in \[1, 16\]"):
        _ops().encode(desc, dev, fe.params(), plan, 1, 48, None, None, want_codes=False)
    assert keep


def test_projected_lfq_at_p16(pkg, gpu):
    """The model's default geometry (patch_size 16: dim 256, codebook_dim 13,
    8 codebooks, with projections; k_lfq_proj_h2 / dctae_lfq_project_out at
    dim != 196): encode_batch's codes against F.linear on the GPU's own
    PatchNorm output inside the GEMM rounding band 4e-6 (|W| |x| + |b|), and
    decode_batch against the oracle's decode of the same codes."""
    c, g = _case(16), gpu(16)
    lcfg = ref_cpu.LFQConfig(dim=256, codebook_size=2 ** 13, num_codebooks=8)
    lfq = pkg.LFQ(dim=256, codebook_size=2 ** 13, num_codebooks=8)
    assert lfq.has_projections and lcfg.has_projections
    gen = torch.Generator().manual_seed(16)
    with torch.no_grad():
        for lin in (lfq.project_in, lfq.project_out):
            k = lin.in_features ** -0.5
            lin.weight.copy_((torch.rand(lin.weight.shape, generator=gen) * 2 - 1) * k)
            lin.bias.copy_((torch.rand(lin.bias.shape, generator=gen) * 2 - 1) * k)
    lfq = lfq.to(DEV).eval()
    imgs = [g.imgs[1], g.imgs[2]]
    assert [tuple(x.shape[1:]) for x in imgs] == [(224, 224), (100, 77)]
    ((dp, codes),) = g.fe.encode_batch(imgs, g.pn, lfq, return_patches=True)
    R, S = dp.key_pad_mask.shape
    assert codes.shape == (R, S, 8) and codes.dtype == torch.long
    y = dp.patches.cpu()
    W, b = lfq.project_in.weight.detach().cpu(), lfq.project_in.bias.detach().cpu()
    h = F.linear(y, W, b)
    _, oidx = ref_cpu.lfq_forward(y, lcfg, project_in=lambda t: F.linear(t, W, b))
    gc = codes.cpu()
    diff = gc != oidx
    band = 4e-6 * F.linear(y.abs(), W.abs(), b.abs())
    near = (h.abs() <= band).view(R, S, 8, 13).any(-1)
    assert torch.all(near[diff]), "code mismatch outside the GEMM rounding band"
    flips, n = int(diff.sum()), gc.numel()
    print(f"[P=16 projected] code mismatches inside the band: {flips} / {n}")
    assert flips <= max(2, n // 1000)
    ((dp2, codes2),) = g.fe.encode_batch(imgs, g.pn, lfq)
    assert torch.equal(codes2.cpu(), gc) and dp2.patches.shape[-1] == 0
    # project_out (dctae_lfq_project_out) inside the same band rule
    Wo, bo = lfq.project_out.weight.detach().cpu(), lfq.project_out.bias.detach().cpu()
    q = ref_cpu.lfq_indices_to_codes(gc, lcfg)
    want = F.linear(q, Wo, bo)
    got = lfq.indices_to_codes(codes).cpu()
    assert got.shape == want.shape == (R, S, 256)
    assert torch.all((got - want).abs() <= 4e-6 * F.linear(q.abs(), Wo.abs(), bo.abs()))
    # decode_batch against the oracle's decode of the same codes
    out = g.fe.decode_batch(dp2, codes, g.pn, lfq)
    kp, ids, pos, ch = (dp.key_pad_mask.cpu(), dp.batched_image_ids.cpu(), dp.patch_positions.cpu(),
                        dp.patch_channels.cpu())
    xin = ref_cpu.norm_inverse(c.tabs, want, ch, pos[..., 0], pos[..., 1])
    refs = ref_cpu.postprocess(ref_cpu.Batch(xin, kp, None, ids, ch, pos, list(dp.patch_sizes),
                                             list(dp.original_sizes)), c.cfg)
    assert len(out) == len(refs) == 2
    for a, r in zip(out, refs):
        assert a.shape == r.shape
        ok, dmax = _rgb_close(a.cpu(), r)
        assert ok, (dmax, float(r.abs().max()))
