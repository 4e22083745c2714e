"""GPU parity: the HIP path (through the C ABI) against the CPU oracle and the
reference's golden vectors.  Run on an MI355X: pytest -m gpu.

Tolerances (stated per test):
  * integer / index work (positions, channels, ids, masks, packing, synth
    bits, LFQ codes given identical fp32 input, PatchNorm given identical
    input): bit-exact;
  * DCT coefficients: |gpu - oracle| <= 2e-6 * max|Y| per image (two fp32
    evaluations of the same transform);
  * end-to-end LFQ codes: a bit may differ only where |x - median| is within
    the measured coefficient difference (guard band); the count is reported;
  * DCT->IDCT round trip / decode RGB: <= 1e-5 absolute (north_star) plus
    1e-5 relative for values beyond 1.
"""
import json
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
from oracle import ref_cpu, rng

pytestmark = pytest.mark.gpu
CFG = ref_cpu.FEConfig()
META = json.load(open(os.path.join(GOLDEN, "meta.json")))
DEV = "cuda"


@pytest.fixture(scope="module")
def fe(pkg):
    return pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)


@pytest.fixture(scope="module")
def pn(pkg, ref_tables):
    m = pkg.PatchNorm(32, 32, 14, 3).to(DEV)
    m.median.data.copy_(ref_tables.median)
    m.b.data.copy_(ref_tables.b)
    m.n.data.copy_(ref_tables.n)
    m.frozen = True
    return m.eval()


@pytest.fixture(scope="module")
def lfq(pkg):
    return pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).to(DEV).eval()


def _case_images(case):
    if case == "real":
        r = golden("real_inputs.npz")
        return [r[f"img{i}"].astype(np.float32) / 255.0 for i in range(len(r.files))]
    if case == "fold":
        # the GEMM DCT's even/odd folding: odd / even sizes without an FFT plan,
        # FFT rows + GEMM columns (fold of T in place) and GEMM rows + FFT columns
        return rng.synth_images(41, [(511, 512), (512, 511), (333, 517), (15, 17), (14, 14), (29, 1024), (448, 449)])
    c = META[case]
    return rng.synth_images(c["seed"], [tuple(s) for s in c["sizes"]], c["first"])


def _key(c, p):
    return (int(c), int(p[0]), int(p[1]))


def test_library_is_the_code_path(pkg):
    import ctypes
    lib = pkg.load_library()
    assert lib._name.endswith("libdctae.so")
    maps = open("/proc/self/maps").read()
    assert "libdctae.so" in maps


def test_synth_matches_numpy_bits(pkg):
    from importlib import import_module
    ops = import_module("dct_autoencoder_amd._ops")
    x = ops.synth_images(3, 37, 53, seed=1234, first_index=5).cpu().numpy()
    for i in range(3):
        assert np.array_equal(x[i], rng.synth_image(1234, 5 + i, 37, 53))


def test_norm_forward_inverse_bit_exact(pkg, pn, ref_tables):
    g = torch.Generator().manual_seed(0)
    R, S = 3, 700
    x = torch.randn(R, S, 196, generator=g) * 3
    ch = torch.randint(0, 3, (R, S), generator=g)
    pos = torch.randint(0, 32, (R, S, 2), generator=g)
    kp = torch.zeros(R, S, dtype=torch.bool)
    dp = pkg.DCTPatches(x.to(DEV), kp.to(DEV), None, torch.zeros(R, S, dtype=torch.long, device=DEV), ch.to(DEV),
                        pos.to(DEV), [], [])
    y = pn(dp).cpu()
    y_ref = ref_cpu.norm_forward_eval(ref_tables, x, ch, pos[..., 0], pos[..., 1])
    assert torch.equal(y, y_ref)
    dp.patches = y.to(DEV)
    xi = pn.inverse_norm(dp).cpu()
    xi_ref = ref_cpu.norm_inverse(ref_tables, y_ref, ch, pos[..., 0], pos[..., 1])
    assert torch.equal(xi, xi_ref)


def test_lfq_bit_exact(pkg, lfq):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 333, 196, generator=g)
    x[0, 0, :5] = 0.0            # zeros quantise to -1 / bit 0 (lfq.py:175)
    x[0, 1, 3] = float("nan")    # NaN > 0 is False
    q, idx, loss, dist = lfq(x.to(DEV), mask=torch.ones(2, 333, dtype=torch.bool, device=DEV))
    q_ref, idx_ref = ref_cpu.lfq_forward(x, ref_cpu.LFQConfig())
    assert torch.equal(idx.cpu(), idx_ref) and idx.dtype == torch.long
    assert torch.equal(q.cpu(), q_ref)
    codes = lfq.indices_to_codes(idx)
    assert torch.equal(codes.cpu(), ref_cpu.lfq_indices_to_codes(idx_ref, ref_cpu.LFQConfig()))


def _oracle_tokens(x_np):
    x = torch.from_numpy(x_np)
    y = ref_cpu.transform_image_in(x)
    ph, pw = ref_cpu.crop_dims(y.shape[1], y.shape[2], 14)
    return ref_cpu.patch_scores(y[:, :ph, :pw], CFG)


@pytest.mark.parametrize("case", ["sq224", "ragged", "real", "fold"])
def test_preprocess_tokens_and_order(fe, case):
    for x_np in _case_images(case):
        out = fe.preprocess(torch.from_numpy(x_np).to(DEV))
        toks, pos, ch, scores = _oracle_tokens(x_np)
        omap = {_key(c, p): i for i, (p, c) in enumerate(zip(pos.tolist(), ch.tolist()))}
        gp, gpos, gch = out["patches"].cpu(), out["positions"].cpu(), out["channels"].cpu()
        assert gp.shape[0] == len(omap) and out["positions"].dtype == torch.long
        idx = torch.tensor([omap[_key(c, p)] for p, c in zip(gpos.tolist(), gch.tolist())])
        assert len(set(idx.tolist())) == len(idx)
        ymax = float(toks.abs().max())
        err = float((gp - toks[idx]).abs().max())
        assert err <= 2e-6 * ymax, (err, ymax)
        # the GPU order is non-increasing in the oracle's scores up to the coefficient error
        s = scores[idx]
        assert torch.all(s[1:] <= s[:-1] + 0.1 * 4 * err + 1e-6)


def _image_slots(kp, ids):
    """(row, image id, token index tensor) in the reference's image enumeration order."""
    out = []
    for r in range(kp.shape[0]):
        for im in torch.unique(ids[r][~kp[r]]).tolist():
            out.append((r, im, torch.nonzero((~kp[r]) & (ids[r] == im)).flatten()))
    return out


@pytest.mark.parametrize("case", ["sq224", "ragged", "real"])
def test_encode_batch_vs_oracle(fe, pn, lfq, ref_tables, case):
    _encode_vs_oracle(fe, pn, lfq, ref_tables, _case_images(case), CFG, case)


def _encode_vs_oracle(fe, pn, lfq, ref_tables, imgs, CFG, case):
    ((dp, codes),) = fe.encode_batch([torch.from_numpy(x).to(DEV) for x in imgs], pn, lfq, return_raw=True)
    raw = dp.patches.cpu()
    codes = codes.cpu()
    kp, ids, pos, ch = (dp.key_pad_mask.cpu(), dp.batched_image_ids.cpu(), dp.patch_positions.cpu(),
                        dp.patch_channels.cpu())
    items = [ref_cpu.preprocess(torch.from_numpy(x), CFG) for x in imgs]
    ((ob, oidx),) = ref_cpu.encode([torch.from_numpy(x) for x in imgs], CFG, ref_tables, ref_cpu.LFQConfig())
    # packing metadata: bit-exact
    assert torch.equal(kp, ob.key_pad_mask)
    assert torch.equal(ids, ob.batched_image_ids)
    # pad tokens: exact (zeros normalised at c = h = w = 0)
    assert torch.equal(codes[kp], oidx[kp])
    assert torch.all(pos[kp] == 0) and torch.all(ch[kp] == 0)
    flips, n_codes = 0, 0
    slots = _image_slots(kp, ids)
    assert len(slots) == len(items)
    for (r, im, tj), it in zip(slots, items):
        gkeys = [_key(c, p) for p, c in zip(pos[r, tj].tolist(), ch[r, tj].tolist())]
        okeys = [_key(c, p) for p, c in zip(it["positions"].tolist(), it["channels"].tolist())]
        assert sorted(gkeys) == sorted(okeys)
        omap = {k: j for j, k in enumerate(okeys)}
        oj = torch.tensor([omap[k] for k in gkeys])
        toks_o = it["patches"][oj]
        d = (raw[r, tj] - toks_o).abs().max().item()
        ymax = toks_o.abs().max().item()
        assert d <= 2e-6 * ymax + 1e-6, (d, ymax)
        # oracle codes of the same tokens (oracle row r holds the same image at its own order)
        osel = torch.nonzero((~ob.key_pad_mask[r]) & (ob.batched_image_ids[r] == im)).flatten()
        ok = {_key(c, p): j for j, (p, c) in zip(osel.tolist(), zip(ob.patch_positions[r, osel].tolist(),
                                                                    ob.patch_channels[r, osel].tolist()))}
        oc = oidx[r, torch.tensor([ok[k] for k in gkeys])]
        gc = codes[r, tj]
        diff = gc != oc
        if diff.any():
            med = ref_tables.median[ch[r, tj], pos[r, tj, 0], pos[r, tj, 1]]
            near = ((toks_o - med).abs() <= 2 * d + 1e-7).view(-1, 14, 14).any(-1)
            assert torch.all(near[diff]), "code mismatch outside the guard band"
            flips += int(diff.sum())
        n_codes += gc.numel()
    print(f"[{case}] code mismatches inside the guard band: {flips} / {n_codes}")
    assert flips <= max(2, n_codes // 10000)


@pytest.mark.parametrize("caps", [(36, 36), (32, 36), (36, 32), (20, 32), (32, 20)])
def test_encode_512_patch_caps_vs_oracle(pkg, lfq, ref_tables, caps):
    """512-wide / 512-high images at max_patch_h / max_patch_w != 32: the kept
    corner is 14 * min(36, cap) (FE:312-345, 392-399), so the 512^2 kernels that
    assume 448 kept rows / columns (k_rows512pk, k_fft_cols7, k_cols512b) must
    hand these to the general kernels.  Tables: the reference fit extended to
    the 36 x 36 grid by repeating the last row / column."""
    mh, mw = caps
    cfg = ref_cpu.FEConfig(max_patch_h=mh, max_patch_w=mw, max_seq_len=3 * mh * mw)
    ih = torch.clamp(torch.arange(mh), max=31)
    iw = torch.clamp(torch.arange(mw), max=31)
    med = ref_tables.median[:, ih][:, :, iw].contiguous()
    b = ref_tables.b[:, ih][:, :, iw].contiguous()
    tables = ref_cpu.NormTables(ref_tables.n[:, ih][:, :, iw].contiguous(), med, b)
    pn = pkg.PatchNorm(mh, mw, 14, 3).to(DEV)
    pn.median.data.copy_(med)
    pn.b.data.copy_(b)
    pn.frozen = True
    pn.eval()
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, mh, mw, 3 * mh * mw)
    imgs = rng.synth_images(57, [(512, 512), (512, 512), (512, 300), (300, 512)])
    _encode_vs_oracle(fe, pn, lfq, tables, imgs, cfg, f"caps {caps}")


def test_norm_lfq_bit_exact_on_reference_tokens(pkg, pn, lfq):
    """Given the reference's own fp32 tokens, PatchNorm + LFQ on the GPU
    reproduce the reference's codes bit for bit (pads included)."""
    for case in ["sq224", "ragged", "real"]:
        g = golden(f"case_{case}.npz")
        n_img = len([k for k in g.files if k.endswith("_positions") and k.startswith("img")])
        R, S = g["key_pad_mask"].shape
        patches = torch.zeros(R, S, 196)
        ids = torch.from_numpy(g["batched_image_ids"].astype(np.int64))
        kp = torch.from_numpy(g["key_pad_mask"])
        # rebuild the row contents from the per-image token lists in packing order
        i = 0
        for r in range(R):
            col = 0
            nimg = len(torch.unique(ids[r][~kp[r]]))
            for _ in range(nimg):
                pt = torch.from_numpy(g[f"img{i}_patches"])
                patches[r, col:col + pt.shape[0]] = pt
                col += pt.shape[0]
                i += 1
        assert i == n_img
        dp = pkg.DCTPatches(patches.to(DEV), kp.to(DEV), None, ids.to(DEV),
                            torch.from_numpy(g["patch_channels"].astype(np.int64)).to(DEV),
                            torch.from_numpy(g["patch_positions"].astype(np.int64)).to(DEV), [], [])
        y = pn(dp)
        _, idx, _, _ = lfq(y, mask=~dp.key_pad_mask)
        assert torch.equal(idx.cpu(), torch.from_numpy(g["indices"].astype(np.int64))), case


def _rgb_close(a, b, atol=1e-5, rtol=1e-5):
    d = (a - b).abs()
    lim = atol + rtol * b.abs()
    return bool(torch.all(d <= lim)), float(d.max())


@pytest.mark.parametrize("case", ["sq224", "ragged"])
def test_decode_reference_codes(pkg, fe, pn, lfq, case):
    """decode_batch on the reference's own codes vs the reference's decoded RGB."""
    g = golden(f"case_{case}.npz")
    n_img = len([k for k in g.files if k.endswith("_positions") and k.startswith("img")])
    R, S = g["key_pad_mask"].shape
    dp = pkg.DCTPatches(torch.zeros(R, S, 0, device=DEV), torch.from_numpy(g["key_pad_mask"]).to(DEV), None,
                        torch.from_numpy(g["batched_image_ids"].astype(np.int64)).to(DEV),
                        torch.from_numpy(g["patch_channels"].astype(np.int64)).to(DEV),
                        torch.from_numpy(g["patch_positions"].astype(np.int64)).to(DEV),
                        [tuple(g[f"img{i}_patch_size"].tolist()) for i in range(n_img)],
                        [tuple(g[f"img{i}_original_size"].tolist()) for i in range(n_img)])
    codes = torch.from_numpy(g["indices"].astype(np.int64)).to(DEV)
    imgs = fe.decode_batch(dp, codes, pn, lfq)
    checked = 0
    for i in range(n_img):
        if f"img{i}_decoded_rgb" not in g.files:
            continue
        ref = torch.from_numpy(g[f"img{i}_decoded_rgb"])
        # decoded LFQ images span a wide range (|rgb| up to ~8 after the
        # 1/0.43 power): 1e-5 of the image's range, as for the round trip
        scale = max(1.0, float(ref.abs().max()))
        ok, dmax = _rgb_close(imgs[i].cpu(), ref, atol=1e-5 * scale, rtol=2e-5)
        assert ok, (i, dmax, scale)
        checked += 1
    assert checked >= 1


@pytest.mark.parametrize("shape", [(224, 224), (100, 77), (30, 700), (512, 512)])
def test_roundtrip_dct_idct(fe, shape):
    """preprocess -> iter_batches -> postprocess reproduces the input on the kept
    spectrum (lossless when nothing is cropped): <= 1e-5 vs the oracle's round trip."""
    x = torch.from_numpy(rng.synth_image(77, 0, *shape))
    item = fe.preprocess(x.to(DEV))
    loader = iter([{k: [v] for k, v in item.items()}])
    (batch,) = list(fe.iter_batches(loader, None))
    (img,) = fe.postprocess(batch)
    ob = list(ref_cpu.iter_batches(iter([{k: [v] for k, v in ref_cpu.preprocess(x, CFG).items()}]), CFG, None,
                                   build_attn_mask=False))[0]
    (ref,) = ref_cpu.postprocess(ob, CFG)
    ok, dmax = _rgb_close(img.cpu(), ref, atol=1e-5, rtol=1e-5)
    assert ok, dmax
    if shape[0] % 14 == 0 and shape[1] % 14 == 0 and shape[0] <= 448 and shape[1] <= 448:
        ok, dmax = _rgb_close(img.cpu(), x, atol=1e-5, rtol=1e-5)
        assert ok, dmax


def _guard_band_flips(gcodes, ocodes, toks_o, ch, pos, tables, d):
    """Code mismatches, each required to lie in the guard band: some element of
    the mismatching codebook row has |x_oracle - median| <= 2 d + 1e-7, d = the
    measured GPU-vs-oracle coefficient difference."""
    diff = gcodes != ocodes
    if not diff.any():
        return 0
    med = tables.median[ch, pos[:, 0], pos[:, 1]]
    near = ((toks_o - med).abs() <= 2 * d + 1e-7).view(-1, 14, 14).any(-1)
    assert torch.all(near[diff]), "code mismatch outside the guard band"
    return int(diff.sum())


def _check_image_vs_oracle(raw_g, codes_g, pos_g, ch_g, x_np, tables):
    """One image's GPU tokens / codes against the oracle, per (c, h, w) key:
    tokens within 2e-6 max|Y|, codes equal but inside the guard band.
    Returns (flips, codes compared)."""
    toks, opos, och, _ = _oracle_tokens(x_np)
    omap = {_key(c, p): i for i, (p, c) in enumerate(zip(opos.tolist(), och.tolist()))}
    gkeys = [_key(c, p) for p, c in zip(pos_g.tolist(), ch_g.tolist())]
    assert len(set(gkeys)) == len(gkeys) and all(k in omap for k in gkeys)
    oj = torch.tensor([omap[k] for k in gkeys])
    toks_o = toks[oj]
    d = (raw_g - toks_o).abs().max().item()
    ymax = toks_o.abs().max().item()
    assert d <= 2e-6 * ymax + 1e-6, (d, ymax)
    y = ref_cpu.norm_forward_eval(tables, toks_o[None], och[oj][None], opos[oj, 0][None], opos[oj, 1][None])
    _, oidx = ref_cpu.lfq_forward(y, ref_cpu.LFQConfig())
    oidx = oidx[0]
    return _guard_band_flips(codes_g, oidx, toks_o, och[oj], opos[oj], tables, d), codes_g.numel()


def test_encode_512_full_size(fe, pn, lfq, ref_tables):
    """Config 3 image size: 2 x 512^2, codes vs oracle inside the guard band, order self-consistent."""
    xs = rng.synth_images(1234, [(512, 512)] * 2, 200)
    x = torch.from_numpy(np.stack(xs)).to(DEV)
    ((dp, codes),) = fe.encode_batch(x, pn, lfq, return_raw=True, return_scores=True)
    assert dp.key_pad_mask.shape == (2, 3072) and not dp.key_pad_mask.any()
    sc = dp._data["scores"].cpu()
    assert torch.all(sc[:, 1:] <= sc[:, :-1])
    raw, codes = dp.patches.cpu(), codes.cpu()
    flips = n = 0
    for r in range(2):
        f, m = _check_image_vs_oracle(raw[r], codes[r], dp.patch_positions[r].cpu(), dp.patch_channels[r].cpu(), xs[r],
                                      ref_tables)
        flips, n = flips + f, n + m
    print(f"[512^2] code mismatches inside the guard band: {flips} / {n}")
    assert flips <= max(2, n // 10000)


def test_sq512_reference_codes(fe, pn, lfq, ref_tables):
    """The headline config against the REFERENCE's own codes (case_sq512: the
    reference run on the 512^2 image seed 1234 #100): per (c, h, w) token the
    GPU's 14 codes equal the reference's, any mismatch inside the guard band;
    the reference's stored 128-token head equals the oracle's tokens (to fp32
    rounding: bit-equal on the build container's CPU)."""
    g = golden("case_sq512.npz")
    m = META["sq512"]
    (x_np,) = rng.synth_images(m["seed"], [tuple(s) for s in m["sizes"]], m["first"])
    ((dp, codes),) = fe.encode_batch(torch.from_numpy(x_np)[None].to(DEV), pn, lfq, return_raw=True)
    raw, codes = dp.patches.cpu()[0], codes.cpu()[0]
    gpos, gch = dp.patch_positions.cpu()[0], dp.patch_channels.cpu()[0]
    rpos = torch.from_numpy(g["patch_positions"][0].astype(np.int64))
    rch = torch.from_numpy(g["patch_channels"][0].astype(np.int64))
    ridx = torch.from_numpy(g["indices"][0].astype(np.int64))
    rmap = {_key(c, p): j for j, (p, c) in enumerate(zip(rpos.tolist(), rch.tolist()))}
    gkeys = [_key(c, p) for p, c in zip(gpos.tolist(), gch.tolist())]
    assert sorted(gkeys) == sorted(rmap)
    rj = torch.tensor([rmap[k] for k in gkeys])
    toks, opos, och, _ = _oracle_tokens(x_np)
    omap = {_key(c, p): i for i, (p, c) in enumerate(zip(opos.tolist(), och.tolist()))}
    toks_o = toks[torch.tensor([omap[k] for k in gkeys])]
    head = torch.from_numpy(g["img0_patches_head"])
    hk = [_key(c, p) for p, c in zip(g["img0_positions"][:128].astype(np.int64).tolist(),
                                     g["img0_channels"][:128].astype(np.int64).tolist())]
    # bit-equal in the build container; other host CPUs round the oracle's FFT differently
    hd = (head - toks[torch.tensor([omap[k] for k in hk])]).abs().max().item()
    assert hd <= 1e-6 * head.abs().max().item(), hd
    d = (raw - toks_o).abs().max().item()
    assert d <= 2e-6 * toks_o.abs().max().item(), d
    flips = _guard_band_flips(codes, ridx[rj], toks_o, gch, gpos, ref_tables, d)
    print(f"[sq512 vs reference codes] mismatches inside the guard band: {flips} / {codes.numel()}")
    assert flips <= max(2, codes.numel() // 10000)


@pytest.mark.parametrize("bluestein", [0, 1])
@pytest.mark.parametrize("sizes", [[(1024, 1024)], [(1023, 997), (768, 1000)], [(1021, 333), (997, 1021)],
                                   [(30, 997), (997, 30), (262, 1000)]])
def test_large_ragged_vs_oracle(fe, pn, lfq, ref_tables, sizes, bluestein):
    """Config 4's sizes: 1024 x 1024 (runtime-plan Makhoul FFT rows / columns),
    768 x 1000 (7-smooth plans of other radices), odd and prime sides 1023,
    997, 1021, 333 and 262 = 2 x 131 (no Makhoul plan: Bluestein FFT,
    dctae_bluestein.hip, with option bluestein=1; the MFMA GEMM by default),
    and sides below 32 (always the GEMM) mixed with those both ways round:
    tokens and codes vs the oracle."""
    xs = rng.synth_images(97, sizes)
    ops = _ops()
    ops.set_option("bluestein", bluestein)
    try:
        ((dp, codes),) = fe.encode_batch([torch.from_numpy(a).to(DEV) for a in xs], pn, lfq, return_raw=True)
    finally:
        ops.set_option("bluestein", 0)
    raw, codes = dp.patches.cpu(), codes.cpu()
    kp, ids = dp.key_pad_mask.cpu(), dp.batched_image_ids.cpu()
    slots = _image_slots(kp, ids)
    assert len(slots) == len(xs)
    flips = n = 0
    for (r, im, tj), x_np in zip(slots, xs):
        f, m = _check_image_vs_oracle(raw[r, tj], codes[r, tj], dp.patch_positions.cpu()[r, tj],
                                      dp.patch_channels.cpu()[r, tj], x_np, ref_tables)
        flips, n = flips + f, n + m
    print(f"[{sizes}] code mismatches inside the guard band: {flips} / {n}")
    assert flips <= max(2, n // 10000)


@pytest.mark.parametrize("B,H", [(1024, 512), (256, 224)])
def test_batch_encoder_matches_encode_batch(pkg, fe, pn, lfq, ref_tables, B, H):
    """Full bench geometry (config 3: 1024 x 512^2; config 2: 256 x 224^2):
    the pre-planned BatchEncoder equals encode_batch on a sampled subset of the
    same images, bit for bit (codes, positions, channels; one image per row
    at 512^2, four at 224^2), and its codes of 3 (512^2) / 4 (224^2) images,
    the last one included, equal the oracle's outside the guard band."""
    from importlib import import_module
    fe_mod = import_module("dct_autoencoder_amd.feature_extraction")
    x = _ops().synth_images(B, H, H, seed=1234, first_index=0, device=DEV)
    enc = fe_mod.BatchEncoder(fe, B, H, H, pn, lfq, device=DEV)
    out = enc(x)
    codes_b = out["codes"].clone()
    pos_b, ch_b, ids_b, kp_b = out["positions"].clone(), out["channels"].clone(), out["image_ids"], out["key_pad_mask"]
    assert not kp_b.all(-1).any()
    sub = sorted(set([0, 1, B - 1] + list(range(5, B, max(1, B // 13)))))
    ((dp, codes_s),) = fe.encode_batch([x[i] for i in sub], pn, lfq)
    pl = enc.plan
    k = enc.k
    for n, i in enumerate(sub):
        r, c0 = pl.row[i], pl.col[i]
        rr, cc = _slot_of(dp, n)
        assert torch.equal(codes_b[r, c0:c0 + k], codes_s[rr, cc:cc + k])
        assert torch.equal(pos_b[r, c0:c0 + k], dp.patch_positions[rr, cc:cc + k])
        assert torch.equal(ch_b[r, c0:c0 + k], dp.patch_channels[rr, cc:cc + k])
        assert torch.all(ids_b[r, c0:c0 + k] == pl.local_id[i])
    # and straight against the oracle: images of the full-grid launch (the first,
    # two inside, the LAST: XCD dealing and the last partial block included);
    # the guard band's d is the coefficient difference of the same kernels on
    # that image (encode_batch with raw tokens, bit-equal codes checked above)
    pick = [0, 1, B // 2 + 3, B - 1] if B < 1024 else [0, B // 2 + 3, B - 1]
    ((dp_r, codes_r),) = fe.encode_batch([x[i] for i in pick], pn, lfq, return_raw=True)
    flips = n = 0
    for m, i in enumerate(pick):
        rr, cc = _slot_of(dp_r, m)
        r, c0 = pl.row[i], pl.col[i]
        assert torch.equal(codes_b[r, c0:c0 + k], codes_r[rr, cc:cc + k])
        f, t = _check_image_vs_oracle(dp_r.patches[rr, cc:cc + k].cpu(), codes_b[r, c0:c0 + k].cpu(),
                                      pos_b[r, c0:c0 + k].cpu(), ch_b[r, c0:c0 + k].cpu(), x[i].cpu().numpy(),
                                      ref_tables)
        flips, n = flips + f, n + t
    print(f"[BatchEncoder {B} x {H}^2 vs oracle, images {pick}] mismatches inside the guard band: {flips} / {n}")
    assert flips <= max(2, n // 10000)


def _slot_of(dp, n):
    """(row, first column) of the n-th image (reference enumeration order) of a packed batch."""
    kp, ids = dp.key_pad_mask.cpu(), dp.batched_image_ids.cpu()
    (r, im, tj) = _image_slots(kp, ids)[n]
    return r, int(tj[0])


def test_to_dict_of_gpu_codes(pkg, fe, pn, lfq, ref_tables):
    """HIP-encoded codes of the ragged case through to_dict give
    the reference's JSON (ragged_to_dict.json, made by the reference's
    dct_patches.to_dict): same images, sizes and per-(c, h, w) codes (a code
    may differ only inside the guard band; token order compared as a map)."""
    from importlib import import_module
    dpm = import_module("dct_autoencoder_amd.dct_patches")
    imgs = _case_images("ragged")
    ((dp, codes),) = fe.encode_batch([torch.from_numpy(a).to(DEV) for a in imgs], pn, lfq, return_raw=True)
    objs = json.loads(json.dumps(dpm.to_dict(dp, codes)))
    ref = json.load(open(os.path.join(GOLDEN, "ragged_to_dict.json")))
    assert len(objs) == len(ref)
    flips = 0
    for a, b in zip(objs, ref):
        assert list(a["size"]) == list(b["size"]) and list(a["original_size"]) == list(b["original_size"])
        ma = {(t["c"], t["h"], t["w"]): t["data"] for t in a["codes"]}
        mb = {(t["c"], t["h"], t["w"]): t["data"] for t in b["codes"]}
        assert ma.keys() == mb.keys()
        flips += sum(x != y for k in ma for x, y in zip(ma[k], mb[k]))
    assert flips <= 2, flips
    # and back: from_dict of the GPU dump decodes like the packed batch
    one, c1 = dpm.from_dict(objs[0])
    assert c1.shape == (len(objs[0]["codes"]), 14)


def test_revert_patching_vs_oracle(fe):
    """FE.revert_patching (FE:607-656) of a packed ragged batch: each image's
    (3, 14 ph, 14 pw) spectrum equals the oracle's, exactly (a scatter)."""
    imgs = _case_images("ragged")
    items = [fe.preprocess(torch.from_numpy(a).to(DEV)) for a in imgs]
    (batch,) = list(fe.iter_batches(iter([{k: [it[k] for it in items] for k in items[0]}]), None))
    got = fe.revert_patching(batch)
    ob = ref_cpu.Batch(batch.patches.cpu(), batch.key_pad_mask.cpu(), None, batch.batched_image_ids.cpu(),
                       batch.patch_channels.cpu(), batch.patch_positions.cpu(), batch.patch_sizes, batch.original_sizes)
    want = ref_cpu.revert_patching(ob, CFG)
    assert len(got) == len(want) == len(imgs)
    for a, b in zip(got, want):
        assert torch.equal(a.cpu(), b)


def test_beta_sampling_matches_reference_k(pkg):
    m = META["beta"]
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, m["beta"], 32, 32, m["max_seq_len"])
    g = golden("case_beta.npz")
    random.seed(m["seed_python_random"])
    for i, x in enumerate(rng.synth_images(m["img_seed"], [tuple(s) for s in m["sizes"]])):
        out = fe.preprocess(torch.from_numpy(x).to(DEV))
        assert out["patches"].shape[0] == int(g[f"img{i}_k"])


def _ops():
    from importlib import import_module
    return import_module("dct_autoencoder_amd._ops")


@pytest.mark.parametrize("shape", [(512, 512), (224, 224), (100, 300), (30, 700), (224, 98), (98, 224), (224, 322)])
def test_fft_path_matches_gemm_path(fe, pn, lfq, shape):
    """The FFT-DCT kernels and the MFMA GEMM DCT are two evaluations of the
    same transform: tokens within 2e-6 * max|Y|, codes equal except inside the
    guard band.  (224, 98) / (224, 322): k_cols224 with an odd column-item
    count (the last pair repeats its item); (98, 224): k_rows224p with a
    partial last block."""
    ops = _ops()
    x = torch.from_numpy(np.stack(rng.synth_images(31, [shape] * 2))).to(DEV)
    ops.set_option("fft_generic", 1)   # sides without a compile-time kernel on the generic FFT kernels too
    try:
        ((dp_f, c_f),) = fe.encode_batch(x, pn, lfq, return_raw=True)
    finally:
        ops.set_option("fft_generic", 0)
    ops.set_fft(False)
    try:
        ((dp_g, c_g),) = fe.encode_batch(x, pn, lfq, return_raw=True)
    finally:
        ops.set_fft(True)
    rf, rg = dp_f.patches.cpu(), dp_g.patches.cpu()
    kp = dp_f.key_pad_mask.cpu()
    for r in range(kp.shape[0]):
        ids_g, ids_f = dp_g.batched_image_ids[r].tolist(), dp_f.batched_image_ids[r].tolist()
        gm = {(ids_g[j],) + _key(c, p): j for j, (p, c) in
              enumerate(zip(dp_g.patch_positions[r].tolist(), dp_g.patch_channels[r].tolist())) if not kp[r, j]}
        fm = [(j, (ids_f[j],) + _key(c, p)) for j, (p, c) in
              enumerate(zip(dp_f.patch_positions[r].tolist(), dp_f.patch_channels[r].tolist())) if not kp[r, j]]
        fj = torch.tensor([j for j, _ in fm])
        gj = torch.tensor([gm[k] for _, k in fm])
        ymax = rg[r, gj].abs().max().item()
        d = (rf[r, fj] - rg[r, gj]).abs().max().item()
        assert d <= 2e-6 * ymax, (d, ymax)
        mism = (c_f.cpu()[r, fj] != c_g.cpu()[r, gj]).sum().item()
        assert mism <= max(2, fj.numel() * 14 // 10000), mism


@pytest.mark.parametrize("shape", [(224, 98), (98, 224), (224, 322), (322, 224)])
def test_224_kernels_odd_shapes_vs_oracle(fe, pn, lfq, ref_tables, shape):
    """Config 2's kernels (k_rows224p for 224-wide rows, k_cols224 for
    224-high columns) on shapes with an odd column-item count (224 x 98,
    224 x 322) or a partial last row block (98 x 224, 322 x 224): tokens and
    codes straight against the oracle (not the GEMM path)."""
    _encode_vs_oracle(fe, pn, lfq, ref_tables, rng.synth_images(43, [shape] * 3), CFG, f"224 kernels {shape}")


@pytest.mark.parametrize("shape", [(105, 225), (225, 105), (245, 63), (189, 175), (135, 256), (256, 135)])
def test_odd_smooth_sides_fft_vs_oracle(fe, pn, lfq, ref_tables, shape):
    """Odd 7-smooth sides (N <= 256) on the generic FFT kernels in the
    real-FFT form (M = N complex points of Makhoul's reordered sequence,
    X_k = Re(w_k Z_k); option fft_odd, off by default: measured slower than
    the GEMM DCT on config 4): tokens and codes against the oracle, rows and
    columns each odd or even."""
    ops = _ops()
    ops.set_option("fft_odd", 1)
    ops.set_option("fft_generic", 1)
    try:
        _encode_vs_oracle(fe, pn, lfq, ref_tables, rng.synth_images(53, [shape] * 2), CFG, f"odd sides {shape}")
    finally:
        ops.set_option("fft_odd", 0)
        ops.set_option("fft_generic", 0)


def test_odd_smooth_sides_fft_matches_gemm(fe):
    """The odd-side FFT plans against the MFMA GEMM DCT they replace
    (fft_odd=0): the same tokens within 2e-6 x max|Y|."""
    ops = _ops()
    xs = rng.synth_images(54, [(105, 225), (243, 175), (63, 98)])
    outs = {}
    for odd in (1, 0):
        ops.set_option("fft_odd", odd)
        ops.set_option("fft_generic", odd)
        try:
            outs[odd] = [fe.preprocess(torch.from_numpy(x).to(DEV)) for x in xs]
        finally:
            ops.set_option("fft_odd", 0)
            ops.set_option("fft_generic", 0)
    for a, b in zip(outs[1], outs[0]):
        # token orders may differ at near-tied scores: match tokens by (c, h, w)
        ka = {(int(c), int(p[0]), int(p[1])): i for i, (p, c) in enumerate(zip(a["positions"].tolist(),
                                                                              a["channels"].tolist()))}
        idx = torch.tensor([ka[(int(c), int(p[0]), int(p[1]))] for p, c in zip(b["positions"].tolist(),
                                                                                 b["channels"].tolist())])
        pa, pb = a["patches"][idx].cpu(), b["patches"].cpu()
        ymax = float(pb.abs().max())
        assert float((pa - pb).abs().max()) <= 2e-6 * ymax, float((pa - pb).abs().max()) / ymax


def test_gemm_h2_accuracy_vs_oracle_and_x3(fe):
    """The encode's DCT GEMMs on k_gemm_h2 (fp16 MFMA, two-piece operands
    scaled into the fp16 range, three products; default) against the oracle's
    tokens and against k_gemm_x3 (split-bf16, six products; gemm_h2=0) on
    sides without an FFT plan (GEMM rows and columns, odd and even folds, FFT
    rows + GEMM columns through k_fold_t, sides below 32): tokens within
    5e-7 x max|Y| of the oracle (the global tolerance is 2e-6)."""
    ops = _ops()
    xs = rng.synth_images(47, [(333, 517), (1021, 997), (512, 511), (448, 449), (15, 17), (256, 1000), (1000, 97)])
    outs = {}
    for h2 in (1, 0):
        ops.set_option("gemm_h2", h2)
        try:
            outs[h2] = [fe.preprocess(torch.from_numpy(x).to(DEV)) for x in xs]
        finally:
            ops.set_option("gemm_h2", 1)
    worst = {0: 0.0, 1: 0.0}
    for n, x_np in enumerate(xs):
        toks, pos, ch, _ = _oracle_tokens(x_np)
        omap = {_key(c, p): i for i, (p, c) in enumerate(zip(pos.tolist(), ch.tolist()))}
        ymax = float(toks.abs().max())
        for h2 in (1, 0):
            out = outs[h2][n]
            idx = torch.tensor([omap[_key(c, p)] for p, c in zip(out["positions"].cpu().tolist(),
                                                                 out["channels"].cpu().tolist())])
            err = float((out["patches"].cpu() - toks[idx]).abs().max()) / ymax
            worst[h2] = max(worst[h2], err)
    print(f"[gemm tokens vs oracle, / max|Y|] h2 {worst[1]:.3g}  x3 {worst[0]:.3g}")
    assert worst[1] <= 5e-7, worst


@pytest.mark.parametrize("shape", [(333, 517), (1021, 997), (97, 1000), (1000, 97), (30, 997), (997, 30)])
def test_bluestein_matches_gemm_path(fe, pn, lfq, shape):
    """Sides without a Makhoul plan: the Bluestein FFT (option bluestein=1)
    and the MFMA GEMM DCT (default) agree on the tokens within 2e-6 * max|Y|
    and on the codes except inside the guard band; rows and columns each take
    either path (sides < 32 stay on the GEMM)."""
    ops = _ops()
    x = torch.from_numpy(np.stack(rng.synth_images(37, [shape] * 2))).to(DEV)
    ((dp_g, c_g),) = fe.encode_batch(x, pn, lfq, return_raw=True)
    ops.set_option("bluestein", 1)
    try:
        ((dp_b, c_b),) = fe.encode_batch(x, pn, lfq, return_raw=True)
    finally:
        ops.set_option("bluestein", 0)
    kp = dp_b.key_pad_mask.cpu()
    assert torch.equal(kp, dp_g.key_pad_mask.cpu())
    rb, rg = dp_b.patches.cpu(), dp_g.patches.cpu()
    for r in range(kp.shape[0]):
        ids_g, ids_b = dp_g.batched_image_ids[r].tolist(), dp_b.batched_image_ids[r].tolist()
        gm = {(ids_g[j],) + _key(c, p): j for j, (p, c) in
              enumerate(zip(dp_g.patch_positions[r].tolist(), dp_g.patch_channels[r].tolist())) if not kp[r, j]}
        bm = [(j, (ids_b[j],) + _key(c, p)) for j, (p, c) in
              enumerate(zip(dp_b.patch_positions[r].tolist(), dp_b.patch_channels[r].tolist())) if not kp[r, j]]
        bj = torch.tensor([j for j, _ in bm])
        gj = torch.tensor([gm[k] for _, k in bm])
        ymax = rg[r, gj].abs().max().item()
        d = (rb[r, bj] - rg[r, gj]).abs().max().item()
        assert d <= 2e-6 * ymax, (d, ymax)
        mism = (c_b.cpu()[r, bj] != c_g.cpu()[r, gj]).sum().item()
        assert mism <= max(2, bj.numel() * 14 // 10000), mism


def test_threshold_bits_equal_normalised_bits(fe, pn, lfq):
    """codes from the exact thresholds (codes-only encode) == codes from the
    PatchNorm values (encode with normalised patches), on identical DCT input."""
    x = torch.from_numpy(np.stack(rng.synth_images(41, [(512, 512)] * 2))).to(DEV)
    ((dp_a, c_a),) = fe.encode_batch(x, pn, lfq)
    ((dp_b, c_b),) = fe.encode_batch(x, pn, lfq, return_patches=True)
    assert torch.equal(c_a, c_b)
    assert torch.equal(dp_a.patch_positions, dp_b.patch_positions)
    # and the normalised patches reproduce the codes through the LFQ kernel
    _, idx, _, _ = lfq(dp_b.patches, mask=~dp_b.key_pad_mask)
    assert torch.equal(idx, c_b)


def test_thresholds_are_exact(pn):
    st = pn.state(thresholds=True)
    thr = st.thr.cpu()
    med, b = st.median.cpu(), st.b.cpu()
    sd = b * 2 ** 0.5 + st.eps
    ok = torch.isfinite(thr)
    t = thr[ok]
    # PatchNorm(thr) > 0 and PatchNorm(prev float below thr) <= 0
    y_at = ((t - med[ok]) / sd[ok]).clamp(-6, 6)
    below = torch.nextafter(t, torch.full_like(t, -float("inf")))
    y_below = ((below - med[ok]) / sd[ok]).clamp(-6, 6)
    assert torch.all(y_at > 0) and torch.all(y_below <= 0)


DEFAULTS = {"rows_kernel": 4, "sort_kernel": 2, "chunk_bytes": 1 << 40, "cols512b": 1}
SPEC_VARIANTS = {  # option sets of the specialised kernels (reset to DEFAULTS afterwards)
    "default": {},
    "rows_lds": {"rows_kernel": 2},
    "cols7": {"cols512b": 0},
    "sort_bitonic": {"sort_kernel": 1},
    "chunks": {"chunk_bytes": 4 << 20},
}


@pytest.mark.parametrize("variant", list(SPEC_VARIANTS))
@pytest.mark.parametrize("shape", [(512, 512), (224, 224)])
def test_specialised_kernels_match_generic(fe, pn, lfq, shape, variant):
    """dctae_fft2.hip (compile-time plans) vs dctae_fft.hip (runtime plans):
    same algorithm, different op order -> tokens within 1e-6 * max|Y|."""
    ops = _ops()
    x = torch.from_numpy(np.stack(rng.synth_images(53, [shape] * 3))).to(DEV)
    for k, v in SPEC_VARIANTS[variant].items():
        ops.set_option(k, v)
    try:
        ((dp_s, c_s),) = fe.encode_batch(x, pn, lfq, return_raw=True, return_scores=True)
    finally:
        for k, v in DEFAULTS.items():
            ops.set_option(k, v)
    ops.set_option("fft_spec", 0)
    ops.set_option("fft_generic", 1)
    try:
        ((dp_g, c_g),) = fe.encode_batch(x, pn, lfq, return_raw=True, return_scores=True)
    finally:
        ops.set_option("fft_spec", 1)
        ops.set_option("fft_generic", 0)
    kp = dp_s.key_pad_mask.cpu()
    ids_s, ids_g = dp_s.batched_image_ids.cpu(), dp_g.batched_image_ids.cpu()
    for r in range(kp.shape[0]):
        gm = {(int(ids_g[r, j]),) + _key(c, p): j for j, (p, c) in
              enumerate(zip(dp_g.patch_positions[r].tolist(), dp_g.patch_channels[r].tolist())) if not kp[r, j]}
        pairs = [(j, gm[(int(ids_s[r, j]),) + _key(c, p)]) for j, (p, c) in
                 enumerate(zip(dp_s.patch_positions[r].tolist(), dp_s.patch_channels[r].tolist())) if not kp[r, j]]
        sj = torch.tensor([a for a, _ in pairs]); gj = torch.tensor([b for _, b in pairs])
        a, b = dp_s.patches.cpu()[r, sj], dp_g.patches.cpu()[r, gj]
        assert (a - b).abs().max().item() <= 1e-6 * b.abs().max().item()
        assert (c_s.cpu()[r, sj] != c_g.cpu()[r, gj]).sum().item() <= 4


@pytest.mark.parametrize("dec_cols", [2, 1])
def test_fft_decode_512_vs_oracle_and_gemm(fe, pn, lfq, ref_tables, dec_cols):
    """Config 3 decode (codes -> indices_to_codes -> inverse_norm -> revert ->
    IDCT -> RGB) of 512^2 images on the FFT path (dctae_idct.hip; columns on
    k_idct_cols512b with the band-layout U (dec_cols_kernel 2, default) or
    k_idct_cols512 with row-major U (1)) against the oracle's decode of the
    same codes (<= 1e-5 x image range) and against the MFMA GEMM decode (two
    fp32 evaluations of the same transform)."""
    ops = _ops()
    x = torch.from_numpy(np.stack(rng.synth_images(71, [(512, 512)] * 3))).to(DEV)
    ((dp, codes),) = fe.encode_batch(x, pn, lfq)
    ops.set_option("dec_cols_kernel", dec_cols)
    try:
        imgs_fft = fe.decode_batch(dp, codes, pn, lfq)
    finally:
        ops.set_option("dec_cols_kernel", 2)
    ops.set_option("fft_decode", 0)
    try:
        imgs_gemm = fe.decode_batch(dp, codes, pn, lfq)
    finally:
        ops.set_option("fft_decode", 1)
    ops.check_device_errors(x.device)
    kp = dp.key_pad_mask.cpu()
    y = ref_cpu.lfq_indices_to_codes(codes.cpu(), ref_cpu.LFQConfig())
    pos = dp.patch_positions.cpu()
    chs = dp.patch_channels.cpu()
    xin = ref_cpu.norm_inverse(ref_tables, y, chs, pos[..., 0], pos[..., 1])
    batch = ref_cpu.Batch(xin, kp, None, dp.batched_image_ids.cpu(), chs, pos, dp.patch_sizes, dp.original_sizes)
    refs = ref_cpu.postprocess(batch, CFG)
    assert len(refs) == len(imgs_fft) == len(imgs_gemm) == 3
    for a, b, r in zip(imgs_fft, imgs_gemm, refs):
        scale = max(1.0, float(r.abs().max()))
        ok, dmax = _rgb_close(a.cpu(), r, atol=1e-5 * scale, rtol=2e-5)
        assert ok, ("fft vs oracle", dmax, scale)
        ok, dmax = _rgb_close(a.cpu(), b.cpu(), atol=1e-5 * scale, rtol=2e-5)
        assert ok, ("fft vs gemm", dmax, scale)


@pytest.mark.parametrize("shapes", [[(512, 512)] * 2, [(224, 224), (100, 140), (300, 262)]], ids=["fft512", "gemm"])
def test_decode_odd_seq_len_vs_oracle(pkg, pn, lfq, ref_tables, shapes):
    """max_seq_len 3073 (odd): every packed row ends in pads and the token count
    is not a multiple of 4, so k_dec_map runs its 4-token vector loop and the
    token-by-token tail; decode (FFT path at 512^2, GEMM otherwise) against
    the oracle's decode of the same codes."""
    cfg = ref_cpu.FEConfig(max_seq_len=3073)
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3073)
    xs = rng.synth_images(91, shapes)
    ((dp, codes),) = fe.encode_batch([torch.from_numpy(a).to(DEV) for a in xs], pn, lfq)
    assert (dp.key_pad_mask.numel() % 4) != 0
    imgs = fe.decode_batch(dp, codes, pn, lfq)
    _ops().check_device_errors(codes.device)
    y = ref_cpu.lfq_indices_to_codes(codes.cpu(), ref_cpu.LFQConfig())
    pos, chs = dp.patch_positions.cpu(), dp.patch_channels.cpu()
    xin = ref_cpu.norm_inverse(ref_tables, y, chs, pos[..., 0], pos[..., 1])
    batch = ref_cpu.Batch(xin, dp.key_pad_mask.cpu(), None, dp.batched_image_ids.cpu(), chs, pos, dp.patch_sizes,
                          dp.original_sizes)
    refs = ref_cpu.postprocess(batch, cfg)
    assert len(refs) == len(imgs) == len(xs)
    for a, r in zip(imgs, refs):
        scale = max(1.0, float(r.abs().max()))
        ok, dmax = _rgb_close(a.cpu(), r, atol=1e-5 * scale, rtol=2e-5)
        assert ok, (dmax, scale)


@pytest.mark.parametrize("caps", [(20, 32), (32, 20)])
def test_fft_decode_512_patch_caps_vs_oracle(pkg, lfq, ref_tables, caps):
    """512^2 decode at max_patch_h / max_patch_w below 32: 20 kept tile rows
    (band-layout column kernel with absent tiles zero) or 20 kept tile columns
    (row-major U, k_idct_cols512 + k_idct_rows2) against the oracle's decode."""
    mh, mw = caps
    cfg = ref_cpu.FEConfig(max_patch_h=mh, max_patch_w=mw, max_seq_len=3 * mh * mw)
    tables = ref_cpu.NormTables(ref_tables.n[:, :mh, :mw].contiguous(), ref_tables.median[:, :mh, :mw].contiguous(),
                                ref_tables.b[:, :mh, :mw].contiguous())
    pn = pkg.PatchNorm(mh, mw, 14, 3).to(DEV)
    pn.median.data.copy_(tables.median)
    pn.b.data.copy_(tables.b)
    pn.frozen = True
    pn.eval()
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, mh, mw, 3 * mh * mw)
    x = torch.from_numpy(np.stack(rng.synth_images(73, [(512, 512)] * 2))).to(DEV)
    ((dp, codes),) = fe.encode_batch(x, pn, lfq)
    imgs = fe.decode_batch(dp, codes, pn, lfq)
    _ops().check_device_errors(x.device)
    y = ref_cpu.lfq_indices_to_codes(codes.cpu(), ref_cpu.LFQConfig())
    pos, chs = dp.patch_positions.cpu(), dp.patch_channels.cpu()
    xin = ref_cpu.norm_inverse(tables, y, chs, pos[..., 0], pos[..., 1])
    batch = ref_cpu.Batch(xin, dp.key_pad_mask.cpu(), None, dp.batched_image_ids.cpu(), chs, pos, dp.patch_sizes,
                          dp.original_sizes)
    refs = ref_cpu.postprocess(batch, cfg)
    for a, r in zip(imgs, refs):
        scale = max(1.0, float(r.abs().max()))
        ok, dmax = _rgb_close(a.cpu(), r, atol=1e-5 * scale, rtol=2e-5)
        assert ok, (dmax, scale)


def test_sort_overlap_bit_identical(fe, pn, lfq):
    """Option sort_overlap (the columns of a band-image batch in two halves,
    the first half's sort / pack on a side stream beside the second half's
    column kernel): every packed output equal to the one-stream encode."""
    ops = _ops()
    x = ops.synth_images(96, 512, 512, seed=77, device=torch.device(DEV))
    ((dp0, c0),) = fe.encode_batch(x, pn, lfq, return_raw=True)
    ops.set_option("sort_overlap", 1)
    try:
        ((dp1, c1),) = fe.encode_batch(x, pn, lfq, return_raw=True)
    finally:
        ops.set_option("sort_overlap", 0)
    torch.cuda.synchronize()
    assert torch.equal(c0, c1)
    for f in ("patches", "key_pad_mask", "batched_image_ids", "patch_channels", "patch_positions"):
        assert torch.equal(getattr(dp0, f), getattr(dp1, f)), f


def test_cols_wide_bit_identical(fe, pn, lfq):
    """Option cols_wide (off by default, measured slower: the codes-only column
    pass of 512^2 band images on k_cols512w, two tile strips per 7-wave block) against
    k_cols512b (cols_wide=0): codes, raw tokens, scores and packing equal bit
    for bit, odd image count included."""
    ops = _ops()
    x = ops.synth_images(7, 512, 512, seed=79, device=torch.device(DEV))
    outs = {}
    for w in (1, 0):
        ops.set_option("cols_wide", w)
        try:
            outs[w] = fe.encode_batch(x, pn, lfq, return_raw=True, return_scores=True)[0]
        finally:
            ops.set_option("cols_wide", 0)
    (dp1, c1), (dp0, c0) = outs[1], outs[0]
    torch.cuda.synchronize()
    assert torch.equal(c0, c1)
    assert torch.equal(dp0._data["scores"], dp1._data["scores"])
    for f in ("patches", "key_pad_mask", "batched_image_ids", "patch_channels", "patch_positions"):
        assert torch.equal(getattr(dp0, f), getattr(dp1, f)), f


HALVES_DEFAULT = 0   # Options::halves (csrc/dctae_options.h)


@pytest.mark.parametrize("n", [33, 64])
def test_halves_bit_identical(fe, pn, lfq, n):
    """Option halves (off by default, measured slower; config 2's 224^2 batches of >= 32 images:
    the first half's columns and sort / pack on a side stream beside the
    second half's rows and columns): every packed output equal to the
    one-stream encode (halves=0), odd image count included."""
    ops = _ops()
    x = ops.synth_images(n, 224, 224, seed=78, device=torch.device(DEV))
    ops.set_option("halves", 1)
    ((dp1, c1),) = fe.encode_batch(x, pn, lfq, return_raw=True)
    ops.set_option("halves", 0)
    ((dp0, c0),) = fe.encode_batch(x, pn, lfq, return_raw=True)
    ops.set_option("halves", HALVES_DEFAULT)
    torch.cuda.synchronize()
    assert torch.equal(c0, c1)
    for f in ("patches", "key_pad_mask", "batched_image_ids", "patch_channels", "patch_positions"):
        assert torch.equal(getattr(dp0, f), getattr(dp1, f)), f


@pytest.mark.parametrize("shapes", [[(512, 512)] * 2, [(224, 224), (300, 262)]], ids=["fft512", "gemm"])
def test_fft_decode_duplicate_tokens_last_wins(fe, pn, lfq, ref_tables, shapes):
    """Two tokens of one image at the same (channel, h, w): the reference's
    revert_patching assigns tokens in packed order (FE:639-643), so the later
    one wins.  FFT decode (512^2: item-major map by atomicMax + staged codes)
    and the GEMM decode (other sizes: the same slot map gates
    k_scatter_tokens' stores) against the oracle's per-token loop on the same
    edited batch."""
    xs = rng.synth_images(83, shapes)
    x = torch.from_numpy(np.stack(xs)).to(DEV) if len(set(shapes)) == 1 else [torch.from_numpy(a).to(DEV) for a in xs]
    ((dp, codes),) = fe.encode_batch(x, pn, lfq)
    pos, chs, codes = dp.patch_positions.clone(), dp.patch_channels.clone(), codes.clone()
    ids, kp = dp.batched_image_ids, dp.key_pad_mask
    # image of row 0's first token: copy (c, h, w) of its slot j0 onto three later slots of the same image
    img0 = int(ids[0, 0])
    js = [j for j in range(ids.shape[1]) if int(ids[0, j]) == img0 and not bool(kp[0, j])]
    j0, later = js[3], [js[len(js) // 8], js[len(js) // 2], js[len(js) - 1]]
    for n, j in enumerate(later):
        pos[0, j] = pos[0, j0]
        chs[0, j] = chs[0, j0]
        codes[0, j] = (codes[0, j0] + 977 * (n + 1)) % (2 ** 14)   # distinguishable codes
    dp.patch_positions, dp.patch_channels = pos, chs
    imgs = fe.decode_batch(dp, codes, pn, lfq)
    _ops().check_device_errors(codes.device)
    y = ref_cpu.lfq_indices_to_codes(codes.cpu(), ref_cpu.LFQConfig())
    xin = ref_cpu.norm_inverse(ref_tables, y, chs.cpu(), pos.cpu()[..., 0], pos.cpu()[..., 1])
    batch = ref_cpu.Batch(xin, kp.cpu(), None, ids.cpu(), chs.cpu(), pos.cpu(), dp.patch_sizes, dp.original_sizes)
    refs = ref_cpu.postprocess(batch, CFG, per_token_loop=True)
    for a, r in zip(imgs, refs):
        scale = max(1.0, float(r.abs().max()))
        ok, dmax = _rgb_close(a.cpu(), r, atol=1e-5 * scale, rtol=2e-5)
        assert ok, (dmax, scale)


def test_fft_decode_patches_roundtrip_512(fe):
    """postprocess (patch-space decode) of a 512^2 preprocess on the FFT path is
    the inverse of the kept-corner DCT: equal to the oracle's round trip."""
    x = torch.from_numpy(rng.synth_image(79, 0, 512, 512))
    item = fe.preprocess(x.to(DEV))
    (batch,) = list(fe.iter_batches(iter([{k: [v] for k, v in item.items()}]), None))
    (img,) = fe.postprocess(batch)
    ob = list(ref_cpu.iter_batches(iter([{k: [v] for k, v in ref_cpu.preprocess(x, CFG).items()}]), CFG, None,
                                   build_attn_mask=False))[0]
    (ref,) = ref_cpu.postprocess(ob, CFG)
    ok, dmax = _rgb_close(img.cpu(), ref, atol=1e-5, rtol=1e-5)
    assert ok, dmax



@pytest.mark.parametrize("cbd", [7, 4, 2, 1])
def test_lfq_groupings_regroup_the_same_bits(pkg, fe, pn, lfq, cbd):
    """Any LFQ grouping with codebook_dim * num_codebooks = 196 (lfq.py:168)
    quantises the same sign bits; its codes are the 14 x 14 codes' bits
    (row-major, MSB first) cut into codebook_dim-bit groups.  Covers the FFT
    (512, 224) and GEMM (odd / unplanned) paths."""
    shapes = [(512, 512), (224, 224), (333, 517), (100, 300)]
    x = [torch.from_numpy(a).to(DEV) for a in rng.synth_images(53, shapes)]
    other = pkg.LFQ(dim=196, codebook_size=2 ** cbd, num_codebooks=196 // cbd).to(DEV).eval()
    ((dp_a, c_a),) = fe.encode_batch(x, pn, lfq)
    ((dp_b, c_b),) = fe.encode_batch(x, pn, other)
    assert torch.equal(dp_a.patch_positions, dp_b.patch_positions)
    w14 = 2 ** torch.arange(13, -1, -1, device=DEV)
    bits = ((c_a[..., None] & w14) != 0).reshape(*c_a.shape[:-1], 196)
    wb = 2 ** torch.arange(cbd - 1, -1, -1, device=DEV)
    want = (bits.reshape(*c_a.shape[:-1], 196 // cbd, cbd).long() * wb).sum(-1)
    assert torch.equal(c_b.long(), want)


@pytest.mark.parametrize("shapes", [[(512, 512)] * 3, [(224, 224), (300, 500), (512, 512)]], ids=["band", "mixed"])
def test_normalised_patches_bit_exact(pkg, fe, pn, lfq, shapes):
    """The PatchNorm output the fused encode returns (return_patches: on 512^2
    images the column kernel's epilogue with the tables held per block and the
    division's reciprocal hoisted, k_cols512b's NORM form; other sizes the
    generic token epilogue) equals PatchNorm.forward (patchnorm.py:157-165,
    the standalone kernel, __fdiv_rn) of the same raw tokens bit for bit --
    including an image with +inf pixels (non-finite coefficients: the full
    division's path)."""
    xs = rng.synth_images(57, shapes)
    xs[-1] = xs[-1].copy()
    xs[-1][:, 5, 7] = np.inf
    imgs = [torch.from_numpy(a).to(DEV) for a in xs]
    ((dp_r, c_r),) = fe.encode_batch(imgs, pn, lfq, return_raw=True)
    ((dp_n, c_n),) = fe.encode_batch(imgs, pn, lfq, return_patches=True)
    assert torch.equal(dp_r.patch_positions, dp_n.patch_positions)
    assert torch.equal(c_r, c_n)
    ref = pn(dp_r.shallow_copy())
    assert ref.shape == dp_n.patches.shape
    assert torch.equal(ref.view(torch.int32), dp_n.patches.view(torch.int32))


def test_tperm_layout_bit_identical(fe, pn, lfq):
    """Option tperm (GEMM-path T / Y parity-planar, ImgDesc::tperm) changes only
    where the row GEMM's parity problems store their outputs: codes, raw tokens
    and scores equal the interleaved layout's bit for bit (GEMM rows and
    columns, odd / even sides, a side < 32, and an FFT image in between)."""
    ops = _ops()
    xs = [torch.from_numpy(a).to(DEV) for a in rng.synth_images(61, [(333, 517), (512, 512), (29, 700), (448, 449)])]
    outs = []
    for tp in (0, 1):
        ops.set_option("tperm", tp)
        try:
            ((dp, codes),) = fe.encode_batch(xs, pn, lfq, return_raw=True, return_scores=True)
        finally:
            ops.set_option("tperm", 1)
        outs.append((dp, codes))
    (d0, c0), (d1, c1) = outs
    assert torch.equal(c0, c1)
    assert torch.equal(d0.patches.view(torch.int32), d1.patches.view(torch.int32))
    assert torch.equal(d0._data["scores"], d1._data["scores"])


def test_gemm_dma_bit_identical(fe, pn, lfq):
    """Option gemm_dma (the row GEMM k_gemm_h2r streaming its operands into LDS
    by buffer_load ... lds, against the register-staged k_gemm_h2<3, 1>): the
    same fp16 pieces in the same MFMA order, so codes, raw tokens and scores are
    bit-identical (rows past M, k past K, odd / even sides, a side < 32, a side
    with K a multiple of the 32-deep chunk and an FFT image in between)."""
    ops = _ops()
    xs = [torch.from_numpy(a).to(DEV) for a in
          rng.synth_images(62, [(333, 517), (512, 512), (29, 700), (448, 449), (130, 128), (1000, 67)])]
    outs = []
    ops.set_option("rows_fused", 0)   # the separate colour pass + row GEMM
    try:
        for dm in (0, 1):
            ops.set_option("gemm_dma", dm)
            try:
                ((dp, codes),) = fe.encode_batch(xs, pn, lfq, return_raw=True, return_scores=True)
            finally:
                ops.set_option("gemm_dma", 1)
            outs.append((dp, codes))
    finally:
        ops.set_option("rows_fused", 1)
    (d0, c0), (d1, c1) = outs
    assert torch.equal(c0, c1)
    assert torch.equal(d0.patches.view(torch.int32), d1.patches.view(torch.int32))
    assert torch.equal(d0._data["scores"], d1._data["scores"])


def test_rows_fused_fixup_matches_separate_path(fe, pn, lfq):
    """k_rows_fused splits at a fixed scale and flags an image whose folded IPT
    leaves the safe fp16 range (large or non-finite pixels); the fix-up launch
    redoes it at k_gemm_h2's per-image scale, which is the separate path's
    (k_rgb_to_ipt + k_gemm_h2r) arithmetic: codes, raw tokens and scores equal
    option rows_fused=0's bit for bit (GEMM-DCT sides only, so every image takes
    the fused path; odd / even sides, a side < 32)."""
    ops = _ops()
    shapes = [(333, 517), (130, 128), (29, 700), (448, 449)]
    xs = [torch.from_numpy(a).to(DEV) for a in rng.synth_images(63, shapes)]
    xs[0] = xs[0] * 3000.0          # |folded IPT| * 2^11 far above 2^15
    xs[1] = xs[1] * 500.0
    xs[2] = xs[2] * 1.0e6
    xs[3] = xs[3].clone()
    xs[3][1, 17, 301] = float("inf")   # a non-finite pixel
    outs = []
    for fz in (0, 1):
        ops.set_option("rows_fused", fz)
        try:
            ((dp, codes),) = fe.encode_batch(xs, pn, lfq, return_raw=True, return_scores=True)
        finally:
            ops.set_option("rows_fused", 1)
        outs.append((dp, codes))
    (d0, c0), (d1, c1) = outs
    assert torch.equal(c0, c1)
    assert torch.equal(d0.patches.view(torch.int32), d1.patches.view(torch.int32))
    assert torch.equal(d0._data["scores"].view(torch.int32), d1._data["scores"].view(torch.int32))


def test_cols_dma_bit_identical(fe, pn, lfq):
    """Option cols_dma (the column GEMM k_gemm_h2c streaming the matrix and T by
    LDS DMA, T's MFMA fragments read down LDS columns, against the
    register-staged k_gemm_h2<3, 2>): the same fp16 pieces in the same MFMA
    order, so codes, raw tokens and scores are bit-identical (both parities'
    row directions, k past K, columns past N, a side < 32, an FFT-row image
    whose T is folded by k_fold_t)."""
    ops = _ops()
    xs = [torch.from_numpy(a).to(DEV) for a in
          rng.synth_images(64, [(333, 517), (29, 700), (448, 449), (130, 128), (1000, 67), (300, 512)])]
    outs = []
    for cd in (0, 1):
        ops.set_option("cols_dma", cd)
        try:
            ((dp, codes),) = fe.encode_batch(xs, pn, lfq, return_raw=True, return_scores=True)
        finally:
            ops.set_option("cols_dma", 1)
        outs.append((dp, codes))
    (d0, c0), (d1, c1) = outs
    assert torch.equal(c0, c1)
    assert torch.equal(d0.patches.view(torch.int32), d1.patches.view(torch.int32))
    assert torch.equal(d0._data["scores"], d1._data["scores"])


def test_rows_fused_deterministic(fe, pn, lfq):
    """k_rows_fused streams its matrices by inline LDS DMA and takes tiles from
    per-XCD counters in whatever order the blocks reach them: the same batch
    must encode bit-identically call after call (a missing wait state after the
    M0 write once made a few tokens of the config-4 batch differ between calls)."""
    xs = [torch.from_numpy(a).to(DEV) for a in
          rng.synth_images(65, [(1000, 1000), (777, 1013), (333, 517), (1021, 65), (448, 449), (96, 998)])]
    ((d0, c0),) = fe.encode_batch(xs, pn, lfq, return_raw=True)
    for _ in range(4):
        ((d1, c1),) = fe.encode_batch(xs, pn, lfq, return_raw=True)
        assert torch.equal(c0, c1)
        assert torch.equal(d0.patches.view(torch.int32), d1.patches.view(torch.int32))
