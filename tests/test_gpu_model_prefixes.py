"""Progressive decode through the transformer on the GPU
(include/dctae_model_prefix.h, DCTAutoencoder.decode_prefixes,
progressive.model_decode_prefixes).

The contract is exact: a sequence of the variable-length attention equals the
existing kernel at R = 1, S = len on that slice bit for bit, and a model prefix
frame equals the loop of the definition (decode_from_codes on the sliced
one-image row, then postprocess) bit for bit.  The loop is computed once per
module and shared."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import stale_state as ss
from oracle import ref_model as R
from test_model_prefixes_host import GAP, GAP_AFTER, MAX_LEN, PREFIXES, SEQ_LENS, TOKENS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))
U8 = torch.uint8
SIZES = [(14, 14), (28, 42), (70, 98), (140, 140)]
NAN_BF16 = 0x7FC1   # a bf16 NaN pattern (a quiet NaN with a payload), as int16


def _mods():
    from importlib import import_module
    return tuple(import_module("dct_autoencoder_amd." + m) for m in ("_lib", "model", "progressive"))


def _bits(x):
    return x.to(torch.bfloat16).view(torch.int16).contiguous()


def _attention(L, qb, r, s, heads, out):
    """the existing kernel with zero ids and no pad"""
    ctx = L.context(DEV)
    ids = torch.zeros(r, s, dtype=torch.long, device=DEV)
    kp = torch.zeros(r, s, dtype=torch.uint8, device=DEV)
    ctx.check(ctx.lib.dctae_model_attention(ctx.h, r, s, heads, 64, L.ptr(qb), L.ptr(ids), L.ptr(kp), L.ptr(out),
                                            out.stride(0), L.stream_ptr(DEV)), "attention")
    torch.cuda.synchronize()
    return out


# ---- 1, 2. the attention kernel ------------------------------------------------------------------
def test_varlen_attention_against_the_existing_kernel(pkg):
    L, M, _ = _mods()
    heads, d = 2, 128
    starts, pos = [], 0
    for j, n in enumerate(SEQ_LENS):
        starts.append(pos)
        pos += n + (GAP if j == GAP_AFTER - 1 else 0)
    rows = pos
    gap = list(range(starts[GAP_AFTER - 1] + SEQ_LENS[GAP_AFTER - 1], starts[GAP_AFTER]))
    assert len(gap) == GAP and SEQ_LENS[7] == 0
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(rows, 3 * d, generator=g).to(torch.bfloat16).float()
    qb = _bits(qkv).to(DEV)
    out = torch.full((rows, d), NAN_BF16, dtype=torch.int16, device=DEV)
    seqs = M.SeqTable(starts, SEQ_LENS, rows, DEV, max_len=MAX_LEN)
    M.attention_varlen(qb, seqs, heads, out)
    torch.cuda.synchronize()
    got = out.cpu()
    covered = torch.zeros(rows, dtype=torch.bool)
    for s0, n in zip(starts, SEQ_LENS):
        if n == 0:
            continue
        covered[s0:s0 + n] = True
        want = _attention(L, qb[s0:s0 + n].contiguous(), 1, n, heads, torch.empty(n, d, dtype=torch.int16, device=DEV))
        assert torch.equal(got[s0:s0 + n], want.cpu()), f"sequence of length {n} at row {s0}"
        q, k, v = (qkv[s0:s0 + n, i * d:(i + 1) * d].view(n, heads, 64).transpose(0, 1) for i in range(3))
        ref = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v).transpose(0, 1).reshape(n, d)
        err = (got[s0:s0 + n].view(torch.bfloat16).float() - ref).abs().max().item()
        assert err <= 2e-2 * ref.abs().max().item(), (n, err)
    assert not covered[gap].any() and int((~covered).sum()) == GAP
    assert (got[~covered] == NAN_BF16).all(), "rows outside every sequence were written"


def test_varlen_attention_full_length(pkg):
    L, M, _ = _mods()
    r, s, heads, d = 3, 320, 2, 128
    g = torch.Generator().manual_seed(11)
    qb = _bits(torch.randn(r * s, 3 * d, generator=g)).to(DEV)
    want = _attention(L, qb, r, s, heads, torch.empty(r * s, d, dtype=torch.int16, device=DEV))
    out = torch.full((r * s, d), NAN_BF16, dtype=torch.int16, device=DEV)
    M.attention_varlen(qb, M.SeqTable([i * s for i in range(r)], [s] * r, r * s, DEV), heads, out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want.cpu())


# ---- 3. the gather ----------------------------------------------------------------------------------
def _gather_batch():
    """(3, 96): two or three images per row, interior padded slots, trailing padding"""
    g = torch.Generator().manual_seed(3)
    R_, S, ncb = 3, 96, 4
    ids = torch.zeros(R_, S, dtype=torch.long)
    kp = torch.zeros(R_, S, dtype=torch.bool)
    for r, cuts in enumerate([(30, 70, 90), (1, 50, 80), (40, 96, 96)]):
        ids[r, cuts[0]:cuts[1]] = 1
        ids[r, cuts[1]:] = 2 if cuts[1] < cuts[2] else 1
        kp[r, cuts[2]:] = True                                     # trailing padding
        kp[r, torch.randperm(cuts[2], generator=g)[:9]] = True     # interior padded slots
    kp[1, 0] = False                                               # image 0 of row 1: exactly one token
    ids[2, 40:] = 1
    kp[2, 90:] = True
    pos = torch.randint(0, 32, (R_, S, 2), generator=g)
    ch = torch.randint(0, 3, (R_, S), generator=g)
    codes = torch.randint(0, 2 ** 13, (R_, S, ncb), generator=g)
    return ids, kp, pos, ch, codes


@pytest.mark.parametrize("dtype", [torch.int64, torch.int16])
def test_gather(pkg, dtype):
    L, _, P = _mods()
    ids, kp, pos, ch, codes = _gather_batch()
    R_, S, ncb = codes.shape
    n_img = sum(len(set(ids[r].tolist())) for r in range(R_))
    assert n_img == 8
    count = [int(((ids[r] == lid) & ~kp[r]).sum()) for r in range(R_) for lid in sorted(set(ids[r].tolist()))]
    assert min(count) == 1
    per = [sorted({0, 1, max(n - 1, 0), n, n + 5}) for n in count]
    pl = P.model_frames(ids, kp, per)
    fr = [f for f in range(len(pl.m)) if pl.m[f] > 0]
    ms = [pl.m[f] for f in fr]
    starts = [sum(ms[:j]) + 2 * j for j in range(len(ms))]           # two spare rows after every frame
    total = starts[-1] + ms[-1] + 2
    garbage = -0x0123456789ABCDEF
    out_c = torch.full((total, ncb), garbage, dtype=torch.long, device=DEV)
    out_ch = torch.full((total,), garbage, dtype=torch.long, device=DEV)
    out_p = torch.full((total, 2), garbage, dtype=torch.long, device=DEV)
    dev = [t.to(DEV).contiguous() for t in (ids, kp.to(torch.uint8), pos, ch, codes.to(dtype))]
    ctx = L.context(DEV)
    keep = (L.i32([pl.row[f] for f in fr]), L.i64([pl.lid[f] for f in fr]), L.i32(ms), L.i64(starts))
    ctx.check(ctx.lib.dctae_prefix_tokens(
        ctx.h, R_, S, *[L.ptr(t) for t in dev], L.CODES_I16 if dtype == torch.int16 else L.CODES_I64, ncb, len(fr),
        C.cast(keep[0], C.POINTER(C.c_int32)), C.cast(keep[1], C.POINTER(C.c_int64)),
        C.cast(keep[2], C.POINTER(C.c_int32)), C.cast(keep[3], C.POINTER(C.c_int64)), L.ptr(out_c), L.ptr(out_ch),
        L.ptr(out_p), L.stream_ptr(DEV)), "prefix_tokens")
    torch.cuda.synchronize()
    # the numpy mirror
    want_c = np.full((total, ncb), garbage, dtype=np.int64)
    want_ch = np.full((total,), garbage, dtype=np.int64)
    want_p = np.full((total, 2), garbage, dtype=np.int64)
    idn, kpn = ids.numpy(), kp.numpy()
    for f, s0, m in zip(fr, starts, ms):
        r = pl.row[f]
        slots = np.nonzero((idn[r] == pl.lid[f]) & ~kpn[r])[0][:m]
        assert len(slots) == m
        want_c[s0:s0 + m] = codes.numpy()[r, slots]
        want_ch[s0:s0 + m] = ch.numpy()[r, slots]
        want_p[s0:s0 + m] = pos.numpy()[r, slots]
    assert np.array_equal(out_c.cpu().numpy(), want_c)
    assert np.array_equal(out_ch.cpu().numpy(), want_ch)
    assert np.array_equal(out_p.cpu().numpy(), want_p)
    written = np.zeros(total, dtype=bool)
    for s0, m in zip(starts, ms):
        written[s0:s0 + m] = True
    assert (want_ch[written] != garbage).all() and (out_ch.cpu().numpy()[~written] == garbage).all()


# ---- 4 .. 8. the model ----------------------------------------------------------------------------
class Setup:
    pass


@pytest.fixture(scope="module")
def su(pkg):
    d = np.load(os.path.join(HERE, "golden", "model_ref.npz"))
    w = {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w.")}
    hid, heads, inter, layers, ncb, cbs, _ = [int(v) for v in d["cfg"]]
    enc = dict(hidden_size=hid, intermediate_size=inter, num_attention_heads=heads, num_hidden_layers=layers)
    cfg = pkg.DCTAutoencoderConfig(image_channels=3, patch_size=14, max_patch_h=32, max_patch_w=32,
                                   vq_codebook_size=cbs, vq_num_codebooks=ncb, vq_type="lfq", encoder_config=enc,
                                   decoder_config=enc)
    m = pkg.DCTAutoencoder(cfg)
    m.load_state_dict(w, strict=False)
    med, b = ss.tables(5, 32, 32, 14)       # a non-trivial PatchNorm state
    with torch.no_grad():
        m.patchnorm.median.copy_(med)
        m.patchnorm.b.copy_(b)
    m.patchnorm.frozen = True
    m = m.to(DEV).eval()
    s = Setup()
    s.model, s.w, s.c = m, w, dict(heads=heads, layers=layers, ncb=ncb, cbd=int(np.log2(cbs)))
    s.fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 320)
    s.dp, s.codes = _encode(s, ss.images(21, SIZES))
    kp, ids = s.dp.key_pad_mask.cpu(), s.dp.batched_image_ids.cpu()
    s.places = [(r, i) for r in range(ids.shape[0]) for i in sorted(set(ids[r].tolist()))]
    s.n = [int(((ids[r] == i) & ~kp[r]).sum()) for r, i in s.places]
    assert sorted(s.n) == TOKENS
    assert any(sum(1 for rr, _ in s.places if rr == r) >= 2 and bool(kp[r].any()) for r in range(ids.shape[0]))
    s.loop = _loop(s, s.dp, s.codes, PREFIXES)
    return s


def _encode(s, imgs):
    ((dp, _),) = s.fe.encode_batch(imgs, s.model.patchnorm, return_patches=True)
    meta = dp.shallow_copy()
    _, codes, _, _ = s.model.encode(dp.shallow_copy())
    torch.cuda.synchronize()
    return meta, codes


def _row(dp, codes, r, lid, m):
    """the first m real tokens of image (r, lid) as a one-row batch without padding"""
    sel = ((dp.batched_image_ids[r] == lid) & ~dp.key_pad_mask[r]).nonzero().flatten()[:m]
    assert sel.numel() == m
    kw = dict(key_pad_mask=torch.zeros(1, m, dtype=torch.bool, device=DEV),
              batched_image_ids=torch.zeros(1, m, dtype=torch.long, device=DEV),
              patch_channels=dp.patch_channels[r, sel][None].contiguous(),
              patch_positions=dp.patch_positions[r, sel][None].contiguous())
    return codes[r, sel][None].long().contiguous(), kw


def _loop(s, dp, codes, prefixes, images=None):
    """the definition: {(image, k): (patches, fp32 frame, uint8 frame)} for m >= 1, by the sliced calls"""
    ids, kp = dp.batched_image_ids.cpu(), dp.key_pad_mask.cpu()
    places = [(r, i) for r in range(ids.shape[0]) for i in sorted(set(ids[r].tolist()))]
    out = {}
    for i, (r, lid) in enumerate(places):
        if images is not None and i not in images:
            continue
        n = int(((ids[r] == lid) & ~kp[r]).sum())
        for k in prefixes:
            m = min(k, n)
            if m == 0 or (i, m) in out:
                continue
            crow, kw = _row(dp, codes, r, lid, m)
            x = s.model.decode_from_codes(crow, do_inv_norm=True, patch_sizes=[dp.patch_sizes[i]],
                                          original_sizes=[dp.original_sizes[i]], **kw)
            out[(i, m)] = (x.patches[0].clone(), s.fe.postprocess(x)[0], s.fe.postprocess(x, U8)[0])
    torch.cuda.synchronize()
    return out


def _same(a, b, what):
    ss.assert_same_bits(ss.flat(a), ss.flat(b), what)


def test_model_frames_equal_the_loop(pkg, su):
    s = su
    f32 = s.fe.model_decode_prefixes(s.model, s.dp, s.codes, PREFIXES)
    u8 = s.fe.model_decode_prefixes(s.model, s.dp, s.codes, PREFIXES, output_dtype=U8)
    clipped = s.fe.model_decode_prefixes(s.model, s.dp, s.codes, PREFIXES, clip="minmax")
    zero = s.fe.postprocess_prefixes(s.dp, [0])
    assert len(f32) == len(s.n) == 4
    for i, n in enumerate(s.n):
        assert len(f32[i]) == len(u8[i]) == len(PREFIXES)
        for j, k in enumerate(PREFIXES):
            m = min(k, n)
            want32, want8 = (zero[i][0], None) if m == 0 else s.loop[(i, m)][1:]
            _same(f32[i][j], want32, f"image {i} prefix {k} fp32")
            if m:
                _same(u8[i][j], want8, f"image {i} prefix {k} uint8")
                (cl,) = s.fe.image_clip([want32])
                _same(clipped[i][j], cl, f"image {i} prefix {k} clipped")
            assert f32[i][j].shape == (3,) + tuple(s.dp.original_sizes[i]) and u8[i][j].dtype == U8
    # the frames batch itself
    frames, which = s.model.decode_prefixes(s.dp, s.codes, PREFIXES)
    assert which == [(i, k) for i, n in enumerate(s.n) for k in PREFIXES if min(k, n) > 0]
    assert frames.key_pad_mask.shape[0] == 1 and not frames.key_pad_mask.any()
    ids = frames.batched_image_ids[0].cpu()
    for f, (i, k) in enumerate(which):
        got = frames.patches[0][ids == f]
        _same(got, s.loop[(i, min(k, s.n[i]))][0], f"frames batch, image {i} prefix {k}")
        assert frames.patch_sizes[f] == s.dp.patch_sizes[i] and frames.original_sizes[f] == s.dp.original_sizes[i]


def test_int16_codes_give_the_same_bits(pkg, su):
    s = su
    a = s.fe.model_decode_prefixes(s.model, s.dp, s.codes, PREFIXES)
    b = s.fe.model_decode_prefixes(s.model, s.dp, s.codes.to(torch.int16), PREFIXES)
    _same(a, b, "int16 codes")


def test_chunks_do_not_change_a_frame(pkg, su, monkeypatch):
    s = su
    _, _, P = _mods()
    a, _ = s.model.decode_prefixes(s.dp, s.codes, PREFIXES)
    monkeypatch.setattr(P, "PREFIX_TOKENS_PER_CALL", 200)
    b, which = s.model.decode_prefixes(s.dp, s.codes, PREFIXES)
    assert b.key_pad_mask.shape[0] > 3 and bool(b.key_pad_mask.any())
    assert b.patch_sizes == a.patch_sizes and b.original_sizes == a.original_sizes
    flat_a = a.patches[~a.key_pad_mask]
    flat_b = b.patches[~b.key_pad_mask]
    _same(flat_b, flat_a, "patches of the frames, budget 200 against the default")
    imgs = s.fe.model_decode_prefixes(s.model, s.dp, s.codes, PREFIXES, output_dtype=U8)
    for i, n in enumerate(s.n):
        for j, k in enumerate(PREFIXES):
            if min(k, n):
                _same(imgs[i][j], s.loop[(i, min(k, n))][2], f"image {i} prefix {k}, budget 200")


def test_nothing_stale(pkg, su):
    s = su
    L = _mods()[0]

    def run():
        return ss.flat([s.fe.model_decode_prefixes(s.model, s.dp, s.codes, [0, 3, 65, 10 ** 6]),
                        s.fe.model_decode_prefixes(s.model, s.dp, s.codes, [2, 257], U8, "minmax")])
    with ss._context(L) as ctx:
        plain = run()
        torch.cuda.synchronize()
        junk = torch.empty(256 << 20, dtype=torch.uint8, device=DEV).fill_(0xFF)   # the allocator's free blocks
        del junk
        ss._set(ctx, "ws_poison", 1)
        ss.assert_same_bits(run(), plain, "second call, free blocks and scratch overwritten")
        ss._set(ctx, "ws_poison", 0)


def test_neighbours_do_not_matter(pkg, su):
    """the frames of an image do not change when the other images of its row are replaced: other codes and
    places for its neighbours, and the row's padding turned into the tokens of one more image"""
    s = su
    i = s.n.index(18)
    r, lid = s.places[i]
    assert sum(1 for rr, _ in s.places if rr == r) >= 2 and bool(s.dp.key_pad_mask[r].any())
    g = torch.Generator().manual_seed(17)
    ids, kp = s.dp.batched_image_ids.clone(), s.dp.key_pad_mask.clone()
    others = (ids[r] != lid).cpu()
    codes2, dp2 = s.codes.clone(), s.dp.shallow_copy()
    codes2[r, others] = torch.randint(0, 2 ** s.c["cbd"], (int(others.sum()), s.c["ncb"]), generator=g).to(DEV)
    dp2.patch_positions = s.dp.patch_positions.clone()
    dp2.patch_positions[r, others] = torch.randint(0, 5, (int(others.sum()), 2), generator=g).to(DEV)
    new_id = int(ids[r].max()) + 1
    ids[r, kp[r]] = new_id
    kp[r] = False
    dp2.batched_image_ids, dp2.key_pad_mask = ids, kp
    # the new image is the last of its row: sizes for it, the images after it move up by one
    at = max(j for j, (rr, _) in enumerate(s.places) if rr == r) + 1
    dp2.patch_sizes = s.dp.patch_sizes[:at] + [(5, 5)] + s.dp.patch_sizes[at:]
    dp2.original_sizes = s.dp.original_sizes[:at] + [(70, 70)] + s.dp.original_sizes[at:]
    per = [[1, 3, 18, 99] if j == i else [] for j in range(len(s.places) + 1)]
    assert i < at
    got = s.fe.model_decode_prefixes(s.model, dp2, codes2, per)[i]
    for k, im in zip([1, 3, 18, 18], got):
        _same(im, s.loop[(i, k)][1], f"prefix {k} with other neighbours")


def test_reference_semantics(pkg, su):
    """the frames' normalised patches against the fp32 oracle on the sliced one-image row, within the
    project's bound for these kernels (test_model_decode_from_reference_codes: 3e-2 of max|ref|)"""
    s = su
    i = s.n.index(105)
    r, lid = s.places[i]
    ks = [1, 3, 64, 105]
    frames, which = s.model.decode_prefixes(s.dp, s.codes, [ks if j == i else [] for j in range(len(s.n))],
                                            do_inv_norm=False)
    torch.cuda.synchronize()
    assert which == [(i, k) for k in ks]
    ids = frames.batched_image_ids[0].cpu()
    for f, k in enumerate(ks):
        crow, kw = _row(s.dp, s.codes, r, lid, k)
        q = R.codes_to_features(s.w, crow.cpu(), s.c["ncb"], s.c["cbd"])
        ref = R.decode(s.w, q, kw["batched_image_ids"].cpu(), kw["key_pad_mask"].cpu(), kw["patch_channels"].cpu(),
                       kw["patch_positions"].cpu(), s.c["heads"], s.c["layers"])[0]
        got = frames.patches[0][ids == f].cpu()
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        print(f"prefix {k}: max rel err {err:.4g}")
        assert err <= 3e-2, (k, err)


# ---- 9. refusals ---------------------------------------------------------------------------------------
def test_refusals(pkg, su):
    s = su
    _, M, _ = _mods()
    with pytest.raises(ValueError, match=">= 0"):
        s.fe.model_decode_prefixes(s.model, s.dp, s.codes, [1, -1])
    with pytest.raises(ValueError, match="per-image"):
        s.fe.model_decode_prefixes(s.model, s.dp, s.codes, [[1], [2]])
    with pytest.raises(TypeError, match="int64 or torch.int16"):
        s.fe.model_decode_prefixes(s.model, s.dp, s.codes.int(), [1])
    with pytest.raises(RuntimeError, match="is on"):
        s.fe.model_decode_prefixes(s.model, s.dp, s.codes.cpu(), [1])
    with pytest.raises(ValueError, match="clip"):
        s.fe.model_decode_prefixes(s.model, s.dp, s.codes, [1], clip="max")
    with pytest.raises(TypeError, match="float32 or torch.uint8"):
        s.fe.model_decode_prefixes(s.model, s.dp, s.codes, [1], output_dtype=torch.float16)
    with pytest.raises(ValueError, match="max_len"):
        M.SeqTable([0, 10], [10, 20], 30, DEV, max_len=19)
    s.model.train()
    try:
        with pytest.raises(NotImplementedError):
            s.fe.model_decode_prefixes(s.model, s.dp, s.codes, [1])
    finally:
        s.model.eval()
