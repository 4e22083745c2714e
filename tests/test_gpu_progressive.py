"""Progressive decode (include/dctae_frames.h, dct_autoencoder_amd.progressive):
the token-prefix frames of a packed batch in one launch sequence, image_clip.

The rule under test: frame (i, k) is, bit for bit, image i of today's
``postprocess`` / ``decode_batch`` on the batch whose ``key_pad_mask`` is
additionally set on every token of image i except its first min(k, n_i) real
tokens.  The yardstick throughout is that call on a masked batch built HERE by
a brute-force count (``masked_key_pad``; the package's ``frame_cuts`` is not
used to build it).  One masked call realises "the j-th prefix of every image",
so the yardstick costs one call per prefix position.  Comparisons are on the
raw bits (``same_bits``); nothing is a tolerance, except the two constants of
test_duplicate_place, which are computed on the CPU.

Cases are those of oracle/decode_cases.py (the perturbed model output as the
patches).  Codes at P = 14 are the sign bits of the patches under the recorded
PatchNorm tables (the ``ref_tables`` fixture), LFQ 14 x 14 as recommended.
"""
import ctypes as C
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import stale_state as ss
from oracle import decode_cases as D
from oracle import ref_cpu
from test_options_host import EINVAL
from test_progressive_host import clip_mirror

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8, F32, I16 = torch.uint8, torch.float32, torch.int16
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _package(pkg):
    return pkg


def _prog():
    return import_module("dct_autoencoder_amd.progressive")


def _ops():
    return import_module("dct_autoencoder_amd._ops")


def _lib():
    return import_module("dct_autoencoder_amd._lib")


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(ss.bits(a), ss.bits(b))


# ---- inputs ---------------------------------------------------------------------------
def make_fe(pkg, cfg, cls=None):
    return (cls or pkg.DCTAutoencoderFeatureExtractor)(3, cfg.patch_size, 0.0, cfg.max_patch_h, cfg.max_patch_w,
                                                       cfg.max_seq_len)


def sizes_of(batch):
    return ([tuple(int(v) for v in s) for s in batch.patch_sizes],
            [tuple(int(v) for v in s) for s in batch.original_sizes])


def dct_patches(pkg, batch, patches, key_pad=None):
    ps, os_ = sizes_of(batch)
    return pkg.DCTPatches(patches=patches.to(DEV), key_pad_mask=(batch.key_pad_mask if key_pad is None else key_pad).to(DEV),
                          batched_image_ids=batch.batched_image_ids.to(DEV),
                          patch_channels=batch.patch_channels.to(DEV), patch_positions=batch.patch_positions.to(DEV),
                          patch_sizes=ps, original_sizes=os_)


def token_counts(img):
    return [int((img == i).sum()) for i in range(int(img.max()) + 1)]


def masked_key_pad(batch, img, ks):
    """key_pad with every token of image i padded except its first min(ks[i], n_i) real tokens, by counting"""
    kp = batch.key_pad_mask.clone()
    R, S = kp.shape
    seen = [0] * len(ks)
    for r in range(R):
        row = img[r].tolist()
        for j in range(S):
            i = row[j]
            if i < 0:
                continue
            if seen[i] >= ks[i]:
                kp[r, j] = True
            seen[i] += 1
    return kp


def standard_prefixes(n):
    return [0, 1, 2, n // 2, n - 1, n, n + 5]


def check_frames(batch, img, per, got, yard):
    """got[i][j] against image i of yard(masked key_pad of position j): per[i] are image i's prefixes"""
    assert len(got) == len(per) and all(len(g) == len(p) for g, p in zip(got, per))
    for j in range(len(per[0])):
        want = yard(masked_key_pad(batch, img, [p[j] for p in per]))
        torch.cuda.synchronize()
        assert len(want) == len(got)
        for i, w in enumerate(want):
            assert same_bits(got[i][j], w), f"image {i}, prefix {per[i][j]} (position {j})"


@functools.lru_cache(maxsize=None)
def codes_of(name):
    """int64 codes (R, S, 14) of the case's patches under the recorded tables: the sign bits, code bit d of
    codebook c = element 14 c + d (lfq.py:105-134)"""
    from conftest import golden
    c = D.build(name)
    t = golden("patchnorm_ref.npz")
    med, b = torch.from_numpy(t["median"]), torch.from_numpy(t["b"])
    ch, pos = c.batch.patch_channels, c.batch.patch_positions
    std = b[ch, pos[..., 0], pos[..., 1]] * 2 ** 0.5 + 1e-6
    bits = ((c.out - med[ch, pos[..., 0], pos[..., 1]]) / std > 0).long()
    R, S, _ = bits.shape
    w = 2 ** torch.arange(13, -1, -1)
    return (bits.view(R, S, 14, 14) * w).sum(-1).contiguous()


@pytest.fixture(scope="module")
def pn(pkg, ref_tables):
    return ss.patchnorm(pkg, ref_tables.median, ref_tables.b)


@pytest.fixture(scope="module")
def lfq(pkg):
    return pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).to(DEV).eval()


# ---- 1, 2, 4. from patches, GEMM path -----------------------------------------------------
def _patch_case(pkg, name, per_of_n, dtype, grad=False):
    c = D.build(name)
    fe = make_fe(pkg, c.cfg)
    per = [per_of_n(n) for n in token_counts(c.img)]
    x = dct_patches(pkg, c.batch, c.out)
    if grad:   # patches that require grad take the no-grad path: the same frames, no grad_fn
        x.patches.requires_grad_()
    got = fe.postprocess_prefixes(x, per, output_dtype=dtype)
    check_frames(c.batch, c.img, per, got,
                 lambda kp: fe.postprocess(dct_patches(pkg, c.batch, c.out, kp), output_dtype=dtype))
    _ops().check_device_errors(torch.device(DEV, torch.cuda.current_device()))
    return got


@pytest.mark.parametrize("dtype", [F32, U8], ids=["f32", "u8"])
@pytest.mark.parametrize("name", ["mid", "holes"])
def test_patches_gemm_path(pkg, name, dtype):
    got = _patch_case(pkg, name, standard_prefixes, dtype, grad=name == "mid")
    assert all(f.dtype == dtype and f.grad_fn is None and not f.requires_grad for g in got for f in g)


@pytest.mark.parametrize("dtype", [F32, U8], ids=["f32", "u8"])
@pytest.mark.parametrize("name", ["caps", "p5", "mixed512"])
def test_patches_other_geometries(pkg, name, dtype):
    _patch_case(pkg, name, lambda n: [1, n // 3, n], dtype)


def test_many_images_shared_prefixes(pkg):
    c = D.build("many300")
    fe = make_fe(pkg, c.cfg)
    n_img = len(c.batch.original_sizes)
    assert n_img > 256
    got = fe.postprocess_prefixes(dct_patches(pkg, c.batch, c.out), [1, 3])
    assert sum(len(g) for g in got) == 2 * n_img
    check_frames(c.batch, c.img, [[1, 3]] * n_img, got,
                 lambda kp: fe.postprocess(dct_patches(pkg, c.batch, c.out, kp)))


# ---- 3. the FFT path ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, U8], ids=["f32", "u8"])
@pytest.mark.parametrize("src", ["patches", "codes64", "codes16"])
def test_fft_path(pkg, pn, lfq, src, dtype):
    c = D.build("sq512x2")
    fe = make_fe(pkg, c.cfg)
    ks = [0, 1, 17, 3071, 3072]
    assert token_counts(c.img) == [3072, 3072]
    ctx = ss.timed(_lib().context(torch.device(DEV, torch.cuda.current_device())))
    try:
        ss._stages(ctx)
        if src == "patches":
            got = fe.postprocess_prefixes(dct_patches(pkg, c.batch, c.out), ks, output_dtype=dtype)
            yard = lambda kp: fe.postprocess(dct_patches(pkg, c.batch, c.out, kp), output_dtype=dtype)  # noqa: E731
        else:
            codes = codes_of("sq512x2").to(DEV)
            codes = codes.to(I16) if src == "codes16" else codes
            got = fe.decode_prefixes(dct_patches(pkg, c.batch, c.out), codes, pn, lfq, ks, output_dtype=dtype)
            yard = lambda kp: fe.decode_batch(dct_patches(pkg, c.batch, c.out, kp), codes, pn, lfq,  # noqa: E731
                                              output_dtype=dtype)
        torch.cuda.synchronize()
        st = ss._stages(ctx)
        # the FFT path: no token scatter, no colour kernel of the GEMM path
        assert st.get("dec_map") == 1 and st.get("idct_cols") == 1 and st.get("idct_rows") == 1, st
        assert not st.get("scatter_tokens") and not st.get("ipt_to_rgb"), st
    finally:
        ctx.check(ctx.lib.dctae_timing_reset(ctx.h))
        ctx.check(ctx.lib.dctae_set_timing(ctx.h, 0))
    check_frames(c.batch, c.img, [ks, ks], got, yard)


# ---- 5. two tokens at one place -------------------------------------------------------------
def test_duplicate_place(pkg):
    """one 28 x 28 image, row slots: 0 (c 0, 0, 0) DC = 14.0 | 1 padded | 2 (c 0, 1, 1) all zero |
    3 (c 0, 0, 0) again, DC = 22.4 | padded.  The image is constant: I = DC / 28, P = T = 0."""
    cfg = ref_cpu.FEConfig(patch_size=14, max_patch_h=4, max_patch_w=4, max_seq_len=8)
    fe = make_fe(pkg, cfg)
    kp = torch.tensor([[False, True, False, False, True, True, True, True]])
    pos = torch.zeros(1, 8, 2, dtype=torch.long)
    pos[0, 2] = torch.tensor([1, 1])
    patches = torch.zeros(1, 8, 196)
    patches[0, 0, 0], patches[0, 3, 0] = 14.0, 22.4
    batch = ref_cpu.Batch(patches=patches, key_pad_mask=kp, attn_mask=None,
                          batched_image_ids=torch.zeros(1, 8, dtype=torch.long),
                          patch_channels=torch.zeros(1, 8, dtype=torch.long), patch_positions=pos,
                          patch_sizes=[(2, 2)], original_sizes=[(28, 28)])
    img = D.token_image(batch.batched_image_ids, kp)
    ks = [0, 1, 2, 3, 9]
    got = fe.postprocess_prefixes(dct_patches(pkg, batch, patches), ks)
    check_frames(batch, img, [ks], got, lambda m: fe.postprocess(dct_patches(pkg, batch, patches, m)))

    def grey(dc):
        return D.ipt_to_rgb(torch.tensor([dc / 28.0, 0.0, 0.0]).view(3, 1, 1)).expand(3, 28, 28)
    # cut before both: nothing; between them: the earlier token shows; past both: the later slot wins
    for k, f in zip(ks, got[0]):
        want = torch.zeros(3, 28, 28) if k == 0 else grey(14.0 if k < 3 else 22.4)
        # 1e-4: the colour matrices' fp32 inverse differs in its last bits from host to host, powf from pow
        assert torch.allclose(f.cpu(), want, rtol=1e-4, atol=1e-6), (k, f.flatten()[:3], want.flatten()[:3])
    assert float((grey(22.4) - grey(14.0)).abs().min()) > 0.1


# ---- 6. projections: the PatchNorm-space branch -----------------------------------------------
def test_decode_prefixes_with_projections(pkg, pn):
    c = D.build("mid")
    fe = make_fe(pkg, c.cfg)
    torch.manual_seed(5)
    lq = pkg.LFQ(dim=196, codebook_size=2 ** 13, num_codebooks=16).to(DEV).eval()
    assert lq.has_projections and lq._fused_proj()
    R, S = c.batch.key_pad_mask.shape
    codes = torch.randint(0, 2 ** 13, (R, S, 16), generator=torch.Generator().manual_seed(9)).to(DEV)
    per = [[1, n // 2, n] for n in token_counts(c.img)]
    for dtype in (F32, U8):
        got = fe.decode_prefixes(dct_patches(pkg, c.batch, c.out), codes, pn, lq, per, output_dtype=dtype)
        check_frames(c.batch, c.img, per, got,
                     lambda kp: fe.decode_batch(dct_patches(pkg, c.batch, c.out, kp), codes, pn, lq, output_dtype=dtype))


# ---- 7. chunking ------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_chunks(pkg, monkeypatch):
    c = D.build("mid")
    fe = make_fe(pkg, c.cfg)
    prog = _prog()
    per = [[1, n // 2, n] for n in token_counts(c.img)]
    dp = dct_patches(pkg, c.batch, c.out)
    want = ss.flat(fe.postprocess_prefixes(dp, per, clip="minmax", output_dtype=U8)
                   + fe.postprocess_prefixes(dp, per))
    ps, os_ = sizes_of(c.batch)
    costs = [prog._frame_scratch_bytes(fe.params(), hw, phw, True) for hw, phw in zip(os_, ps) for _ in range(3)]
    assert len(costs) == 9 and len(prog._chunks(costs, prog.FRAME_SCRATCH_BYTES)) == 1
    # one frame per chunk; the first image's frames one by one, the rest in two runs
    for budget, n_chunks in ((1, 9), (max(costs), 5)):
        assert len(prog._chunks(costs, budget)) == n_chunks
        monkeypatch.setattr(prog, "FRAME_SCRATCH_BYTES", budget)
        got = ss.flat(fe.postprocess_prefixes(dp, per, clip="minmax", output_dtype=U8)
                      + fe.postprocess_prefixes(dp, per))
        ss.assert_same_bits(got, want, f"budget {budget}")


# ---- 8. the scalar map path --------------------------------------------------------------------
def _misaligned(t):
    """a contiguous view of t's values one element into a fresh buffer"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    return v


def test_views_off_16_bytes(pkg, pn, lfq):
    for name in ("mid", "sq512x2"):
        c = D.build(name)
        fe = make_fe(pkg, c.cfg)
        per = [[1, n // 2, n] for n in token_counts(c.img)]
        dp = dct_patches(pkg, c.batch, c.out)
        want = ss.flat(fe.postprocess_prefixes(dp, per))
        dq = dp.shallow_copy()
        dq.batched_image_ids, dq.patch_channels = _misaligned(dp.batched_image_ids), _misaligned(dp.patch_channels)
        dq.patch_positions, dq.key_pad_mask = _misaligned(dp.patch_positions), _misaligned(dp.key_pad_mask)
        assert dq.batched_image_ids.data_ptr() % 16 == 8 and dq.key_pad_mask.data_ptr() % 4 == 1
        assert dq.batched_image_ids.is_contiguous() and dq.patch_positions.is_contiguous()
        ss.assert_same_bits(ss.flat(fe.postprocess_prefixes(dq, per)), want, name)


# ---- 9. stale scratch ----------------------------------------------------------------------------
def test_poisoned_scratch_and_a_large_call_before(pkg, pn, lfq):
    lib = ss.mods()[0]
    small, large = D.build("mid"), D.build("sq512x2")
    fe_s, fe_l = make_fe(pkg, small.cfg), make_fe(pkg, large.cfg)
    per = [[1, n // 2, n] for n in token_counts(small.img)]
    codes = codes_of("sq512x2").to(DEV)

    def run():
        dp = dct_patches(pkg, small.batch, small.out)
        return ss.flat([fe_s.postprocess_prefixes(dp, per), fe_s.postprocess_prefixes(dp, per, U8, "minmax")])

    def run_large():
        dl = dct_patches(pkg, large.batch, large.out)
        return ss.flat([fe_l.decode_prefixes(dl, codes, pn, lfq, [5, 3072], clip="minmax"),
                        fe_l.postprocess_prefixes(dl, [7, 100], U8, "minmax")])
    with ss._context(lib) as ctx:
        plain = run()
        big_plain = run_large()
        ss._set(ctx, "ws_poison", 1)
        ss.assert_same_bits(run(), plain, "small call, poisoned scratch")
        ss.assert_same_bits(run_large(), big_plain, "large call, poisoned scratch")
        ss.assert_same_bits(run(), plain, "small call after a large one, poisoned scratch")
        ss._set(ctx, "ws_poison", 0)
        run_large()
        ss.assert_same_bits(run(), plain, "small call after a large one, stale scratch")


# ---- the C ABI directly ----------------------------------------------------------------------------
class Raw:
    """dctae_decode_frames through ctypes on a case's batch, from patches"""

    def __init__(self, pkg, name):
        lib, ops = _lib(), _ops()
        c = D.build(name)
        self.c, self.fe = c, make_fe(pkg, c.cfg)
        ps, os_ = sizes_of(c.batch)
        self.p = self.fe.params(c.batch.key_pad_mask.shape[1])
        b = c.batch
        self.table = ops.DecodeTable(self.p, b.batched_image_ids.to(DEV), b.key_pad_mask.to(DEV),
                                     b.patch_positions.to(DEV), b.patch_channels.to(DEV), ps, os_)
        self.patches = c.out.to(DEV).contiguous()
        self.dev = torch.device(DEV, torch.cuda.current_device())
        self.ctx = lib.context(self.dev)
        self.numel = [3 * h * w for h, w in os_]

    def call(self, img, cut, offs, out, px, clip=0, n_frames=None, null=(), cfg=None, patch_hw=None, stream=None):
        lib, t = _lib(), self.table
        keep = (lib.i32(img), lib.i32(cut), lib.i64(offs))
        arr = [C.cast(keep[0], C.POINTER(C.c_int32)), C.cast(keep[1], C.POINTER(C.c_int32)),
               C.cast(keep[2], C.POINTER(C.c_int64))]
        for k in null:
            arr[k] = None
        fr = lib.Frames(len(img) if n_frames is None else n_frames, *arr)
        lut, lut_w, n_img, out_hw, _, phw = t.c_args()
        cfg = cfg if cfg is not None else self.p.c(t.S)
        if patch_hw is not None:
            keep += (lib.i32(patch_hw),)
            phw = C.cast(keep[-1], C.POINTER(C.c_int32))
        return self.ctx.lib.dctae_decode_frames(
            self.ctx.h, C.byref(cfg), t.R, lut, lut_w, n_img, out_hw, phw, lib.ptr(t.ids), lib.ptr(t.key_pad),
            lib.ptr(t.pos), lib.ptr(t.ch), C.byref(fr), None, None, None, 0, lib.ptr(self.patches), 0, clip,
            lib.ptr(out), px, stream if stream is not None else lib.stream_ptr(self.dev))

    def error(self):
        return self.ctx.lib.dctae_last_error(self.ctx.h).decode()


def _filled(n, dtype):
    out = torch.empty(n, dtype=dtype, device=DEV)
    if dtype == U8:
        out.fill_(0xAB)
    else:
        out.fill_(float("nan"))
    return out


# ---- 10. the output is written exactly ---------------------------------------------------------------
@pytest.mark.parametrize("clip", [0, 1], ids=["plain", "minmax"])
@pytest.mark.parametrize("dtype", [F32, U8], ids=["f32", "u8"])
@pytest.mark.parametrize("name", ["mid", "sq512x2"])
def test_output_written_exactly(pkg, name, dtype, clip):
    raw = Raw(pkg, name)
    n = token_counts(raw.c.img)
    per = [[2, k // 2, k] for k in n]
    img, cut = _prog().frame_cuts(raw.c.batch.batched_image_ids, raw.c.batch.key_pad_mask, per)
    offs, total = [], GUARD
    for i in img:
        offs.append(total)
        total += raw.numel[i] + GUARD + (-raw.numel[i]) % 4   # guards of at least GUARD elements, 4-byte aligned starts
    out = _filled(total, dtype)
    rc = raw.call(img, cut, offs, out, 1 if dtype == U8 else 0, clip=clip)
    assert rc == 0, raw.error()
    want = raw.fe.postprocess_prefixes(dct_patches(pkg, raw.c.batch, raw.c.out), per, output_dtype=dtype,
                                       clip="minmax" if clip else None)
    want = [f for fs in want for f in fs]
    torch.cuda.synchronize()
    o = out.cpu()
    inside = torch.zeros(total, dtype=torch.bool)
    for f, (i, off) in enumerate(zip(img, offs)):
        got = o[off: off + raw.numel[i]]
        inside[off: off + raw.numel[i]] = True
        assert same_bits(got.view(want[f].shape), want[f].cpu()), f"frame {f}"
        if not clip and dtype == F32:
            assert not torch.isnan(got).any(), f"frame {f}: an element was not written"
    rest = o[~inside]
    assert (rest == 0xAB).all() if dtype == U8 else torch.isnan(rest).all(), "a guard zone was written"
    if dtype == U8:   # every byte inside was written: a second call on another fill gives the same bytes
        out2 = torch.full((total,), 0x54, dtype=U8, device=DEV)
        assert raw.call(img, cut, offs, out2, 1, clip=clip) == 0
        assert torch.equal(out2.cpu()[inside], o[inside])


# ---- 11. a side stream ---------------------------------------------------------------------------------
def test_side_stream(pkg):
    c = D.build("mid")
    fe = make_fe(pkg, c.cfg)
    per = [[1, n // 2, n] for n in token_counts(c.img)]
    dp = dct_patches(pkg, c.batch, c.out)
    want_f, want_i = ss.flat(fe.postprocess_prefixes(dp, per, clip="minmax")), ss.flat(fe.postprocess(dp))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got_f = fe.postprocess_prefixes(dp, per, clip="minmax")
        got_i = fe.postprocess(dp)          # takes the same scratch, on the same stream
        got_f2 = fe.postprocess_prefixes(dp, per, clip="minmax")
    s.synchronize()
    ss.assert_same_bits(ss.flat(got_f), want_f, "frames on a side stream")
    ss.assert_same_bits(ss.flat(got_i), want_i, "the decode after them")
    ss.assert_same_bits(ss.flat(got_f2), want_f, "frames after the decode")


# ---- 12. image_clip ---------------------------------------------------------------------------------------
def _clip_inputs():
    g = np.random.default_rng(12)
    shapes = [(3, 1, 1), (3, 14, 14), (3, 127, 257), (3, 520, 600)]
    return [(g.standard_normal(s) * 1.5 + 0.4).astype(np.float32) for s in shapes]


def test_image_clip_against_the_mirror(pkg):
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
    xs = _clip_inputs()
    assert all(x.min() < 0 and x.max() > 1 for x in xs[1:])
    g = np.random.default_rng(13)
    small = [(g.standard_normal((3, 1 + i % 7, 1 + i % 5)) * 2).astype(np.float32) for i in range(300)]
    for xs_ in (xs, small):
        dev = [torch.from_numpy(x).to(DEV) for x in xs_]
        got = fe.image_clip(dev)
        got8 = fe.image_clip(dev, output_dtype=U8)
        torch.cuda.synchronize()
        for x, y, b in zip(xs_, got, got8):
            want = clip_mirror(x)
            assert y.dtype == F32 and b.dtype == U8 and y.shape == x.shape == b.shape
            assert np.array_equal(y.cpu().numpy(), want, equal_nan=True), x.shape
            assert torch.equal(b, _ops().f32_to_u8(y)), x.shape
    # an image that starts 4 bytes off a 16-byte boundary (the kernels' scalar path), beside an aligned one
    buf = torch.empty(xs[2].size + 1, device=DEV)
    off = buf[1:].view(xs[2].shape).copy_(torch.from_numpy(xs[2]))
    assert off.data_ptr() % 16 == 4
    for dtype in (F32, U8):
        a, b = fe.image_clip([off, torch.from_numpy(xs[1]).to(DEV)], output_dtype=dtype)
        c, d = fe.image_clip([torch.from_numpy(xs[2]).to(DEV), torch.from_numpy(xs[1]).to(DEV)], output_dtype=dtype)
        assert same_bits(a, c) and same_bits(b, d)
    # the module-level form, one tensor; the input is left as it was
    x = torch.from_numpy(xs[2]).to(DEV)
    y = pkg.image_clip(x)
    assert np.array_equal(y.cpu().numpy(), clip_mirror(xs[2])) and np.array_equal(x.cpu().numpy(), xs[2])
    assert float(y.min()) == 0.0 and float(y.max()) == 1.0


def test_image_clip_of_a_constant_image(pkg):
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
    x = [torch.full((3, 9, 11), 0.37, device=DEV), torch.arange(3 * 4 * 5, dtype=F32, device=DEV).view(3, 4, 5)]
    y, y8 = fe.image_clip(x), fe.image_clip(x, output_dtype=U8)
    assert torch.isnan(y[0]).all() and (y8[0] == 0).all()
    assert np.array_equal(y[1].cpu().numpy(), clip_mirror(x[1].cpu().numpy()))


@pytest.mark.parametrize("name", ["mid", "sq512x2"])
def test_clip_in_the_prefix_calls(pkg, pn, lfq, name):
    c = D.build(name)
    fe = make_fe(pkg, c.cfg)
    per = [[1, n // 2, n] for n in token_counts(c.img)]
    dp = dct_patches(pkg, c.batch, c.out)
    plain = [f for fs in fe.postprocess_prefixes(dp, per) for f in fs]
    for dtype in (F32, U8):
        got = [f for fs in fe.postprocess_prefixes(dp, per, output_dtype=dtype, clip="minmax") for f in fs]
        ss.assert_same_bits(ss.flat(got), ss.flat(fe.image_clip(plain, output_dtype=dtype)), f"{name} {dtype}")
    if name == "sq512x2":
        codes = codes_of(name).to(DEV).to(I16)
        plain = [f for fs in fe.decode_prefixes(dp, codes, pn, lfq, per) for f in fs]
        got = [f for fs in fe.decode_prefixes(dp, codes, pn, lfq, per, output_dtype=U8, clip="minmax") for f in fs]
        ss.assert_same_bits(ss.flat(got), ss.flat(fe.image_clip(plain, output_dtype=U8)), "codes")


# ---- 13. overridden hooks -------------------------------------------------------------------------------------
def test_overridden_transform_gives_the_masked_spectra(pkg):
    c = D.build("mid")

    class Spectrum(pkg.DCTAutoencoderFeatureExtractor):
        def _transform_image_out(self, x):
            return x
    fe = make_fe(pkg, c.cfg, Spectrum)
    per = [[0, 3, n] for n in token_counts(c.img)]
    got = fe.postprocess_prefixes(dct_patches(pkg, c.batch, c.out), per)
    for j in range(3):
        kp = masked_key_pad(c.batch, c.img, [p[j] for p in per])
        spectra = fe.revert_patching(dct_patches(pkg, c.batch, c.out, kp))
        for i, (sp, (h, w)) in enumerate(zip(spectra, c.batch.original_sizes)):
            want = torch.zeros(3, int(h), int(w), device=DEV)
            want[:, :sp.shape[1], :sp.shape[2]] = sp
            assert same_bits(got[i][j], want), (i, j)
    assert not bool(got[0][0].any()) and bool(got[0][1].any())


# ---- 14. refusals ------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    lib = ss.mods()[0]
    with ss._context(lib) as ctx:
        ss.timed(ctx)
        mid, sq = Raw(pkg, "mid"), Raw(pkg, "sq512x2")
        assert mid.ctx is ctx
        S = mid.table.S
        n = max(mid.numel)
        out = _filled(2 * n + 8, F32)
        out8 = _filled(2 * 3 * 512 * 512 + 8, U8)
        bad_cfg = mid.p.c(S)
        bad_cfg.patch_size = 0
        big_grid = list(mid.table.phw)
        big_grid[0] = 1000
        cases = [
            ("what dctae_decode refuses: the configuration", lambda: mid.call([0], [1], [0], out, 0, cfg=bad_cfg), ""),
            ("what dctae_decode refuses: patch_sizes", lambda: mid.call([0], [1], [0], out, 0, patch_hw=big_grid),
             "patch_sizes do not fit"),
            ("image above range", lambda: mid.call([0, 3], [1, 1], [0, n], out, 0), "out of range"),
            ("image below range", lambda: mid.call([-1], [1], [0], out, 0), "out of range"),
            ("cut above max_seq_len", lambda: mid.call([0], [S + 1], [0], out, 0), "max_seq_len"),
            ("cut below zero", lambda: mid.call([0], [-1], [0], out, 0), "max_seq_len"),
            ("NULL image array", lambda: mid.call([0], [1], [0], out, 0, null=(0,)), "NULL frame array"),
            ("NULL cut array", lambda: mid.call([0], [1], [0], out, 0, null=(1,)), "NULL frame array"),
            ("NULL offset array", lambda: mid.call([0], [1], [0], out, 0, null=(2,)), "NULL frame array"),
            ("negative offset", lambda: mid.call([0], [1], [-4], out, 0), "negative"),
            ("negative n_frames", lambda: mid.call([0], [1], [0], out, 0, n_frames=-1), "n_frames"),
            ("unknown output type", lambda: mid.call([0], [1], [0], out, 2), "out_type"),
            ("unknown clip", lambda: mid.call([0], [1], [0], out, 0, clip=2), "clip"),
            ("a 512 x 512 byte frame off 4 bytes", lambda: sq.call([0, 1], [9, 9], [0, 3 * 512 * 512 + 2], out8, 1),
             "4-byte aligned"),
        ]
        for what, call, msg in cases:
            rc = call()
            assert rc != 0 and (rc == EINVAL or what.startswith("what dctae_decode refuses")), (what, rc)
            assert msg in mid.error(), (what, mid.error())
        # nothing to do: no launch, no error
        assert mid.call([], [], [], out, 0, n_frames=0, null=(0, 1, 2)) == 0
        torch.cuda.synchronize()
        assert not any(ss._stages(ctx).values()), "a refused call launched something"
        assert torch.isnan(out).all() and (out8 == 0xAB).all(), "a refused call wrote its output"
        # the same frame tables, in order, are accepted
        assert sq.call([0, 1], [9, 9], [0, 3 * 512 * 512 + 4], out8, 1) == 0, sq.error()
        assert mid.call([0, 2], [1, S], [0, n], out, 0) == 0, mid.error()
        torch.cuda.synchronize()
        assert ss._stages(ctx).get("dec_map") == 2
