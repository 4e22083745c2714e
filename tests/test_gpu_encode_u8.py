"""The encode straight from uint8 images (include/dctae_u8.h).

The rule under test: a byte image means the fp32 image ``u8.float() / 255``,
and the byte path's outputs are BIT-IDENTICAL to the fp32 path fed that image:
codes, positions, channels, image ids, key_pad, PatchNorm patches, raw tokens
and scores, for every row-kernel family that reads the caller's pixels and
under every library option that picks another one.  After the load the
arithmetic is the same values in the same order, so nothing here is a
tolerance; the one tolerance test is the oracle anchor (both paths wrong
together), at the bound tests/test_gpu_parity.py applies to raw tokens.

The fp32 reference image is divided on the CPU, where torch's ``/ 255`` is the
IEEE division the semantics name (``pil_to_tensor(img) / 255`` in the
reference's scripts is a CPU operation too).  On the GPU torch divides a
tensor by a Python scalar by multiplying with the rounded reciprocal, which is
an ulp off for about half of the byte values (test_u8_to_f32_all_values
prints the count): not the image a byte image means.

Inputs: ``torch.randint(0, 256, dtype=torch.uint8)`` with a fixed seed, one row
of every image overwritten with ``arange(256)`` tiled or cut to W.  Sizes are
the smallest that reach each kernel's edges:
  k_rows512pk   W = 512; H = 512 (band layout with k_cols512b), H = 70 / 14
                (row-major; H not a multiple of the block's 16 rows: the
                min(y, H - 1) clamp), 512^2 with cols512b = 0
  224 kernels   224 x 224, 99 x 224 (the last wave holds one row), 98 x 224
  generic FFT   (fft_generic = 1) 28 x 60, 30 x 1024; with fft_spec = 0 on 512^2
                and 224^2; rows_kernel = 2 (k_fft_rows2<512>) on 512^2
  GEMM          14 x 14, 45 x 75, 46 x 58, 38 x 254 and 37 x 251 (a side above
                224 of either parity): k_rows_fused by default, k_rgb_to_ipt
                with rows_fused = 0; gemm_h2 = 0; fft = 0
  GEMM rows, FFT columns (k_rgb_to_ipt alone; fft_generic = 1)   60 x 46
  Bluestein     58 x 46, 46 x 58 (bluestein = 1); 45 x 75 with fft_odd = 1 (and
                fft_generic = 1: the odd plans run on the generic kernels)
By default the sides without a compile-time FFT kernel take the GEMM DCT
(Options::fft_generic), so the ragged list runs once at the defaults and once
with every route switched on.
"""
import ctypes as C
from importlib import import_module

import pytest
import torch

from oracle import ref_cpu
from test_options_host import DEFAULTS, EINVAL

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = ref_cpu.FEConfig()

S512 = [(512, 512)] * 3
ROWMAJOR = [(70, 512), (14, 512)]
K224 = [(224, 224), (99, 224), (98, 224)]
GENERIC = [(28, 60), (30, 1024)]
GEMM = [(14, 14), (45, 75), (46, 58), (38, 254), (37, 251)]
GEMM_FFT = [(60, 46)]
BLUESTEIN = [(58, 46), (46, 58)]
RAGGED = [(512, 512)] + ROWMAJOR + K224 + GENERIC + GEMM + GEMM_FFT + BLUESTEIN


@pytest.fixture(scope="module", autouse=True)
def _package(pkg):
    """the package loaded before any test imports its modules by name"""
    return pkg


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


@pytest.fixture(scope="module")
def lfq_p(pkg):
    torch.manual_seed(5)
    return pkg.LFQ(dim=196, codebook_size=2 ** 13, num_codebooks=16).to(DEV).eval()   # with projections


def _ops():
    return import_module("dct_autoencoder_amd._ops")


def byte_images(seed, sizes):
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in sizes:
        u = torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
        u[:, h // 2, :] = (torch.arange(w) % 256).to(torch.uint8)   # arange(256), tiled or cut to W
        out.append(u.to(DEV))
    return out


def exact_f32(u):
    """u8.float() / 255 with fp32 division (on the CPU: see the module docstring), on u's device"""
    return (u.cpu().float() / 255).to(u.device)


def as_f32(images):
    if isinstance(images, torch.Tensor):
        return exact_f32(images)
    return [exact_f32(u) for u in images]


def _fields(dp, codes):
    d = dp._data or {}
    return {"codes": codes, "patches": dp.patches, "raw": d.get("raw_patches"), "scores": d.get("scores"),
            "key_pad": dp.key_pad_mask, "image_ids": dp.batched_image_ids, "channels": dp.patch_channels,
            "positions": dp.patch_positions, "sizes": (dp.patch_sizes, dp.original_sizes)}


def encode(fe, images, pn, lfq, u8, **kw):
    if u8:
        kw["uint8_images"] = True
    outs = fe.encode_batch(images, pn, lfq, return_patches=True, return_raw=True, return_scores=True, **kw)
    torch.cuda.synchronize()
    return [_fields(dp, codes) for dp, codes in outs]


def assert_same(a, b, what=""):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert fa.keys() == fb.keys()
        for k in fa:
            if k == "sizes":
                assert fa[k] == fb[k], (what, k)
            else:
                assert fa[k] is not None and fa[k].dtype == fb[k].dtype and torch.equal(fa[k], fb[k]), (what, k)


def check(fe, pn, lfq, images, what=""):
    """every field of the byte call equals the fp32 call on u8.float() / 255"""
    got = encode(fe, images, pn, lfq, True)
    want = encode(fe, as_f32(images), pn, lfq, False)
    assert_same(got, want, what)
    return got


class options:
    """set library options for a block and restore the defaults on exit, failing case or not"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        try:
            for k, v in self.kv.items():
                _ops().set_option(k, v)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        for k in self.kv:
            _ops().set_option(k, DEFAULTS[k])


def _stage_names(fn):
    """the launch stages (dctae_timing_get names) of the encodes fn() makes"""
    lib_mod = import_module("dct_autoencoder_amd._lib")
    ctx = lib_mod.context(torch.device(DEV, torch.cuda.current_device()))
    ctx.check(ctx.lib.dctae_set_timing(ctx.h, 1))
    try:
        ctx.check(ctx.lib.dctae_timing_reset(ctx.h))
        fn()
        torch.cuda.synchronize()
        ctx.check(ctx.lib.dctae_timing_collect(ctx.h))
        out, name, ms, n = set(), C.c_char_p(), C.c_double(), C.c_int64()
        i = 0
        while ctx.lib.dctae_timing_get(ctx.h, i, C.byref(name), C.byref(ms), C.byref(n)) == 0:
            if n.value:
                out.add(name.value.decode())
            i += 1
        return out
    finally:
        ctx.check(ctx.lib.dctae_timing_reset(ctx.h))
        ctx.check(ctx.lib.dctae_set_timing(ctx.h, 0))


# ---- 1. the conversion itself
def test_u8_to_f32_all_values():
    x = (torch.arange(1000) % 256).to(torch.uint8).to(DEV)   # 1,000 elements: not a multiple of 4
    y = _ops().u8_to_f32(x)
    assert y.dtype == torch.float32 and torch.equal(y, exact_f32(x))
    assert torch.equal(y.cpu()[:256], torch.arange(256, dtype=torch.uint8) / 255)
    # at an odd base address, 2-D shape kept
    z = _ops().u8_to_f32(x[1:991].view(10, 99))
    assert z.shape == (10, 99) and torch.equal(z, exact_f32(x[1:991].view(10, 99)))
    # for the record: torch's own division by the scalar on this device
    n_off = int(((x[:256].float() / 255) != y[:256]).sum())
    print(f"torch's GPU `u8.float() / 255` differs from fp32 division for {n_off} of 256 byte values")


# ---- 2. k_rows512pk, band layout
def test_rows512_band_batch(fe, pn, lfq):
    x = torch.stack(byte_images(11, S512)).contiguous()   # 3 images: the column blocks take 2 and 3
    got = check(fe, pn, lfq, x, "512^2 x 3")
    # the same through the pre-planned encoders
    fe_mod = import_module("dct_autoencoder_amd.feature_extraction")
    e8 = fe_mod.BatchEncoder(fe, 3, 512, 512, pn, lfq, device=DEV, want_patches=True, input_dtype=torch.uint8)
    ef = fe_mod.BatchEncoder(fe, 3, 512, 512, pn, lfq, device=DEV, want_patches=True)
    o8 = {k: v.clone() for k, v in e8(x).items()}
    of = ef(as_f32(x).contiguous())
    torch.cuda.synchronize()
    assert o8.keys() == of.keys()
    for k in o8:
        assert torch.equal(o8[k], of[k]), k
    assert torch.equal(o8["codes"], got[0]["codes"]) and torch.equal(o8["patches"], got[0]["patches"])


def test_rows512_band_lfq_projections(fe, pn, lfq_p):
    x = torch.stack(byte_images(12, S512)).contiguous()
    fe_mod = import_module("dct_autoencoder_amd.feature_extraction")
    e8 = fe_mod.BatchEncoder(fe, 3, 512, 512, pn, lfq_p, device=DEV, input_dtype=torch.uint8)
    ef = fe_mod.BatchEncoder(fe, 3, 512, 512, pn, lfq_p, device=DEV)
    assert e8.proj_staged and ef.proj_staged   # dctae_encode_lfq_proj_u8 / dctae_encode_lfq_proj
    o8 = {k: v.clone() for k, v in e8(x).items()}
    of = ef(as_f32(x).contiguous())
    torch.cuda.synchronize()
    for k in o8:
        assert torch.equal(o8[k], of[k]), k
    check(fe, pn, lfq_p, x, "512^2 x 3, LFQ with projections")   # encode_batch: dctae_encode_u8 + project_in


# ---- 3. k_rows512pk, row-major layout
def test_rows512_row_major(fe, pn, lfq):
    check(fe, pn, lfq, byte_images(13, ROWMAJOR), "70 x 512, 14 x 512")
    with options(cols512b=0):
        check(fe, pn, lfq, byte_images(14, S512[:1]), "512^2, cols512b = 0")


# ---- 4. 224 kernels
def test_rows224(fe, pn, lfq):
    check(fe, pn, lfq, byte_images(15, K224), "224-wide")


# ---- 5. generic FFT rows
def test_fft_rows_generic(fe, pn, lfq):
    imgs = byte_images(16, GENERIC)
    with options(fft_generic=1):
        st = _stage_names(lambda: check(fe, pn, lfq, imgs, "28 x 60, 30 x 1024"))
        assert "fft_rows" in st
    with options(fft_generic=1, fft_spec=0):
        check(fe, pn, lfq, byte_images(17, [(512, 512), (224, 224)]), "fft_spec = 0")
    with options(rows_kernel=2):
        check(fe, pn, lfq, byte_images(18, [(512, 512)]), "rows_kernel = 2")


# ---- 6. GEMM rows and columns
def test_gemm_rows(fe, pn, lfq):
    imgs = byte_images(19, GEMM)
    assert "rows_fused" in _stage_names(lambda: check(fe, pn, lfq, imgs, "GEMM sizes"))
    with options(rows_fused=0):
        st = _stage_names(lambda: check(fe, pn, lfq, imgs, "rows_fused = 0"))
        assert "rgb_to_ipt" in st and "rows_fused" not in st
    with options(gemm_h2=0):
        check(fe, pn, lfq, imgs, "gemm_h2 = 0")
    with options(fft=0):
        check(fe, pn, lfq, imgs, "fft = 0")


# ---- 7. GEMM rows with FFT columns
def test_gemm_rows_fft_cols(fe, pn, lfq):
    imgs = byte_images(20, GEMM_FFT)
    with options(fft_generic=1):
        st = _stage_names(lambda: check(fe, pn, lfq, imgs, "60 x 46"))
        assert "rgb_to_ipt" in st and "fft_cols" in st


# ---- 8. Bluestein
def test_bluestein_rows(fe, pn, lfq):
    imgs = byte_images(21, BLUESTEIN)
    with options(bluestein=1):
        assert "bs_rows" in _stage_names(lambda: check(fe, pn, lfq, imgs, "bluestein = 1"))
    with options(fft_odd=1, fft_generic=1):
        st = _stage_names(lambda: check(fe, pn, lfq, byte_images(22, [(45, 75)]), "fft_odd = 1"))
        assert "fft_rows" in st


# ---- 9. ragged list, unaligned views, odd image starts
def _views_at_odd_offsets(images):
    """every image a view into one flat uint8 buffer, at byte offsets 1, 2 and 3 mod 4 in turn"""
    n = sum(u.numel() + 8 for u in images) + 8
    flat = torch.zeros(n, dtype=torch.uint8, device=DEV)
    assert flat.data_ptr() % 4 == 0
    views, off = [], 0
    for i, u in enumerate(images):
        off = (off + 3) // 4 * 4 + 1 + i % 3
        v = flat[off:off + u.numel()].view(u.shape)
        v.copy_(u)
        assert v.data_ptr() % 4 == 1 + i % 3
        views.append(v)
        off += u.numel()
    return views


def test_ragged_list_and_unaligned_views(fe, pn, lfq):
    imgs = byte_images(23, RAGGED)
    want = encode(fe, as_f32(imgs), pn, lfq, False)
    assert_same(encode(fe, imgs, pn, lfq, True), want, "ragged list")
    views = _views_at_odd_offsets(imgs)   # the 512-wide ones are cloned by the wrapper
    assert_same(encode(fe, views, pn, lfq, True), want, "ragged list, views at odd offsets")
    # every route in one call (generic and odd FFT, Bluestein), in several chunk jobs
    with options(fft_generic=1, fft_odd=1, bluestein=1, chunk_bytes=2 ** 20):
        st = _stage_names(lambda: assert_same(encode(fe, views, pn, lfq, True),
                                              encode(fe, as_f32(imgs), pn, lfq, False), "every route, chunked"))
        assert {"fft_rows", "bs_rows"} <= st


def test_batch_with_odd_image_starts(fe, pn, lfq):
    x = torch.stack(byte_images(24, [(45, 75)] * 4)).contiguous()   # 3 H W odd: every second image at an odd byte
    assert (3 * 45 * 75) % 2 == 1
    check(fe, pn, lfq, x, "4 x 45 x 75")


def test_iterator_and_non_contiguous_inputs(fe, pn, lfq):
    """a generator of images is read once; a non-contiguous image is encoded as its dense copy"""
    imgs = byte_images(30, [(28, 60), (46, 58)])
    want = encode(fe, imgs, pn, lfq, True)
    assert_same(encode(fe, (u for u in imgs), pn, lfq, True), want, "generator")
    wide = torch.zeros((3, 28, 120), dtype=torch.uint8, device=DEV)
    wide[:, :, ::2] = imgs[0]
    view = wide[:, :, ::2]
    assert not view.is_contiguous() and torch.equal(view, imgs[0])
    assert_same(encode(fe, [view, imgs[1]], pn, lfq, True), want, "non-contiguous view")


# ---- 10. the staged path
def test_staged_hooks_see_fp32_images(pkg, pn, lfq):
    imgs = byte_images(25, [(28, 60), (45, 75)])

    def staged_fe():
        f = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
        seen, orig = [], f._transform_image_in

        def hook(x):
            seen.append(x.clone())
            return orig(x)

        f._transform_image_in = hook
        assert f._staged_in()
        return f, seen

    f8, seen8 = staged_fe()
    ff, seenf = staged_fe()
    got = f8.encode_batch(imgs, pn, lfq, return_patches=True, return_raw=True, uint8_images=True)
    want = ff.encode_batch(as_f32(imgs), pn, lfq, return_patches=True, return_raw=True)
    torch.cuda.synchronize()
    assert len(seen8) == len(imgs)
    for s, u in zip(seen8, imgs):
        assert s.dtype == torch.float32 and torch.equal(s, exact_f32(u))
    assert len(got) == len(want) >= 1
    for (da, ca), (db, cb) in zip(got, want):
        # the staged path returns the raw tokens as .patches and the PatchNorm output beside them (no scores)
        na, nb = da._data["normalised_patches"], db._data["normalised_patches"]
        for a, b in ((ca, cb), (da.patches, db.patches), (na, nb), (da.key_pad_mask, db.key_pad_mask),
                     (da.batched_image_ids, db.batched_image_ids), (da.patch_channels, db.patch_channels),
                     (da.patch_positions, db.patch_positions)):
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert da.patches.shape[-1] == 196 and na.shape == da.patches.shape and not torch.equal(na, da.patches)
        assert (da.patch_sizes, da.original_sizes) == (db.patch_sizes, db.original_sizes)


# ---- 11. oracle anchor
@pytest.mark.parametrize("shape", [(70, 512), (45, 75)])
def test_oracle_anchor(fe, shape):
    (u,) = byte_images(26, [shape])
    ((dp, _),) = fe.encode_batch([u], None, None, return_raw=True, uint8_images=True)
    keep = ~dp.key_pad_mask[0].cpu()
    gp, gpos, gch = dp.patches[0].cpu()[keep], dp.patch_positions[0].cpu()[keep], dp.patch_channels[0].cpu()[keep]
    y = ref_cpu.transform_image_in(u.cpu().float() / 255)
    ph, pw = ref_cpu.crop_dims(y.shape[1], y.shape[2], 14)
    toks, pos, ch, _ = ref_cpu.patch_scores(y[:, :ph, :pw], CFG)
    omap = {(int(c), int(p[0]), int(p[1])): i for i, (p, c) in enumerate(zip(pos.tolist(), ch.tolist()))}
    idx = torch.tensor([omap[(int(c), int(p[0]), int(p[1]))] for p, c in zip(gpos.tolist(), gch.tolist())])
    assert len(set(idx.tolist())) == len(idx) == len(omap)
    ymax = float(toks.abs().max())
    err = float((gp - toks[idx]).abs().max())
    print(f"{shape}: max |gpu - oracle| = {err:.3e}, max|Y| = {ymax:.3e}, ratio {err / ymax:.2e}")
    assert err <= 2e-6 * ymax, (err, ymax)


# ---- 12. refusals
def test_python_refusals(pkg, fe, pn, lfq):
    imgs = byte_images(27, [(28, 60)])
    with pytest.raises(TypeError):
        fe.encode_batch(as_f32(imgs), pn, lfq, uint8_images=True)
    with pytest.raises(TypeError):
        fe.encode_batch(torch.stack(as_f32(imgs)), pn, lfq, uint8_images=True)
    fe_mod = import_module("dct_autoencoder_amd.feature_extraction")
    e8 = fe_mod.BatchEncoder(fe, 1, 28, 60, pn, lfq, device=DEV, input_dtype=torch.uint8)
    ef = fe_mod.BatchEncoder(fe, 1, 28, 60, pn, lfq, device=DEV)
    x = torch.stack(imgs).contiguous()
    with pytest.raises(AssertionError):
        e8(as_f32(x))
    with pytest.raises(AssertionError):
        ef(x)
    with pytest.raises(TypeError):
        fe_mod.BatchEncoder(fe, 1, 28, 60, pn, lfq, device=DEV, input_dtype=torch.float16)


def _raw_call(fe, pn, entry, base, H, W):
    """dctae_encode_u8 / dctae_spectrum_tokens_u8 through ctypes on one (3, H, W) image at address base"""
    lib_mod = import_module("dct_autoencoder_amd._lib")
    packing = import_module("dct_autoencoder_amd.packing")
    ctx = lib_mod.context(torch.device(DEV, torch.cuda.current_device()))
    ptr, S = lib_mod.ptr, 3072
    k = fe._tokens(H, W)
    offs, hw = lib_mod.i64([0]), lib_mod.i32([H, W])
    desc = lib_mod.ImagesU8(C.c_void_p(base), C.cast(offs, C.POINTER(C.c_int64)), C.cast(hw, C.POINTER(C.c_int32)), 1)
    plan = packing.layout([[0]], {0: k})
    arrs = [lib_mod.i32(a) for a in (plan.row, plan.col, plan.k, plan.local_id, plan.row_len)]
    pk = lib_mod.Packing(*[C.cast(a, C.POINTER(C.c_int32)) for a in arrs], 1)
    t = dict(positions=torch.empty((1, S, 2), dtype=torch.long, device=DEV),
             channels=torch.empty((1, S), dtype=torch.long, device=DEV),
             image_ids=torch.empty((1, S), dtype=torch.long, device=DEV),
             key_pad=torch.empty((1, S), dtype=torch.bool, device=DEV),
             raw=torch.empty((1, S, 196), dtype=torch.float32, device=DEV))
    po = lib_mod.PackedOut(None, ptr(t["positions"]), ptr(t["channels"]), ptr(t["image_ids"]), ptr(t["key_pad"]), None,
                           ptr(t["raw"]), None)
    cfg = fe.params(S).c(S)
    rc = getattr(ctx.lib, entry)(ctx.h, C.byref(cfg), C.byref(desc), C.byref(pk), None, None, C.byref(po),
                                 lib_mod.stream_ptr(torch.device(DEV, torch.cuda.current_device())))
    torch.cuda.synchronize()
    return rc, (ctx.lib.dctae_last_error(ctx.h) or b"").decode(), t


def test_abi_refusals(fe, pn):
    (u,) = byte_images(28, [(14, 512)])
    buf = torch.zeros(u.numel() + 8, dtype=torch.uint8, device=DEV)
    buf[1:1 + u.numel()].copy_(u.flatten())
    assert buf.data_ptr() % 4 == 0
    # a misaligned 512-wide image on k_rows512pk: refused, naming the image and the alignment
    rc, msg, _ = _raw_call(fe, pn, "dctae_encode_u8", buf.data_ptr() + 1, 14, 512)
    assert rc == EINVAL and "image 0" in msg and "4-byte aligned" in msg, (rc, msg)
    # the same bytes at an aligned address encode, and equal the Python path
    buf[:u.numel()].copy_(u.flatten())
    rc, msg, t = _raw_call(fe, pn, "dctae_encode_u8", buf.data_ptr(), 14, 512)
    assert rc == 0, msg
    ((dp, _),) = fe.encode_batch([u], None, None, return_raw=True, uint8_images=True)
    keep = ~dp.key_pad_mask[0]
    assert torch.equal(t["key_pad"], dp.key_pad_mask) and torch.equal(t["raw"][0][keep], dp.patches[0][keep])
    # the refusal does not depend on the order of calls: the aligned call above left its plan cached, and the
    # same descriptor one byte further (same offsets, sizes and options) is refused all the same, then the
    # aligned one encodes again
    buf[1:1 + u.numel()].copy_(u.flatten())
    rc, msg, _ = _raw_call(fe, pn, "dctae_encode_u8", buf.data_ptr() + 1, 14, 512)
    assert rc == EINVAL and "image 0" in msg and "4-byte aligned" in msg, (rc, msg)
    buf[:u.numel()].copy_(u.flatten())
    rc, msg, t3 = _raw_call(fe, pn, "dctae_encode_u8", buf.data_ptr(), 14, 512)
    assert rc == 0 and torch.equal(t3["raw"][0][keep], dp.patches[0][keep]), msg
    # with the rows on the per-pixel kernel the misaligned image is legal, and gives the same tokens
    buf[1:1 + u.numel()].copy_(u.flatten())
    with options(rows_kernel=2):
        rc, msg, t2 = _raw_call(fe, pn, "dctae_encode_u8", buf.data_ptr() + 1, 14, 512)
        assert rc == 0, msg
        ((dp2, _),) = fe.encode_batch([exact_f32(u)], None, None, return_raw=True)
        assert torch.equal(t2["raw"][0][keep], dp2.patches[0][keep])
    # NULL pixels with n_img > 0, as the fp32 entry
    rc, msg, _ = _raw_call(fe, pn, "dctae_encode_u8", None, 14, 512)
    assert rc == EINVAL and "image descriptor" in msg, (rc, msg)


def test_spectrum_tokens_u8(fe):
    """the token-mode entry (flat token order), byte images at odd offsets against the fp32 entry"""
    lib_mod = import_module("dct_autoencoder_amd._lib")
    dev = torch.device(DEV, torch.cuda.current_device())
    ctx = lib_mod.context(dev)
    sizes = [(28, 60), (46, 58), (14, 512)]
    imgs = byte_images(29, sizes)
    desc8, _, keep8 = _ops().image_set_u8(_views_at_odd_offsets(imgs))
    descf, _, keepf = _ops().image_set(as_f32(imgs))
    n = [fe._tokens(h, w) for h, w in sizes]
    tok_off = lib_mod.i64([0, n[0], n[0] + n[1]])
    cfg = fe.params(3072).c(3072)
    res = []
    for entry, desc in (("dctae_spectrum_tokens_u8", desc8), ("dctae_spectrum_tokens", descf)):
        tokens = torch.empty((sum(n), 196), dtype=torch.float32, device=DEV)
        scores = torch.empty(sum(n), dtype=torch.float32, device=DEV)
        ctx.check(getattr(ctx.lib, entry)(ctx.h, C.byref(cfg), C.byref(desc), C.cast(tok_off, C.POINTER(C.c_int64)),
                                          lib_mod.ptr(tokens), lib_mod.ptr(scores), lib_mod.stream_ptr(dev)), entry)
        torch.cuda.synchronize()
        res.append((tokens, scores))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ---- 13. run to run
def test_run_to_run(fe, pn, lfq):
    imgs = byte_images(23, RAGGED)
    first = encode(fe, imgs, pn, lfq, True)
    first = [{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in f.items()} for f in first]
    for _ in range(4):
        assert_same(encode(fe, imgs, pn, lfq, True), first, "run to run")
