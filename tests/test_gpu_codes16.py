"""Compact LFQ codes (include/dctae_codes16.h): int16 out of the encode and
into the decode.

The rule under test: an int16 code c means the int64 code int64(c).  Every
check is an equality: the int16 encode's codes, widened with ``.long()``, are
the int64 encode's, and every other output is ``torch.equal``; images decoded
from int16 codes are ``torch.equal`` to images decoded from ``codes.long()``.

Shapes are the smallest that reach each code sink and source:
  k_sort_pack2<256, 3>   224 x 224, 14 x 14 (three tokens), 45 x 75
  k_sort_pack2<512, 6>   512 x 512, 70 x 512 (ncb == 14: two codes per store)
  generic branch         28 codebooks of 7 bits on 45 x 75 and 224 x 224;
                         patch size 5 with 5 codebooks of 5 bits on 23 x 37
                         (odd ncb: packed rows only 2-byte aligned)
  k_sort_pack            option sort_kernel = 1
  k_pad_fill             the ragged list in one call (rows end in pads)
  k_idct_cols512b / k_idct_cols512 / k_scatter_tokens   3 x 512^2 at the
                         defaults and with dec_cols_kernel = 1, the ragged
                         list and 224^2 with fft_decode = 0
  LFQ projections        196 -> 16 x 13, fused (3 x 512^2), standalone
                         (5 x 224^2, the ragged list), lfq_ws = 0, gemm_h2 = 0
"""
import ctypes as C
from importlib import import_module

import pytest
import torch

from test_gpu_encode_u8 import _fields, byte_images, options
from test_options_host import EINVAL

pytestmark = pytest.mark.gpu
DEV = "cuda"
I16, I64, U8 = torch.int16, torch.int64, torch.uint8
RAGGED = [(512, 512), (70, 512), (224, 224), (99, 224), (45, 75), (14, 14)]
SENTINEL = -21846   # 0xAAAA: no code is negative


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
def lfq28(pkg):
    return pkg.LFQ(dim=196, codebook_size=2 ** 7, num_codebooks=28).to(DEV).eval()


@pytest.fixture(scope="module")
def lfq_p(pkg):
    torch.manual_seed(5)
    return pkg.LFQ(dim=196, codebook_size=2 ** 13, num_codebooks=16).to(DEV).eval()   # with projections


@pytest.fixture(scope="module")
def p5(pkg):
    """patch size 5 with 5 codebooks of 5 bits: an odd number of codes per token"""
    g = torch.Generator().manual_seed(55)
    m = pkg.PatchNorm(8, 8, 5, 3).to(DEV)
    m.median.data.copy_(0.05 * torch.randn(m.median.shape, generator=g))
    m.b.data.copy_(0.02 + 0.1 * torch.rand(m.b.shape, generator=g))
    m.frozen = True
    return (pkg.DCTAutoencoderFeatureExtractor(3, 5, 0.0, 8, 8, 256), m.eval(),
            pkg.LFQ(dim=25, codebook_size=2 ** 5, num_codebooks=5).to(DEV).eval())


def _fe_mod():
    return import_module("dct_autoencoder_amd.feature_extraction")


def f32_images(seed, sizes):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand((3, h, w), generator=g).to(DEV) for h, w in sizes]


def encode(fe, images, pn, lfq, dtype, **kw):
    outs = fe.encode_batch(images, pn, lfq, return_patches=True, return_raw=True, return_scores=True,
                           codes_dtype=dtype, **kw)
    torch.cuda.synchronize()
    return [_fields(dp, codes) for dp, codes in outs]


def assert_codes16(got, want, what=""):
    """got: the int16 call's fields, want: the int64 call's"""
    assert len(got) == len(want) >= 1
    for fa, fb in zip(got, want):
        assert fa.keys() == fb.keys()
        for k in fa:
            if k == "sizes":
                assert fa[k] == fb[k], (what, k)
            elif k == "codes":
                assert fa[k].dtype == I16 and fb[k].dtype == I64, what
                assert torch.equal(fa[k].long(), fb[k]), (what, k)   # pads included
                assert torch.equal(fa[k], fb[k].to(I16)), (what, k)
            else:
                assert fa[k] is not None and fa[k].dtype == fb[k].dtype and torch.equal(fa[k], fb[k]), (what, k)


def check(fe, pn, lfq, images, what="", **kw):
    got = encode(fe, images, pn, lfq, I16, **kw)
    want = encode(fe, images, pn, lfq, I64, **kw)
    assert_codes16(got, want, what)
    return got, want


def batch_pair(fe, pn, lfq, x, **kw):
    """the int16 and the int64 BatchEncoder on x; outputs cloned"""
    B, _, H, W = x.shape
    e16 = _fe_mod().BatchEncoder(fe, B, H, W, pn, lfq, device=DEV, codes_dtype=I16, **kw)
    e64 = _fe_mod().BatchEncoder(fe, B, H, W, pn, lfq, device=DEV, **kw)
    o16 = {k: v.clone() for k, v in e16(x).items()}
    o64 = {k: v.clone() for k, v in e64(x).items()}
    torch.cuda.synchronize()
    assert o16.keys() == o64.keys()
    for k in o16:
        if k == "codes":
            assert o16[k].dtype == I16 and o64[k].dtype == I64
            assert torch.equal(o16[k].long(), o64[k]), k
        else:
            assert o16[k].dtype == o64[k].dtype and torch.equal(o16[k], o64[k]), k
    return e16, e64, o16, o64


# ---- 1. encode identity ---------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[(224, 224)], [(14, 14)], [(45, 75)], [(512, 512)], [(70, 512)]],
                         ids=lambda s: "x".join(map(str, s[0])))
def test_encode_sort_pack2(fe, pn, lfq, sizes):
    check(fe, pn, lfq, f32_images(101, sizes), str(sizes))


@pytest.mark.parametrize("shape", [(45, 75), (224, 224)], ids=lambda s: "x".join(map(str, s)))
def test_encode_generic_branch(fe, pn, lfq28, shape):
    check(fe, pn, lfq28, f32_images(102, [shape]), f"28 codebooks, {shape}")


def test_encode_generic_branch_odd_ncb(p5):
    fe5, pn5, lfq5 = p5
    got, _ = check(fe5, pn5, lfq5, f32_images(103, [(23, 37)]), "patch size 5, 5 codebooks")
    assert got[0]["codes"].shape[-1] == 5


@pytest.mark.parametrize("shape", [(45, 75), (224, 224)], ids=lambda s: "x".join(map(str, s)))
def test_encode_sort_kernel_1(fe, pn, lfq, shape):
    with options(sort_kernel=1):
        check(fe, pn, lfq, f32_images(104, [shape]), f"sort_kernel = 1, {shape}")


def test_encode_ragged_list_with_pads(fe, pn, lfq):
    got, want = check(fe, pn, lfq, f32_images(105, RAGGED), "ragged list")
    pads = torch.cat([f["key_pad"].flatten() for f in got])
    assert bool(pads.any()) and not bool(pads.all())   # rows end in pads: k_pad_fill wrote their codes
    for fa, fb in zip(got, want):
        kp = fa["key_pad"]
        assert torch.equal(fa["codes"][kp].long(), fb["codes"][kp])
    with options(sort_kernel=1):
        check(fe, pn, lfq, f32_images(105, RAGGED), "ragged list, sort_kernel = 1")


def test_encode_negative_codebook_scale(pkg, fe, pn):
    neg = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14, codebook_scale=-1.0).to(DEV).eval()
    pos = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).to(DEV).eval()
    imgs = f32_images(106, [(45, 75)])
    got, _ = check(fe, pn, neg, imgs, "codebook_scale = -1")
    assert not torch.equal(got[0]["codes"], encode(fe, imgs, pn, pos, I16)[0]["codes"])   # the masks were applied


def test_encode_uint8_images(fe, pn, lfq):
    check(fe, pn, lfq, byte_images(107, [(512, 512)]), "bytes, 512^2", uint8_images=True)
    check(fe, pn, lfq, byte_images(108, RAGGED), "bytes, ragged list", uint8_images=True)


def test_batch_encoder(fe, pn, lfq):
    x = torch.stack(f32_images(109, [(512, 512)] * 3)).contiguous()
    _, _, o16, _ = batch_pair(fe, pn, lfq, x, want_patches=True)
    assert torch.equal(o16["codes"], encode(fe, x, pn, lfq, I16)[0]["codes"])
    y = torch.stack(f32_images(110, [(224, 224)] * 5)).contiguous()   # 4 images per row: the second row is half full
    e16, _, o16, _ = batch_pair(fe, pn, lfq, y)
    assert e16.n_rows == 2 and bool(o16["key_pad_mask"][1].any())
    # byte input
    u = torch.stack(byte_images(111, [(512, 512)] * 3)).contiguous()
    batch_pair(fe, pn, lfq, u, input_dtype=U8)
    v = torch.stack(byte_images(112, [(224, 224)] * 5)).contiguous()
    batch_pair(fe, pn, lfq, v, input_dtype=U8)


# ---- 2. LFQ projections (196 -> 16 x 13) --------------------------------------------------
def test_projections_encode(fe, pn, lfq_p):
    x = torch.stack(f32_images(120, [(512, 512)] * 3)).contiguous()
    e16, _, _, _ = batch_pair(fe, pn, lfq_p, x)
    assert e16.proj_staged                      # dctae_encode_lfq_proj_c16: the sort / pack stores int16
    batch_pair(fe, pn, lfq_p, torch.stack(byte_images(121, [(512, 512)] * 3)).contiguous(), input_dtype=U8)
    y = torch.stack(f32_images(122, [(224, 224)] * 5)).contiguous()
    e16, _, _, _ = batch_pair(fe, pn, lfq_p, y)
    assert e16.proj and not e16.proj_staged     # rows not full: dctae_lfq_project_in_c16
    imgs = f32_images(123, RAGGED)
    check(fe, pn, lfq_p, imgs, "projections, ragged list")   # dctae_lfq_project_in_bounded_c16
    for opt in ("lfq_ws", "gemm_h2"):
        with options(**{opt: 0}):
            check(fe, pn, lfq_p, imgs[2:], f"projections, {opt} = 0")
            batch_pair(fe, pn, lfq_p, y)


def test_projections_negative_scale(pkg, fe, pn):
    """the standalone project_in's int16 sink applies the index rule of a scale <= 0 (lfq_index_bits)"""
    torch.manual_seed(6)
    neg = pkg.LFQ(dim=196, codebook_size=2 ** 13, num_codebooks=16, codebook_scale=-1.0).to(DEV).eval()
    check(fe, pn, neg, f32_images(124, [(45, 75), (224, 224)]), "projections, codebook_scale = -1")


@pytest.mark.parametrize("out_dtype", [torch.float32, U8], ids=["f32", "u8"])
def test_projections_decode(fe, pn, lfq_p, out_dtype):
    x = torch.stack(f32_images(125, [(512, 512)] * 3)).contiguous()
    enc = _fe_mod().BatchEncoder(fe, 3, 512, 512, pn, lfq_p, device=DEV)
    packed = {k: v.clone() for k, v in enc(x).items()}
    p16 = dict(packed, codes=packed["codes"].to(I16))
    dec = _fe_mod().BatchDecoder(enc, pn, lfq_p, output_dtype=out_dtype)
    for normed in (True, False):   # proj_normed: project_out + dctae_decode_normed; proj_inverse: the fused inverse
        dec.normed_decode = normed
        want = dec(packed).clone()
        got = dec(p16).clone()
        torch.cuda.synchronize()
        assert got.dtype == out_dtype and torch.equal(got, want), normed
    ((dp, codes),) = fe.encode_batch(f32_images(126, RAGGED[2:]), pn, lfq_p)
    want = fe.decode_batch(dp, codes, pn, lfq_p, output_dtype=out_dtype)
    got = fe.decode_batch(dp, codes.to(I16), pn, lfq_p, output_dtype=out_dtype)
    torch.cuda.synchronize()
    assert len(got) == len(want) == 4
    for a, b in zip(got, want):
        assert a.dtype == out_dtype and torch.equal(a, b)


# ---- 3. decode identity -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def packed512(fe, pn, lfq):
    x = torch.stack(f32_images(130, [(512, 512)] * 3)).contiguous()
    enc = _fe_mod().BatchEncoder(fe, 3, 512, 512, pn, lfq, device=DEV)
    packed = {k: v.clone() for k, v in enc(x).items()}
    torch.cuda.synchronize()
    return enc, packed


def _decode_both(enc, pn, lfq, packed, codes16, out_dtype):
    dec = _fe_mod().BatchDecoder(enc, pn, lfq, output_dtype=out_dtype)
    want = dec(dict(packed, codes=codes16.long())).clone()
    got = dec(dict(packed, codes=codes16)).clone()
    torch.cuda.synchronize()
    assert got.dtype == out_dtype and torch.equal(got, want)
    return got


@pytest.mark.parametrize("out_dtype", [torch.float32, U8], ids=["f32", "u8"])
@pytest.mark.parametrize("opts", [{}, {"dec_cols_kernel": 1}, {"dec_rows_kernel": 2}], ids=["defaults", "cols1", "rows2"])
def test_decode_batch_decoder_512(pn, lfq, packed512, opts, out_dtype):
    enc, packed = packed512
    with options(**opts):
        got = _decode_both(enc, pn, lfq, packed, packed["codes"].to(I16), out_dtype)
    assert float(got.float().std()) > 0   # an image, not a constant


@pytest.mark.parametrize("out_dtype", [torch.float32, U8], ids=["f32", "u8"])
def test_decode_any_int16_value(pn, lfq, packed512, out_dtype):
    """codes drawn from the whole int16 range: negative values, bit 15 set; .long() defines the result"""
    enc, packed = packed512
    g = torch.Generator().manual_seed(131)
    codes = torch.randint(-2 ** 15, 2 ** 15, packed["codes"].shape, generator=g, dtype=I16).to(DEV)
    assert bool((codes < 0).any())
    _decode_both(enc, pn, lfq, packed, codes, out_dtype)
    with options(dec_cols_kernel=1):
        _decode_both(enc, pn, lfq, packed, codes, out_dtype)


@pytest.mark.parametrize("out_dtype", [torch.float32, U8], ids=["f32", "u8"])
def test_decode_batch_ragged_scatter(fe, pn, lfq, out_dtype):
    ((dp, codes),) = fe.encode_batch(f32_images(132, RAGGED), pn, lfq)
    c16 = codes.to(I16)
    want = fe.decode_batch(dp, codes, pn, lfq, output_dtype=out_dtype)
    got = fe.decode_batch(dp, c16, pn, lfq, output_dtype=out_dtype)
    torch.cuda.synchronize()
    assert len(got) == len(want) == len(RAGGED)
    for a, b in zip(got, want):
        assert a.dtype == out_dtype and torch.equal(a, b)
    # any int16 value through k_scatter_tokens too
    g = torch.Generator().manual_seed(133)
    wild = torch.randint(-2 ** 15, 2 ** 15, codes.shape, generator=g, dtype=I16).to(DEV)
    for a, b in zip(fe.decode_batch(dp, wild, pn, lfq, output_dtype=out_dtype),
                    fe.decode_batch(dp, wild.long(), pn, lfq, output_dtype=out_dtype)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("out_dtype", [torch.float32, U8], ids=["f32", "u8"])
def test_decode_224_without_fft_decode(fe, pn, lfq, out_dtype):
    x = torch.stack(f32_images(134, [(224, 224)] * 5)).contiguous()
    enc = _fe_mod().BatchEncoder(fe, 5, 224, 224, pn, lfq, device=DEV)
    packed = {k: v.clone() for k, v in enc(x).items()}
    _decode_both(enc, pn, lfq, packed, packed["codes"].to(I16), out_dtype)
    with options(fft_decode=0):
        _decode_both(enc, pn, lfq, packed, packed["codes"].to(I16), out_dtype)


def test_decode_512_without_fft_decode(pn, lfq, packed512):
    enc, packed = packed512
    with options(fft_decode=0):
        _decode_both(enc, pn, lfq, packed, packed["codes"].to(I16), torch.float32)


# ---- 4. round trip: bytes in, int16 codes, bytes out -------------------------------------------
@pytest.mark.parametrize("shape", [(28, 42), (224, 224)], ids=lambda s: "x".join(map(str, s)))
def test_bytes_codes16_bytes(fe, pn, lfq, shape):
    (u,) = byte_images(140 + shape[0], [shape])
    ((dp16, c16),) = fe.encode_batch([u], pn, lfq, uint8_images=True, codes_dtype=I16)
    ((dp64, c64),) = fe.encode_batch([u], pn, lfq, uint8_images=True)
    assert c16.dtype == I16 and torch.equal(c16.long(), c64)
    (a,) = fe.decode_batch(dp16, c16, pn, lfq, output_dtype=U8)
    (b,) = fe.decode_batch(dp64, c64, pn, lfq, output_dtype=U8)
    torch.cuda.synchronize()
    assert a.dtype == U8 and a.shape == u.shape and torch.equal(a, b)


# ---- 5. stores stay in bounds -----------------------------------------------------------------
def _raw_encode16(fe, pn, lfq, img, codes_ptr):
    """dctae_encode_c16 through ctypes on one fp32 image, the codes at address codes_ptr"""
    lib_mod = import_module("dct_autoencoder_amd._lib")
    ops = import_module("dct_autoencoder_amd._ops")
    packing = import_module("dct_autoencoder_amd.packing")
    dev = torch.device(DEV, torch.cuda.current_device())
    ctx = lib_mod.context(dev)
    ptr, S = lib_mod.ptr, fe.max_seq_len
    _, H, W = img.shape
    k = min(fe._tokens(H, W), S)
    desc, _, keep = ops.image_set([img])
    plan = packing.layout([[0]], {0: k})
    arrs = [lib_mod.i32(a) for a in (plan.row, plan.col, plan.k, plan.local_id, plan.row_len)]
    pk = lib_mod.Packing(*[C.cast(a, C.POINTER(C.c_int32)) for a in arrs], 1)
    t = dict(positions=torch.empty((1, S, 2), dtype=I64, device=DEV), channels=torch.empty((1, S), dtype=I64, device=DEV),
             image_ids=torch.empty((1, S), dtype=I64, device=DEV), key_pad=torch.empty((1, S), dtype=torch.bool, device=DEV))
    po = lib_mod.PackedOut16(C.c_void_p(codes_ptr), ptr(t["positions"]), ptr(t["channels"]), ptr(t["image_ids"]),
                             ptr(t["key_pad"]), None, None, None)
    norm = pn.state()
    nc, lc, cfg = norm.c(), lfq.cfg(), fe.params(S).c(S)
    rc = ctx.lib.dctae_encode_c16(ctx.h, C.byref(cfg), C.byref(desc), C.byref(pk), C.byref(nc), C.byref(lc),
                                  C.byref(po), lib_mod.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, (ctx.lib.dctae_last_error(ctx.h) or b"").decode(), t


def _in_bounds(fe, pn, lfq, shape, off, seed):
    (img,) = f32_images(seed, [shape])
    ncb, S = lfq.num_codebooks, fe.max_seq_len
    n = S * ncb
    buf = torch.full((n + 64,), SENTINEL, dtype=I16, device=DEV)
    assert buf.data_ptr() % 16 == 0
    rc, msg, t = _raw_encode16(fe, pn, lfq, img, buf.data_ptr() + 2 * off)
    assert rc == 0, msg
    assert bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all())
    ((dp, want),) = fe.encode_batch([img], pn, lfq, codes_dtype=I16)
    assert bool(t["key_pad"].any())   # the row ends in pads: every element of the slice is written
    assert torch.equal(buf[off:off + n].view(1, S, ncb), want) and torch.equal(t["key_pad"], dp.key_pad_mask)
    assert not bool((buf[off:off + n] == SENTINEL).any())


def test_stores_stay_in_bounds(fe, pn, lfq, lfq28, p5):
    # num_codebooks = 14: 4-byte aligned, and not 8; the other two: 2-byte aligned, and not 4
    _in_bounds(fe, pn, lfq, (434, 512), 2, 150)   # 2,976 of 3,072 slots: k_sort_pack2<512, 6> and k_pad_fill
    _in_bounds(fe, pn, lfq28, (45, 75), 1, 151)
    _in_bounds(*p5, (23, 37), 1, 152)


def test_full_rows_stay_in_bounds(fe, pn, lfq):
    """512^2: the row is full (no pad fill), two codes per store up to the last element"""
    (img,) = f32_images(153, [(512, 512)])
    n = 3072 * 14
    buf = torch.full((n + 64,), SENTINEL, dtype=I16, device=DEV)
    rc, msg, t = _raw_encode16(fe, pn, lfq, img, buf.data_ptr() + 4)
    assert rc == 0, msg
    assert bool((buf[:2] == SENTINEL).all()) and bool((buf[2 + n:] == SENTINEL).all())
    ((_, want),) = fe.encode_batch([img], pn, lfq, codes_dtype=I16)
    assert not bool(t["key_pad"].any()) and torch.equal(buf[2:2 + n].view(1, 3072, 14), want)


def test_misaligned_code_pointer_is_refused(fe, pn, lfq, lfq28):
    (img,) = f32_images(154, [(45, 75)])
    buf = torch.full((3072 * 28 + 64,), SENTINEL, dtype=I16, device=DEV)
    rc, msg, _ = _raw_encode16(fe, pn, lfq, img, buf.data_ptr() + 2)     # 14 codebooks: 2 mod 4
    assert rc == EINVAL and "4-byte aligned" in msg, (rc, msg)
    rc, msg, _ = _raw_encode16(fe, pn, lfq28, img, buf.data_ptr() + 1)   # an odd address
    assert rc == EINVAL and "2-byte aligned" in msg, (rc, msg)
    assert bool((buf == SENTINEL).all())   # nothing was launched


# ---- 6. refusals --------------------------------------------------------------------------------
def test_codebook_dim_16_is_refused(pkg, fe, pn):
    torch.manual_seed(7)
    wide = pkg.LFQ(dim=196, codebook_size=2 ** 16, num_codebooks=12).to(DEV).eval()   # with projections
    assert wide.has_projections and wide.codebook_dim == 16
    imgs = f32_images(160, [(45, 75)])
    with pytest.raises(ValueError, match="codebook_dim"):
        fe.encode_batch(imgs, pn, wide, codes_dtype=I16)
    with pytest.raises(ValueError, match="codebook_dim"):
        _fe_mod().BatchEncoder(fe, 1, 224, 224, pn, wide, device=DEV, codes_dtype=I16)
    with pytest.raises(ValueError, match="codebook_dim"):
        wide.project_codes(torch.zeros((4, 196), device=DEV), codes_dtype=I16)
    ((dp, codes),) = fe.encode_batch(imgs, pn, wide)   # int64 still encodes and decodes
    assert codes.dtype == I64
    fe.decode_batch(dp, codes, pn, wide)
    with pytest.raises(ValueError, match="codebook_dim"):
        fe.decode_batch(dp, codes.to(I16), pn, wide)
    # a 4 x 4 patch with one 16-bit codebook: no projections, the fused encode and decode
    fe4 = pkg.DCTAutoencoderFeatureExtractor(3, 4, 0.0, 8, 8, 192)
    pn4 = pkg.PatchNorm(8, 8, 4, 3).to(DEV)
    pn4.b.data.fill_(0.1)
    pn4.frozen = True
    pn4.eval()
    one = pkg.LFQ(dim=16, codebook_size=2 ** 16, num_codebooks=1).to(DEV).eval()
    small = f32_images(161, [(20, 24)])
    with pytest.raises(ValueError, match="codebook_dim"):
        fe4.encode_batch(small, pn4, one, codes_dtype=I16)
    ((dp4, c4),) = fe4.encode_batch(small, pn4, one)
    with pytest.raises(ValueError, match="codebook_dim"):
        fe4.decode_batch(dp4, c4.to(I16), pn4, one)
    # the C entry refuses on its own, before any launch, and names the limit
    buf = torch.full((192 + 8,), SENTINEL, dtype=I16, device=DEV)
    rc, msg, _ = _raw_encode16(fe4, pn4, one, small[0], buf.data_ptr())
    assert rc == EINVAL and "codebook_dim <= 15" in msg, (rc, msg)
    assert bool((buf == SENTINEL).all())


@pytest.mark.parametrize("bad", [torch.int32, U8, torch.float32], ids=["int32", "uint8", "float32"])
def test_other_code_dtypes_are_refused(fe, pn, lfq, lfq_p, bad):
    imgs = f32_images(162, [(45, 75)])
    with pytest.raises(TypeError):
        fe.encode_batch(imgs, pn, lfq, codes_dtype=bad)
    with pytest.raises(TypeError):
        _fe_mod().BatchEncoder(fe, 1, 224, 224, pn, lfq, device=DEV, codes_dtype=bad)
    with pytest.raises(TypeError):
        lfq_p.project_codes(torch.zeros((4, 196), device=DEV), codes_dtype=bad)


def test_other_code_dtypes_into_the_decode_are_refused(fe, pn, lfq):
    x = torch.stack(f32_images(163, [(224, 224)])).contiguous()
    enc = _fe_mod().BatchEncoder(fe, 1, 224, 224, pn, lfq, device=DEV)
    packed = {k: v.clone() for k, v in enc(x).items()}
    dec = _fe_mod().BatchDecoder(enc, pn, lfq)
    with pytest.raises(TypeError):
        dec(dict(packed, codes=packed["codes"].to(torch.int32)))
    ((dp, codes),) = fe.encode_batch(list(x), pn, lfq)
    with pytest.raises(TypeError):
        fe.decode_batch(dp, codes.to(torch.int32), pn, lfq)
    with pytest.raises(TypeError):
        fe.decode_batch(dp, codes.to(U8), pn, lfq)


# ---- 7. the staged path -------------------------------------------------------------------------
def test_staged_hook_returns_the_requested_dtype(pkg, pn, lfq):
    """An overridden stage hook: the staged path's codes in the requested dtype by a torch conversion,
    equal to the staged int64 codes.  Against the fused codes the staged path is held to the bound
    tests/test_gpu_hooks.py holds it to (its DCT is another kernel: codes inside the guard band may differ)."""
    imgs = f32_images(170, [(28, 60), (45, 75)])

    def staged_fe():
        f = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
        orig = f._transform_image_in
        f._transform_image_in = lambda x: orig(x)
        assert f._staged_in()
        return f

    ((d16, c16),) = staged_fe().encode_batch(imgs, pn, lfq, codes_dtype=I16)
    ((d64, c64),) = staged_fe().encode_batch(imgs, pn, lfq)
    ((df, cf),) = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072).encode_batch(imgs, pn, lfq,
                                                                                         codes_dtype=I16)
    torch.cuda.synchronize()
    assert c16.dtype == I16 and c64.dtype == I64 and torch.equal(c16.long(), c64)
    assert d16.patch_positions.dtype == I64 and torch.equal(d16.patch_positions, d64.patch_positions)
    assert cf.dtype == I16 and torch.equal(d16.key_pad_mask, df.key_pad_mask)
    keep = ~df.key_pad_mask
    assert int((c16[keep] != cf[keep]).sum()) <= 4
