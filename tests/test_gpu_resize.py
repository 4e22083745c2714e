"""The antialiased resize on the GPU (include/dctae_resize.h,
dct_autoencoder_amd.resize) and the dataset crop in front of the encode.
Run on an MI355X: pytest -m gpu tests/test_gpu_resize.py

The reference of every value is tests/resize_mirror.py, the numpy float32
mirror of csrc/dctae_resize_math.h: the kernel must equal it bit for bit, for
fp32 and for byte images.  The tolerance against torch's float64 interpolate
is the host test's (4 x torch's own fp32 deviation, floor 2^-20).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import resize_mirror as mirror
from conftest import golden
from test_resize_host import HEADER_SHAPES, image, tolerance

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# the mirror's shapes; several tiles on both axes with ragged edges; two rows of the size table; and two
# whose horizontal windows span more source columns than one staged piece holds (weights computed
# in place at 667 taps, and from the table at 13)
SHAPES = HEADER_SHAPES + [((300, 500), (97, 161)), ((769, 100), (761, 99)), ((4000, 13), (615, 2)),
                          ((7, 1000), (7, 3)), ((40, 1500), (20, 250))]
GUARD = 256   # floats of NaN before, between and after the output images


@functools.lru_cache(maxsize=None)
def case(shape, size, u8):
    """(input (3, h, w) numpy, mirror result (3, oh, ow)), computed once"""
    x = np.stack([image(shape, 20 + c, u8) for c in range(3)])
    want = mirror.resize(x, *size)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def unit(u8):
    """u8.float() / 255 with the CPU's correctly rounded division (torch's GPU division by a
    scalar multiplies by the reciprocal instead), back on the device"""
    return (u8.cpu().float() / 255).to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def abi_resize(images, sizes, out=None, check=True):
    """dctae_resize_aa / _u8 through ctypes into a NaN-filled buffer with guard
    floats around every output image; returns (rc, views, context).  The guards
    must still be NaN afterwards and no NaN may be left inside the views."""
    from dct_autoencoder_amd import _lib
    ctx = _lib.context(DEV)
    u8 = images[0].dtype == torch.uint8
    ptrs = [im.data_ptr() for im in images]
    base = min(ptrs)
    in_off = _lib.i64([(p - base) // (1 if u8 else 4) for p in ptrs])
    in_hw = _lib.i32([v for im in images for v in im.shape[1:]])
    desc = (_lib.ImagesU8 if u8 else _lib.Images)(C.c_void_p(base), C.cast(in_off, C.POINTER(C.c_int64)),
                                                  C.cast(in_hw, C.POINTER(C.c_int32)), len(images))
    offs, total = [], GUARD
    for oh, ow in sizes:
        offs.append(total)
        total += 3 * oh * ow + GUARD
    if out is None:
        out = torch.full((total,), float("nan"), dtype=torch.float32, device=DEV)
    out_off = _lib.i64(offs)
    out_hw = _lib.i32([v for s in sizes for v in s])
    odesc = _lib.ImagesOut(_lib.ptr(out), C.cast(out_off, C.POINTER(C.c_int64)), C.cast(out_hw, C.POINTER(C.c_int32)),
                           len(sizes))
    fn = ctx.lib.dctae_resize_aa_u8 if u8 else ctx.lib.dctae_resize_aa
    rc = fn(ctx.h, C.byref(desc), C.byref(odesc), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    views = [out[o:o + 3 * oh * ow].view(3, oh, ow) for o, (oh, ow) in zip(offs, sizes)]
    if check and rc == 0:
        inside = torch.zeros(total, dtype=torch.bool, device=DEV)
        for o, (oh, ow) in zip(offs, sizes):
            inside[o:o + 3 * oh * ow] = True
        assert torch.isnan(out[~inside]).all(), "the call wrote outside its output images"
        assert not torch.isnan(out[inside]).any(), "an output pixel was left unwritten"
    return rc, views, ctx


# ---- against the mirror ---------------------------------------------------------

@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("shape,size", SHAPES)
def test_gpu_equals_mirror(pkg, shape, size, u8):
    x, want = case(shape, size, u8)
    rc, (got,), _ = abi_resize([dev(x)], [size])
    assert rc == 0
    got = got.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f"{int((got != want).sum())} of {got.size} pixels differ from the mirror, max {np.abs(got - want).max():.3e}"


def test_python_api_equals_mirror(pkg):
    from dct_autoencoder_amd import resize
    x, want = case((300, 500), (97, 161), False)
    (got,) = resize.resize_antialias([dev(x)], [(97, 161)])
    assert got.dtype == torch.float32 and got.shape == (3, 97, 161)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


RAGGED = [((37, 53), (9, 13)), ((17, 19), (40, 23)), ((64, 64), (64, 64)), ((300, 500), (97, 161)),
          ((1000, 7), (3, 7)), ((64, 64), (64, 31)), ((1, 1), (4, 3))]


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_poisoned_outputs_and_ragged_call(pkg, u8):
    """one call over the mixed list: nothing unwritten, nothing outside the
    views, and every image bit-identical to its own call"""
    xs = [dev(np.stack([image(s, 40 + c, u8) for c in range(3)])) for s, _ in RAGGED]
    sizes = [z for _, z in RAGGED]
    rc, together, _ = abi_resize(xs, sizes)
    assert rc == 0
    for x, z, t in zip(xs, sizes, together):
        rc, (alone,), _ = abi_resize([x], [z])
        assert rc == 0 and same_bits(alone, t), (tuple(x.shape), z)
    # the equal-size image passes through bit for bit (as the fp32 values the bytes mean)
    src = unit(xs[2]) if u8 else xs[2]
    assert same_bits(together[2], src)
    # 64 -> 31 columns with the rows unchanged: the horizontal pass alone
    one_axis = mirror.resize_axis(mirror.unit_from_byte(xs[5].cpu().numpy()) if u8 else xs[5].cpu().numpy(), 31, -1)
    assert np.array_equal(together[5].cpu().numpy().view(np.uint32), one_axis.view(np.uint32))


@pytest.mark.parametrize("shape,size", SHAPES)
def test_tolerance_against_torch_float64(pkg, shape, size):
    x, _ = case(shape, size, False)
    rc, (got,), _ = abi_resize([dev(x)], [size])
    assert rc == 0
    got = got.cpu().numpy().astype(np.float64)
    for c in range(3):
        bound, dev32, t64 = tolerance(x[c], size)
        err = float(np.abs(got[c] - t64).max())
        print(f"{shape} -> {size} plane {c}: GPU {err:.3e}, torch fp32 {dev32:.3e}, bound {bound:.3e}")
        assert err <= bound


def test_unaligned_bytes(pkg):
    """byte images at byte offsets 1, 2 and 3 of one buffer, widths no multiple of 4"""
    shapes = [((37, 53), (9, 13)), ((17, 19), (40, 23)), ((30, 41), (11, 17))]
    buf = torch.zeros(8 + sum(3 * h * w + 8 for (h, w), _ in shapes), dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 4 == 0
    xs, at = [], 0
    for k, ((h, w), _) in enumerate(shapes):
        at = (at + 3) // 4 * 4 + (k + 1)
        v = buf[at:at + 3 * h * w].view(3, h, w)
        v.copy_(dev(np.stack([image((h, w), 60 + c, True) for c in range(3)])))
        assert v.data_ptr() % 4 == k + 1
        xs.append(v)
        at += 3 * h * w
    rc, got, _ = abi_resize(xs, [z for _, z in shapes])
    assert rc == 0
    for x, (_, z), g in zip(xs, shapes, got):
        want = mirror.resize(x.cpu().numpy(), *z)
        assert np.array_equal(g.cpu().numpy().view(np.uint32), want.view(np.uint32)), tuple(x.shape)


def test_repeatable(pkg):
    from dct_autoencoder_amd import resize
    xs = [dev(case(s, z, False)[0]) for s, z in SHAPES[:6]]
    sizes = [z for _, z in SHAPES[:6]]
    a = resize.resize_antialias(xs, sizes)
    b = resize.resize_antialias(xs, sizes)
    assert all(same_bits(u, v) for u, v in zip(a, b))
    assert len({t.untyped_storage().data_ptr() for t in a}) == 1   # one allocation, views of it


def test_byte_contract(pkg):
    """resize(u8) == resize(u8.float() / 255), the size-preserving image of a mixed list included"""
    from dct_autoencoder_amd import resize
    shapes = [((37, 53), (9, 13)), ((64, 64), (64, 64)), ((300, 500), (97, 161)), ((17, 19), (40, 23))]
    u = [dev(np.stack([image(s, 70 + c, True) for c in range(3)])) for s, _ in shapes]
    f = [unit(t) for t in u]
    sizes = [z for _, z in shapes]
    got_u, got_f = resize.resize_antialias(u, sizes), resize.resize_antialias(f, sizes)
    assert all(g.dtype == torch.float32 for g in got_u)
    assert all(same_bits(a, b) for a, b in zip(got_u, got_f))
    assert got_f[1] is f[1]                      # fp32 of matching size: returned as it is
    assert same_bits(got_u[1], f[1])             # bytes of matching size: exactly u8 / 255


# ---- the dataset crop -------------------------------------------------------------

CROP_SIZES = [(769, 100), (100, 769), (60, 80), (770, 768)]
CROP_WANT = [(761, 99), (99, 761), (60, 80), (767, 766)]


@pytest.fixture(scope="module")
def crop_setup(pkg):
    tabs = golden("patchnorm_ref.npz")
    pn = pkg.PatchNorm(32, 32, 14, 3).to(DEV)
    pn.median.data.copy_(torch.from_numpy(tabs["median"]))
    pn.b.data.copy_(torch.from_numpy(tabs["b"]))
    pn.frozen = True
    pn.eval()
    lfq = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).to(DEV).eval()
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
    u = [dev(np.stack([image(s, 80 + c, True) for c in range(3)])) for s in CROP_SIZES]
    return fe, pn, lfq, u


def encoded(outs):
    ts = []
    for dp, codes in outs:
        ts += [dp.patches, dp.key_pad_mask, dp.batched_image_ids, dp.patch_channels, dp.patch_positions, codes]
        ts += [torch.tensor(dp.patch_sizes), torch.tensor(dp.original_sizes)]
    return ts


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_dataset_crop(pkg, crop_setup, u8):
    fe, pn, lfq, u = crop_setup
    images = u if u8 else [unit(t) for t in u]
    cropped = fe.dataset_crop(images)
    assert [tuple(t.shape[1:]) for t in cropped] == CROP_WANT
    assert all(t.dtype == torch.float32 for t in cropped)
    if u8:
        assert same_bits(cropped[2], unit(u[2]))   # the small image: exactly u8 / 255
    else:
        assert cropped[2] is images[2]                     # returned as it is
    assert same_bits(cropped[0], fe.dataset_crop([unit(t) for t in u])[0])
    # within max_size: untouched, bytes stay bytes
    small = [images[2]]
    back = fe.dataset_crop(small)
    assert len(back) == 1 and back[0] is small[0]
    assert fe.dataset_crop(images, max_size=4096)[3] is images[3]

    a = fe.encode_batch(images, pn, lfq, return_patches=True, dataset_crop=True, uint8_images=u8)
    b = fe.encode_batch(cropped, pn, lfq, return_patches=True)
    assert len(a) == len(b) and all(same_bits(s, t) for s, t in zip(encoded(a), encoded(b)))
    assert sorted(tuple(z) for dp, _ in a for z in dp.original_sizes) == sorted(CROP_WANT)

    pa = fe.preprocess_many(images, dataset_crop=True)
    pb = fe.preprocess_many(cropped)
    for s, t in zip(pa, pb):
        assert s["original_sizes"] == t["original_sizes"] and s["patch_sizes"] == t["patch_sizes"]
        assert all(same_bits(s[k], t[k]) for k in ("patches", "positions", "channels"))

    # nothing to resize: the option changes nothing, and the default is the existing call
    c = fe.encode_batch(small, pn, lfq, return_patches=True, uint8_images=u8)
    for flag in (False, True):
        d = fe.encode_batch(small, pn, lfq, return_patches=True, uint8_images=u8, dataset_crop=flag)
        assert all(same_bits(s, t) for s, t in zip(encoded(c), encoded(d)))


def test_dataset_crop_reaches_the_stage_hooks(pkg, crop_setup):
    fe0, pn, lfq, u = crop_setup
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
    seen = []
    plain = fe._transform_image_in

    def hook(x):
        seen.append((x.dtype, tuple(x.shape[1:])))
        return plain(x)
    fe._transform_image_in = hook
    fe.encode_batch(u[:3], pn, lfq, dataset_crop=True, uint8_images=True)
    assert seen == [(torch.float32, z) for z in CROP_WANT[:3]]


# ---- streams ------------------------------------------------------------------------

def test_resize_is_ordered_across_streams(pkg):
    """the ordering harness of tests/test_gpu_streams.py (its Rig, unchanged) for
    dctae_resize_aa against dctae_lfq_project_out, in both roles"""
    from dct_autoencoder_amd import _lib
    from test_gpu_streams import Rig
    torch.cuda.set_device(DEV)
    ctx = _lib.context(DEV)
    rig = Rig()
    keep = []
    gen = torch.Generator().manual_seed(3)
    pcfg = _lib.LFQCfg(13, 16, 1.0)
    n = 300
    idx = torch.randint(0, 2 ** 13, (n, 16), generator=gen).to(DEV)
    w_out = (torch.randn(196, 208, generator=gen) / 14).to(DEV)
    b_out = (torch.randn(196, generator=gen) * 0.1).to(DEV)
    xout = torch.empty((n, 196), dtype=torch.float32, device=DEV)

    def partner(stream):
        ctx.check(ctx.lib.dctae_lfq_project_out(ctx.h, C.byref(pcfg), _lib.ptr(idx), n, 196, _lib.ptr(w_out),
                                                _lib.ptr(b_out), _lib.ptr(xout), C.c_void_p(stream.cuda_stream)),
                  "dctae_lfq_project_out")

    x = dev(case((300, 500), (97, 161), False)[0])
    y = torch.empty(3 * 97 * 161, dtype=torch.float32, device=DEV)
    in_off, in_hw, out_off, out_hw = _lib.i64([0]), _lib.i32([300, 500]), _lib.i64([0]), _lib.i32([97, 161])
    desc = _lib.Images(_lib.ptr(x), C.cast(in_off, C.POINTER(C.c_int64)), C.cast(in_hw, C.POINTER(C.c_int32)), 1)
    odesc = _lib.ImagesOut(_lib.ptr(y), C.cast(out_off, C.POINTER(C.c_int64)), C.cast(out_hw, C.POINTER(C.c_int32)), 1)
    keep.extend([in_off, in_hw, out_off, out_hw, desc, odesc])

    def resize_call(stream):
        ctx.check(ctx.lib.dctae_resize_aa(ctx.h, C.byref(desc), C.byref(odesc), C.c_void_p(stream.cuda_stream)),
                  "dctae_resize_aa")

    for first, second, what in ((resize_call, partner, "resize on A, partner on B"),
                                (partner, resize_call, "partner on A, resize on B")):
        conclusive, ordered, lag = rig.run(first, second)
        print(f"{what}: conclusive {conclusive}, ordered {ordered}, eA behind B {lag:.3f} ms")
        assert conclusive, f"{what}: the host was held up behind the blocker: inconclusive"
        assert ordered, f"{what}: the call on stream B finished while the call on stream A had not"


# ---- errors ---------------------------------------------------------------------------

def test_errors(pkg):
    from dct_autoencoder_amd import resize
    f = torch.zeros(3, 8, 8, device=DEV)
    with pytest.raises(TypeError):
        resize.resize_antialias([f, f.to(torch.uint8)], [(4, 4), (4, 4)])
    with pytest.raises(TypeError):
        resize.resize_antialias([f.double()], [(4, 4)])
    with pytest.raises(ValueError):
        resize.resize_antialias([torch.zeros(1, 8, 8, device=DEV)], [(4, 4)])
    with pytest.raises(ValueError):
        resize.resize_antialias([f], [(4, 0)])
    with pytest.raises(TypeError):
        resize.dataset_crop([f.half()], 4)

    # through the raw ABI: the second image's output lies inside the first input image
    buf = torch.zeros(3 * 16 * 16 + 3 * 8 * 8 + 64, dtype=torch.float32, device=DEV)
    a = buf[:3 * 16 * 16].view(3, 16, 16)
    b = buf[3 * 16 * 16:3 * 16 * 16 + 3 * 8 * 8].view(3, 8, 8)
    out = buf[32:]   # output image 0 at +GUARD floats of it: inside a
    rc, _, ctx = abi_resize([a, b], [(4, 4), (4, 4)], out=out, check=False)
    assert rc == -1   # DCTAE_EINVAL
    msg = ctx.lib.dctae_last_error(ctx.h).decode()
    assert "overlaps" in msg and "output image 0" in msg and "input image 0" in msg, msg
    assert not buf.any()   # nothing ran
    # a side <= 0 and a differing n_img name the image / the counts
    from dct_autoencoder_amd import _lib
    off, hw, ohw = _lib.i64([0]), _lib.i32([16, 16]), _lib.i32([0, 4])
    fresh = torch.empty(64, dtype=torch.float32, device=DEV)
    desc = _lib.Images(_lib.ptr(a), C.cast(off, C.POINTER(C.c_int64)), C.cast(hw, C.POINTER(C.c_int32)), 1)
    for n_out, want in ((1, "image 0 has a side <= 0"), (2, "1 input images, 2 output images")):
        odesc = _lib.ImagesOut(_lib.ptr(fresh), C.cast(off, C.POINTER(C.c_int64)), C.cast(ohw, C.POINTER(C.c_int32)),
                               n_out)
        rc = ctx.lib.dctae_resize_aa(ctx.h, C.byref(desc), C.byref(odesc), None)
        assert rc == -1 and want in ctx.lib.dctae_last_error(ctx.h).decode()
