"""The decode straight to uint8 images (include/dctae_u8_out.h).

The rule under test: every byte a byte call writes equals ``byte_from_unit`` of
the fp32 value the fp32 call writes for the same inputs, on every decode path
and under every library option.  ``byte_from_unit`` is the torch expression
``x.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)`` evaluated ON THE CPU on
the fp32 call's output after it is copied to the host
(test_u8_quantise_host.quantise_cpu): that expression is the definition, and
every comparison here is ``torch.equal`` against it.  Nothing is a tolerance.

Decode inputs (built once per case on the CPU, ``case_inputs``):
  patches form   the case's perturbed model output (oracle/decode_cases.py: the
                 target plus 5 % noise), whose images overshoot [0, 1] on both
                 sides at factor 1: no scaling was needed for any case.
  normed form    (P = 14) the same patches through PatchNorm's forward WITHOUT
                 its +-6 clamp, so the inverse inside the decode gives those
                 images back; the tables are the recorded ones times
                 min(1, 1.4 sqrt(H0 W0) / 512) (H0 x W0 the first image): their
                 low-frequency medians are those of 512^2 images, and unscaled
                 they put every pixel of a small image far above 1.
  codes form     (P = 14, 14 x 14 LFQ) the sign bits of the normed patches, the
                 same scaled tables (on the CPU oracle the three 45 x 75 images
                 stay below 1 at sqrt(H0 W0) / 512 and nearly all above 1 at
                 twice that; 1.4 reaches both sides and the inside in every case).
Each test asserts that its fp32 output has values below 0, above 1 and inside
(0, 1), so both clamps and the rounding are exercised.
"""
import ctypes as C
import functools
from importlib import import_module

import pytest
import torch

from oracle import decode_cases as D
from oracle import ref_cpu, rng
from test_options_host import DEFAULTS, EINVAL
from test_u8_quantise_host import quantise_cpu, value_set

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8, F32 = torch.uint8, torch.float32
GUARD, FILL = 64, 0xA5
B45 = "b45x75"   # three 45 x 75 images: 3375 pixels per plane, consecutive image starts alternate in parity
CASE_NAMES = ["sq512x2", "mixed512", "p5", "caps", "zero", B45]


@pytest.fixture(scope="module", autouse=True)
def _package(pkg):
    """the package loaded before any test imports its modules by name"""
    return pkg


def _ops():
    return import_module("dct_autoencoder_amd._ops")


def _lib():
    return import_module("dct_autoencoder_amd._lib")


def _dev():
    return torch.device(DEV, torch.cuda.current_device())


# ---- inputs, on the CPU --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """cfg, batch, patches and, at P = 14, (median, b, normed, codes) of the module docstring; read-only"""
    if name == B45:
        cfg = ref_cpu.FEConfig()
        batch = D.pack([torch.from_numpy(x) for x in rng.synth_images(7100, [(45, 75)] * 3)], cfg)
        g = torch.Generator().manual_seed(7100)
        patches, _ = D.perturb(batch, g)
    else:
        c = D.build(name)
        cfg, batch, patches = c.cfg, c.batch, c.out
    out = {"cfg": cfg, "batch": batch, "patches": patches.float().contiguous()}
    if cfg.patch_size == 14:
        from conftest import golden
        t = golden("patchnorm_ref.npz")
        h0, w0 = (int(v) for v in batch.original_sizes[0])
        s = min(1.0, 1.4 * (h0 * w0) ** 0.5 / 512)
        med = (torch.from_numpy(t["median"])[:, :cfg.max_patch_h, :cfg.max_patch_w] * s).contiguous()
        b = (torch.from_numpy(t["b"])[:, :cfg.max_patch_h, :cfg.max_patch_w] * s).contiguous()
        ch, pos = batch.patch_channels, batch.patch_positions
        std = b[ch, pos[..., 0], pos[..., 1]] * 2 ** 0.5 + 1e-6
        normed = ((out["patches"] - med[ch, pos[..., 0], pos[..., 1]]) / std).contiguous()
        _, idx = ref_cpu.lfq_forward(normed, ref_cpu.LFQConfig())
        out.update(median=med, b=b, normed=normed, codes=idx.long().contiguous())
    return out


def on_device(name):
    """the case's decode arguments on the device: (FEParams, index tensors + sizes, inputs dict)"""
    ci = case_inputs(name)
    cfg, b = ci["cfg"], ci["batch"]
    p = _ops().FEParams(patch_size=cfg.patch_size, max_patch_h=cfg.max_patch_h, max_patch_w=cfg.max_patch_w,
                        max_seq_len=cfg.max_seq_len)
    args = (b.batched_image_ids.to(DEV), b.key_pad_mask.to(DEV), b.patch_positions.to(DEV), b.patch_channels.to(DEV),
            [tuple(int(v) for v in s) for s in b.patch_sizes], [tuple(int(v) for v in s) for s in b.original_sizes])
    t = {k: v.to(DEV) for k, v in ci.items() if isinstance(v, torch.Tensor)}
    return p, args, t


def forms(name):
    """(label, decode keyword arguments) of every input form the case runs in"""
    p, args, t = on_device(name)
    out = [("patches", dict(patches=t["patches"]))]
    if p.patch_size == 14:
        st = _ops().NormState(t["median"], t["b"])
        out.append(("normed", dict(patches=t["normed"], norm=st, normed=True)))
        out.append(("codes", dict(codes=t["codes"], norm=st, lfq=_lib().LFQCfg(14, 14, 1.0))))
    return p, args, out


def assert_exercised(flat, what):
    """the fp32 output reaches below 0, above 1 and inside (0, 1): both clamps and the rounding"""
    f = flat.detach().cpu().flatten()
    assert torch.isfinite(f).all(), what
    assert (f < 0).any() and (f > 1).any() and ((f > 0) & (f < 1)).any(), \
        (what, float(f.min()), float(f.max()))


def assert_bytes(got, want_f32, what):
    assert got.dtype == U8 and got.shape == want_f32.shape, what
    g, w = got.cpu(), quantise_cpu(want_f32)
    bad = (g != w)
    assert not bad.any(), (what, int(bad.sum()), want_f32.cpu()[bad][:4].tolist(), g[bad][:4].tolist(),
                           w[bad][:4].tolist())


def check_decode(p, args, kw, what):
    """the byte decode against the quantised fp32 decode, image by image; returns the byte images"""
    want, flat = _ops().decode(p, *args, return_flat=True, **kw)
    got, gflat = _ops().decode(p, *args, return_flat=True, out_dtype=U8, **kw)
    torch.cuda.synchronize()
    assert_exercised(flat, what)
    assert gflat.dtype == U8 and gflat.numel() == flat.numel() and len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_bytes(g, w, f"{what}, image {i}")
    _ops().check_device_errors(_dev())
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
        try:
            torch.cuda.synchronize()
        finally:
            for k in self.kv:
                _ops().set_option(k, DEFAULTS[k])


def _stage_names(fn):
    """the launch stages (dctae_timing_get names) of the calls fn() makes"""
    ctx = _lib().context(_dev())
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


# ---- 1. the conversion itself ----------------------------------------------------------
@pytest.fixture(scope="module")
def values():
    v = value_set()
    want = quantise_cpu(torch.where(torch.isnan(v), torch.zeros_like(v), v))   # NaN gives 0
    return v.to(DEV), want


def test_f32_to_u8_value_set(values):
    v, want = values
    got = _ops().f32_to_u8(v)
    torch.cuda.synchronize()
    assert got.dtype == U8 and got.shape == v.shape
    bad = got.cpu() != want
    assert not bad.any(), (int(bad.sum()), v.cpu()[bad][:4].tolist(), got.cpu()[bad][:4].tolist(), want[bad][:4].tolist())
    nan = torch.isnan(v).cpu()
    assert nan.any() and torch.all(got.cpu()[nan] == 0)
    x2 = v[: 6 * 255].view(6, 255)   # the shape is kept
    assert torch.equal(_ops().f32_to_u8(x2).cpu(), want[: 6 * 255].view(6, 255))
    with pytest.raises(TypeError):
        _ops().f32_to_u8(got)


@pytest.mark.parametrize("n", [1, 255, 1027, 65536 * 3 + 1])
def test_f32_to_u8_lengths_and_unaligned_outputs(values, n):
    v, want = values
    ctx = _lib().context(_dev())
    for off in (1, 2, 3):
        first = (off - 1) * 300   # other values of the set for every view
        x = v[first:first + n].contiguous()
        buf = torch.full((GUARD + off + n + GUARD,), FILL, dtype=U8, device=DEV)
        assert buf.data_ptr() % 4 == 0
        y = buf.data_ptr() + GUARD + off
        ctx.check(ctx.lib.dctae_f32_to_u8(ctx.h, _lib().ptr(x), n, C.c_void_p(y), _lib().stream_ptr(_dev())),
                  "dctae_f32_to_u8")
        torch.cuda.synchronize()
        h = buf.cpu()
        assert torch.all(h[:GUARD + off] == FILL) and torch.all(h[GUARD + off + n:] == FILL), (n, off)
        assert torch.equal(h[GUARD + off:GUARD + off + n], want[first:first + n]), (n, off)


# ---- 2. bit identity, per path and input form ----------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_bit_identity(name):
    p, args, fs = forms(name)
    assert [f for f, _ in fs] == (["patches", "normed", "codes"] if p.patch_size == 14 else ["patches"])
    for form, kw in fs:
        st = _stage_names(lambda: check_decode(p, args, kw, f"{name}, {form}"))
        assert ("ipt_to_rgb" in st) == (name != "sq512x2"), (name, form, st)   # sq512x2 alone runs the FFT path
    if name == B45:
        sizes = args[5]
        assert len(sizes) == 3 and all(s == (45, 75) for s in sizes) and (3 * 45 * 75) % 2 == 1


# ---- 3. the FFT path's kernel variants -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fft3(max_patch_w=32):
    """three 512 x 512 images (an odd count) as a packed batch with its perturbed patches; with
    max_patch_w < 32 the batch keeps that many tile columns (as tests/test_gpu_parity.py's caps cases)"""
    cfg = ref_cpu.FEConfig(max_patch_w=max_patch_w, max_seq_len=3 * 32 * max_patch_w)
    batch = D.pack([torch.from_numpy(x) for x in rng.synth_images(7200, [(512, 512)] * 3)], cfg)
    patches, _ = D.perturb(batch, torch.Generator().manual_seed(7200))
    return cfg, batch, patches.float().contiguous()


def fft3_args(max_patch_w=32):
    cfg, b, patches = fft3(max_patch_w)
    p = _ops().FEParams(max_patch_w=max_patch_w, max_seq_len=cfg.max_seq_len)
    args = (b.batched_image_ids.to(DEV), b.key_pad_mask.to(DEV), b.patch_positions.to(DEV), b.patch_channels.to(DEV),
            [tuple(int(v) for v in s) for s in b.patch_sizes], [tuple(int(v) for v in s) for s in b.original_sizes])
    return p, args, patches.to(DEV)


@pytest.mark.parametrize("setting", ["default", "dec_cols_kernel=1", "dec_rows_kernel=2", "max_patch_w=24"])
def test_fft_path_kernel_variants(setting):
    """k_idct_rows512<448, true>, <448, false>, k_idct_rows2 by option, k_idct_rows2 by qw != 32"""
    if setting == "max_patch_w=24":
        p, args, patches = fft3_args(24)
        assert int(args[2][..., 1].max()) == 23
        opts = {}
    else:
        p, args, patches = fft3_args()
        opts = {} if setting == "default" else {setting.split("=")[0]: int(setting.split("=")[1])}
    with options(**opts):
        st = _stage_names(lambda: check_decode(p, args, dict(patches=patches), setting))
    assert "idct_rows" in st and "ipt_to_rgb" not in st, st


# ---- 4. stores stay in bounds ---------------------------------------------------------------
def _guarded_table(p, args):
    """the batch's DecodeTable with GUARD bytes before and after every image, the buffer length"""
    table = _ops().decode_table(p, *args)
    offs, total = [], 0
    for i in range(table.n_img):
        offs.append(total + GUARD)
        total += GUARD + 3 * table.hw[2 * i] * table.hw[2 * i + 1]
    _set_offsets(table, offs)
    return table, total + GUARD


def _set_offsets(table, offs):
    table.offs = list(offs)
    table.keep[2] = _lib().i64(offs)
    c = list(table._c)
    c[4] = C.cast(table.keep[2], C.POINTER(C.c_int64))
    table._c = tuple(c)


def _raw_decode(p, table, patches, rgb_ptr):
    """dctae_decode_u8 from patches through ctypes with the output at address rgb_ptr: (rc, message)"""
    ctx = _lib().context(_dev())
    ptr = _lib().ptr
    rc = ctx.lib.dctae_decode_u8(ctx.h, C.byref(p.c(table.S)), table.R, *table.c_args(), ptr(table.ids),
                                 ptr(table.key_pad), ptr(table.pos), ptr(table.ch), None, None, None, ptr(patches),
                                 C.c_void_p(rgb_ptr), _lib().stream_ptr(_dev()))
    torch.cuda.synchronize()
    return rc, (ctx.lib.dctae_last_error(ctx.h) or b"").decode()


@pytest.mark.parametrize("which", ["fft", B45])
def test_stores_stay_in_bounds(which):
    if which == "fft":
        p, args, patches = fft3_args()
    else:
        p, args, t = on_device(B45)
        patches = t["patches"]
    want = _ops().decode(p, *args, patches=patches)
    table, n = _guarded_table(p, args)
    buf = torch.full((n,), FILL, dtype=U8, device=DEV)
    rc, msg = _raw_decode(p, table, patches, buf.data_ptr())
    assert rc == 0, msg
    h, mask = buf.cpu(), torch.ones(n, dtype=torch.bool)
    for i, (img, w) in enumerate(zip(table.images(buf), want)):
        assert_bytes(img, w, f"{which}, image {i}")
        mask[table.offs[i]:table.offs[i] + w.numel()] = False
    assert int(mask.sum()) == GUARD * (table.n_img + 1)
    assert torch.all(h[mask] == FILL), f"{which}: {int((h[mask] != FILL).sum())} guard bytes written"
    if which == B45:
        assert {o % 2 for o in table.offs} == {0, 1}


# ---- 5. refusals ---------------------------------------------------------------------------
def test_refusals():
    p, args, patches = fft3_args()
    want = _ops().decode(p, *args, patches=patches)
    table = _ops().decode_table(p, *args)
    buf = torch.full((table.total + 8,), FILL, dtype=U8, device=DEV)
    assert buf.data_ptr() % 4 == 0
    rc, msg = _raw_decode(p, table, patches, buf.data_ptr() + 1)
    assert rc == EINVAL and "image 0" in msg and "4-byte aligned" in msg, (rc, msg)
    assert torch.all(buf == FILL)   # refused before any launch
    rc, msg = _raw_decode(p, table, patches, buf.data_ptr())
    assert rc == 0, msg
    for i, (img, w) in enumerate(zip(table.images(buf[:table.total]), want)):
        assert_bytes(img, w, f"aligned call after the refusal, image {i}")
    # one image's offset off by two: the refusal names that image
    offs = list(table.offs)
    _set_offsets(table, [offs[0], offs[1] + 2, offs[2] + 4])
    rc, msg = _raw_decode(p, table, patches, buf.data_ptr())
    assert rc == EINVAL and "image 1" in msg and "4-byte aligned" in msg, (rc, msg)
    # on the per-pixel row kernel the same placement is legal (its own fp32 output is the reference:
    # another kernel's last bits differ, and with them a few bytes at a rounding boundary)
    with options(dec_rows_kernel=2):
        buf.fill_(FILL)
        _set_offsets(table, offs)
        want2 = _ops().decode(p, *args, patches=patches)
        rc, msg = _raw_decode(p, table, patches, buf.data_ptr() + 1)
        assert rc == 0, msg
        for i, (img, w) in enumerate(zip(table.images(buf[1:1 + table.total]), want2)):
            assert_bytes(img, w, f"dec_rows_kernel = 2 at base + 1, image {i}")
    rc, msg = _raw_decode(p, table, patches, None)
    assert rc == EINVAL and "decode descriptor" in msg, (rc, msg)
    _set_offsets(table, [offs[0], -4, offs[2]])
    rc, msg = _raw_decode(p, table, patches, buf.data_ptr())
    assert rc == EINVAL and "negative image offset" in msg, (rc, msg)
    _ops().check_device_errors(_dev())


# ---- 6. bytes in, bytes out -------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(28, 42), (224, 224)])
def test_bytes_in_bytes_out(pkg, shape):
    """both sides multiples of 14 and the whole spectrum kept: the fp32 round trip is within 1e-5
    (test_gpu_parity.py) and the nearest rounding boundary 1 / 510 away, so the bytes come back exactly"""
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
    g = torch.Generator().manual_seed(31 + shape[0])
    u = torch.randint(0, 256, (3, *shape), generator=g, dtype=U8)
    u[:, shape[0] // 2, :] = (torch.arange(shape[1]) % 256).to(U8)
    ((dp, _),) = fe.encode_batch([u.to(DEV)], None, None, return_raw=True, uint8_images=True)
    assert int((~dp.key_pad_mask).sum()) == 3 * (shape[0] // 14) * (shape[1] // 14)   # every token kept
    (img,) = fe.postprocess(dp, output_dtype=U8)
    torch.cuda.synchronize()
    assert img.dtype == U8 and img.shape == u.shape
    assert torch.equal(img.cpu(), u), int((img.cpu() != u).sum())


# ---- 7. the Python surface -----------------------------------------------------------------
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


@pytest.fixture(scope="module")
def images512():
    return torch.stack([torch.from_numpy(x) for x in rng.synth_images(7300, [(512, 512)] * 4)]).contiguous().to(DEV)


@pytest.mark.parametrize("form", ["codes", "proj_normed", "proj_inverse"])
def test_batch_decoder(pkg, pn, lfq, lfq_p, images512, form):
    fe_mod = import_module("dct_autoencoder_amd.feature_extraction")
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
    q = lfq if form == "codes" else lfq_p
    enc = fe_mod.BatchEncoder(fe, 4, 512, 512, pn, q, device=DEV)
    packed = enc(images512)
    df, d8 = fe_mod.BatchDecoder(enc, pn, q), fe_mod.BatchDecoder(enc, pn, q, output_dtype=U8)
    assert df.proj == d8.proj == (form != "codes")
    df.normed_decode = d8.normed_decode = form != "proj_inverse"
    want = df(packed).clone()
    got = d8(packed).clone()
    again = d8(packed)
    torch.cuda.synchronize()
    assert got.dtype == U8 and got.shape == (4, 3, 512, 512) and d8.out.dtype == U8
    assert_bytes(got, want, form)
    assert torch.equal(again, got), "two identical byte calls"
    f = want.cpu()
    assert (f <= 0).any() or (f >= 1).any()   # a reconstruction from sign bits: the clamps are reached


def test_decode_batch_and_postprocess(pkg, pn, lfq, lfq_p):
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
    imgs = [torch.from_numpy(x).to(DEV) for x in rng.synth_images(7400, [(512, 512), (100, 77), (224, 224)])]
    for q in (lfq, lfq_p):
        ((dp, codes),) = fe.encode_batch(imgs, pn, q)
        want = fe.decode_batch(dp, codes, pn, q)
        got = fe.decode_batch(dp, codes, pn, q, output_dtype=U8)
        again = fe.decode_batch(dp, codes, pn, q, output_dtype=U8)
        torch.cuda.synchronize()
        assert len(got) == len(want) == 3
        for i, (g, w, a) in enumerate(zip(got, want, again)):
            assert_bytes(g, w, f"decode_batch image {i}")
            assert torch.equal(a, g)
    # postprocess: patches that require grad take the no-grad path for bytes
    ((dp, _),) = fe.encode_batch(imgs, None, None, return_raw=True)
    want = fe.postprocess(dp)
    dp.patches = dp.patches.clone().requires_grad_(True)
    assert fe.postprocess(dp)[0].grad_fn is not None
    got = fe.postprocess(dp, output_dtype=U8)
    torch.cuda.synchronize()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.grad_fn is None and not g.requires_grad
        assert_bytes(g, w, f"postprocess image {i}")


def test_staged_hook_returns_bytes(pkg, pn, lfq):
    imgs = [torch.from_numpy(x).to(DEV) for x in rng.synth_images(7500, [(28, 60), (45, 75)])]

    def staged_fe():
        f = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
        seen, orig = [], f._transform_image_out

        def hook(x):
            seen.append(x.dtype)
            return orig(x)

        f._transform_image_out = hook
        assert f._staged_out()
        return f, seen

    fe, seen = staged_fe()
    ((dp, codes),) = fe.encode_batch(imgs, pn, lfq)
    want = fe.decode_batch(dp, codes, pn, lfq)
    got = fe.decode_batch(dp, codes, pn, lfq, output_dtype=U8)
    torch.cuda.synchronize()
    assert len(seen) == 4 and all(d == F32 for d in seen)   # the stages run in fp32 either way
    for i, (g, w) in enumerate(zip(got, want)):
        assert_bytes(g, w, f"staged image {i}")


def test_other_dtypes_are_refused(pkg, pn, lfq):
    fe_mod = import_module("dct_autoencoder_amd.feature_extraction")
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
    imgs = [torch.from_numpy(x).to(DEV) for x in rng.synth_images(7600, [(28, 60)])]
    ((dp, codes),) = fe.encode_batch(imgs, pn, lfq, return_raw=True)
    enc = fe_mod.BatchEncoder(fe, 1, 28, 60, pn, lfq, device=DEV)
    for bad in (torch.float16, torch.int8):
        with pytest.raises(TypeError):
            fe.postprocess(dp, output_dtype=bad)
        with pytest.raises(TypeError):
            fe.decode_batch(dp, codes, pn, lfq, output_dtype=bad)
        with pytest.raises(TypeError):
            fe_mod.BatchDecoder(enc, pn, lfq, output_dtype=bad)
        with pytest.raises(TypeError):
            _ops().decode(fe.params(dp.patches.shape[1]), dp.batched_image_ids, dp.key_pad_mask, dp.patch_positions,
                          dp.patch_channels, dp.patch_sizes, dp.original_sizes, patches=dp.patches, out_dtype=bad)
