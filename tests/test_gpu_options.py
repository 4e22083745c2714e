"""The encode plan cache follows the options: after dctae_set_option flips a
plan-shaping switch on a live context, the next encode equals, bit for bit,
the encode of a fresh context created with the switch already set (a stale
cached plan would repeat the previous result), and flipping back restores the
first result.  Also: dctae_set_option's status codes over the whole table."""
import contextlib
import ctypes as C
import threading
from importlib import import_module

import pytest
import torch

from oracle import rng
from test_options_host import BYTES, DEFAULTS, EINVAL, EUNSUP, LEGAL, PLAN, PROFILING

pytestmark = pytest.mark.gpu
DEV = "cuda"
# one image per route: even 7-smooth sides without a compile-time kernel
# (fft_generic, fft, fft_spec), odd 7-smooth sides (fft_odd with fft_generic),
# prime sides >= 32 (the GEMM DCT by default: bluestein, gemm_x3, gemm_h2,
# tperm, rows_fused, xcd_order)
SIZES = [(64, 96), (45, 75), (37, 53)]
BIT_IDENTICAL = {"tperm", "xcd_order", "rows_fused"}   # documented so; rows_fused: for [0, 1] RGB
FIELDS = ("patches", "key_pad_mask", "batched_image_ids", "patch_channels", "patch_positions")


def _flipped(key):
    if key in BYTES:
        return 2 ** 20
    if key in LEGAL:
        return min(LEGAL[key][0] - {DEFAULTS[key]})
    return 1 - DEFAULTS[key]


# (switches set on both contexts beforehand, the option that is flipped): every
# plan-shaping option a shipped build accepts from the defaults, and the FFT
# switches once more where the generic kernels take the smooth sides, so that
# the flip changes the launches of the first two images
CASES = [({}, k) for k in sorted(PLAN - PROFILING)] + \
        [({"fft_generic": 1}, "fft"), ({"fft_generic": 1}, "fft_spec"), ({"fft_generic": 1}, "fft_odd")]
# a launch stage (dctae_timing_get name) that the flip from the defaults must add to the call
ADDS_STAGE = {"bluestein": "bs_rows", "fft_generic": "fft_rows", "rows_fused": "rgb_to_ipt"}


@contextlib.contextmanager
def _context(lib_mod):
    """A new dctae_ctx in place of this thread's shared one for the block."""
    key = (torch.cuda.current_device(), threading.get_ident())
    shared = lib_mod._ctx_by_key.get(key)
    ctx = lib_mod.Context(key[0])
    lib_mod._ctx_by_key[key] = ctx
    try:
        yield ctx
    finally:
        torch.cuda.synchronize()
        if shared is None:
            del lib_mod._ctx_by_key[key]
        else:
            lib_mod._ctx_by_key[key] = shared


def _set(ctx, key, value):
    ctx.check(ctx.lib.dctae_set_option(ctx.h, key.encode(), int(value)), f"dctae_set_option({key})")


def _stages(ctx):
    """{stage name: launches} since the last call, from the library's timing."""
    ctx.check(ctx.lib.dctae_timing_collect(ctx.h))
    out, name, ms, n = {}, C.c_char_p(), C.c_double(), C.c_int64()
    i = 0
    while ctx.lib.dctae_timing_get(ctx.h, i, C.byref(name), C.byref(ms), C.byref(n)) == 0:
        out[name.value.decode()] = n.value
        i += 1
    ctx.check(ctx.lib.dctae_timing_reset(ctx.h))
    return out


@pytest.fixture(scope="module")
def setup(pkg, ref_tables):
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
    pn = pkg.PatchNorm(32, 32, 14, 3).to(DEV)
    pn.median.data.copy_(ref_tables.median)
    pn.b.data.copy_(ref_tables.b)
    pn.n.data.copy_(ref_tables.n)
    pn.frozen = True
    lfq = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).to(DEV).eval()
    imgs = [torch.from_numpy(x).to(DEV) for x in rng.synth_images(53, SIZES)]   # [0, 1) RGB
    assert all(0.0 <= float(x.min()) and float(x.max()) <= 1.0 for x in imgs)
    lib_mod = import_module("dct_autoencoder_amd._lib")

    def encode(ctx):
        ((dp, codes),) = fe.encode_batch(imgs, pn.eval(), lfq, return_raw=True)
        torch.cuda.synchronize()
        return [codes.cpu()] + [getattr(dp, f).cpu() for f in FIELDS], _stages(ctx)

    return lib_mod, encode


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def live(setup):
    """The one context every case flips its option on."""
    lib_mod, _ = setup
    with _context(lib_mod) as ctx:
        ctx.check(ctx.lib.dctae_set_timing(ctx.h, 1))
        yield ctx


@pytest.fixture(scope="module")
def default_out(setup, live):
    _, encode = setup
    return encode(live)[0]


@pytest.mark.parametrize("base,key", CASES, ids=[("+".join(b) + ":" if b else "") + k for b, k in CASES])
def test_flipped_option_is_not_served_a_stale_plan(setup, live, default_out, base, key):
    lib_mod, encode = setup
    value = _flipped(key)
    for k, v in base.items():
        _set(live, k, v)
    try:
        first, first_stages = encode(live)
        _set(live, key, value)
        try:
            second, second_stages = encode(live)
        finally:
            _set(live, key, DEFAULTS[key])
        third, third_stages = encode(live)
    finally:
        for k in base:
            _set(live, k, DEFAULTS[k])
    with _context(lib_mod) as fresh:
        fresh.check(fresh.lib.dctae_set_timing(fresh.h, 1))
        for k, v in list(base.items()) + [(key, value)]:
            _set(fresh, k, v)
        want, want_stages = encode(fresh)
    print(f"[{base} {key}={value}] stages {first_stages} -> {second_stages}")
    assert _same(second, want), "the flipped option's encode differs from a fresh context's"
    assert second_stages == want_stages
    assert _same(third, first), "flipping back does not restore the first result"
    assert third_stages == first_stages
    if not base:
        if key in ADDS_STAGE:
            assert ADDS_STAGE[key] in second_stages and ADDS_STAGE[key] not in first_stages
        assert _same(first, default_out)
        if key in BIT_IDENTICAL:
            assert _same(second, default_out), "documented as bit-identical to the default"


@pytest.mark.parametrize("key", ["cols_dma", "gemm_dma"])
def test_launch_time_switches_bit_identical(setup, live, default_out, key):
    """The two documented bit-identical switches that are read at launch (not plan-shaping)."""
    _, encode = setup
    _set(live, key, 0)
    try:
        out, _ = encode(live)
    finally:
        _set(live, key, 1)
    assert _same(out, default_out)
    assert _same(encode(live)[0], default_out)


def test_set_option_status_over_the_table(setup):
    lib_mod, _ = setup
    with _context(lib_mod) as ctx:
        def call(key, value):
            rc = ctx.lib.dctae_set_option(ctx.h, key.encode(), int(value))
            return rc, ctx.lib.dctae_last_error(ctx.h).decode()

        for key, default in DEFAULTS.items():
            if key in PROFILING:   # the suite runs the shipped library
                assert call(key, 1) == (EUNSUP, f"option {key} exists only in a profiling build (make PROFILING=1)")
                continue
            assert call(key, _flipped(key))[0] == 0, key
            assert call(key, default)[0] == 0, key
            bad = LEGAL[key][1] if key in LEGAL else 2 ** 20 - 1 if key in BYTES else None
            if bad is not None:
                assert call(key, bad) == (EINVAL, f"unknown option or bad value: {key}")
        assert call("no_such_option", 1) == (EINVAL, "unknown option or bad value: no_such_option")
        assert ctx.lib.dctae_set_option(ctx.h, None, 1) == EINVAL
        assert ctx.lib.dctae_set_option(None, b"fft", 1) == EINVAL
