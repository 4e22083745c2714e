"""The packed-batch description that dctae_decode, dctae_decode_normed and
dctae_decode_backward share (csrc/dctae_decode.hip: DecodeBatch; _ops.py:
DecodeTable), at the two places no other test reaches:

* a negative image offset is refused by all three entry points on the host,
  before anything is launched, and leaves the context usable;
* BatchDecoder with several images per packed row (the second column of the
  image LUT), whose table comes from the packing layout without reading a
  device tensor, against decode_batch and against the table built by walking
  the batch's image ids.
Run on an MI355X.
"""
import ctypes as C

import pytest
import torch

from test_gpu_pixel_loss import _stage_names

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777.0


def test_negative_image_offset_is_refused(pkg):
    """one 14 x 14 image, P = 14, one row of S = 3 tokens, out_off = [-1]"""
    from dct_autoencoder_amd import _lib, _ops
    from dct_autoencoder_amd._lib import i32, i64, ptr
    dev = torch.device(DEV, torch.cuda.current_device())
    ctx, st = _lib.context(dev), _lib.stream_ptr(dev)
    p = _ops.FEParams(3, 14, 1, 1, 3)
    cfg = p.c()
    g = torch.Generator().manual_seed(5)
    ids = torch.zeros(1, 3, dtype=torch.long, device=DEV)
    kp = torch.zeros(1, 3, dtype=torch.bool, device=DEV)
    pos = torch.zeros(1, 3, 2, dtype=torch.long, device=DEV)
    ch = torch.arange(3, device=DEV).view(1, 3)
    patches = torch.randn(1, 3, 196, generator=g).to(DEV)
    norm = _ops.NormState(torch.zeros(3, 1, 1, 196, device=DEV), torch.ones(3, 1, 1, 196, device=DEV))
    # the images sit 64 floats inside their buffers: a library that took the offset would still write inside them
    n = 3 * 14 * 14
    rgb = torch.full((64 + n,), SENTINEL, device=DEV)
    grad = torch.ones(64 + n, device=DEV)
    dp = torch.full((1, 3, 196), SENTINEL, device=DEV)

    def calls(off):
        head = (ctx.h, C.byref(cfg), 1, i32([0]), 1, 1, i32([14, 14]), i64([off]), i32([1, 1]), ptr(ids), ptr(kp),
                ptr(pos), ptr(ch))
        yield "dctae_decode", lambda: ctx.lib.dctae_decode(*head, None, None, None, ptr(patches), ptr(rgb[64:]), st)
        yield "dctae_decode_normed", lambda: ctx.lib.dctae_decode_normed(*head, C.byref(norm.c()), ptr(patches),
                                                                          ptr(rgb[64:]), st)
        yield "dctae_decode_backward", lambda: ctx.lib.dctae_decode_backward(*head, ptr(patches), ptr(grad[64:]), None,
                                                                              None, None, ptr(dp), st)

    for name, call in calls(-1):
        rc = []
        launched = _stage_names(ctx, lambda: rc.append(call()))
        assert rc == [-1], f"{name}: returned {rc[0]}, not DCTAE_EINVAL"
        assert ctx.lib.dctae_last_error(ctx.h).decode() == "negative image offset", name
        assert launched == {}, f"{name}: launched {launched} before it refused"
        assert torch.all(rgb == SENTINEL) and torch.all(dp == SENTINEL), f"{name}: wrote before it refused"
    for name, call in calls(0):
        assert call() == 0, f"{name} after the refusals: {ctx.lib.dctae_last_error(ctx.h).decode()}"
        assert ctx.lib.dctae_check_device_errors(ctx.h, st) == 0, name
    assert torch.all(rgb[:64] == SENTINEL) and torch.isfinite(rgb[64:]).all() and torch.isfinite(dp).all()
    assert bool((rgb[64:] != SENTINEL).all()) and bool((dp != SENTINEL).all())


def test_batch_decoder_two_images_per_row(pkg, ref_tables):
    """6 images of 28 x 42 (18 tokens each) in rows of 40 tokens: two images share a row"""
    from dct_autoencoder_amd import _ops, feature_extraction as fe_mod
    B, H, W, P, S = 6, 28, 42, 14, 40
    fe = pkg.DCTAutoencoderFeatureExtractor(3, P, 0.0, 32, 32, S)
    pn = pkg.PatchNorm(32, 32, P, 3).to(DEV)
    pn.median.data.copy_(ref_tables.median)
    pn.b.data.copy_(ref_tables.b)
    pn.n.data.copy_(ref_tables.n)
    pn.frozen = True
    pn.eval()
    lfq = pkg.LFQ(dim=P * P, codebook_size=2 ** 14, num_codebooks=14).to(DEV).eval()
    enc = fe_mod.BatchEncoder(fe, B, H, W, pn, lfq, device=DEV)
    assert enc.k == 18 and enc.n_rows == 3 and sorted(enc.plan.local_id) == [0, 0, 0, 1, 1, 1]
    packed = enc(_ops.synth_images(B, H, W, seed=77, device=DEV))
    dec = fe_mod.BatchDecoder(enc, pn, lfq)
    out = dec(packed)
    _ops.check_device_errors(out.device)
    psizes, sizes = [(H // P, W // P)] * B, [(H, W)] * B
    dp = pkg.DCTPatches(patches=torch.empty(enc.n_rows, S, 0, device=DEV), key_pad_mask=packed["key_pad_mask"],
                        batched_image_ids=packed["image_ids"], patch_channels=packed["channels"],
                        patch_positions=packed["positions"], patch_sizes=psizes, original_sizes=sizes)
    want = fe.decode_batch(dp, packed["codes"], pn, lfq)
    assert len(want) == B and out.shape == (B, 3, H, W)
    for i, img in enumerate(want):
        assert torch.equal(img, out[i]), f"BatchDecoder image {i} != decode_batch"
    assert len({out[i].sum().item() for i in range(B)}) == B, "the images differ from one another"
    walked = _ops.DecodeTable(enc.p, packed["image_ids"], packed["key_pad_mask"], packed["positions"],
                              packed["channels"], psizes, sizes)
    t = dec.table
    assert (t.R, t.S, t.lut_w, t.n_img, t.total) == (walked.R, walked.S, walked.lut_w, walked.n_img, walked.total)
    assert t.lut_w == 2 and -1 not in list(t.keep[0])
    for a, b in zip(t.keep, walked.keep):
        assert list(a) == list(b)
