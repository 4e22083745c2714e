"""Every byte of every output is written by the call.

``_ops`` allocates outputs with ``torch.empty``, and the caching allocator
usually hands back the block that held the previous, identical result: an
output element no kernel writes (a pad slot, a ``key_pad`` byte, the last bytes
of a byte image, a pixel) would keep the right value by accident.  Here the
outputs are passed in, filled once with byte 0x5A and once with 0xA5; the two
results must be equal bit for bit, and equal to the call that allocated its
own outputs.  An element no kernel wrote keeps its fill and differs."""
import pytest
import torch

import stale_state as ss

pytestmark = pytest.mark.gpu
DEV = ss.DEV
FILLS = (0x5A, 0xA5)

# packings at max_seq_len 3072: every row full (a 512^2 image is 3072 tokens), one padded row
# (3 x 768 tokens), a full row followed by a last row of 18 tokens
PACKINGS = {"full": [(512, 512)] * 2, "padded": [(224, 224)] * 3, "short-last": [(512, 512), (37, 53)]}
SINKS = {"codes": {}, "all": dict(patches=True, raw=True, scores=True), "c16": dict(codes_dtype=torch.int16),
         "c16-all": dict(codes_dtype=torch.int16, patches=True, raw=True, scores=True),
         "u8-all": dict(uint8=True, patches=True, raw=True, scores=True)}


@pytest.fixture(scope="module")
def env(pkg, ref_tables):
    FE = pkg.DCTAutoencoderFeatureExtractor
    fes = {"fe": FE(3, 14, 0.0, 32, 32, 3072), "drop": FE(3, 14, 0.0, 32, 32, 2000), "drop_s": FE(3, 14, 0.0, 32, 32, 50)}
    pn = ss.patchnorm(pkg, ref_tables.median, ref_tables.b)
    lfq = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).to(DEV).eval()
    return fes, pn, lfq


@pytest.mark.parametrize("sinks", SINKS)
@pytest.mark.parametrize("packing", PACKINGS)
def test_encode_writes_every_output_byte(env, packing, sinks):
    fes, pn, lfq = env
    kw = SINKS[sinks]
    x = (ss.byte_images if kw.get("uint8") else ss.images)(71, PACKINGS[packing])
    own = ss.encode(fes["fe"], x, pn, lfq, **kw)
    assert {"codes", "positions", "channels", "image_ids", "key_pad_mask"} <= set(ss.tensors(own))
    n_pad = int(own["key_pad_mask"].sum())
    assert (n_pad > 0) == (packing != "full")
    got = []
    for byte in FILLS:
        out = ss.filled_like(own, byte)
        res = ss.tensors(ss.encode(fes["fe"], x, pn, lfq, out=dict(out), **kw))
        assert all(res[k] is out[k] for k in out), "the call did not write into the tensors it was given"
        torch.cuda.synchronize()
        got.append(ss.flat(res))
    ss.assert_same_bits(got[0], got[1], "outputs pre-filled with 0x5A against 0xA5")
    ss.assert_same_bits(got[0], ss.flat(ss.tensors(own)), "pre-filled outputs against the call's own allocation")


RAGGED = [(224, 98), (333, 517), (37, 53)]   # the last image is 3 x 37 x 53 = 5883 elements: an odd byte count
DECODES = {
    "512": ("fe", [(512, 512)] * 2, "codes"), "512-normed": ("fe", [(512, 512)] * 2, "normed"),
    "512-dropped": ("drop", [(512, 512)] * 2, "codes"), "ragged": ("fe", RAGGED, "codes"),
    "ragged-patches": ("fe", RAGGED, "patches"), "ragged-normed": ("fe", RAGGED, "normed"),
    "ragged-dropped": ("drop_s", [(64, 96), (37, 53), (45, 75)], "codes"),
}


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("case", DECODES)
def test_decode_writes_every_output_byte(env, case, out_dtype):
    fes, pn, lfq = env
    lib, ops, _, _ = ss.mods()
    which, sizes, src = DECODES[case]
    fe = fes[which]
    r = ss.encode(fe, ss.images(72, sizes), pn, lfq, patches=True, raw=True)
    assert (3 * sizes[-1][0] * sizes[-1][1]) % 2 == (1 if "ragged" in case else 0)
    table = ops.decode_table(*ss.decode_args(fe, r))
    st = pn.state()
    norm = st.c() if src != "patches" else None
    codes = r["codes"] if src == "codes" else None
    patches = None if src == "codes" else (r["raw"] if src == "patches" else r["patches"])
    ctx = lib.context(torch.device(DEV, torch.cuda.current_device()))
    got = []
    for byte in FILLS:
        out = torch.empty(table.total, dtype=out_dtype, device=DEV)
        out.view(torch.uint8).fill_(byte)
        ops._decode_call(ctx, fe.params(table.S).c(table.S), table, table.ids, table.key_pad, table.pos, table.ch,
                         norm, lfq.cfg() if src == "codes" else None, codes, patches, out, src == "normed", out_dtype)
        torch.cuda.synchronize()
        got.append(ss.flat(out))
    ss.assert_same_bits(got[0], got[1], "images pre-filled with 0x5A against 0xA5")
    kw = {"codes": dict(codes=codes, norm=st, lfq=lfq.cfg()), "patches": dict(patches=patches),
          "normed": dict(patches=patches, norm=st, normed=True)}[src]
    _, flat = ops.decode(*ss.decode_args(fe, r), out_dtype=out_dtype, return_flat=True, **kw)
    ss.assert_same_bits(got[0], ss.flat(flat), "the pre-filled buffer against decode's own allocation")
