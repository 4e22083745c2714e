"""CPU-only checks of the byte-output extension header include/dctae_u8_out.h,
by the rules tests/test_u8_abi_host.py applies to include/dctae_u8.h: the
library exports exactly the symbols the header declares, _lib._SIGS declares
each with the stream last, every entry is classified by the context memory it
reaches, and the sources agree with that table (an ORDERED entry opens an
OrderedCall, a NONE entry reaches no scratch).

The two decode entries are the dctae.h calls with another output pixel type:
each must share its fp32 twin's call body (decode_impl) and so carries the
twin's row."""
import os
import re

from conftest import ROOT
from test_stream_contract_host import (_DEC, NONE, ORDERED, SCOPE, SCRATCH, TABLE, _bodies, _closure,
                                       _stream_symbols_of_header)

# symbol -> (resources, ordering, reason for NONE rows, the dctae.h twin)
TABLE_U8_OUT = {
    "dctae_decode_u8": (_DEC, ORDERED, "", "dctae_decode"),
    "dctae_decode_normed_u8": (_DEC, ORDERED, "", "dctae_decode_normed"),
    "dctae_f32_to_u8": ((), NONE, "element-wise on the caller's tensors", None),
}


def _header():
    with open(os.path.join(ROOT, "include", "dctae_u8_out.h")) as f:
        return f.read()


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.load_library()
    syms = sorted(set(re.findall(r"^int\s+(dctae_\w+)\(", _header(), re.M)))
    assert syms == sorted(TABLE_U8_OUT)
    for s in syms:
        assert hasattr(lib, s), s
    assert lib.dctae_abi_version() == 1   # additive: the version stays


def test_every_stream_entry_point_is_classified(pkg):
    from dct_autoencoder_amd import _lib
    header = _stream_symbols_of_header(_header())
    assert header == set(TABLE_U8_OUT)
    for k in header:
        assert k in _lib._SIGS, k
        assert _lib._SIGS[k][0][-1] is _lib._P, f"{k}: the stream must be the last argument, a void pointer"
    # the byte decodes take their twins' arguments, the image pointer apart (a void pointer in both)
    for k, (_, _, _, twin) in TABLE_U8_OUT.items():
        if twin:
            assert _lib._SIGS[k] == _lib._SIGS[twin], k


def test_sources_agree_with_the_table():
    funcs = _bodies()
    for k, (res, how, why, twin) in TABLE_U8_OUT.items():
        assert k in funcs, f"{k}: no definition found under csrc/"
        body = _closure(funcs, k)
        uses = re.search(SCRATCH, body) is not None
        ordered = re.search(SCOPE, body) is not None
        if how == ORDERED:
            assert uses and ordered, f"{k}: a decode entry outside the OrderedCall scope"
            # the same planner and launch sequence as the fp32 entry: one shared call body, hence the twin's row
            assert "decode_impl" in funcs[k] and "decode_impl" in funcs[twin]
            assert "decode_impl" in funcs["dctae_decode_frames"]   # the frames entry shares it too
            assert (res, how) == TABLE[twin][:2], k
        else:
            assert how == NONE and not res and why
            assert not uses and not ordered, f"{k}: reaches the context's scratch but is classified {how}"
        assert ("err_dev" in res) == ("err_dev" in body), k


def test_the_existing_headers_are_untouched():
    """the new entries are declared in their own header only"""
    for h in ("dctae.h", "dctae_u8.h"):
        with open(os.path.join(ROOT, "include", h)) as f:
            text = f.read()
        for k in TABLE_U8_OUT:
            assert not re.search(rf"\b{k}\s*\(", text), (h, k)


def test_header_states_the_rules():
    text = " ".join(_header().replace("\n *", " ").split())
    assert "ordered after the context's previous call on another stream" in text
    assert "4-byte aligned" in text and "DCTAE_EINVAL" in text
    assert "bit-identical" in text
