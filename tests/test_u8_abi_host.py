"""CPU-only checks of the byte-image extension header include/dctae_u8.h, by
the rules tests/test_abi_host.py and tests/test_stream_contract_host.py apply
to include/dctae.h: the library exports every symbol the header declares,
_lib._SIGS declares each with the stream last, every entry is classified by
the context memory it reaches, and the sources agree with that table (an
ORDERED entry opens an OrderedCall, a NONE entry reaches no scratch).

The three encode entries are the dctae.h calls with another pixel type: each
must share its fp32 twin's call body and so carries the twin's row."""
import os
import re

from conftest import ROOT
from test_stream_contract_host import (NONE, ORDERED, SCOPE, SCRATCH, TABLE, _bodies, _closure, _ENC,
                                       _stream_symbols_of_header)

# symbol -> (resources, ordering, reason for NONE rows), the dctae.h twin
TABLE_U8 = {
    "dctae_encode_u8": (_ENC, ORDERED, "", "dctae_encode"),
    "dctae_encode_lfq_proj_u8": (_ENC + ("proj_ws",), ORDERED, "", "dctae_encode_lfq_proj"),
    "dctae_spectrum_tokens_u8": (_ENC, ORDERED, "", "dctae_spectrum_tokens"),
    "dctae_u8_to_f32": ((), NONE, "element-wise on the caller's tensors", None),
}


def _header():
    with open(os.path.join(ROOT, "include", "dctae_u8.h")) as f:
        return f.read()


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.load_library()
    syms = sorted(set(re.findall(r"^int\s+(dctae_\w+)\(", _header(), re.M)))
    assert syms == sorted(TABLE_U8)
    for s in syms:
        assert hasattr(lib, s), s
    assert lib.dctae_abi_version() == 1   # additive: the version stays


def test_every_stream_entry_point_is_classified(pkg):
    from dct_autoencoder_amd import _lib
    header = _stream_symbols_of_header(_header())
    assert header == set(TABLE_U8)
    for k in header:
        assert k in _lib._SIGS, k
        assert _lib._SIGS[k][0][-1] is _lib._P, f"{k}: the stream must be the last argument, a void pointer"


def test_sources_agree_with_the_table():
    funcs = _bodies()
    for k, (res, how, _, twin) in TABLE_U8.items():
        assert k in funcs, f"{k}: no definition found under csrc/"
        body = _closure(funcs, k)
        uses = re.search(SCRATCH, body) is not None
        ordered = re.search(SCOPE, body) is not None
        if how == ORDERED:
            assert uses and ordered, f"{k}: an encode entry outside the OrderedCall scope"
            # the same planner and launch sequence as the fp32 entry: one shared call body, hence the twin's row
            assert "encode_call" in body and "encode_call" in _closure(funcs, twin)
            assert (res, how) == TABLE[twin][:2], k
        else:
            assert how == NONE and not res
            assert not uses and not ordered, f"{k}: reaches the context's scratch but is classified {how}"
        assert ("err_dev" in res) == ("err_dev" in body), k


def test_header_states_the_rules():
    text = " ".join(_header().replace("\n *", " ").split())
    assert "ordered after the context's previous call on another stream" in text
    assert "4-byte aligned" in text and "DCTAE_EINVAL" in text
    assert "bit-identical" in text
