"""CPU-only checks of the int16-code extension header include/dctae_codes16.h,
by the rules tests/test_u8_out_abi_host.py applies to include/dctae_u8_out.h:
the library exports exactly the symbols the header declares, _lib._SIGS
declares each with the stream last, every entry carries the row (resources,
ordering) of its int64 twin in test_stream_contract_host.TABLE (or in the byte
headers' tables), and the sources agree with that row.

Every entry is its twin with another code type: each must share the twin's
call body, named in SHARED below."""
import os
import re

from conftest import ROOT
from test_stream_contract_host import ORDERED, SCOPE, SCRATCH, TABLE, _bodies, _closure, _stream_symbols_of_header
from test_u8_abi_host import TABLE_U8
from test_u8_out_abi_host import TABLE_U8_OUT

# symbol -> (the int64 twin, the call body the two share)
TWINS = {
    "dctae_encode_c16": ("dctae_encode", "encode_call"),
    "dctae_encode_u8_c16": ("dctae_encode_u8", "encode_call"),
    "dctae_encode_lfq_proj_c16": ("dctae_encode_lfq_proj", "encode_call"),
    "dctae_encode_lfq_proj_u8_c16": ("dctae_encode_lfq_proj_u8", "encode_call"),
    "dctae_decode_c16": ("dctae_decode", "decode_impl"),
    "dctae_decode_u8_c16": ("dctae_decode_u8", "decode_impl"),
    "dctae_lfq_project_in_c16": ("dctae_lfq_project_in", "lfq_project_in_impl"),
    "dctae_lfq_project_in_bounded_c16": ("dctae_lfq_project_in_bounded", "lfq_project_in_impl"),
    "dctae_lfq_project_out_c16": ("dctae_lfq_project_out", "lfq_project_out_impl"),
    "dctae_lfq_project_out_inverse_norm_c16": ("dctae_lfq_project_out_inverse_norm",
                                               "lfq_project_out_inverse_norm_impl"),
}


def _row(twin):
    """(resources, ordering) of an existing entry, whichever header declares it"""
    for table in (TABLE, TABLE_U8, TABLE_U8_OUT):
        if twin in table:
            return table[twin][:2]
    raise KeyError(twin)


# symbol -> (resources, ordering, twin): each entry's own row, written out
TABLE_C16 = {k: (*_row(twin), twin) for k, (twin, _) in TWINS.items()}


def _header():
    with open(os.path.join(ROOT, "include", "dctae_codes16.h")) as f:
        return f.read()


def test_library_exports_exactly_the_declared_symbols(pkg):
    lib = pkg.load_library()
    syms = sorted(set(re.findall(r"^int\s+(dctae_\w+)\(", _header(), re.M)))
    assert syms == sorted(TWINS)
    for s in syms:
        assert hasattr(lib, s), s
    assert lib.dctae_abi_version() == 1   # additive: the version stays
    # nothing else of the library carries the suffix
    from dct_autoencoder_amd import _lib
    assert sorted(k for k in _lib._SIGS if k.endswith("_c16")) == syms


def test_every_entry_is_in_sigs_with_the_stream_last(pkg):
    from dct_autoencoder_amd import _lib
    header = _stream_symbols_of_header(_header())
    assert header == set(TWINS)
    for k, (twin, _) in TWINS.items():
        assert k in _lib._SIGS, k
        args, res = _lib._SIGS[k]
        assert args[-1] is _lib._P, f"{k}: the stream must be the last argument, a void pointer"
        targs, tres = _lib._SIGS[twin]
        assert res is tres and len(args) == len(targs), k
        # the twin's arguments; the packed-output struct is the int16 one where the twin takes dctae_packed_out
        for a, t in zip(args, targs):
            if t is _lib.C.POINTER(_lib.PackedOut):
                assert a is _lib.C.POINTER(_lib.PackedOut16), k
            else:
                assert a is t, k
    assert [f[0] for f in _lib.PackedOut16._fields_] == [f[0] for f in _lib.PackedOut._fields_]


def test_every_entry_has_its_twins_row_and_call_body():
    funcs = _bodies()
    for k, (res, how, twin) in TABLE_C16.items():
        shared = TWINS[k][1]
        assert k in funcs, f"{k}: no definition found under csrc/"
        assert (res, how) == _row(twin) and how == ORDERED, k
        body = _closure(funcs, k)
        assert re.search(SCRATCH, body) and re.search(SCOPE, body), f"{k}: outside the OrderedCall scope"
        # one shared call body: the same planner and launch sequence, hence the twin's row
        assert shared in funcs, shared
        assert shared in body and shared in _closure(funcs, twin), (k, shared)
        assert re.search(SCOPE, _closure(funcs, shared)), f"{shared}: the OrderedCall is opened in the shared body"
        assert ("err_dev" in res) == ("err_dev" in body), k
    # the decode entries call decode_impl themselves, as their twins and the frames entry do
    for k in ("dctae_decode_c16", "dctae_decode_u8_c16"):
        assert "decode_impl" in funcs[k] and "decode_impl" in funcs[TWINS[k][0]]
    assert "decode_impl" in funcs["dctae_decode_frames"]


def test_the_existing_headers_are_untouched():
    """the new entries are declared in their own header only"""
    for h in ("dctae.h", "dctae_u8.h", "dctae_u8_out.h"):
        with open(os.path.join(ROOT, "include", h)) as f:
            text = f.read()
        assert "c16" not in text and "packed_out16" not in text, h
        for k in TWINS:
            assert not re.search(rf"\b{k}\s*\(", text), (h, k)


def test_the_code_pointers_are_honestly_typed():
    flat = " ".join(_header().split())
    assert "int16_t* codes_dev;" in flat and "} dctae_packed_out16;" in flat
    for k in TWINS:
        decl = re.search(rf"int {k}\((.*?)\);", flat).group(1)
        assert "int64_t* codes_dev" not in decl and "int64_t* indices_dev" not in decl, k
        assert "dctae_packed_out*" not in decl, k
        assert re.search(r"int16_t\* (codes_dev|indices_dev)|dctae_packed_out16\* out", decl), k


def test_header_states_the_rules():
    text = " ".join(_header().replace("\n *", " ").split())
    assert "an int16 code c means the int64 code int64(c), the sign extension" in text
    assert "bit-identical" in text
    assert "codebook_dim <= 15" in text and "codebook_dim >= 16" in text
    assert "2-byte aligned" in text and "4-byte aligned" in text and "DCTAE_EINVAL" in text
    assert "before anything is launched" in text
    assert "ordered after the context's previous call on another stream" in text
