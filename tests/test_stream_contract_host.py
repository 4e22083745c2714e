"""The stream contract of the C ABI, entry point by entry point (DESIGN.md
"Streams and the context's scratch").

Every entry point whose last argument is the stream is classified here by the
context-owned device memory it touches and by how a call on one stream is kept
apart from the context's previous call on another:

  ORDERED    the call runs inside an OrderedCall scope (csrc/dctae_ctx.h), the
             only way to the context's scratch: its stream waits for the
             context's previous ordered call, and the next ordered call waits
             for it.  These are the rows tests/test_gpu_streams.py
             parametrises over.
  HOST_SYNC  ordered in the same way, and the call also waits on the host for
             its own stream before it returns, so the ordering harness (which
             needs the host to run ahead of a parked stream) cannot time it;
             test_gpu_streams.py::test_error_flag_crosses_streams covers it.
  FLAG_ONLY  no scratch; the kernels only raise bits of the sticky error flag
             ctx->err_dev (a set-only word that dctae_check_device_errors reads
             and clears).  Raising needs no order among the raisers; the caller
             orders the check after them as after any of its own tensors.
  NONE       no context-owned device memory at all; the reason is in the row.

The test keeps the table complete: a new entry point that takes a stream cannot
be added to _lib._SIGS without a row here.
"""
import os
import re

from conftest import ROOT

ORDERED, HOST_SYNC, FLAG_ONLY, NONE = "ordered", "host-sync", "flag-only", "none"

# the context-owned device memory of csrc/dctae_ctx.h
RESOURCES = ("ws", "stage", "plan", "dct", "fft_tab", "proj_ws", "st_ws", "vq_ws", "err_dev")

_ENC = ("ws", "stage", "plan", "dct", "fft_tab")
_DEC = ("ws", "stage", "plan", "dct", "fft_tab", "err_dev")
_ELEMENTWISE = "element-wise on the caller's tensors"
_CALLER_WS = "workspace supplied by the caller"

# symbol -> (resources, ordering, reason for NONE rows)
TABLE = {
    "dctae_encode": (_ENC, ORDERED, ""),
    "dctae_encode_lfq_proj": (_ENC + ("proj_ws",), ORDERED, ""),
    "dctae_spectrum_tokens": (_ENC, ORDERED, ""),
    "dctae_dct2": (("ws", "plan", "dct"), ORDERED, ""),
    "dctae_patch_spectrum": (("ws", "stage", "plan"), ORDERED, ""),
    "dctae_decode": (_DEC, ORDERED, ""),
    "dctae_decode_normed": (_DEC, ORDERED, ""),
    "dctae_decode_backward": (("ws", "plan", "dct", "err_dev"), ORDERED, ""),
    "dctae_pixel_loss_forward": (("ws", "plan"), ORDERED, ""),
    "dctae_rec_loss_forward": (("ws", "err_dev"), ORDERED, ""),
    "dctae_lfq_entropy_forward": (("ws",), ORDERED, ""),
    "dctae_lfq_entropy_backward": (("ws",), ORDERED, ""),
    "dctae_lfq_project_in": (("proj_ws",), ORDERED, ""),
    "dctae_lfq_project_in_bounded": (("proj_ws",), ORDERED, ""),
    "dctae_lfq_project_out": (("proj_ws",), ORDERED, ""),
    "dctae_lfq_project_out_inverse_norm": (("proj_ws", "err_dev"), ORDERED, ""),
    "dctae_vq_forward": (("vq_ws", "plan"), ORDERED, ""),
    "dctae_vq_output_from_indices": (("vq_ws", "plan", "err_dev"), ORDERED, ""),
    "dctae_norm_batch_stats": (("st_ws", "err_dev"), ORDERED, ""),
    "dctae_norm_batch_mad": (("st_ws", "err_dev"), ORDERED, ""),
    "dctae_norm_train_step": (("st_ws", "err_dev"), ORDERED, ""),
    "dctae_check_device_errors": (("err_dev",), HOST_SYNC, ""),
    "dctae_norm_thresholds": (("err_dev",), HOST_SYNC, ""),
    "dctae_norm_forward": (("err_dev",), FLAG_ONLY, ""),
    "dctae_norm_inverse": (("err_dev",), FLAG_ONLY, ""),
    "dctae_norm_inverse_backward": (("err_dev",), FLAG_ONLY, ""),
    "dctae_rec_loss_backward": (("err_dev",), FLAG_ONLY, ""),
    "dctae_vq_codes_from_indices": (("err_dev",), FLAG_ONLY, ""),
    "dctae_norm_merge": ((), NONE, _ELEMENTWISE),
    "dctae_lfq_forward": ((), NONE, _ELEMENTWISE),
    "dctae_lfq_indices_to_codes": ((), NONE, _ELEMENTWISE),
    "dctae_linear_ordered": ((), NONE, "a GEMM on the caller's tensors, no scratch"),
    "dctae_synth_images": ((), NONE, _ELEMENTWISE),
    "dctae_model_linear": ((), NONE, "a GEMM on the caller's tensors, no scratch"),
    "dctae_model_attention": ((), NONE, "caller's tensors only"),
    "dctae_model_attention_lse": ((), NONE, "caller's tensors only"),
    "dctae_model_attention_bwd": ((), NONE, _CALLER_WS + " (delta_ws)"),
    "dctae_model_layernorm": ((), NONE, _ELEMENTWISE),
    "dctae_model_embed_norm": ((), NONE, _ELEMENTWISE),
    "dctae_model_pos_add": ((), NONE, _ELEMENTWISE),
    "dctae_model_to_bf16": ((), NONE, _ELEMENTWISE),
    "dctae_model_lfq": ((), NONE, _ELEMENTWISE),
    "dctae_model_transpose_pack": ((), NONE, _ELEMENTWISE),
    "dctae_model_colsum": ((), NONE, _CALLER_WS + " (ws)"),
    "dctae_model_layernorm_bwd": ((), NONE, _CALLER_WS + " (part_g / part_b)"),
    "dctae_model_qgelu": ((), NONE, _ELEMENTWISE),
    "dctae_model_qgelu_bwd": ((), NONE, _ELEMENTWISE),
    "dctae_model_pos_grad": ((), NONE, "caller's tensors only"),
    "dctae_optim_gradnorm": ((), NONE, _CALLER_WS + " (ws) and table"),
    "dctae_optim_adamw_pack": ((), NONE, "the caller's segment table and tensors"),
}

HARNESS_ROWS = sorted(k for k, v in TABLE.items() if v[1] == ORDERED)


def _header():
    with open(os.path.join(ROOT, "include", "dctae.h")) as f:
        return f.read()


def _stream_symbols_of_header(text):
    """the functions of include/dctae.h whose last parameter is ``void* stream``"""
    flat = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    flat = re.sub(r"//[^\n]*", " ", flat)
    out = set()
    for m in re.finditer(r"\bint\s+(dctae_\w+)\s*\(([^;{]*?)\)\s*;", flat, flags=re.S):
        args = " ".join(m.group(2).split())
        if re.search(r"void\s*\*\s*stream$", args):
            out.add(m.group(1))
    return out


def test_every_stream_entry_point_is_classified(pkg):
    from dct_autoencoder_amd import _lib
    header = _stream_symbols_of_header(_header())
    assert header, "no entry point with a stream parameter found in include/dctae.h"
    # _SIGS does not name its arguments: the header says which last argument is the stream
    sigs = {k for k, (args, _) in _lib._SIGS.items() if k in header}
    assert sigs == header, f"include/dctae.h and _lib._SIGS disagree: {sorted(sigs ^ header)}"
    for k in sigs:
        assert _lib._SIGS[k][0][-1] is _lib._P, f"{k}: the stream must be the last argument, a void pointer"
    assert set(TABLE) == sigs, (f"unclassified: {sorted(sigs - set(TABLE))}; "
                                f"classified but not in the ABI: {sorted(set(TABLE) - sigs)}")


def test_rows_are_well_formed():
    for k, (res, how, why) in TABLE.items():
        assert how in (ORDERED, HOST_SYNC, FLAG_ONLY, NONE), k
        assert set(res) <= set(RESOURCES) and len(set(res)) == len(res), k
        if how == NONE:
            assert not res and why, f"{k}: a row without resources needs its one-line reason"
        elif how == FLAG_ONLY:
            assert res == ("err_dev",), k
        else:
            assert res, k
    assert len(HARNESS_ROWS) == 21


def _sources(suffixes):
    d = os.path.join(ROOT, "dct-autoencoder_amd", "csrc")
    src = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(suffixes):
            with open(os.path.join(d, f)) as fh:
                src[f] = fh.read()
    return src


def _bodies():
    """name -> body text of every extern "C" function, helpers they call by name included once
    (host functions of any plain return type: ``int``, ``void``, a struct by value)"""
    text = "\n".join(_sources(".hip").values())
    funcs = {}
    for m in re.finditer(r"^(?:static\s+)?[\w:]+\s+(?:dctae::)?(\w+)\s*\([^;{]*?\)\s*(?:const\s*)?\{", text,
                         flags=re.M | re.S):
        i, depth = m.end(), 1
        while depth and i < len(text):
            depth += {"{": 1, "}": -1}.get(text[i], 0)
            i += 1
        funcs.setdefault(m.group(1), text[m.end():i])
    return funcs


def _closure(funcs, name, seen=None):
    """the body of ``name`` with the bodies of the project functions it calls"""
    seen = seen if seen is not None else set()
    if name in seen or name not in funcs:
        return ""
    seen.add(name)
    body = funcs[name]
    for callee in set(re.findall(r"\b(\w+)\s*\(", body)):
        if callee in funcs:
            body += _closure(funcs, callee, seen)
    return body


# an OrderedCall's accessors (the scratch buffers, the plan) and its construction
SCRATCH = r"\.scratch\(|\.upload\("
SCOPE = r"\bOrderedCall\s+\w+\s*\("


def test_sources_agree_with_the_table():
    """every entry point that reaches the context's scratch, directly or through
    a helper, opens an OrderedCall, and is an ORDERED row; every other row
    reaches no scratch"""
    funcs = _bodies()
    for k, (res, how, _) in TABLE.items():
        assert k in funcs, f"{k}: no definition found under csrc/"
        body = _closure(funcs, k)
        uses = re.search(SCRATCH, body) is not None
        ordered = re.search(SCOPE, body) is not None
        if how == ORDERED:
            assert uses, f"{k}: classified as a scratch user, but its body reaches none"
            assert ordered, f"{k}: uses the context's scratch without an OrderedCall"
        elif how == HOST_SYNC:
            assert ordered and "hipStreamSynchronize" in body, k
        else:
            assert not uses, f"{k}: reaches the context's scratch but is classified {how}"
        assert ("err_dev" in res) == ("err_dev" in body), f"{k}: the table and the source disagree on ctx->err_dev"


def test_old_spellings_are_gone():
    """the free functions and the raw members that OrderedCall replaced: the
    buffers are private to the context now, so nothing may name them"""
    old = r"\b(?:order_after_previous|mark_done|ensure_ws|upload_plan|proj_scratch|vq_scratch)\s*\(|" \
          r"ctx->(?:ws|stage|st_ws|vq_ws|proj_ws|plan_dev)\b"
    for f, text in _sources((".hip", ".h")).items():
        m = re.search(old, text)
        assert m is None, f"csrc/{f}: {m.group(0)!r} bypasses OrderedCall"


def test_header_states_the_rule():
    text = " ".join(_header().replace("\n *", " ").split())
    assert "ordered after the context's previous call on another stream" in text
