"""CPU-only checks of the progressive decode through the transformer
(include/dctae_model_prefix.h, progressive.model_frames / model_frame_chunks):

  * the frame planner as pure host functions: (row, id, m) per frame, the
    frames with m == 0, the chunks and the starts inside a chunk, on batches
    with interior pads, k > n_i, empty prefix lists and a budget below one frame;
  * the length list and the prefix list of tests/test_gpu_model_prefixes.py
    reach every edge of the attention kernel they are there for;
  * the C ABI by the rules tests/test_progressive_host.py applies to
    include/dctae_frames.h.
"""
import os
import re

import pytest
import torch

from conftest import ROOT
from test_stream_contract_host import SCOPE, SCRATCH, _bodies, _closure

CSRC = os.path.join(ROOT, "dct-autoencoder_amd", "csrc")
NEW = ("dctae_model_attention_varlen", "dctae_prefix_tokens")

# shared with tests/test_gpu_model_prefixes.py
SEQ_LENS = [1, 31, 32, 33, 63, 64, 65, 0, 255, 256, 257, 320, 700]
GAP_AFTER, GAP = 4, 5
MAX_LEN = 700
PREFIXES = [0, 1, 2, 3, 64, 65, 256, 257, 10 ** 6]
TOKENS = [3, 18, 105, 300]   # of the 14x14, 28x42, 70x98 and 140x140 images at patch size 14
AQ, AK = 256, 64             # queries per block, keys per block of k_attention


# ---- the planner -------------------------------------------------------------------------------
def _batch():
    """row 0: image 0 (real slots 0, 2, 5), image 1 (slots 3, 4), trailing pad; row 1: image 2 (slot 1 of 6 real)"""
    ids = torch.tensor([[0, 0, 0, 1, 1, 0, 1, 1], [0, 0, 0, 0, 0, 0, 0, 0]])
    kp = torch.tensor([[0, 1, 0, 0, 0, 0, 1, 1], [1, 0, 0, 0, 0, 0, 0, 1]]).bool()
    return ids, kp


def test_model_frames(pkg):
    from dct_autoencoder_amd.progressive import model_frames
    ids, kp = _batch()
    pl = model_frames(ids, kp, [0, 1, 2, 3, 9])
    assert pl.n_img == 3
    assert pl.img == [0] * 5 + [1] * 5 + [2] * 5
    assert pl.k == [0, 1, 2, 3, 9] * 3
    assert pl.row == [0] * 10 + [1] * 5
    assert pl.lid == [0] * 5 + [1] * 5 + [0] * 5
    assert pl.m == [0, 1, 2, 3, 3, 0, 1, 2, 2, 2, 0, 1, 2, 3, 6]      # min(k, n_i): interior pads do not count
    pl = model_frames(ids, kp, [[2, 0], [], [7]])                        # per image, an empty list, k > n_i
    assert (pl.img, pl.k, pl.row, pl.lid, pl.m) == ([0, 0, 2], [2, 0, 7], [0, 0, 1], [0, 0, 0], [2, 0, 6])
    pl = model_frames(ids, kp, [])
    assert pl.img == [] and pl.n_img == 3
    kp[1] = True                                                         # a fully padded row still names its image
    assert model_frames(ids, kp, [[], [], [0, 4]]).m == [0, 0]
    with pytest.raises(ValueError, match=">= 0"):
        model_frames(ids, kp, [1, -2])
    with pytest.raises(ValueError, match="per-image"):
        model_frames(ids, kp, [[1], [2]])


def test_model_frames_against_a_count(pkg):
    from dct_autoencoder_amd.progressive import model_frames
    from test_progressive_host import _random_batch
    for seed in range(8):
        ids, kp = _random_batch(seed)
        S = ids.shape[1]
        ks = [0, 1, S // 2, S + 3]
        pl = model_frames(ids, kp, ks)
        f = 0
        for r in range(ids.shape[0]):
            for lid in sorted(set(ids[r].tolist())):
                n = sum(1 for j in range(S) if ids[r, j] == lid and not kp[r, j])
                for k in ks:
                    assert (pl.row[f], pl.lid[f], pl.k[f], pl.m[f]) == (r, lid, k, min(k, n)), (seed, f)
                    f += 1
        assert f == len(pl.m)


def test_model_frame_chunks(pkg):
    from dct_autoencoder_amd import progressive
    ch = progressive.model_frame_chunks
    assert ch([], 10) == []
    assert ch([3, 3, 3, 3], 6) == [(0, 2), (2, 4)]
    assert ch([3, 3, 3, 3], 7) == [(0, 2), (2, 4)]
    assert ch([5, 9, 1, 1], 4) == [(0, 1), (1, 2), (2, 4)]            # a frame above the budget is a run of its own
    assert ch([1] * 5, 100) == [(0, 5)]
    assert ch([2, 2], None) == [(0, 2)] and progressive.PREFIX_TOKENS_PER_CALL >= 3072
    # the GPU test's chunk case: budget 200 over the model-level frames
    ms = [min(k, n) for n in TOKENS for k in PREFIXES if min(k, n) > 0]
    runs = ch(ms, 200)
    assert len(runs) > 3 and any(e - b == 1 and ms[b] > 200 for b, e in runs)
    assert [j for b, e in runs for j in range(b, e)] == list(range(len(ms)))
    assert all(sum(ms[b:e]) <= 200 or e - b == 1 for b, e in runs)


# ---- the edges ---------------------------------------------------------------------------------
def test_the_lengths_reach_every_edge():
    assert {n % AK for n in SEQ_LENS if n} >= {0, 1, AK - 1}                 # exact key blocks, one key over, one short
    assert {255, 256, 257} <= set(SEQ_LENS)                                  # the query-block boundary
    assert any(0 < n < AK for n in SEQ_LENS) and 0 in SEQ_LENS               # a tail inside the first key block; empty
    assert MAX_LEN == max(SEQ_LENS) and -(-MAX_LEN // AQ) == 3
    blocks = -(-MAX_LEN // AQ)
    assert any(0 < n <= AQ * (blocks - 2) for n in SEQ_LENS)                 # whole query blocks with no query
    assert sum(1 for n in SEQ_LENS if -(-n // AQ) < blocks) >= 10
    assert GAP_AFTER < len(SEQ_LENS) and GAP > 0
    # the model-level prefixes on the four images give frame lengths at the same edges
    ms = {min(k, n) for n in TOKENS for k in PREFIXES}
    assert {0, 1, 2, 3, 18, 64, 65, 105, 256, 257, 300} <= ms
    assert {m % AK for m in ms if m} >= {0, 1} and any(m > AQ for m in ms) and any(m == AQ for m in ms)


# ---- the C ABI ---------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "dctae_model_prefix.h")) as f:
        return f.read()


def test_header_and_library(pkg):
    from dct_autoencoder_amd import _lib
    lib = pkg.load_library()
    flat = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split())
            for m in re.finditer(r"\bint\s+(dctae_\w+)\s*\(([^;{]*?)\)\s*;", flat, flags=re.S)}
    assert sorted(decl) == sorted(NEW)
    for k, args in decl.items():
        assert hasattr(lib, k), k
        assert k in _lib._SIGS, k
        assert re.search(r"void\s*\*\s*stream$", args), f"{k}: the stream is the last parameter"
        assert _lib._SIGS[k][0][-1] is _lib._P
        assert len(_lib._SIGS[k][0]) == args.count(",") + 1
        assert not k.endswith(("_u8", "_c16", "_lse"))
    assert lib.dctae_abi_version() == 1   # additive: the version stays
    text = " ".join(_header().replace("\n *", " ").split())
    assert "ordered after the context's previous call on another stream" in text
    assert "DCTAE_EINVAL" in text and "bit for bit" in text and "do not overlap" in text


def test_the_existing_headers_are_untouched():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h == "dctae_model_prefix.h":
            continue
        with open(os.path.join(ROOT, "include", h)) as f:
            text = f.read()
        for k in NEW:
            assert k not in text, (h, k)


def test_sources_agree(pkg):
    funcs = _bodies()
    for k in NEW:
        assert k in funcs, f"{k}: no definition found under csrc/"
        assert "hipStreamSynchronize" not in _closure(funcs, k) and "hipDeviceSynchronize" not in funcs[k]
    # the gather uploads its frame tables: inside an OrderedCall, opened before the upload
    body = funcs["dctae_prefix_tokens"]
    assert re.search(SCOPE, body) and re.search(SCRATCH, body)
    assert re.search(SCOPE, body).start() < re.search(SCRATCH, body).start()
    # the attention touches the caller's tensors only
    assert not re.search(SCRATCH, _closure(funcs, "dctae_model_attention_varlen"))
    with open(os.path.join(CSRC, "dctae_model_prefix.hip")) as f:
        assert not re.search(r"ctx->(?:scratch|plan\b|plan_host|plan_last)", f.read())
    assert "dctae_model_prefix.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_argument_checks_come_first(pkg):
    from dct_autoencoder_amd.model import SeqTable
    with pytest.raises(ValueError, match="max_len"):
        SeqTable([0, 4], [4, 3], 7, "cpu", max_len=3)
    with pytest.raises(ValueError, match="overlaps"):
        SeqTable([0, 3], [4, 3], 7, "cpu")
    with pytest.raises(ValueError, match="outside"):
        SeqTable([0, 4], [4, 4], 7, "cpu")
    t = SeqTable([5, 0, 4], [2, 4, 0], 7, "cpu")
    assert (t.n_seq, t.max_len, t.start.dtype, t.len.dtype) == (3, 4, torch.int64, torch.int32)
    enc = dict(hidden_size=64, intermediate_size=64, num_attention_heads=1, num_hidden_layers=1)
    model = pkg.DCTAutoencoder(pkg.DCTAutoencoderConfig(patch_size=14, vq_codebook_size=16, vq_num_codebooks=2,
                                                        encoder_config=enc, decoder_config=enc)).eval()
    S = 4
    dp = pkg.DCTPatches(patches=torch.zeros(1, S, 196), key_pad_mask=torch.zeros(1, S, dtype=torch.bool),
                        batched_image_ids=torch.zeros(1, S, dtype=torch.long),
                        patch_channels=torch.zeros(1, S, dtype=torch.long),
                        patch_positions=torch.zeros(1, S, 2, dtype=torch.long), patch_sizes=[(2, 2)],
                        original_sizes=[(28, 28)])
    codes = torch.zeros(1, S, 2, dtype=torch.long)
    with pytest.raises(TypeError, match="int64 or torch.int16"):
        model.decode_prefixes(dp, codes.int(), [1])
    with pytest.raises(ValueError, match=">= 0"):
        model.decode_prefixes(dp, codes, [-1])
    with pytest.raises(ValueError, match="per-image"):
        model.decode_prefixes(dp, codes, [[1], [2]])
    with pytest.raises(NotImplementedError):
        model.train().decode_prefixes(dp, codes, [1])
    model.eval()
    assert model.decode_prefixes(dp, codes, [0, 0]) == (None, [])   # nothing goes through the model: no device needed
    with pytest.raises(pkg.DCTAEUnavailable):
        model.decode_prefixes(dp, codes, [1])
