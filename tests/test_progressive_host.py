"""CPU-only checks of the progressive decode (include/dctae_frames.h,
dct_autoencoder_amd.progressive):

  * the C ABI: the library exports the symbols the header declares and _lib._SIGS
    declares each with the stream last; each has a row in the style of
    tests/test_stream_contract_host.py's TABLE (not edited) and the sources agree
    with it: both entries reach the context's scratch only inside an OrderedCall;
  * ``frame_cuts`` against a brute-force count on seeded random batches (interior
    pads, several images per row, fully padded rows, k = 0, k > n_i);
  * the Python argument checks raise before any device is touched;
  * the recorded reference (tests/golden/progressive_ref.npz): the numpy mirror
    of ``image_clip`` equals the reference's bit for bit, and the masking
    definition of a prefix frame gives the pixels of the reference's slicing
    (``ref_cpu.postprocess`` of the masked batch within test_oracle.py's bound
    for that function, rtol = atol = 1e-6).
"""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from oracle import ref_cpu
from oracle.decode_cases import token_image
from test_stream_contract_host import _DEC, ORDERED, RESOURCES, SCOPE, SCRATCH, _bodies, _closure

CSRC = os.path.join(ROOT, "dct-autoencoder_amd", "csrc")

# symbol -> (resources, ordering, reason for NONE rows): the decode's resources, ordered; image_clip's
# min / max words live in the workspace and its image table travels through the plan
TABLE_FRAMES = {
    "dctae_decode_frames": (_DEC, ORDERED, ""),
    "dctae_image_clip": (("ws", "plan"), ORDERED, ""),
}


def clip_mirror(x):
    """util.py:143-147 in numpy fp32: (x - min) / (max - min), every operation rounded to fp32"""
    x = np.asarray(x, dtype=np.float32)
    lo, hi = x.min(), x.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((x - lo) / (hi - lo)).astype(np.float32)


# ---- the C ABI ----------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "dctae_frames.h")) as f:
        return f.read()


def test_header_and_library(pkg):
    from dct_autoencoder_amd import _lib
    lib = pkg.load_library()
    flat = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split())
            for m in re.finditer(r"\bint\s+(dctae_\w+)\s*\(([^;{]*?)\)\s*;", flat, flags=re.S)}
    assert sorted(decl) == sorted(TABLE_FRAMES)
    for k, args in decl.items():
        assert hasattr(lib, k), k
        assert k in _lib._SIGS, k
        assert re.search(r"void\s*\*\s*stream$", args), f"{k}: the stream is the last parameter"
        assert _lib._SIGS[k][0][-1] is _lib._P
        assert len(_lib._SIGS[k][0]) == args.count(",") + 1
    assert lib.dctae_abi_version() == 1   # additive: the version stays
    # the struct mirror and the type tags
    assert [f[0] for f in _lib.Frames._fields_] == re.findall(r"(\w+);", re.search(
        r"typedef struct \{(.*?)\} dctae_frames;", flat, flags=re.S).group(1))
    tags = dict(re.findall(r"#define (DCTAE_(?:PIXEL|CODES|CLIP)_\w+) (\d+)", flat))
    assert {k: int(v) for k, v in tags.items()} == {
        "DCTAE_PIXEL_F32": _lib.PIXEL_F32, "DCTAE_PIXEL_U8": _lib.PIXEL_U8, "DCTAE_CODES_I64": _lib.CODES_I64,
        "DCTAE_CODES_I16": _lib.CODES_I16, "DCTAE_CLIP_NONE": _lib.CLIP_NONE, "DCTAE_CLIP_MINMAX": _lib.CLIP_MINMAX}
    text = " ".join(_header().replace("\n *", " ").split())
    assert "ordered after the context's previous call on another stream" in text
    assert "DCTAE_EINVAL" in text and "bit for bit" in text and "4-byte aligned" in text and "finite" in text


def test_the_existing_headers_are_untouched():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h == "dctae_frames.h":
            continue
        with open(os.path.join(ROOT, "include", h)) as f:
            text = f.read()
        for k in TABLE_FRAMES:
            assert not re.search(rf"\b{k}\s*\(", text), (h, k)


def test_rows_and_sources_agree():
    funcs = _bodies()
    for k, (res, how, why) in TABLE_FRAMES.items():
        assert how == ORDERED and res and set(res) <= set(RESOURCES) and len(set(res)) == len(res), k
        assert k in funcs, f"{k}: no definition found under csrc/"
        body = _closure(funcs, k)
        assert re.search(SCRATCH, body), f"{k}: classified as a scratch user, but its body reaches none"
        assert re.search(SCOPE, body), f"{k}: uses the context's scratch without an OrderedCall"
        assert ("err_dev" in res) == ("err_dev" in body), f"{k}: the table and the source disagree on ctx->err_dev"
        assert "hipStreamSynchronize" not in body and "hipDeviceSynchronize" not in funcs[k], f"{k} waits on the host"
    # the decode entry plans with the decode family's helpers
    body = _closure(funcs, "dctae_decode_frames")
    for helper in ("decode_check", "decode_geometry", "decode_gemm_pair", "decode_args"):
        assert re.search(rf"\b{helper}\s*\(", body), helper


def test_scratch_only_inside_an_ordered_call():
    with open(os.path.join(CSRC, "dctae_frames.hip")) as f:
        unit = f.read()
    # nothing in the unit names the context's buffers directly
    assert not re.search(r"ctx->(?:scratch|plan\b|plan_host|plan_last)", unit)
    funcs = _bodies()
    for name in ("decode_impl", "dctae_image_clip"):   # the scope opens before the first use
        body = funcs[name]
        assert re.search(SCOPE, body).start() < re.search(SCRATCH, body).start(), name
    assert "dctae_frames.hip" in open(os.path.join(CSRC, "Makefile")).read()


# ---- frame_cuts ------------------------------------------------------------------------
def _random_batch(seed):
    """ids / key_pad with several ids per row (some absent), interior pads, a fully padded row"""
    g = torch.Generator().manual_seed(seed)
    R, S = 2 + seed % 3, 5 + 3 * (seed % 5)
    ids = torch.randint(0, 1 + seed % 4, (R, S), generator=g)
    ids = ids.sort(dim=1).values if seed % 2 else ids        # packed order, or ids interleaved
    kp = torch.rand(R, S, generator=g) < 0.3
    kp[R - 1] = seed % 3 == 0 or kp[R - 1]                   # a fully padded row (it still names its ids)
    return ids, kp


def _brute(ids, kp, per):
    """(img, cut) by counting: the cut of prefix k is the least c with min(k, n_i) real tokens at slots < c"""
    img, cut, n = [], [], 0
    for r in range(ids.shape[0]):
        for lid in sorted(set(ids[r].tolist())):
            real = [j for j in range(ids.shape[1]) if ids[r, j] == lid and not kp[r, j]]
            for k in per[n]:
                want = min(k, len(real))
                c = 0
                while sum(1 for j in real if j < c) < want:
                    c += 1
                img.append(n)
                cut.append(c)
            n += 1
    return img, cut, n


@pytest.mark.parametrize("seed", range(12))
def test_frame_cuts_against_a_count(pkg, seed):
    from dct_autoencoder_amd.progressive import frame_cuts, prefix_key_pad
    ids, kp = _random_batch(seed)
    S = ids.shape[1]
    shared = [0, 1, 2, S // 2, S, S + 7]
    n_img = _brute(ids, kp, [[]] * (ids.shape[0] * S))[2]
    img, cut, _ = _brute(ids, kp, [shared] * n_img)
    assert frame_cuts(ids, kp, shared) == (img, cut)
    assert any(c == 0 for c in cut) and max(cut) <= S
    g = torch.Generator().manual_seed(100 + seed)
    per = [torch.randint(0, S + 3, (int(torch.randint(0, 4, (1,), generator=g)),), generator=g).tolist()
           for _ in range(n_img)]
    img, cut, _ = _brute(ids, kp, per)
    assert frame_cuts(ids, kp, per) == (img, cut)
    # a frame's cut keeps exactly the first min(k, n_i) real tokens of its image and leaves the others alone
    tok = token_image(ids, kp)
    ks = [k for ks_ in per for k in ks_]
    for f, (i, c) in enumerate(zip(img, cut)):
        m = prefix_key_pad(ids, kp, [c if j == i else None for j in range(n_img)])
        left = torch.where(m, torch.full_like(tok, -1), tok)
        assert int((left == i).sum()) == min(ks[f], int((tok == i).sum())), (f, i, c)
        assert torch.equal(left[tok != i], tok[tok != i])
        kept, dropped = (left == i).nonzero()[:, 1], ((tok == i) & m).nonzero()[:, 1]
        assert not len(kept) or not len(dropped) or int(kept.max()) < int(dropped.min())


def test_frame_cuts_on_the_tokens_of_one_row(pkg):
    from dct_autoencoder_amd.progressive import frame_cuts
    ids = torch.tensor([[0, 0, 1, 1, 1, 0], [0, 0, 0, 0, 0, 0]])
    kp = torch.tensor([[0, 1, 0, 0, 1, 0], [1, 1, 1, 1, 1, 1]]).bool()
    # image 0: real slots 0, 5; image 1: slots 2, 3; image 2 (the padded row): none
    assert frame_cuts(ids, kp, [0, 1, 2, 9]) == ([0] * 4 + [1] * 4 + [2] * 4, [0, 1, 6, 6, 0, 3, 4, 4, 0, 0, 0, 0])
    assert frame_cuts(ids, kp, [[1], [2], []]) == ([0, 1], [1, 4])
    assert frame_cuts(ids, kp, []) == ([], [])


# ---- argument checks, no device ------------------------------------------------------------
def test_argument_checks_come_first(pkg):
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 8)
    S = 8
    x = pkg.DCTPatches(patches=torch.zeros(1, S, 196), key_pad_mask=torch.zeros(1, S, dtype=torch.bool),
                       batched_image_ids=torch.zeros(1, S, dtype=torch.long),
                       patch_channels=torch.zeros(1, S, dtype=torch.long),
                       patch_positions=torch.zeros(1, S, 2, dtype=torch.long), patch_sizes=[(2, 2)],
                       original_sizes=[(28, 28)])
    lfq = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).eval()
    lfq16 = pkg.LFQ(dim=256, codebook_size=2 ** 16, num_codebooks=16).eval()
    pn = pkg.PatchNorm(32, 32, 14, 3)
    codes = torch.zeros(1, S, 14, dtype=torch.long)
    with pytest.raises(ValueError, match=">= 0"):
        fe.postprocess_prefixes(x, [1, -1])
    with pytest.raises(ValueError, match=">= 0"):
        fe.decode_prefixes(x, codes, pn, lfq, [[-3]])
    with pytest.raises(ValueError, match="per-image"):
        fe.postprocess_prefixes(x, [[1], [2]])
    with pytest.raises(ValueError):
        fe.postprocess_prefixes(x, [1, [2]])
    with pytest.raises(ValueError, match="clip"):
        fe.postprocess_prefixes(x, [1], clip="max")
    with pytest.raises(TypeError, match="float32 or torch.uint8"):
        fe.postprocess_prefixes(x, [1], output_dtype=torch.float16)
    with pytest.raises(TypeError, match="float32 or torch.uint8"):
        fe.decode_prefixes(x, codes, pn, lfq, [1], output_dtype=torch.int8)
    with pytest.raises(TypeError, match="int64 or torch.int16"):
        fe.decode_prefixes(x, codes.int(), pn, lfq, [1])
    with pytest.raises(ValueError, match="codebook_dim"):
        fe.decode_prefixes(x, torch.zeros(1, S, 16, dtype=torch.int16), pn, lfq16, [1])
    with pytest.raises(TypeError):
        fe.image_clip([torch.zeros(3, 4, 4, dtype=torch.float64)])
    with pytest.raises(ValueError):
        fe.image_clip([torch.zeros(1, 4, 4)])
    with pytest.raises(TypeError):
        fe.image_clip([torch.zeros(3, 4, 4)], output_dtype=torch.float16)
    with pytest.raises(ValueError):
        pkg.image_clip(torch.zeros(4, 4))
    # well-formed arguments on CPU tensors get as far as the device check
    with pytest.raises(pkg.DCTAEUnavailable):
        fe.postprocess_prefixes(x, [1])
    with pytest.raises(pkg.DCTAEUnavailable):
        fe.image_clip([torch.zeros(3, 4, 4)])
    assert fe.image_clip([]) == []


# ---- the recorded reference ------------------------------------------------------------------
def test_clip_mirror_is_the_reference(pkg):
    g = golden("progressive_ref.npz")
    n = len([k for k in g.files if k.startswith("clip") and k.endswith("_in")])
    assert n >= 4
    for i in range(n):
        x, want = g[f"clip{i}_in"], g[f"clip{i}_out"]
        got = clip_mirror(x)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), i
    assert np.isnan(g[f"clip{n - 1}_out"]).all() and g["clip1_in"].min() < 0 and g["clip1_in"].max() > 1


@pytest.mark.parametrize("j", [0, 1])
def test_masked_batch_gives_the_pixels_of_the_reference_slice(pkg, j):
    g = golden("progressive_ref.npz")
    pre = f"im{j}_"
    cfg = ref_cpu.FEConfig(patch_size=14, max_patch_h=4, max_patch_w=4, max_seq_len=48)
    kp = torch.from_numpy(g[pre + "key_pad_mask"])
    n = int((~kp).sum())
    assert list(g[pre + "prefixes"]) == [1, 2, 3, n // 2, n - 1, n]
    from dct_autoencoder_amd.progressive import frame_cuts, prefix_key_pad
    ids = torch.from_numpy(g[pre + "batched_image_ids"]).long()
    for i in g[pre + "prefixes"]:
        (_, (cut,)) = frame_cuts(ids, kp, [int(i)])
        assert cut == int(i)   # one image, no interior pads: the cut is the reference's slice
        batch = ref_cpu.Batch(patches=torch.from_numpy(g[pre + "patches"]), key_pad_mask=prefix_key_pad(ids, kp, [cut]),
                              attn_mask=None, batched_image_ids=ids,
                              patch_channels=torch.from_numpy(g[pre + "patch_channels"]).long(),
                              patch_positions=torch.from_numpy(g[pre + "patch_positions"]).long(),
                              patch_sizes=[tuple(int(v) for v in g[pre + "patch_size"])],
                              original_sizes=[tuple(int(v) for v in g[pre + "original_size"])])
        (rgb,) = ref_cpu.postprocess(batch, cfg)
        np.testing.assert_allclose(rgb.numpy(), g[f"{pre}rgb{int(i)}"], rtol=1e-6, atol=1e-6)
