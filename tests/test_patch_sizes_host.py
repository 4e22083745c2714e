"""The CPU oracle against the reference at patch sizes other than 14
(tests/golden/patch_sizes_ref.npz: the reference's own preprocess, packing,
PatchNorm (eval) and LFQ (eval) at P in {16, 15, 8, 7, 5, 2, 1}, see
tests/golden/gen_patch_sizes_golden.py).  No GPU.

oracle.ref_cpu reproduces the file: tokens, positions, channels and codes bit
for bit; token order equal except inside runs of bit-equal reference scores
(the reference's sort is unstable there), where the oracle's order must be
flat-index ascending.  This is what lets tests/test_gpu_patch_sizes.py use
the oracle as its reference at P != 14.

Like the other bit-exact pins of tests/test_oracle.py, the comparison holds on
the build container's CPU, where the golden file was made: a host whose FFT
rounds the oracle's DCT differently gets other token bits.
"""
import hashlib

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import ref_cpu, rng

G = golden("patch_sizes_ref.npz")
CASES = [(int(P), int(mh), int(mw), [tuple(int(v) for v in s) for s in G[f"case{i}_sizes"]],
          [int(c) for c in G[f"case{i}_cds"]]) for i, (P, mh, mw) in enumerate(G["cases"])]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


def _tables(P, mh, mw):
    g = torch.Generator().manual_seed(P)
    median = torch.randn(3, mh, mw, P * P, generator=g) * 0.05
    b = torch.rand(3, mh, mw, P * P, generator=g) * 0.1 + 0.01
    return ref_cpu.NormTables(torch.ones(3, mh, mw), median, b)


def test_table_is_the_issue_table():
    assert [(c[0], c[1], c[2]) for c in CASES] == [(16, 32, 32), (15, 32, 32), (8, 32, 32), (7, 32, 32), (5, 6, 9),
                                                   (2, 40, 40), (1, 8, 8)]


@pytest.mark.parametrize("case", CASES, ids=[f"P{c[0]}" for c in CASES])
def test_oracle_reproduces_reference(case):
    P, mh, mw, sizes, cds = case
    cfg = ref_cpu.FEConfig(patch_size=P, max_patch_h=mh, max_patch_w=mw, max_seq_len=3 * mh * mw)
    pre = f"p{P}_"
    imgs = [torch.from_numpy(x) for x in rng.synth_images(100 + P, sizes)]
    perms = []          # per image: oracle token j is the reference's token perm[j]
    ties = 0
    for i, x in enumerate(imgs):
        it = ref_cpu.preprocess(x, cfg)
        ip = f"{pre}img{i}_"
        rpos = G[ip + "positions"].astype(np.int64)
        rch = G[ip + "channels"].astype(np.int64)
        rsc = G[ip + "scores"]
        assert tuple(G[ip + "original_size"]) == tuple(it["original_sizes"])
        assert tuple(G[ip + "patch_size"]) == tuple(it["patch_sizes"])
        opos, och = it["positions"].numpy(), it["channels"].numpy()
        assert opos.shape == rpos.shape and och.shape == rch.shape
        rmap = {(int(c), int(p[0]), int(p[1])): j for j, (p, c) in enumerate(zip(rpos, rch))}
        assert len(rmap) == len(rch)
        perm = np.array([rmap[(int(c), int(p[0]), int(p[1]))] for p, c in zip(opos, och)])
        assert sorted(perm.tolist()) == list(range(len(perm)))
        # a token moved only inside a run of bit-equal reference scores (rsc is sorted)
        assert np.all(rsc[1:] <= rsc[:-1])
        assert np.array_equal(rsc[perm].view(np.int32), rsc.view(np.int32))
        # ... and inside such a run the oracle's order is flat-index ascending
        qw = min(int(G[ip + "patch_size"][1]), mw)
        flat = (opos[:, 0] * qw + opos[:, 1]) * 3 + och
        tied = rsc[1:].view(np.int32) == rsc[:-1].view(np.int32)
        assert np.all(flat[1:][tied] > flat[:-1][tied])
        ties += int(tied.sum())
        if not tied.any():
            assert np.array_equal(perm, np.arange(len(perm)))
        # tokens bit for bit, in the reference's order
        inv = np.argsort(perm)
        toks = it["patches"].numpy()[inv]
        assert _sha(toks) == G[ip + "patches_sha"].tobytes()
        assert np.array_equal(toks[:8].view(np.int32), G[ip + "patches_head"].view(np.int32))
        assert np.array_equal(toks[-8:].view(np.int32), G[ip + "patches_tail"].view(np.int32))
        if ip + "patches" in G.files:
            assert np.array_equal(toks.view(np.int32), G[ip + "patches"].view(np.int32))
        perms.append(perm)
    if P == 2:
        assert ties > 0, "the P = 2 images are there for their score ties"
    # packed batch + PatchNorm + LFQ, every grouping
    tabs = _tables(P, mh, mw)
    rkp = G[pre + "key_pad_mask"]
    rids = G[pre + "batched_image_ids"].astype(np.int64)
    for n, cd in enumerate(cds):
        lcfg = ref_cpu.LFQConfig(dim=P * P, codebook_size=2 ** cd, num_codebooks=P * P // cd)
        ((ob, oidx),) = ref_cpu.encode(imgs, cfg, tabs, lcfg)
        assert np.array_equal(ob.key_pad_mask.numpy(), rkp)
        assert np.array_equal(ob.batched_image_ids.numpy(), rids)
        # the oracle's batch in the reference's token order: per image the permutation above
        src = np.tile(np.arange(rkp.shape[1]), (rkp.shape[0], 1))
        i = 0
        for r in range(rkp.shape[0]):
            col = 0
            for im in np.unique(rids[r][~rkp[r]]):
                k = len(perms[i])
                assert np.all(rids[r, col:col + k] == im)
                src[r, col:col + k] = col + np.argsort(perms[i])
                col += k
                i += 1
        assert i == len(imgs)
        rows = np.arange(rkp.shape[0])[:, None]
        assert np.array_equal(ob.patch_positions.numpy()[rows, src], G[pre + "patch_positions"].astype(np.int64))
        assert np.array_equal(ob.patch_channels.numpy()[rows, src], G[pre + "patch_channels"].astype(np.int64))
        codes = oidx.numpy().astype(np.int64)[rows, src]
        assert codes.shape == (*rkp.shape, P * P // cd)
        assert _sha(codes) == G[f"{pre}codes_cd{cd}_sha"].tobytes(), cd
        if n == 0:
            rc = G[f"{pre}codes_cd{cd}"].astype(np.int64)
            if P * P // cd == 1:   # the reference drops the codebook axis of a single codebook (lfq.py:83)
                assert rc.shape == rkp.shape
                rc = rc[..., None]
            assert np.array_equal(codes, rc)
