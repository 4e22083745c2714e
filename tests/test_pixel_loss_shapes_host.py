"""CPU side of test_gpu_pixel_loss_shapes.py: that every case of
oracle/decode_cases.py reaches the edge it is there for, by arithmetic from its
sizes and the constants read out of the library's sources (a changed tile,
chunk, grid cap or threshold makes the assertion of the case that no longer
reaches its edge fail); that the case builder packs as the reference did (the
recorded ragged14 batch); and the structure of the float64 / fp32 oracle's
gradients on every case."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import decode_cases as D
from test_pixel_loss_host import CFG, G

CSRC = os.path.join(ROOT, "dct-autoencoder_amd", "csrc")


def constant(file, pattern):
    with open(os.path.join(CSRC, file)) as f:
        m = re.findall(pattern, f.read())
    assert len(m) == 1, f"{file}: expected one match of {pattern!r}, found {len(m)}; update this test with the code"
    return int(m[0])


XK = constant("dctae_gemm_x3.hip", r"constexpr int XK = (\d+);")                       # k chunk
TILE = constant("dctae_plan.hip", r"g\.tile_m = g\.tile_n = (\d+);")                  # per-channel operand
TILE_SH = constant("dctae_plan.hip", r"if \(sh == 1\) g\.tile_n = (\d+);")             # shared DCT matrix
assert TILE_SH == constant("dctae_plan.hip", r"if \(sh == 2\) g\.tile_m = (\d+);")
DEAL_MIN = constant("dctae_plan.hip", r"if \(t\.size\(\) < (\d+) \|\| share == 0\) return;")
DEAL_PER_PROBLEM = constant("dctae_plan.hip", r"per_problem = n_prob >= (\d+);")
THREADS = constant("dctae_decode_bwd.hip", r"constexpr int kThreads = (\d+);")
COLOR_BLOCKS = constant("dctae_decode_bwd.hip", r"\(4 \* kThreads\), (\d+)\);")
GATHER_BLOCKS = constant("dctae_decode_bwd.hip", r"/ kThreads, (\d+)\);")
FFT_SIDE = constant("dctae_decode.hip", r"fftdec = D\[i\]\.H == (\d+) && D\[i\]\.W == \1")


def kept(name, hw):
    """(Kh, Kw) of an image of the case: the kept corner of its spectrum"""
    P, (mh, mw), _, _ = D.CASES[name]
    return P * min(hw[0] // P, mh), P * min(hw[1] // P, mw)


def gemms(name, hw):
    """g1 .. g4 of dctae_decode_backward as (M, N, K, the side the shared DCT matrix is on)"""
    (H, W), (Kh, Kw) = hw, kept(name, hw)
    return {"g1": (H, Kw, Kh, "M"), "g2": (H, W, Kw, "N"), "g3": (H, Kw, W, "N"), "g4": (Kh, Kw, H, "M")}


def tiling(M, N, K, shared):
    """tiles and tails of one problem: (tiles_m, tail_m, tiles_n, tail_n, chunks, tail_k)"""
    tm, tn = (TILE_SH, TILE) if shared == "M" else (TILE, TILE_SH)
    return -(-M // tm), M % tm, -(-N // tn), N % tn, -(-K // XK), K % XK


def tiles(name, g):
    return sum(t[0] * t[2] for t in (tiling(*gemms(name, hw)[g]) for hw in D.CASES[name][3]))


def test_constants_are_the_documented_ones():
    """the figures the case table of decode_cases.py is written in"""
    assert (XK, TILE, TILE_SH) == (32, 64, 128)
    assert (DEAL_MIN, DEAL_PER_PROBLEM, THREADS, COLOR_BLOCKS, GATHER_BLOCKS, FFT_SIDE) == (16, 64, 256, 256, 16384, 512)


def test_mid_geometry():
    s = D.CASES["mid"][3]
    assert s == [(300, 262), (127, 257), (65, 129)] and D.CASES["holes"][3] == s
    # several tiles in both directions with ragged M, N and K tails at once
    tm, rm, tn, rn, ck, rk = tiling(*gemms("mid", s[0])["g2"])
    assert tm >= 3 and tn >= 3 and ck >= 3 and rm and rn and rk
    tm, rm, tn, rn, ck, rk = tiling(*gemms("mid", s[0])["g4"])
    assert tm >= 3 and tn >= 3 and ck >= 3 and rm and rn and rk
    assert kept("mid", s[1])[0] == TILE_SH - 2                    # Kh = 126: two short of the 128 tile (g4's M)
    assert s[1][1] == 8 * XK + 1                                  # g3's K: eight chunks and one element
    assert s[2] == (TILE + 1, TILE_SH + 1)                        # g2's M and N one past a tile
    assert D.build("mid").batch.patches.shape[0] == 1            # one row, three images


def test_p16_geometry():
    s = D.CASES["p16"][3]
    assert kept("p16", s[0]) == (TILE_SH, TILE_SH) and kept("p16", s[1]) == (TILE, TILE)    # full tiles, no tail
    assert s[0] == (TILE_SH + 1, TILE_SH + 2) and s[1] == (TILE, TILE + 1)
    assert kept("p16", s[1])[0] == 2 * XK and kept("p16", s[2])[1] == 10 * XK == s[2][1]    # K = 64 and 320: whole chunks
    assert tiling(*gemms("p16", s[1])["g1"])[4:] == (2, 0)
    assert tiling(*gemms("p16", s[2])["g2"])[5] == 0 and tiling(*gemms("p16", s[2])["g3"])[5] == 0


def test_caps_geometry():
    P, (mh, mw), S, s = D.CASES["caps"]
    rows_cap = P * max(mh, mw)
    for hw in s:
        assert kept("caps", hw) == (P * mh, P * mw) == (112, 168)
        assert hw[0] // P > mh and hw[1] // P > mw                 # patch_sizes above both caps
        assert rows_cap < hw[1] and rows_cap < hw[0]               # cached matrices with fewer rows than columns
        assert 4 * P * mh < hw[0] + hw[1]                          # Kh << H
    c = D.build("caps")
    assert [tuple(p) for p in c.batch.patch_sizes] == [(23, 36), (14, 32)] and c.batch.patches.shape[0] == 2


def test_big_geometry():
    s = D.CASES["big"][3]
    assert s == [(520, 600), (521, 97), (1000, 97)]
    hw = s[0][0] * s[0][1]
    # image 0 sits at offset 0 with hw % 4 == 0: the vectorised colour adjoint, whose grid is capped
    assert hw % 4 == 0 and -(-hw // (4 * THREADS)) > COLOR_BLOCKS and hw // 4 > COLOR_BLOCKS * THREADS
    assert (3 * s[1][0] * s[1][1]) % 4 != 0                        # misaligns the image after it ...
    off2 = 3 * hw + 3 * s[1][0] * s[1][1]
    assert (s[2][0] * s[2][1]) % 4 == 0 and off2 % 4 != 0          # ... which alone would take the float4 branch
    assert gemms("big", s[2])["g1"][0] == 1000 and gemms("big", s[2])["g4"][2] == 1000      # M = K = 1000
    assert tiling(*gemms("big", s[2])["g4"])[4:] == (32, 1000 % XK) and 1000 % XK


def test_512_geometry():
    s = D.CASES["mixed512"][3]
    assert s.count((FFT_SIDE, FFT_SIDE)) == 2 and any(hw != (FFT_SIDE, FFT_SIDE) for hw in s)   # the GEMM decode
    assert s[0] == (FFT_SIDE, FFT_SIDE) and s[1] != s[0]
    P, _, S, s = D.CASES["sq512x2"]
    assert s == [(FFT_SIDE, FFT_SIDE)] * 2                                                       # the FFT decode
    c = D.build("sq512x2")
    assert c.batch.patches.shape[0] == 2 and not c.batch.key_pad_mask.any() and S == 3 * 32 * 32  # every token


def test_p5_geometry():
    P, _, S, s = D.CASES["p5"]
    assert (P * P) % 4 != 0                                        # the scalar gather
    assert max(max(hw) for hw in s) > TILE_SH and int((~D.build("p5").batch.key_pad_mask).sum()) > S


def deal(name, g):
    """lane lengths of xcd_deal_tiles in its per-problem mode: every image's tiles to the least-loaded of 8 lanes"""
    lanes = [0] * 8
    for hw in D.CASES[name][3]:
        t = tiling(*gemms(name, hw)[g])
        lanes[lanes.index(min(lanes))] += t[0] * t[2]
    return lanes


def test_many_geometry():
    s = D.CASES["many72"][3]
    assert len(s) == 72 >= DEAL_PER_PROBLEM and all(28 <= v <= 90 for hw in s for v in hw)
    assert len(set(s)) > 60
    for g in ("g1", "g2", "g3", "g4"):
        assert tiles("many72", g) >= max(DEAL_MIN, len(s))        # one problem per image in every list
    # the lanes are padded to equal length with empty tiles
    assert any(len(set(deal("many72", g))) > 1 for g in ("g1", "g2", "g3", "g4"))
    assert max(tiling(*gemms("many72", hw)["g2"])[0] for hw in s) == 2    # an image's tiles: more than one per problem
    s = D.CASES["many300"][3]
    assert len(s) == 300 > THREADS                                 # the finish kernel's second round
    assert all(14 <= h <= 30 and 14 <= w <= 45 for h, w in s)
    c = D.build("many300")
    per_row = [len(torch.unique(r[~p])) for r, p in zip(c.batch.batched_image_ids, c.batch.key_pad_mask)]
    assert sum(per_row) == 300 and max(per_row) >= 8              # many ids per row of the LUT


def test_holes_and_zero():
    mid, c = D.build("mid"), D.build("holes")
    gone = c.batch.key_pad_mask & ~mid.batch.key_pad_mask
    pos, ch = c.batch.patch_positions, c.batch.patch_channels
    dc = (pos[..., 0] == 0) & (pos[..., 1] == 0)
    assert torch.equal(mid.batch.patches, c.batch.patches)
    assert int((gone & dc & (mid.img == 0)).sum()) >= 1 and bool((gone & dc & (mid.img == 0) & (ch == 0)).any())
    assert int((gone & dc & (mid.img == 1)).sum()) == 3            # every DC token of image 1
    share = float(gone.sum()) / float((mid.img >= 0).sum())
    assert 0.25 < share < 0.35
    assert all(int((c.img == i).sum()) >= 1 for i in range(3))
    assert bool((c.img[gone] == -1).all())
    # the removed slots lie between real ones
    assert bool(c.batch.key_pad_mask[0, :100].any()) and not bool(c.batch.key_pad_mask[0, :100].all())
    z = D.build("zero")
    assert z.zero_images == (1,) and torch.all(z.out[z.img == 1] == 0) and bool((z.out[z.img == 0] != 0).any())
    assert bool((z.batch.patches[z.img == 1] != 0).any())


@pytest.mark.parametrize("name", list(D.GRID_CAP))
def test_grid_cap_geometry(name):
    small, big, out2, outR, factors = D.grid_cap_case(name)
    P, _, S, s = D.CASES[name]
    R = D.GRID_CAP[name]
    U = P * P // 4 if (P * P) % 4 == 0 else P * P
    step = GATHER_BLOCKS * THREADS
    assert step == 4194304 and big.patches.shape == (R, S, P * P)
    assert R * S * U > step                                        # the grid-stride loop's second iteration ...
    assert (R - 1) * S >= -(-step // U)                            # ... owns every unit of the last row
    assert R * S < 2 ** 31 and 4 * R * S * P * P < 100e6           # and the batch is small
    assert not big.key_pad_mask[0].all() and not big.key_pad_mask[R - 1].all() and big.key_pad_mask[1:R - 1].all()
    assert torch.equal(big.patches[0], small.patches[0]) and torch.equal(big.patches[R - 1], small.patches[1])
    assert len(big.original_sizes) == len(s) + R - 2 and big.original_sizes[0] == s[0]
    assert list(big.original_sizes[R - 1:]) == s[1:]
    assert (3 * D.PLACEHOLDER[0] * D.PLACEHOLDER[1]) % 4 == 0


def test_builder_reproduces_the_recorded_packing():
    """fed the images, sizes and config of the recorded ragged14 batch (gen_pixel_loss_golden.py:
    torch.rand of generator 900), the builder gives the reference's own packing"""
    name = "ragged14"
    P, mh, mw, S = CFG[name]
    g = torch.Generator().manual_seed(900)
    images = [torch.rand(3, int(h), int(w), generator=g) for h, w in G[f"{name}_original_sizes"]]
    b = D.pack(images, D.ref_cpu.FEConfig(patch_size=P, max_patch_h=mh, max_patch_w=mw, max_seq_len=S))
    assert np.array_equal(b.key_pad_mask.numpy(), G[f"{name}_key_pad"])
    assert np.array_equal(b.batched_image_ids.numpy(), G[f"{name}_ids"])
    assert np.array_equal(b.patch_positions.numpy(), G[f"{name}_pos"])
    assert np.array_equal(b.patch_channels.numpy(), G[f"{name}_ch"])
    assert [tuple(s) for s in b.original_sizes] == [tuple(s) for s in G[f"{name}_original_sizes"]]
    assert [tuple(s) for s in b.patch_sizes] == [tuple(s) for s in G[f"{name}_patch_sizes"]]
    assert np.abs(b.patches.numpy() - G[f"{name}_patches"]).max() <= 1e-4 * np.abs(G[f"{name}_patches"]).max()
    assert np.array_equal(D.token_image(b.batched_image_ids, b.key_pad_mask).numpy()[0, :3], [0, 0, 0])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", D.NAMES)
def test_oracle_structure(name, dtype):
    c, r = D.build(name), D.results(name, dtype)
    kp, img = c.batch.key_pad_mask.numpy(), c.img.numpy()
    assert np.array_equal(img < 0, kp) and np.isfinite(r["loss"]) and r["loss"] > 0
    assert len(r["x"]) == len(r["x_hat"]) == len(c.sizes)
    for key in ("grad", "vjp"):
        g = r[key]
        assert g.dtype == (np.float64 if dtype == torch.float64 else np.float32) and np.isfinite(g).all()
        assert np.all(g[kp] == 0), "padded tokens get exact zeros"
        hit = np.abs(g).max(axis=-1) > 0
        for i in range(len(c.sizes)):
            assert (not hit[img == i].any()) if i in c.zero_images else hit[img == i].all()
    for i in c.zero_images:
        assert torch.all(r["x_hat"][i] == 0)
