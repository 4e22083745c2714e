"""CPU-only checks of the decode family's layouts (csrc/dctae_dec_layout.h): a
small host program that includes only that header fills ImgDescs by the
arithmetic of decode_geometry (dctae_decode.hip: qh = min(ph, cap),
Kh = P qh), patch 14, caps 32 x 32, and prints the path choice, the forward
layout of a list of targets (the images of a plain decode, the sorted frames of
dctae_decode_frames) and the backward's layout.

The pinned values are worked out by hand from the formulas of the parent's
decode_impl / decode_fft / decode_frames_impl / dctae_decode_backward, all in
floats; up64 rounds up to 64:

GEMM path, per target unrounded: ws_y, then ws_t = ws_y + 3 Kh Kw, then
ws_p = ws_t + 3 H Kw, then 3 H W; map_off = up64(wsf); map_n = 3 * 32 * 32 = 3072
per target; with clip mm_off = up64(map_off + map_n) and two words per target;
staged (clip to bytes) every target then gets up64(end) and 3 H W floats.

* 300 x 262 (21 x 18 patches): Kh = 294, Kw = 252.  Y = 3 * 294 * 252 = 222264,
  U = 3 * 300 * 252 = 226800, ipt = 3 * 300 * 262 = 235800: regions at 0, 222264,
  449064; wsf = 684864 = 10701 * 64 = map_off; request (684864 + 3072) * 4 =
  2751744 bytes.
* 30 x 45 (2 x 3): Kh = 28, Kw = 42: Y = 3528, U = 3 * 30 * 42 = 3780,
  ipt = 3 * 30 * 45 = 4050: regions 0, 3528, 7308, end 11358.  17 x 14 (1 x 1):
  Kh = Kw = 14: Y = 588, U = 3 * 17 * 14 = 714, ipt = 714: regions 11358, 11946,
  12660; wsf = 13374, no multiple of 64: map_off = 209 * 64 = 13376;
  map_n = 6144; request (13376 + 6144) * 4 = 78080.  With clip to fp32:
  mm_off = 19520 = 305 * 64, request (19520 + 4) * 4 = 78096.
* frames 30 x 45, 30 x 45, 17 x 14 staged: wsf = 2 * 11358 + 2016 = 24732,
  map_off = 387 * 64 = 24768, map_n = 9216, mm_off = 33984 = 531 * 64, end
  33990; staging at 34048, then 34048 + 4050 = 38098 -> 38144, then 42194 ->
  42240; request (42240 + 714) * 4 = 171816.  Unstaged, no clip:
  (24768 + 9216) * 4 = 135936.
* two frames of 300 x 262 staged: wsf = 1369728 = map_off, map_n = 6144,
  mm_off = 1375872 = 21498 * 64, end 1375876 -> staging at 1375936, then
  1375936 + 235800 = 1611736 -> 25184 * 64 = 1611776; request
  (1611776 + 235800) * 4 = 7390304.  Unstaged, no clip: 1375872 * 4 = 5503488.

FFT path, per target ws_t alone, up64(3 H Kw), row blocks (target, y0) every 16
rows; map_off = wsf:

* two 512 x 512 at qw = 32: Kw = 448, 3 * 512 * 448 = 688128 = 10752 * 64:
  ws_t = 0, 688128; map_off = 1376256; request (1376256 + 6144) * 4 = 5529600;
  2 * 32 = 64 row blocks.
* three at qw = 20 (36 x 20 patches, qh = 32): Kw = 280, 3 * 512 * 280 = 430080 =
  6720 * 64: ws_t = 0, 430080, 860160; request (1290240 + 9216) * 4 = 5197824;
  96 row blocks.

Backward (every Y first, then U / T and ipt per image, each up64), images
30 x 45 and 17 x 14: Y 3528 -> 3584 and 588 -> 640: ws_y = 0, 3584,
y_floats = 4224.  Image 0: ws_t = 4224, U 3780 -> 3840, ws_p = 8064, ipt 4050 ->
4096; image 1: ws_t = 12160, 714 -> 768, ws_p = 12928, 768 more: map_off = 13696,
map_n = 6144, dc_off = up64(19840) = 19840 = 310 * 64; request
(19840 + 6) * 4 = 79384.  No image: everything 0 and the 512-byte floor.

progressive._frame_scratch_bytes (the chunking's per-frame bound) is
4 * (3 (Kh Kw + H Kw + H W) + 3072 + 256), staged 4 * (3 H W + 64) more:
300 x 262: 4 * 688192 = 2752768, staged 3696224; 30 x 45: 4 * 14686 = 58744,
staged 75200; 17 x 14: 4 * 5344 = 21376, staged 24488.  Sums: staged
2 * 3696224 = 7392448 >= 7390304 and 2 * 75200 + 24488 = 174888 >= 171816;
unstaged 5505536 >= 5503488 and 138864 >= 135936.
"""
import os
import subprocess
import types

import pytest

from conftest import ROOT
from test_options_host import _compiler

CSRC = os.path.join(ROOT, "dct-autoencoder_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h")),
                                reason="no HIP headers")

PROGRAM = r"""
#include "%s/dctae_dec_layout.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace dctae;
// fwd fft clip staged                                         H W ph pw ...
// bwd                                                         H W ph pw ...
// path fft_decode dec_rows_kernel dec_cols_kernel P codes cb_dim ncb cap   H W ph pw ...
int main(int argc, char** argv) {
  const bool fwd = !std::strcmp(argv[1], "fwd"), path = !std::strcmp(argv[1], "path");
  const int P = 14, cap = path ? std::atoi(argv[9]) : 32;
  std::vector<ImgDesc> D;
  for (int a = fwd ? 5 : path ? 10 : 2; a + 3 < argc; a += 4) {
    ImgDesc d;
    std::memset(&d, 0, sizeof(d));
    d.H = std::atoi(argv[a]), d.W = std::atoi(argv[a + 1]);
    d.ph = std::atoi(argv[a + 2]), d.pw = std::atoi(argv[a + 3]);
    d.qh = std::min(d.ph, cap), d.qw = std::min(d.pw, cap);
    d.Kh = P * d.qh, d.Kw = P * d.qw;
    d.rgb_off = 1000 + (int64_t)D.size();   // the caller's offset: kept unless staged
    D.push_back(d);
  }
  const int n = (int)D.size();
  if (path) {
    Options opt;
    opt.fft_decode = std::atoi(argv[2]), opt.dec_rows_kernel = std::atoi(argv[3]);
    opt.dec_cols_kernel = std::atoi(argv[4]);
    const DecPath p = decode_path(opt, std::atoi(argv[5]), std::atoi(argv[6]) != 0, std::atoi(argv[7]),
                                  std::atoi(argv[8]), D.data(), n);
    std::printf("%%d %%d %%d\n", (int)p.fft, (int)p.rows512, (int)p.band);
  } else if (fwd) {
    const DecLayout L = decode_layout(D.data(), n, std::atoi(argv[2]) != 0, cap, cap, std::atoi(argv[3]) != 0,
                                      std::atoi(argv[4]) != 0);
    std::printf("lay %%lld %%lld %%lld %%lld %%lld\n", (long long)L.wsf, (long long)L.map_off, (long long)L.map_n,
                (long long)L.mm_off, (long long)L.total * 4);
    for (const int2& b : L.row_blocks) std::printf("rb %%d %%d\n", b.x, b.y);
  } else {
    const DecBwdLayout L = decode_bwd_layout(D.data(), n, cap, cap);
    std::printf("lay %%lld %%lld %%lld %%lld %%zu\n", (long long)L.y_floats, (long long)L.map_off, (long long)L.map_n,
                (long long)L.dc_off, L.request);
  }
  for (const ImgDesc& d : D)
    std::printf("tg %%lld %%lld %%lld %%lld\n", (long long)d.ws_y, (long long)d.ws_t, (long long)d.ws_p,
                (long long)d.rgb_off);
  return 0;
}
"""

FLAGS = ["-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include"]

BIG = (300, 262, 21, 18)
A, B = (30, 45, 2, 3), (17, 14, 1, 1)
SQ32, SQ20 = (512, 512, 36, 36), (512, 512, 36, 20)


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("dec_layout")
    (d / "layout_main.cpp").write_text(PROGRAM % CSRC)
    exe = str(d / "layout")
    subprocess.run(_compiler() + FLAGS + ["-o", exe, str(d / "layout_main.cpp")], check=True)

    def call(head, imgs):
        args = [str(v) for v in head] + [str(v) for im in imgs for v in im]
        return subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.splitlines()

    def rows(out, tag):
        return [tuple(int(v) for v in l.split()[1:]) for l in out if l.startswith(tag + " ")]

    def fwd(imgs, fft=False, clip=False, staged=False):
        """-> dict(wsf, map_off, map_n, mm_off, request), [(ws_y, ws_t, ws_p, rgb_off)], [(target, y0)]"""
        out = call(["fwd", int(fft), int(clip), int(staged)], imgs)
        (lay,) = rows(out, "lay")
        return dict(zip(("wsf", "map_off", "map_n", "mm_off", "request"), lay)), rows(out, "tg"), rows(out, "rb")

    def bwd(imgs):
        out = call(["bwd"], imgs)
        (lay,) = rows(out, "lay")
        return dict(zip(("y_floats", "map_off", "map_n", "dc_off", "request"), lay)), rows(out, "tg")

    def path(imgs, fft_decode=1, rows_kernel=3, cols_kernel=2, P=14, codes=None, cap=32):
        """codes: None, or (codebook_dim, num_codebooks) -> (fft, rows512, band)"""
        cb = (1,) + tuple(codes) if codes else (0, 0, 0)
        line = call(["path", fft_decode, rows_kernel, cols_kernel, P, *cb, cap], imgs)[0]
        return tuple(int(v) for v in line.split())

    fwd.bwd, fwd.path = bwd, path
    return fwd


def test_pinned_gemm_image(layout):
    lay, tg, rb = layout([BIG])
    assert tg == [(0, 222264, 449064, 1000)] and rb == []
    assert (lay["wsf"], lay["map_off"], lay["map_n"], lay["request"]) == (684864, 684864, 3072, 2751744)


def test_pinned_gemm_pair_off_the_boundary(layout):
    lay, tg, _ = layout([A, B])
    assert [t[:3] for t in tg] == [(0, 3528, 7308), (11358, 11946, 12660)]
    assert (lay["wsf"], lay["map_off"], lay["map_n"], lay["request"]) == (13374, 13376, 6144, 78080)
    lay, tg2, _ = layout([A, B], clip=True)
    assert tg2 == tg and (lay["mm_off"], lay["request"]) == (19520, 78096)
    assert [t[3] for t in tg] == [1000, 1001]   # unstaged: the caller's offsets stay


def test_pinned_staged_frames(layout):
    lay, tg, _ = layout([A, A, B], clip=True, staged=True)
    assert (lay["wsf"], lay["map_off"], lay["map_n"], lay["mm_off"]) == (24732, 24768, 9216, 33984)
    assert [t[3] for t in tg] == [34048, 38144, 42240] and lay["request"] == 171816
    assert [t[0] for t in tg] == [0, 11358, 22716]
    lay, tg, _ = layout([BIG, BIG], clip=True, staged=True)
    assert lay["wsf"] == 1369728 and [t[3] for t in tg] == [1375936, 1611776] and lay["request"] == 7390304


def test_pinned_fft(layout):
    lay, tg, rb = layout([SQ32, SQ32], fft=True)
    assert [t[1] for t in tg] == [0, 688128] and lay["map_off"] == lay["wsf"] == 1376256
    assert lay["request"] == 5529600 and rb == [(g, y) for g in range(2) for y in range(0, 512, 16)] and len(rb) == 64
    lay, tg, rb = layout([SQ20] * 3, fft=True)
    assert [t[1] for t in tg] == [0, 430080, 860160] and lay["request"] == 5197824
    assert rb == [(g, y) for g in range(3) for y in range(0, 512, 16)] and len(rb) == 96
    assert all(t[0] == 0 and t[2] == 0 for t in tg)   # no Y, no ipt image on this path


def _plain(imgs, fft):
    """the parent's plain decode (decode_impl / decode_fft): the region offsets and the scratch request in bytes"""
    wsf, offs = 0, []
    for h, w, ph, pw in imgs:
        kh, kw = 14 * min(ph, 32), 14 * min(pw, 32)
        if fft:
            offs.append((0, wsf, 0))
            wsf += (3 * h * kw + 63) // 64 * 64
        else:
            offs.append((wsf, wsf + 3 * kh * kw, wsf + 3 * kh * kw + 3 * h * kw))
            wsf += 3 * (kh * kw + h * kw + h * w)
    map_n = len(imgs) * 3 * 32 * 32
    return offs, ((wsf if fft else (wsf + 63) // 64 * 64) + map_n) * 4


@pytest.mark.parametrize("imgs,fft", [([BIG], False), ([A, B], False), ([A, A, B], False), ([BIG, BIG], False),
                                      ([SQ32, SQ32], True), ([SQ20] * 3, True)])
def test_plain_equals_frames(layout, imgs, fft):
    """n frames without clip are laid out as the plain decode lays out n images of their geometry"""
    lay, tg, _ = layout(imgs, fft=fft)
    offs, request = _plain(imgs, fft)
    assert [t[:3] for t in tg] == offs and lay["request"] == request
    assert [t[3] for t in tg] == [1000 + g for g in range(len(imgs))]


def test_path_choice(layout):
    path = layout.path
    assert path([SQ32, SQ32]) == (1, 1, 1)
    assert path([SQ32], codes=(14, 14)) == (1, 1, 1)
    assert path([SQ32], cols_kernel=1) == (1, 1, 0)       # band only with dec_cols_kernel == 2
    assert path([SQ32], rows_kernel=2) == (1, 0, 0)       # rows512 only with dec_rows_kernel == 3 ...
    assert path([SQ20, SQ20]) == (1, 0, 0)                # ... and only at qw == 32
    assert path([(512, 512, 20, 36)] * 2) == (1, 1, 1)    # qh below 32 is served
    # one failing case per clause
    assert path([SQ32], fft_decode=0) == (0, 0, 0)
    assert path([SQ32], P=16) == (0, 0, 0)
    assert path([SQ32], codes=(7, 28)) == (0, 0, 0)
    assert path([SQ32], codes=(14, 13)) == (0, 0, 0)
    assert path([SQ32, (512, 510, 36, 36)]) == (0, 0, 0)
    assert path([(510, 512, 36, 36), SQ32]) == (0, 0, 0)
    assert path([SQ32, SQ20]) == (0, 0, 0)                # unequal qw
    # qh <= 32 holds at caps 32 x 32 (qh = min(ph, 32)); the clause guards larger caps: 36 kept tile rows
    assert path([(512, 512, 36, 32)], cap=36) == (0, 0, 0) and path([(512, 512, 36, 32)]) == (1, 1, 1)


def test_pinned_backward(layout):
    lay, tg = layout.bwd([A, B])
    assert [t[:3] for t in tg] == [(0, 4224, 8064), (3584, 12160, 12928)]
    assert lay == dict(y_floats=4224, map_off=13696, map_n=6144, dc_off=19840, request=79384)
    lay, tg = layout.bwd([])
    assert tg == [] and lay == dict(y_floats=0, map_off=0, map_n=0, dc_off=0, request=512)


def test_python_bound_covers_the_request(layout, pkg):
    from dct_autoencoder_amd.progressive import _frame_scratch_bytes
    p = types.SimpleNamespace(patch_size=14, max_patch_h=32, max_patch_w=32)
    for frames, staged, bound in (([BIG, BIG], True, 7392448), ([A, A, B], True, 174888),
                                  ([BIG, BIG], False, 5505536), ([A, A, B], False, 138864)):
        total = sum(_frame_scratch_bytes(p, (h, w), (ph, pw), staged) for h, w, ph, pw in frames)
        lay, _, _ = layout(frames, clip=staged, staged=staged)
        assert total == bound and total >= lay["request"], (frames, staged, total, lay["request"])
    # clip to fp32 adds the min / max words only: still inside the unstaged bound
    assert layout([A, A, B], clip=True)[0]["request"] <= 138864
