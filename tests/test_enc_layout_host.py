"""CPU-only checks of the encode plan's layouts (csrc/dctae_enc_layout.h): a
small host program that includes only that header fills ImgDescs by the
arithmetic of describe() (dctae_plan.hip), takes each side's route from the
command line and prints the chunk cut, the workspace layout and the staging
carve.  The XCD dealing of the column blocks (dctae_plan.hip) is called in the
built library by a second program.

The pinned values are worked out by hand from the formulas of the parent's
build_encode_plan (regions in floats, each rounded up to 64 floats in the
offset pass; the job's |max| words 3 n + 9 rounded up to 64 after them;
ws_need in bytes), patch 14, caps 32 x 32:

* 512 x 512, both sides FFT: Kh = Kw = 14 * 32 = 448, only T is kept:
  3 * 448 * 512 = 688128 floats, a multiple of 64, so ws_t = 688128 i.
  Eight images: amax_off = 8 * 688128 = 5505024; the |max| words
  3 * 8 + 9 = 33 round up to 64; ws_need = (5505024 + 64) * 4 = 22020352.
  The cut counts (688128 + 64) * 4 = 2752768 bytes per image: 8 fit one job
  under the default chunk_bytes (2^40), one image per job under 4 << 20
  (two would be 5505536 > 4194304).
* staging, codes only, ncb 14, 8 * 3072 = 24576 tokens: need =
  24576 * (4 + 2 * 14) + 4096 = 790528; scores at 0 take 24576 * 4 = 98304
  bytes (a multiple of 256), so the codes start at 98304.
* 300 x 262, both sides GEMM: qh = 21, qw = 18, Kh = 294, Kw = 252.
  T = 3 * 252 * 300 = 226800 -> 226816 (ws_t = 0, ws_p = 226816);
  IPT = 3 * 300 * 262 = 235800 -> 235840 (ws_y = 462656);
  Y = 3 * 294 * 252 = 222264 -> 222272 (amax_off = 684928);
  3 + 9 = 12 words -> 64; ws_need = (684928 + 64) * 4 = 2739968.
"""
import itertools
import os
import subprocess

import pytest

from conftest import ROOT
from oracle import rng
from test_options_host import _compiler

CSRC = os.path.join(ROOT, "dct-autoencoder_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h")),
                                reason="no HIP headers")
G, B, F = 0, 1, 2   # a side's route: GEMM, Bluestein, FFT

PROGRAM = r"""
#include "%s/dctae_enc_layout.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace dctae;
// layout P cap chunk_bytes ws_limit  H W row_route col_route band ...   |   stage n_tok ncb PP want_norm raw
int main(int argc, char** argv) {
  if (!std::strcmp(argv[1], "stage")) {
    const StageLayout s(std::atoll(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]) != 0,
                        std::atoi(argv[6]) != 0);
    std::printf("%%zu %%zu %%zu %%zu %%zu\n", s.scores, s.codes, s.norm, s.raw, s.need);
    return 0;
  }
  const int P = std::atoi(argv[2]), cap = std::atoi(argv[3]);
  Options opt;
  opt.chunk_bytes = std::atoll(argv[4]);
  opt.ws_limit = std::atoll(argv[5]);
  std::vector<ImgDesc> D;
  for (int a = 6; a + 4 < argc; a += 5) {
    ImgDesc d;
    std::memset(&d, 0, sizeof(d));
    d.H = std::atoi(argv[a]), d.W = std::atoi(argv[a + 1]);
    d.ph = std::max(d.H / P, 1), d.pw = std::max(d.W / P, 1);
    d.qh = std::min(d.ph, cap), d.qw = std::min(d.pw, cap);
    d.Kh = P * d.qh, d.Kw = P * d.qw;
    d.T = 3 * d.qh * d.qw;
    const int r = std::atoi(argv[a + 2]), c = std::atoi(argv[a + 3]);
    d.plan_w = r == 0 ? -1 : 0, d.plan_h = c == 0 ? -1 : 0;
    d.bs = (r == 1 ? 1 : 0) | (c == 1 ? 2 : 0);
    d.tband = std::atoi(argv[a + 4]);
    if ((int)row_route(d) != r || (int)col_route(d) != (d.tband ? 3 : c)) return 2;
    D.push_back(d);
  }
  const WsLayout L = lay_out_workspace(D.data(), (int)D.size(), opt);
  std::printf("need %%zu\n", L.ws_need);
  for (const JobRange& j : L.jobs) std::printf("job %%d %%d %%lld\n", j.i0, j.i1, (long long)j.amax_off);
  for (const ImgDesc& d : D) {
    const Regions r = regions_of(d);
    std::printf("img %%lld %%lld %%lld %%lld %%lld %%lld %%lld %%d\n", (long long)d.ws_t, (long long)d.ws_p,
                (long long)d.ws_y, (long long)r.t, (long long)r.ipt, (long long)r.y, (long long)chunk_estimate(d),
                (int)all_fft(d));
  }
  return 0;
}
"""

DEAL = r"""
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
namespace dctae { void xcd_deal_col_blocks(std::vector<int4>& L); }
// argv: the tile-column count of each image; three channels each, in list order
int main(int argc, char** argv) {
  std::vector<int4> L;
  for (int i = 1; i < argc; ++i)
    for (int c = 0; c < 3; ++c)
      for (int w = 0; w < std::atoi(argv[i]); ++w) L.push_back(make_int4(i - 1, c, w, 1));
  dctae::xcd_deal_col_blocks(L);
  for (const int4& b : L) std::printf("%%d %%d %%d %%d\n", b.x, b.y, b.z, b.w);
  return 0;
}
"""

FLAGS = ["-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include"]


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("enc_layout")
    (d / "layout_main.cpp").write_text(PROGRAM % CSRC)
    exe = str(d / "layout")
    subprocess.run(_compiler() + FLAGS + ["-o", exe, str(d / "layout_main.cpp")], check=True)

    def run(imgs, P=14, cap=32, chunk_bytes=1 << 40, ws_limit=8 << 30):
        """imgs: (H, W, row route, column route, band) -> (ws_need, [(i0, i1, amax_off)], [per-image dict])"""
        args = [str(v) for im in imgs for v in im]
        out = subprocess.run([exe, "layout", str(P), str(cap), str(chunk_bytes), str(ws_limit)] + args, check=True,
                             capture_output=True, text=True).stdout.splitlines()
        need = int(out[0].split()[1])
        jobs = [tuple(int(v) for v in l.split()[1:]) for l in out if l.startswith("job")]
        keys = ("ws_t", "ws_p", "ws_y", "t", "ipt", "y", "estimate", "all_fft")
        rows = [dict(zip(keys, (int(v) for v in l.split()[1:]))) for l in out if l.startswith("img")]
        assert len(rows) == len(imgs)
        return need, jobs, rows

    def stage(n_tok, ncb, PP, want_norm, raw):
        out = subprocess.run([exe, "stage", str(n_tok), str(ncb), str(PP), str(int(want_norm)), str(int(raw))],
                             check=True, capture_output=True, text=True).stdout.split()
        return dict(zip(("scores", "codes", "norm", "raw", "need"), (int(v) for v in out)))

    run.stage = stage
    return run


SQ512 = [(512, 512, F, F, 1)] * 8


def test_pinned_512_batch(layout):
    need, jobs, rows = layout(SQ512)
    assert jobs == [(0, 8, 5505024)] and need == 22020352
    assert [r["ws_t"] for r in rows] == [688128 * i for i in range(8)]
    assert all(r["ipt"] == 0 and r["y"] == 0 and r["all_fft"] == 1 for r in rows)
    assert layout.stage(24576, 14, 196, False, False) == dict(scores=0, codes=98304, norm=98304 + 688128,
                                                              raw=98304 + 688128, need=790528)


def test_pinned_gemm_image(layout):
    need, jobs, rows = layout([(300, 262, G, G, 0)])
    assert (rows[0]["ws_t"], rows[0]["ws_p"], rows[0]["ws_y"]) == (0, 226816, 462656)
    assert jobs == [(0, 1, 684928)] and need == 2739968


def test_pinned_small_chunks(layout):
    need, jobs, rows = layout(SQ512, chunk_bytes=4 << 20)
    assert [(a, b) for a, b, _ in jobs] == [(i, i + 1) for i in range(8)]
    assert all(r["ws_t"] == 0 for r in rows) and all(j[2] == 688128 for j in jobs)
    assert need == (688128 + 64) * 4


def _default_route(n):
    return F if n in (512, 224) else G   # the sides with a compile-time plan kernel; fft_generic = 0, bluestein = 0


RAGGED = rng.ragged_sizes(7, 64, 28, 600)
ASSIGNMENTS = {
    "defaults": [(h, w, _default_route(w), _default_route(h), 0) for h, w in RAGGED],
    "gemm": [(h, w, G, G, 0) for h, w in RAGGED],
    "bluestein": [(h, w, B, B, 0) for h, w in RAGGED],
    "fft": [(h, w, F, F, 0) for h, w in RAGGED],
}


@pytest.mark.parametrize("name", sorted(ASSIGNMENTS))
def test_layout_invariants(layout, name):
    imgs = ASSIGNMENTS[name]
    chunk, limit = 4 << 20, 16 << 20   # small enough that the list is cut into many jobs
    need, jobs, rows = layout(imgs, chunk_bytes=chunk, ws_limit=limit)
    assert jobs[0][0] == 0 and jobs[-1][1] == len(imgs)
    assert all(a[1] == b[0] for a, b in zip(jobs, jobs[1:])) and all(i0 < i1 for i0, i1, _ in jobs)
    assert len(jobs) > 4
    for i0, i1, amax in jobs:
        spans = [(amax, amax + 3 * (i1 - i0) + 9)]
        total = 0
        for (h, w, r, c, _), row in zip(imgs[i0:i1], rows[i0:i1]):
            kh, kw = 14 * min(max(h // 14, 1), 32), 14 * min(max(w // 14, 1), 32)
            assert (row["t"], row["ipt"], row["y"]) == (3 * kw * h, 3 * h * w if r == G else 0,
                                                        3 * kh * kw if c in (G, B) else 0)
            spans += [(row[k], row[k] + row[s]) for k, s in (("ws_t", "t"), ("ws_p", "ipt"), ("ws_y", "y")) if row[s]]
            present = [row[s] for s in ("t", "ipt", "y") if row[s]]
            assert row["estimate"] == sum(4 * (s + 64) for s in present)
            total += row["estimate"]
            cap = min(chunk, limit) if row["all_fft"] else limit
            assert row["all_fft"] == (r != G and c != G)
            assert total <= cap or total == row["estimate"], "a job of several images exceeds its cap"
        spans.sort()
        assert all(a % 64 == 0 for a, _ in spans)
        assert all(e0 <= s1 for (_, e0), (s1, _) in zip(spans, spans[1:])), "regions overlap"
        assert spans[0][0] == 0 and spans[-1][1] * 4 <= need


def test_staging_carve(layout):
    for ncb, want_norm, raw, n_tok in itertools.product((0, 14), (False, True), (False, True),
                                                        (0, 1, 63, 3072, 24576)):
        s = layout.stage(n_tok, ncb, 196, want_norm, raw)
        patch = n_tok * 4 * 196
        assert s["need"] == n_tok * (4 + 2 * ncb + (4 * 196 if raw else 0) + (4 * 196 if want_norm else 0)) + 4096
        assert s["scores"] == 0 and s["scores"] % 256 == 0 and s["codes"] % 256 == 0
        assert s["codes"] >= n_tok * 4 and s["norm"] >= s["codes"] + n_tok * 2 * ncb
        assert s["raw"] == s["norm"] + (patch if want_norm else 0)
        assert s["raw"] + (patch if raw else 0) <= s["need"]


@pytest.fixture(scope="module")
def deal(tmp_path_factory, pkg):
    """xcd_deal_col_blocks of the built library on the blocks of images with the given tile-column counts."""
    lib_dir = os.path.dirname(pkg.__file__)
    assert os.path.exists(os.path.join(lib_dir, "libdctae.so")), "libdctae.so is not built"
    d = tmp_path_factory.mktemp("enc_deal")
    (d / "deal_main.cpp").write_text(DEAL.replace("%%", "%"))
    exe = str(d / "deal")
    subprocess.run(_compiler() + FLAGS + ["-o", exe, str(d / "deal_main.cpp"), f"-L{lib_dir}", "-ldctae", f"-L{ROCM}/lib",
                                  "-lamdhip64", f"-Wl,-rpath,{lib_dir}", f"-Wl,-rpath,{ROCM}/lib"], check=True)

    def run(qws):
        out = subprocess.run([exe] + [str(q) for q in qws], check=True, capture_output=True, text=True).stdout
        return [tuple(int(v) for v in l.split()) for l in out.splitlines()]

    return run


def _blocks(qws):
    return [(i, c, w, 1) for i, q in enumerate(qws) for c in range(3) for w in range(q)]


@pytest.mark.parametrize("qws", [[16] * 3, [32] * 8, [3, 16, 7, 1, 32, 9, 9, 2, 5, 11, 16]])
def test_deal_is_an_order_preserving_permutation(deal, qws):
    src, out = _blocks(qws), deal(qws)
    assert sorted(out) == sorted(src) and out != src
    for unit in {(b[0], b[1]) for b in src}:
        assert [b for b in out if b[:2] == unit] == [b for b in src if b[:2] == unit]
    # blocks b and b + 8 share an XCD: the first eight units start on eight different lanes
    units = sorted({(b[0], b[1]) for b in src})[:8]
    assert len({out.index((i, c, 0, 1)) % 8 for i, c in units}) == len(units)


def test_deal_leaves_short_lists_alone(deal):
    for qws in ([5], [1, 2, 2], [5] * 1 + [0]):
        assert len(_blocks(qws)) < 16 and deal(qws) == _blocks(qws)
