"""CPU-only checks of the antialiased resize (include/dctae_resize.h,
csrc/dctae_resize_math.h, dct_autoencoder_amd.resize):

  * the size rule of the reference's dataset crop (dataset.py:59-73 followed by
    torchvision 0.16.1's Resize(int)), pinned as literals worked out by hand;
  * the header's arithmetic, run by a stand-alone host program that includes
    nothing but the header, against the numpy mirror (tests/resize_mirror.py),
    bit for bit, under both contraction settings of the caller;
  * the mirror against torch's float64 interpolate, within 4 x the deviation
    of torch's own fp32 CPU result from float64 on the same input (floor 2^-20);
  * an axis that keeps its size passes values through bit for bit;
  * the C ABI: exported symbols, ctypes signatures, and that both entries reach
    the context's scratch only inside an OrderedCall scope.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_mirror as mirror
from conftest import ROOT
from test_options_host import _compiler

CSRC = os.path.join(ROOT, "dct-autoencoder_amd", "csrc")

SIZES_768 = [((768, 768), None), ((769, 769), (768, 768)), ((1000, 1500), (512, 768)), ((1500, 1000), (768, 512)),
             ((3000, 800), (765, 204)), ((801, 3001), (204, 764)), ((1023, 777), (767, 583)),
             ((769, 100), (761, 99)), ((100, 769), (99, 761)), ((770, 768), (767, 766)), ((900, 901), (767, 767)),
             ((4000, 13), (615, 2))]
SIZES_96 = [((100, 150), (64, 96)), ((300, 80), (93, 25)), ((97, 40), (94, 39)), ((130, 131), (95, 95)),
            ((96, 96), None)]

# (ih, iw) -> (oh, ow)
HEADER_SHAPES = [((37, 53), (9, 13)), ((17, 19), (40, 23)), ((5, 9), (1, 1)), ((1, 1), (4, 3)), ((1000, 7), (3, 7))]
TORCH_SHAPES = HEADER_SHAPES + [((300, 500), (97, 161)), ((100, 150), (63, 94))]


def image(shape, seed, u8=False):
    """a plane with structure at every scale: smooth waves plus noise, in [0, 1]"""
    h, w = shape
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = 0.5 + 0.25 * np.sin(0.37 * x + 0.11 * y) + 0.15 * np.cos(0.05 * x * y / max(h, w)) + 0.1 * g.standard_normal((h, w))
    v = np.clip(v, 0.0, 1.0)
    return np.round(v * 255).astype(np.uint8) if u8 else v.astype(np.float32)


# ---- the size rule ----------------------------------------------------------

@pytest.mark.parametrize("max_size,table", [(768, SIZES_768), (96, SIZES_96)])
def test_size_rule(pkg, max_size, table):
    from dct_autoencoder_amd import resize
    for (h, w), want in table:
        assert resize.dataset_crop_size(h, w, max_size) == want, (h, w)


def test_max_size(pkg):
    from dct_autoencoder_amd import resize
    assert resize.dataset_max_size(14, 32, 32) == 768
    assert resize.dataset_max_size(32, 32, 32) == 1024
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
    assert fe.dataset_max_size == 768


# ---- the header against the mirror ------------------------------------------

PROGRAM = r"""
#include "%s/dctae_resize_math.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace dctae;
// argv: input file, "f" or "b", ih iw oh ow, output file
int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const bool bytes = argv[2][0] == 'b';
  const int ih = std::atoi(argv[3]), iw = std::atoi(argv[4]), oh = std::atoi(argv[5]), ow = std::atoi(argv[6]);
  std::vector<float> x((size_t)ih * iw);
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  if (bytes) {
    std::vector<uint8_t> u(x.size());
    if (std::fread(u.data(), 1, u.size(), f) != u.size()) return 4;
    for (size_t i = 0; i < u.size(); ++i) x[i] = unit_from_byte((float)u[i]);
  } else if (std::fread(x.data(), 4, x.size(), f) != x.size()) {
    return 4;
  }
  std::fclose(f);
  std::vector<float> t((size_t)ih * ow), y((size_t)oh * ow);
  const ResizeAxis ax = resize_axis(iw, ow), ay = resize_axis(ih, oh);
  for (int o = 0; o < ow; ++o) {
    const ResizeWindow w = resize_window(ax, o, iw);
    const float sum = resize_weight_sum(ax, w);
    for (int r = 0; r < ih; ++r) {
      float acc = 0.0f;
      for (int j = w.lo; j < w.hi; ++j)
        acc = resize_tap(j == w.lo, acc, resize_weight(ax, w.center, sum, j), x[(size_t)r * iw + j]);
      t[(size_t)r * ow + o] = acc;
    }
  }
  for (int o = 0; o < oh; ++o) {
    const ResizeWindow w = resize_window(ay, o, ih);
    const float sum = resize_weight_sum(ay, w);
    for (int c = 0; c < ow; ++c) {
      float acc = 0.0f;
      for (int j = w.lo; j < w.hi; ++j)
        acc = resize_tap(j == w.lo, acc, resize_weight(ay, w.center, sum, j), t[(size_t)j * ow + c]);
      y[(size_t)o * ow + c] = acc;
    }
  }
  f = std::fopen(argv[7], "wb");
  if (!f) return 5;
  std::fwrite(y.data(), 4, y.size(), f);
  std::fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    """the host program, built with -ffp-contract=off and with -ffp-contract=fast"""
    d = tmp_path_factory.mktemp("resize_host")
    (d / "resize_main.cpp").write_text(PROGRAM % CSRC)
    exes = []
    for k, flags in enumerate((["-O2", "-ffp-contract=off"], ["-O2", "-ffp-contract=fast"])):
        exe = str(d / f"resize{k}")
        subprocess.run(_compiler() + ["-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, str(d / "resize_main.cpp")],
                       check=True)
        exes.append(exe)
    return d, exes


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("shape,size", HEADER_SHAPES)
def test_header_equals_mirror(progs, shape, size, u8):
    d, exes = progs
    x = image(shape, 11, u8)
    want = mirror.resize(x, *size)
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    x.tofile(src)
    for exe in exes:
        subprocess.run([exe, src, "b" if u8 else "f", str(shape[0]), str(shape[1]), str(size[0]), str(size[1]), dst],
                       check=True)
        got = np.fromfile(dst, dtype=np.float32).reshape(size)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
            f"{exe}: {int((got != want).sum())} of {got.size} pixels differ from the mirror"


# ---- the mirror against torch ------------------------------------------------

def torch_resize(x, size, dtype):
    t = torch.from_numpy(np.array(x)).to(dtype)[None, None]
    return F.interpolate(t, size=size, mode="bilinear", antialias=True, align_corners=False)[0, 0].numpy()


def tolerance(x, size):
    """(bound, torch's fp32 deviation): 4 x the deviation of torch's fp32 CPU result from float64, floor 2^-20"""
    t64 = torch_resize(x, size, torch.float64)
    dev32 = float(np.abs(torch_resize(x, size, torch.float32).astype(np.float64) - t64).max())
    return max(4.0 * dev32, 2.0 ** -20), dev32, t64


@pytest.mark.parametrize("shape,size", TORCH_SHAPES)
def test_mirror_against_torch_float64(shape, size):
    x = image(shape, 5)
    bound, dev32, t64 = tolerance(x, size)
    err = float(np.abs(mirror.resize(x, *size).astype(np.float64) - t64).max())
    print(f"{shape} -> {size}: mirror {err:.3e}, torch fp32 {dev32:.3e}, ratio {err / max(dev32, 1e-300):.3f}, "
          f"bound {bound:.3e}")
    assert err <= bound


# ---- identity -----------------------------------------------------------------

def test_equal_size_is_the_identity():
    x = image((64, 64), 3)
    y = mirror.resize(x, 64, 64)
    assert np.array_equal(y.view(np.uint32), x.view(np.uint32))
    lo, hi, w = mirror.axis_weights(64, 64)
    assert np.array_equal(w[0], np.ones(64, np.float32)) and not w[1:].any()


def test_unchanged_axis_is_the_identity():
    x = image((64, 64), 4)
    y = mirror.resize(x, 64, 31)
    one_axis = mirror.resize_axis(x, 31, -1)   # the horizontal pass alone
    assert np.array_equal(y.view(np.uint32), one_axis.view(np.uint32))


# ---- the C ABI ------------------------------------------------------------------

SYMBOLS = ["dctae_resize_aa", "dctae_resize_aa_u8"]


def _header():
    with open(os.path.join(ROOT, "include", "dctae_resize.h")) as f:
        return f.read()


def test_header_and_library(pkg):
    from dct_autoencoder_amd import _lib
    lib = pkg.load_library()
    flat = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split())
            for m in re.finditer(r"\bint\s+(dctae_\w+)\s*\(([^;{]*?)\)\s*;", flat, flags=re.S)}
    assert sorted(decl) == SYMBOLS
    for k, args in decl.items():
        assert hasattr(lib, k), k
        assert k in _lib._SIGS, k
        assert re.search(r"void\s*\*\s*stream$", args), f"{k}: the stream is the last parameter"
        assert _lib._SIGS[k][0][-1] is _lib._P
        assert len(_lib._SIGS[k][0]) == args.count(",") + 1
    assert lib.dctae_abi_version() == 1   # additive: the version stays
    text = " ".join(_header().replace("\n *", " ").split())
    assert "ordered after the context's previous call on another stream" in text
    assert "DCTAE_EINVAL" in text and "bit-identical" in text and "finite" in text


def _contract_patterns():
    """SCRATCH and SCOPE as tests/test_stream_contract_host.py spells them, read from its text"""
    with open(os.path.join(ROOT, "tests", "test_stream_contract_host.py")) as f:
        text = f.read()
    pats = {k: re.search(rf'^{k} = r"(.*)"$', text, flags=re.M).group(1) for k in ("SCRATCH", "SCOPE")}
    return pats["SCRATCH"], pats["SCOPE"]


def _bodies():
    """name -> body of every function defined under csrc/ (the rule of test_stream_contract_host.py)"""
    text = ""
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".hip"):
            with open(os.path.join(CSRC, f)) as fh:
                text += fh.read() + "\n"
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
    seen = seen if seen is not None else set()
    if name in seen or name not in funcs:
        return ""
    seen.add(name)
    body = funcs[name]
    for callee in set(re.findall(r"\b(\w+)\s*\(", body)):
        if callee in funcs:
            body += _closure(funcs, callee, seen)
    return body


def test_scratch_only_inside_an_ordered_call():
    scratch, scope = _contract_patterns()
    funcs = _bodies()
    for k in SYMBOLS:
        assert k in funcs, f"{k}: no definition found under csrc/"
        body = _closure(funcs, k)
        assert "resize_call" in body, f"{k}: both entries share one call body"
        assert re.search(scratch, body), f"{k}: the image table must travel through the context's plan"
        assert re.search(scope, body), f"{k}: reaches the context's scratch without an OrderedCall"
    call = funcs["resize_call"]   # the scope opens before the first use
    assert re.search(scope, call).start() < re.search(scratch, call).start()
    # nothing in the unit names the context's buffers directly
    with open(os.path.join(CSRC, "dctae_resize.hip")) as f:
        unit = f.read()
    assert not re.search(r"ctx->(?:scratch|plan\b|plan_host|plan_last)", unit)


# ---- no GPU -----------------------------------------------------------------------

def test_cpu_tensors_are_refused(pkg):
    from dct_autoencoder_amd import resize
    with pytest.raises(pkg.DCTAEUnavailable):
        resize.resize_antialias([torch.zeros(3, 8, 8)], [(4, 4)])
    with pytest.raises(pkg.DCTAEUnavailable):
        resize.resize_antialias([torch.zeros(3, 8, 8, dtype=torch.uint8)], [(8, 8)])
    with pytest.raises(TypeError):
        resize.resize_antialias([torch.zeros(3, 8, 8, dtype=torch.float64)], [(4, 4)])
    with pytest.raises(TypeError):
        resize.resize_antialias([torch.zeros(3, 8, 8), torch.zeros(3, 8, 8, dtype=torch.uint8)], [(4, 4), (4, 4)])
    with pytest.raises(ValueError):
        resize.resize_antialias([torch.zeros(1, 8, 8)], [(4, 4)])
    with pytest.raises(ValueError):
        resize.resize_antialias([torch.zeros(3, 8, 8)], [(0, 4)])
