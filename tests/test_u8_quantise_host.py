"""CPU-only check of the output quantisation of csrc/dctae_pixel.h: a small host
program that includes only that header reads fp32 values and writes
byte_from_unit of each.

The contract is torch's ``x.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)`` on
the CPU (two fp32 roundings, then clamp, then truncation: save_image's
rounding), byte for byte, on ``value_set()``: every k / 255 and every half-way
point (k + 0.5) / 255 with their +-1 and +-2 ulp neighbours, the special
values, and 2^20 seeded fp32 bit patterns.  NaN, which torch leaves undefined,
gives 0.  The program is built with contraction off and on: the header's result
must not depend on the caller's setting.  tests/test_gpu_decode_u8.py runs the
same values through the device kernel."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_options_host import _compiler

CSRC = os.path.join(ROOT, "dct-autoencoder_amd", "csrc")

PROGRAM = r"""
#include "%s/dctae_pixel.h"
#include <cstdio>
#include <vector>
using namespace dctae;
int main(int argc, char** argv) {
  if (argc > 1) {   // the round trip of all 256 bytes
    for (int b = 0; b < 256; ++b) std::printf("%%d\n", (int)byte_from_unit(unit_from_byte((float)b)));
    return 0;
  }
  std::vector<float> x(1 << 16);
  std::vector<uint8_t> y(1 << 16);
  size_t n;
  while ((n = std::fread(x.data(), 4, x.size(), stdin)) > 0) {
    for (size_t i = 0; i < n; ++i) y[i] = byte_from_unit(x[i]);
    if (std::fwrite(y.data(), 1, n, stdout) != n) return 1;
  }
  const float four[4] = {0.0f, 1.0f / 255.0f, 127.0f / 255.0f, 1.0f};
  return dword_from_units(four) == 0xff7f0100u ? 0 : 2;   // p[0] at the lowest address
}
"""


def quantise_cpu(x):
    """the definition: torch on the CPU (NaN-free input)"""
    x = x.detach().cpu()
    assert x.dtype == torch.float32 and not torch.isnan(x).any()
    return x.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)


def _neighbours(x):
    """x with its +-1 and +-2 ulp neighbours (next representable values, through zero and the denormals)"""
    up, dn = torch.full_like(x, float("inf")), torch.full_like(x, float("-inf"))
    u1, d1 = torch.nextafter(x, up), torch.nextafter(x, dn)
    return torch.cat([x, u1, d1, torch.nextafter(u1, up), torch.nextafter(d1, dn)])


def value_set():
    """the fp32 inputs of the quantisation tests, NaNs (from the random bit patterns) included"""
    k = torch.arange(256, dtype=torch.float32) / 255
    half = ((torch.arange(255, dtype=torch.float64) + 0.5) / 255).float()
    one = torch.tensor(1.0)
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 1e-45, -1e-45, 1e-39, -1e-39, 1.1754942e-38,
                            float(torch.nextafter(one, torch.tensor(2.0))), float(torch.nextafter(one, torch.tensor(0.0))),
                            -1e-9, 1.002, 1e30, -1e30, 3.0e38, 0.5, 1.0, 2.0], dtype=torch.float32)
    g = torch.Generator().manual_seed(20261)
    bits = torch.randint(-2 ** 31, 2 ** 31, (1 << 20,), generator=g, dtype=torch.int64).to(torch.int32)
    return torch.cat([_neighbours(k), _neighbours(half), special, bits.view(torch.float32)])


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("u8_quantise")
    (d / "q_main.cpp").write_text(PROGRAM % CSRC)
    out = []
    for i, flags in enumerate((["-O2", "-ffp-contract=off"], ["-O2", "-ffp-contract=fast"])):
        exe = str(d / f"q{i}")
        subprocess.run(_compiler() + ["-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, str(d / "q_main.cpp")],
                       check=True)
        out.append(exe)
    return out


def _run(exe, x):
    r = subprocess.run([exe], input=x.numpy().tobytes(), check=True, capture_output=True)
    assert len(r.stdout) == x.numel()
    return torch.from_numpy(np.frombuffer(r.stdout, dtype=np.uint8).copy())


def test_value_set_has_what_it_names():
    v = value_set()
    assert v.numel() == 5 * 256 + 5 * 255 + 19 + (1 << 20)
    nan = torch.isnan(v)
    assert nan.any() and (v == float("inf")).any() and (v == float("-inf")).any()
    f = v[~nan]
    assert ((f > 0) & (f < 1.1754944e-38)).any() and (f < 0).any() and (f > 1).any() and ((f > 0) & (f < 1)).any()
    q = quantise_cpu(f)
    assert sorted(set(q[: 5 * 256].tolist())) == list(range(256))   # every byte value is reached


def test_byte_from_unit_equals_torch(exes):
    v = value_set()
    nan = torch.isnan(v)
    got = [_run(exe, v) for exe in exes]
    assert torch.equal(got[0], got[1]), "the quantisation depends on -ffp-contract"
    want = quantise_cpu(v[~nan])
    bad = (got[0][~nan] != want).nonzero().flatten()
    assert bad.numel() == 0, (f"{bad.numel()} values differ from torch, first {v[~nan][bad[:4]].tolist()}: "
                              f"{got[0][~nan][bad[:4]].tolist()} != {want[bad[:4]].tolist()}")
    assert int(nan.sum()) > 0 and torch.all(got[0][nan] == 0), "NaN gives 0"


def test_named_values(exes):
    x = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, -1e-9, 1.002, 1e30, 0.0, 1.0,
                      0.5 / 255, 254.5 / 255], dtype=torch.float32)
    assert _run(exes[0], x).tolist()[:9] == [0, 255, 0, 0, 0, 255, 255, 0, 255]


def test_round_trip_of_all_bytes(exes):
    b = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(quantise_cpu(b / 255), b)   # the rule itself, in torch
    for exe in exes:
        lines = subprocess.run([exe, "rt"], check=True, capture_output=True, text=True).stdout.split()
        assert [int(l) for l in lines] == list(range(256))
