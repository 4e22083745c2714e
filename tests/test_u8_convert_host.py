"""CPU-only check of the byte-pixel conversion of csrc/dctae_pixel.h: a small
host program that includes only that header prints the bit patterns of
unit_from_byte(u) and of the plain multiply unit_from_byte_plain(u) for
u = 0 .. 255, and of the four bytes of one dword through unit_from_dword.

The contract is the 256 values of ``torch.arange(256, dtype=torch.uint8) /
255`` (fp32 division, correctly rounded), bit for bit: the byte-image encode
means exactly that fp32 image.  ``u * (1.0f / 255)`` is not that (it is an ulp
off for about half of the values), which is why the header carries its FMA
correction; the test pins both facts."""
import os
import struct
import subprocess

import pytest
import torch

from conftest import ROOT
from test_options_host import _compiler

CSRC = os.path.join(ROOT, "dct-autoencoder_amd", "csrc")

PROGRAM = r"""
#include "%s/dctae_pixel.h"
#include <cstdio>
using namespace dctae;
static unsigned bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, 4);
  return u;
}
int main() {
  for (int u = 0; u < 256; ++u)
    std::printf("v %%d %%08x %%08x\n", u, bits(unit_from_byte((float)u)), bits(unit_from_byte_plain((float)u)));
  const uint32_t w = 0xff7f0100u;   // bytes 0x00, 0x01, 0x7f, 0xff from the lowest address
  for (int k = 0; k < 4; ++k) std::printf("d %%d %%08x\n", k, bits(unit_from_dword(w, k)));
  return 0;
}
"""


def _bits(t):
    return [struct.unpack("<I", struct.pack("<f", float(v)))[0] for v in t.tolist()]


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    d = tmp_path_factory.mktemp("u8_convert")
    (d / "px_main.cpp").write_text(PROGRAM % CSRC)
    exe = str(d / "px")
    results = []
    # built twice: the header's result must not depend on the caller's contraction setting
    for flags in (["-O2", "-ffp-contract=off"], ["-O2", "-ffp-contract=fast"]):
        subprocess.run(_compiler() + ["-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, str(d / "px_main.cpp")],
                       check=True)
        lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
        vals = {int(l.split()[1]): (int(l.split()[2], 16), int(l.split()[3], 16)) for l in lines if l.startswith("v")}
        dw = {int(l.split()[1]): int(l.split()[2], 16) for l in lines if l.startswith("d")}
        assert len(vals) == 256 and len(dw) == 4
        results.append((vals, dw))
    assert results[0] == results[1], "the conversion depends on -ffp-contract"
    return results[0]


@pytest.fixture(scope="module")
def want():
    ref = torch.arange(256, dtype=torch.uint8) / 255
    assert ref.dtype == torch.float32
    return _bits(ref)


def test_all_256_values_equal_torch_division(out, want):
    vals, _ = out
    bad = [u for u in range(256) if vals[u][0] != want[u]]
    assert not bad, f"unit_from_byte differs from torch's u8 / 255 at {bad[:8]} ({len(bad)} values)"
    # and torch's own u8.float() / 255 is the same tensor
    assert _bits(torch.arange(256, dtype=torch.uint8).float() / 255) == want


def test_plain_multiply_is_not_the_contract(out, want):
    vals, _ = out
    off = [u for u in range(256) if vals[u][1] != want[u]]
    print(f"u * (1.0f / 255) differs from u / 255 for {len(off)} of 256 byte values")
    assert off, "the plain multiply would do: the FMA correction of unit_from_byte is not needed"
    assert all(abs(vals[u][1] - want[u]) == 1 for u in off)   # one ulp each (same sign and exponent range)


def test_dword_bytes_in_address_order(out, want):
    _, dw = out
    assert [dw[k] for k in range(4)] == [want[0x00], want[0x01], want[0x7f], want[0xff]]
