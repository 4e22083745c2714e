"""CPU-only checks of the plain C++ part of csrc/dctae_mfma_tile.h: a small host
program that includes only that header prints the fp16 operand exponent
(h2_operand_exp, clamped) and the matrix-side exponent (h2_matrix_exp,
unclamped) of the |max| bit patterns given on its command line, then
lds_off(r, kq) of every row r < 128 and k quad kq < 4.

The pinned values: a finite max in [2^(e-1), 2^e) has exponent 14 - e, so 1.0
(e = 1) gives 13, 2^13 and every value below 2^14 (e = 14) give 0, 2^14 gives
-1; FLT_MAX (e = 128) gives -114, clamped to -100 for an operand; the smallest
denormal 2^-149 (e = -148) gives 162, clamped to 100; zero, Inf and NaN leave
the operand unscaled (0)."""
import os
import struct
import subprocess

import pytest

from conftest import ROOT
from test_options_host import _compiler

CSRC = os.path.join(ROOT, "dct-autoencoder_amd", "csrc")

PROGRAM = r"""
#include "%s/dctae_mfma_tile.h"
#include <cstdio>
#include <cstdlib>
using namespace dctae;
int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    const uint32_t bits = (uint32_t)std::strtoul(argv[a], nullptr, 16);
    std::printf("exp %%08x %%d %%d\n", bits, h2_operand_exp(bits), h2_matrix_exp(bits));
  }
  for (int r = 0; r < 128; ++r)
    std::printf("row %%d %%d %%d %%d %%d\n", r, lds_off(r, 0), lds_off(r, 1), lds_off(r, 2), lds_off(r, 3));
  std::printf("xk %%d\n", XK);
  return 0;
}
"""


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


BELOW_2_14 = 0x467fffff   # the largest float below 2^14 = 0x46800000
FLT_MAX = 0x7f7fffff
PINNED = [(0, 0), (0x7f800000, 0), (0x7fc00000, 0), (bits(1.0), 13), (bits(2.0 ** 13), 0), (BELOW_2_14, 0),
          (bits(2.0 ** 14), -1), (FLT_MAX, -100), (1, 100)]
# the same finite inputs, unclamped: 14 - e
MATRIX = [(bits(1.0), 13), (bits(2.0 ** 13), 0), (BELOW_2_14, 0), (bits(2.0 ** 14), -1), (FLT_MAX, 14 - 128),
          (1, 14 + 148)]


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    d = tmp_path_factory.mktemp("mfma_tile")
    (d / "tile_main.cpp").write_text(PROGRAM % CSRC)
    exe = str(d / "tile")
    subprocess.run(_compiler() + ["-std=c++17", "-Wall", "-Werror", "-o", exe, str(d / "tile_main.cpp")], check=True)
    args = [f"{b:x}" for b, _ in PINNED]
    lines = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.splitlines()
    exps = {int(l.split()[1], 16): (int(l.split()[2]), int(l.split()[3])) for l in lines if l.startswith("exp")}
    rows = {int(l.split()[1]): [int(v) for v in l.split()[2:]] for l in lines if l.startswith("row")}
    xk = int([l for l in lines if l.startswith("xk")][0].split()[1])
    assert len(exps) == len(PINNED) and len(rows) == 128
    return exps, rows, xk


def test_operand_exponent_pinned(out):
    assert BELOW_2_14 == bits(2.0 ** 14) - 1 and bits(2.0 ** -149) == 1
    for b, want in PINNED:
        assert out[0][b][0] == want, hex(b)


def test_matrix_exponent_is_unclamped(out):
    for b, want in MATRIX:
        assert out[0][b][1] == want, hex(b)
    for b in (0, 0x7f800000, 0x7fc00000):
        assert out[0][b][1] == 0, hex(b)


def test_lds_off_permutes_a_rows_slots(out):
    _, rows, xk = out
    assert xk == 32
    for r, offs in rows.items():
        # halves: the row's four 16-byte slots start at r * XK + 8 s
        assert sorted(offs) == [r * xk + 8 * s for s in range(4)], r
