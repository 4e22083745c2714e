"""CPU-only checks of the option table (csrc/dctae_options.h): a tiny host
program that includes only that header prints the table and applies
(key, value) pairs; the keys, defaults, legal values, status codes and the
plan-shaping set are compared with include/dctae.h and with the lists below."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "dct-autoencoder_amd", "csrc", "dctae_options.h")
EINVAL, EUNSUP = -1, -4

PROGRAM = r"""
#include "%s"
#include <cstdio>
#include <cstdlib>
using namespace dctae;
int main(int argc, char** argv) {
  if (argc == 1) {
    const Options d;
    for (const OptionRow& r : kOptions)
      std::printf("%%s %%lld %%lld %%lld %%d %%d\n", r.key, (long long)(d.*r.member), (long long)r.lo, (long long)r.hi,
                  (int)r.plan, (int)r.profiling);
    return 0;
  }
  // each "key=value" on a fresh Options: status, the member afterwards ("-" for an unknown key), the message
  for (int a = 1; a < argc; ++a) {
    std::string kv(argv[a]);
    const size_t eq = kv.find('=');
    const std::string key = kv.substr(0, eq);
    Options o;
    std::string err;
    const int rc = apply_option(o, key.c_str(), std::atoll(kv.c_str() + eq + 1), &err);
    const OptionRow* row = nullptr;
    for (const OptionRow& r : kOptions)
      if (key == r.key) row = &r;
    if (row)
      std::printf("%%d %%lld %%s\n", rc, (long long)(o.*(row->member)), err.c_str());
    else
      std::printf("%%d - %%s\n", rc, err.c_str());
  }
  return 0;
}
"""

DEFAULTS = {
    "fft": 1, "fft_spec": 1, "bluestein": 0, "xcd_order": 1, "rows_kernel": 4, "cols512b": 1, "cols_wide": 0,
    "sort_overlap": 0, "halves": 0, "fft_decode": 1, "dec_rows_kernel": 3, "dec_cols_kernel": 2, "sort_kernel": 2,
    "gemm_x3": 1, "gemm_h2": 1, "gemm_dma": 1, "rows_fused": 1, "cols_dma": 1, "lfq_ws": 1, "fft_odd": 0,
    "fft_generic": 0, "tperm": 1, "ws_poison": 0, "chunk_bytes": 2 ** 40, "workspace_limit": 8 * 2 ** 30,
    "t_alias": 0, "bs_ablate": 0, "gate": 0,
}
PROFILING = {"t_alias", "bs_ablate", "gate"}
# legal value sets of the restricted keys, with one illegal value each
LEGAL = {"rows_kernel": ({2, 4}, 3), "dec_rows_kernel": ({2, 3}, 4), "dec_cols_kernel": ({1, 2}, 0),
         "sort_kernel": ({1, 2}, 3)}
BYTES = ("chunk_bytes", "workspace_limit")   # >= 2^20
# what describe, fft_plan_for, bs_plan_for and build_encode_plan read
PLAN = {"fft", "fft_spec", "bluestein", "t_alias", "xcd_order", "gemm_x3", "cols512b", "rows_kernel", "gemm_h2",
        "fft_odd", "fft_generic", "tperm", "rows_fused", "chunk_bytes", "workspace_limit"}


def _compiler():
    for cxx in ("c++", "g++", "clang++"):
        if shutil.which(cxx):
            return [cxx]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no host C++ compiler and no hipcc found"
    return [hipcc, "-x", "c++"]   # hipcc as a plain C++ compiler


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    """The host program built without and with DCTAE_PROFILING."""
    d = tmp_path_factory.mktemp("options")
    src = d / "options_main.cpp"
    src.write_text(PROGRAM % HEADER)
    out = {}
    for name, flags in (("shipped", []), ("profiling", ["-DDCTAE_PROFILING"])):
        exe = d / name
        subprocess.run(_compiler() + ["-std=c++17", "-Wall", "-Werror", *flags, "-o", str(exe), str(src)], check=True)
        out[name] = str(exe)
    return out


def _rows(exe):
    rows = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        key, default, lo, hi, plan, prof = line.split()
        assert key not in rows, key
        rows[key] = dict(default=int(default), lo=int(lo), hi=int(hi), plan=int(plan), profiling=int(prof))
    return rows


def _apply(exe, *pairs):
    """[(status, stored value or None, message)] of each (key, value) on fresh options."""
    args = [f"{k}={v}" for k, v in pairs]
    res = []
    for line in subprocess.run([exe, *args], check=True, capture_output=True, text=True).stdout.splitlines():
        rc, val, msg = (line + " ").split(" ", 2)
        res.append((int(rc), None if val == "-" else int(val), msg.strip()))
    assert len(res) == len(pairs)
    return res


def _documented_keys():
    src = open(os.path.join(ROOT, "include", "dctae.h")).read()
    end = src.index("int dctae_set_option(")
    comment = src[src.rindex("/*", 0, end):end]
    return set(re.findall(r'"(\w+)"', comment))


def test_keys_match_the_header_comment(progs):
    assert set(_rows(progs["shipped"])) == _documented_keys()


def test_defaults(progs):
    rows = _rows(progs["shipped"])
    assert {k: r["default"] for k, r in rows.items()} == DEFAULTS
    assert rows == _rows(progs["profiling"])


def test_plan_and_profiling_flags(progs):
    rows = _rows(progs["shipped"])
    assert {k for k, r in rows.items() if r["plan"]} == PLAN
    assert {k for k, r in rows.items() if r["profiling"]} == PROFILING


def test_legal_values(progs):
    exe = progs["shipped"]
    rows = _rows(exe)
    for key, (legal, bad) in LEGAL.items():
        assert {rows[key]["lo"], rows[key]["hi"]} == legal
        for (rc, val, _), v in zip(_apply(exe, *[(key, v) for v in sorted(legal)]), sorted(legal)):
            assert (rc, val) == (0, v), key
        (rc, val, msg), = _apply(exe, (key, bad))
        assert (rc, val, msg) == (EINVAL, DEFAULTS[key], f"unknown option or bad value: {key}")
    for key in BYTES:
        assert rows[key]["lo"] == 2 ** 20 and rows[key]["hi"] >= 2 ** 62
        (ok, ok_val, _), (rc, val, msg) = _apply(exe, (key, 2 ** 20), (key, 2 ** 20 - 1))
        assert (ok, ok_val) == (0, 2 ** 20)
        assert (rc, val, msg) == (EINVAL, DEFAULTS[key], f"unknown option or bad value: {key}")


def test_unknown_key(progs):
    for exe in progs.values():
        (rc, val, msg), = _apply(exe, ("no_such_option", 1))
        assert (rc, val, msg) == (EINVAL, None, "unknown option or bad value: no_such_option")


def test_booleans_are_normalised(progs):
    exe = progs["shipped"]
    rows = _rows(exe)
    restricted = set(LEGAL) | set(BYTES) | PROFILING
    booleans = sorted(set(rows) - restricted)
    assert "tperm" in booleans
    for key, (rc, val, _) in zip(booleans, _apply(exe, *[(k, 7) for k in booleans])):
        assert (rc, val) == (0, 1), key
    for key, (rc, val, _) in zip(booleans, _apply(exe, *[(k, 0) for k in booleans])):
        assert (rc, val) == (0, 0), key
    for key, (rc, val, _) in zip(booleans, _apply(exe, *[(k, -3) for k in booleans])):
        assert (rc, val) == (0, 1), key


def test_profiling_keys(progs):
    for key in sorted(PROFILING):
        for v in (0, 1):   # the shipped build rejects them whatever the value
            (rc, val, msg), = _apply(progs["shipped"], (key, v))
            assert (rc, val) == (EUNSUP, 0)
            assert msg == f"option {key} exists only in a profiling build (make PROFILING=1)"
    exe = progs["profiling"]
    good = _apply(exe, ("t_alias", 16), ("bs_ablate", 7), ("gate", 6))
    assert [(rc, val) for rc, val, _ in good] == [(0, 16), (0, 7), (0, 6)]
    bad = _apply(exe, ("t_alias", -1), ("bs_ablate", 8), ("gate", 7), ("gate", -1))
    assert [(rc, val) for rc, val, _ in bad] == [(EINVAL, 0)] * 4
