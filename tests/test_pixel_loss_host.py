"""CPU side of the pixel loss (main.py:95-110): the fixture of
tests/golden/pixel_loss_ref*.npz (gen_pixel_loss_golden.py) is pinned by
oracle.ref_cpu under autograd (the recipe of oracle.decode_cases) -- in fp32 it
reproduces the reference's recorded losses and gradients exactly, and the
float64 recipe (revert_patching with the per-token loop, zero pad, idct2,
ipt_to_rgb on double tensors) reproduces the ``_f64`` entries -- so the GPU
tests' oracle, at the recorded shapes and at those of decode_cases.CASES, rests
on code that travels with the repository.  Also: the structure of the recorded gradients, the step's
argument check and the C ABI's two new entry points."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from oracle import decode_cases as oracle
from oracle import ref_cpu
from oracle.decode_cases import upstream

G = {}
for _f in ("pixel_loss_ref.npz", "pixel_loss_ref_sq512.npz", "pixel_loss_ref_sq512_f64.npz"):
    _g = golden(_f)
    G.update({k: _g[k] for k in _g.files})
NAMES = [str(n) for n in G["names"]]
CFG = {n: (int(p), int(m[0]), int(m[1]), int(s)) for n, p, m, s in
       zip(NAMES, G["patch_size"], G["max_patch"], G["max_seq_len"])}
SYMBOLS = ("dctae_decode_backward", "dctae_pixel_loss_forward")


def case(name):
    """the recorded batch as a ref_cpu.Batch (patches = the target), the perturbed output, the upstream images"""
    t = {k: torch.from_numpy(G[f"{name}_{k}"]) for k in ("patches", "out", "key_pad", "ids", "pos", "ch")}
    sizes = [tuple(int(v) for v in s) for s in G[f"{name}_original_sizes"]]
    batch = ref_cpu.Batch(patches=t["patches"], key_pad_mask=t["key_pad"], attn_mask=None,
                          batched_image_ids=t["ids"].long(), patch_channels=t["ch"].long(),
                          patch_positions=t["pos"].long(),
                          patch_sizes=[tuple(int(v) for v in s) for s in G[f"{name}_patch_sizes"]],
                          original_sizes=sizes)
    ws = [upstream(*(torch.from_numpy(G[f"{name}_w{i}_{k}"]) for k in "auv")) for i in range(len(sizes))]
    P, mh, mw, S = CFG[name]
    return batch, t["out"], ws, ref_cpu.FEConfig(patch_size=P, max_patch_h=mh, max_patch_w=mw, max_seq_len=S)


def oracle_results(name, dtype):
    batch, out, ws, cfg = case(name)
    r = oracle.oracle_results(batch, cfg, out, ws, dtype)
    return r["loss"], r["grad"], r["vjp"]


def token_image(name):
    """image index of every packed slot of the recorded batch (-1 at padding)"""
    return oracle.token_image(G[f"{name}_ids"], G[f"{name}_key_pad"])


@pytest.mark.parametrize("name", NAMES)
def test_ref_cpu_fp32_reproduces_the_reference(name):
    loss, grad, vjp = oracle_results(name, torch.float32)
    assert np.array_equal(loss, G[f"{name}_loss_f32"])
    assert np.array_equal(grad, G[f"{name}_grad_f32"])
    assert np.array_equal(vjp, G[f"{name}_vjp_f32"])


@pytest.mark.parametrize("name", NAMES)
def test_float64_recipe(name):
    loss, grad, vjp = oracle_results(name, torch.float64)
    assert loss.dtype == np.float64 and abs(loss - G[f"{name}_loss_f64"]) <= 1e-12 * abs(G[f"{name}_loss_f64"])
    for got, key in ((grad, "grad"), (vjp, "vjp")):
        want = G[f"{name}_{key}_f64"]
        assert want.dtype == np.float64 and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("name", NAMES)
def test_fixture_gradient_structure(name):
    kp = G[f"{name}_key_pad"]
    for key in ("grad_f32", "vjp_f32", "grad_f64", "vjp_f64"):
        g = G[f"{name}_{key}"]
        assert np.all(g[kp] == 0), "padded tokens get exact zeros"
        real = np.abs(g[~kp]).max(axis=-1) > 0
        if name == "dup":
            assert not real[0] and np.all(real[1:])   # slot 1 (the later one) wins the place, slot 0 is overwritten
        else:
            assert np.all(real)
    if name == "dup":
        assert np.array_equal(G["dup_pos"][0, 0], G["dup_pos"][0, 1]) and G["dup_ch"][0, 0] == G["dup_ch"][0, 1]
        assert np.abs(G["dup_grad_f64"][0, 0]).max() == 0 and np.abs(G["dup_grad_f64"][0, 1]).max() > 0


def test_fixture_geometry():
    """what the cases are there to exercise"""
    assert int(G["ragged14_key_pad"].sum()) == 17 and G["ragged14_key_pad"].shape == (2, 40)
    assert [tuple(s) for s in G["ragged14_original_sizes"]] == [(61, 47), (30, 75), (14, 14)]
    assert G["ragged14_patch_sizes"][1][1] == 5 > CFG["ragged14"][2]          # an image wider than the cap
    assert CFG["p5"][0] ** 2 % 4 and CFG["p1"][0] ** 2 % 4                      # the scalar paths
    assert [tuple(s) for s in G["sq512_original_sizes"]] == [(512, 512)] and int((~G["sq512_key_pad"]).sum()) == 256
    for f in ("pixel_loss_ref.npz", "pixel_loss_ref_sq512.npz", "pixel_loss_ref_sq512_f64.npz"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) < 2 ** 20


def test_step_losses_needs_the_extractor(pkg):
    with pytest.raises(ValueError, match="proc"):
        pkg.step_losses({}, None, None, None, 64, decode_pixels=True)
    assert callable(pkg.pixel_loss)


def test_header_declares_and_library_exports_the_entry_points(pkg):
    with open(os.path.join(ROOT, "include", "dctae.h")) as f:
        text = f.read()
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert f"int {s}(" in text
        assert getattr(lib, s).restype is not None
    assert "#define DCTAE_ABI_VERSION 1" in text and lib.dctae_abi_version() == 1
