"""CPU checks around the training step's fixture (tests/golden/model_train_ref*.npz,
gen_model_train_golden.py): the oracle's encode / decode under float64 autograd
reproduce the reference's half gradients (so the oracle's backward is pinned to
the reference), every yardstick is usable, and training refuses a model the HIP
kernels cannot serve."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import ref_model as R

SEED_ENC, SEED_DEC = 7001, 7002


def load_fixture():
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "model_train_ref*.npz"))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def ref_inputs():
    d = np.load(os.path.join(GOLDEN, "model_ref.npz"))
    w = {k[2:]: torch.from_numpy(d[k]).double().requires_grad_(True) for k in d.files if k.startswith("w.")}
    t = {k: torch.from_numpy(d[k]) for k in d.files if not k.startswith("w.")}
    hid, heads, inter, layers, ncb, cbs, s = [int(v) for v in d["cfg"]]
    return w, t, dict(heads=heads, layers=layers, ncb=ncb, cbd=int(np.log2(cbs)))


def _upstream(fx, case, seed, shape):
    up = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    chk = fx[f"{case}.upstream_check"]
    assert abs(up.double().sum().item() - chk[0]) < 1e-6 and up[0, 0, 0].item() == chk[1] and up[-1, -1, -1].item() == chk[2]
    return up


def _compare(fx, case, names, grads):
    """1e-6 relative L2 per tensor.  k_proj.bias has an analytically zero gradient
    (softmax shift invariance): both sides hold float64 rounding noise there, which
    is measured against the same layer's q_proj.bias gradient instead."""
    for n, g in zip(names, grads):
        ref = torch.from_numpy(fx[f"{case}.g.{n}"]).double()
        scale = ref.norm().item()
        if n.endswith("k_proj.bias"):
            scale = np.linalg.norm(fx[f"{case}.g.{n.replace('k_proj', 'q_proj')}"])
        assert (g - ref).norm().item() <= 1e-6 * scale, n


def test_oracle_encoder_gradients_match_reference(fx, ref_inputs):
    w, t, c = ref_inputs
    x = t["patches_in"].double().requires_grad_(True)
    hidden, _, _ = R.encode(w, x, t["batched_image_ids"], t["key_pad_mask"], t["patch_channels"], t["patch_positions"],
                            c["heads"], c["layers"], c["ncb"], c["cbd"])
    names = [k[len("enc.g."):] for k in fx if k.startswith("enc.g.")]
    assert len(names) == 2 * 16 + 3 + 3 + 1
    leaves = [x if n == "patches_in" else w[n] for n in names]
    grads = torch.autograd.grad(hidden, leaves, _upstream(fx, "enc", SEED_ENC, hidden.shape).double())
    _compare(fx, "enc", names, grads)


def test_oracle_decoder_gradients_match_reference(fx, ref_inputs):
    w, t, c = ref_inputs
    with torch.no_grad():
        xq = R.codes_to_features({k: v.float() for k, v in w.items()}, t["codes"], c["ncb"], c["cbd"])
    x = xq.double().requires_grad_(True)
    out = R.decode(w, x, t["batched_image_ids"], t["key_pad_mask"], t["patch_channels"], t["patch_positions"],
                   c["heads"], c["layers"])
    names = [k[len("dec.g."):] for k in fx if k.startswith("dec.g.")]
    assert len(names) == 2 * 16 + 3 + 3 + 1
    leaves = [x if n == "x_q" else w[n] for n in names]
    grads = torch.autograd.grad(out, leaves, _upstream(fx, "dec", SEED_DEC, out.shape).double())
    _compare(fx, "dec", names, grads)


def test_fixture_yardsticks_are_usable(fx):
    devs = [k for k in fx if ".dev." in k]
    assert len(devs) == 2 * 39 + len(fx["step_subset"]) + 5
    for k in devs:
        assert np.isfinite(fx[k]) and fx[k] > 0, k
    for k in fx:
        if ".g." in k or ".loss." in k:
            assert np.isfinite(fx[k]).all(), k
    curve = fx["adamw.loss"]
    assert len(curve) == 11 and curve[0] - curve[-1] >= 0.05 * abs(curve[0]) and fx["adamw.lr"] > 0


def _small_model(pkg):
    enc = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_hidden_layers=1)
    return pkg.DCTAutoencoder(pkg.DCTAutoencoderConfig(patch_size=14, vq_codebook_size=2 ** 13, vq_num_codebooks=4,
                                                       encoder_config=enc, decoder_config=enc))


def test_cpu_and_fp16_models_refuse_training(pkg):
    for m in (_small_model(pkg), _small_model(pkg).half()):
        m.train()
        for call in (lambda: m.encode(None), lambda: m.decode(None), lambda: m(None),
                     lambda: m.decode_from_codes(None)):
            with pytest.raises(NotImplementedError):
                call()


def test_dropout_refuses_training(pkg):
    m = _small_model(pkg).train()
    m.config.decoder_config.dropout = 0.1
    with pytest.raises(NotImplementedError, match="HIP|dropout"):
        m.encode(None)
