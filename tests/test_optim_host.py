"""CPU-only checks of the fused optimizer's host side: the
segment plan of a DCTAutoencoder, the table planner of the C ABI
(dctae_optim_plan runs on the host), the refusals, and the per-step scalars
against torch's own double-precision AdamW."""
import ctypes as C
import os
from importlib import import_module

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _optim(pkg):
    return import_module("dct_autoencoder_amd.optim")


@pytest.fixture(scope="module")
def model(pkg):
    d = np.load(os.path.join(HERE, "golden", "model_ref.npz"))
    hid, heads, inter, layers, ncb, cbs, _ = [int(v) for v in d["cfg"]]
    enc = dict(hidden_size=hid, intermediate_size=inter, num_attention_heads=heads, num_hidden_layers=layers)
    return pkg.DCTAutoencoder(pkg.DCTAutoencoderConfig(image_channels=3, patch_size=14, max_patch_h=32, max_patch_w=32,
                                                       vq_codebook_size=cbs, vq_num_codebooks=ncb, vq_type="lfq",
                                                       encoder_config=enc, decoder_config=enc))


def test_segment_plan_covers_every_trainable_parameter_once(pkg, model):
    plan = _optim(pkg).segment_plan(model)
    want = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    assert [e["name"] for e in plan] == [n for n, _ in want]
    assert len({id(e["param"]) for e in plan}) == len(plan)
    for e, (_, p) in zip(plan, want):
        assert e["param"] is p and e["rows"] * e["cols"] == p.numel()
    assert not any(e["name"].startswith("patchnorm.") for e in plan)
    # every weight _Packed holds has a destination, and nothing else has
    packed = import_module("dct_autoencoder_amd.model")._Packed(model, training=True)
    by_pack = {}
    for e in plan:
        if "pack" in e:
            by_pack.setdefault(e["pack"], []).append(e)
    assert sorted(by_pack) == sorted(packed.w)
    for name, es in by_pack.items():
        assert sum(e["rows"] for e in es) == packed.w[name].shape[0] == es[0]["pack_rows"]
        assert packed.w[name].shape[1] == (es[0]["cols"] + 63) // 64 * 64
        assert packed.wt[name].shape == (es[0]["cols"], (es[0]["pack_rows"] + 63) // 64 * 64)


def test_segment_plan_places_q_k_v_in_the_qkv_pack(pkg, model):
    plan = {e["name"]: e for e in _optim(pkg).segment_plan(model)}
    d = model.config.encoder_config.hidden_size
    for side in ("encoder", "decoder"):
        for i in range(len(getattr(model, side).layers)):
            for j, k in enumerate(("q_proj", "k_proj", "v_proj")):
                w = plan[f"{side}.layers.{i}.self_attn.{k}.weight"]
                b = plan[f"{side}.layers.{i}.self_attn.{k}.bias"]
                assert (w["pack"], w["row_off"], w["pack_rows"]) == (f"{side}.{i}.qkv", j * d, 3 * d)
                assert (b["bias_pack"], b["bias_off"]) == (f"{side}.{i}.qkv", j * d)
            assert plan[f"{side}.layers.{i}.self_attn.out_proj.weight"]["row_off"] == 0
            assert "pack" not in plan[f"{side}.layers.{i}.layer_norm1.weight"]


def test_table_planner_prefixes_and_refusals(pkg):
    L = import_module("dct_autoencoder_amd._lib")
    lib = pkg.load_library()
    shapes = [(1, 3), (130, 196), (1, 0), (1, 2 ** 20 + 3), (52, 128)]
    segs = (L.OptimSeg * len(shapes))()
    for s, (r, c) in zip(segs, shapes):
        s.p = s.exp_avg = s.exp_avg_sq = 64   # never dereferenced by the planner
        s.rows, s.cols = r, c
    segs[1].w_dst, segs[1].ldw = 64, 256      # packed: 3 x 4 tiles of 64 x 64
    segs[4].wt_dst, segs[4].ldwt, segs[4].wt_col_off = 64, 128, 52
    nb, nw = C.c_int64(), C.c_int64()
    assert lib.dctae_optim_plan(None, segs, len(shapes), C.byref(nb), C.byref(nw)) == 0
    assert [s.norm0 for s in segs] == [0, 1, 3, 3, 68] and nb.value == 69      # 16384 gradients per block
    assert [s.work0 for s in segs] == [0, 1, 13, 13, 270] and nw.value == 272  # 4096 per flat item, 64 x 64 tiles
    segs[4].ldwt = 103   # 52 + 52 columns do not fit
    assert lib.dctae_optim_plan(None, segs, len(shapes), C.byref(nb), C.byref(nw)) != 0
    segs[4].ldwt = 128
    segs[1].copy_dst = 64
    assert lib.dctae_optim_plan(None, segs, len(shapes), C.byref(nb), C.byref(nw)) != 0
    segs[1].copy_dst = None
    segs[0].group = L.OPTIM_MAX_GROUPS
    assert lib.dctae_optim_plan(None, segs, len(shapes), C.byref(nb), C.byref(nw)) != 0


def test_construction_refusals(pkg):
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(NotImplementedError):
        pkg.FusedAdamW([p])
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(NotImplementedError):
            pkg.FusedAdamW([p], **{flag: True})
    assert issubclass(pkg.FusedAdamW, torch.optim.Optimizer)


def test_step_scalars_are_torchs_double_precision_ones(pkg):
    """A float64 torch.optim.AdamW run, redone by hand with step_scalars: bit-equal
    for steps 1 to 5 only if step_size, bias_correction2_sqrt and 1 - lr * wd are
    the doubles torch computes."""
    lr, b1, b2, eps, wd = 3e-3, 0.9, 0.99, 1e-8, 0.1
    g = torch.Generator().manual_seed(11)
    p = torch.nn.Parameter(torch.randn(257, dtype=torch.float64, generator=g))
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    q, m, v = p.detach().clone(), torch.zeros(257, dtype=torch.float64), torch.zeros(257, dtype=torch.float64)
    for step in range(1, 6):
        grad = torch.randn(257, dtype=torch.float64, generator=g)
        p.grad = grad.clone()
        opt.step()
        decay, step_size, bc2_sqrt = _optim(pkg).step_scalars(lr, b1, b2, wd, float(step))
        q = q * decay
        m = torch.lerp(m, grad, 1 - b1)
        v = v * b2 + (1 - b2) * grad * grad
        q = q + (-step_size) * m / (v.sqrt() / bc2_sqrt + eps)
        assert torch.equal(q, p.detach()), step
