"""GPU tests of FusedAdamW: gradient-norm clip, AdamW and the
bf16 weight packs in one HIP pass.

Oracle: torch itself, ``clip_grad_norm_`` + ``torch.optim.AdamW(foreach=False)``
on CPU float64 copies.  Yardstick: the same in CPU fp32.  Tolerance (the
project's 4 x yardstick rule) for ``p``, ``exp_avg`` and ``exp_avg_sq`` of each
tensor: max |ours - float64| <= max(4 x max |CPU fp32 - float64|, one fp32 ulp of
the tensor's largest magnitude).  The margin covers an equally valid fp32
evaluation order of sqrt, the division and lerp.  The model cases run on the
reference's golden weights and inputs (tests/golden/model_ref.npz: hidden 128,
patch 14 -> 196-wide rows padded to 256, LFQ 4 x 2^13 -> 52-wide projections
padded to 64: ragged tiles in both pack directions)."""
import copy
import ctypes as C
import functools
import os
from importlib import import_module

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1,), (3,), (63,), (64,), (65,), (257, 1), (130, 196), (196, 128), (52, 128), (128, 52), (2 ** 20 + 3,)]
VIEWS = (4, 6)          # gradients supplied as buf[1:1 + n]: 4-byte aligned views
BETAS, WD = (0.9, 0.99), 0.1
TWO_GROUPS = [(list(range(0, 11, 2)), dict(lr=1e-2, weight_decay=0.0)), (list(range(1, 11, 2)), dict(lr=1e-4))]


# ---------------------------------------------------------------- data, oracle, bound
@functools.lru_cache(maxsize=None)
def _data(steps=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(*s, generator=g) for s in SHAPES]
    grads = [[torch.randn(*s, generator=g) * (1 + 2 * t) for s in SHAPES] for t in range(steps)]
    return p0, grads


def _groups(params, lr, groups):
    if groups is None:
        return [dict(params=params, lr=lr)]
    return [dict(params=[params[i] for i in idx], **kw) for idx, kw in groups]


def _snapshot(opt, params):
    out = []
    for p in params:
        st = opt.state.get(p, {})
        out.append((p.detach().clone(), st["exp_avg"].clone() if st else None, st["exp_avg_sq"].clone() if st else None,
                    float(st["step"]) if st else 0.0))
    return out


@functools.lru_cache(maxsize=None)
def _torch_run(dtype, lr, two_groups=False, max_norm=None, sched=False, steps=3, skip=None):
    """clip_grad_norm_ + torch.optim.AdamW(foreach=False) on CPU copies of _data() in ``dtype``:
    (snapshot after the last step, [total norm of each step])."""
    p0, grads = _data()
    params = [torch.nn.Parameter(p.to(dtype).clone()) for p in p0]   # .to() alone would alias the fp32 data
    opt = torch.optim.AdamW(_groups(params, lr, TWO_GROUPS if two_groups else None), lr=lr, betas=BETAS,
                            weight_decay=WD, foreach=False)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 0.5 ** s) if sched else None
    norms = []
    for t in range(steps):
        for i, p in enumerate(params):
            p.grad = None if skip == (t, i) else grads[t][i].to(dtype).clone()
        norms.append(torch.nn.utils.clip_grad_norm_(params, float("inf") if max_norm is None else max_norm, foreach=False))
        opt.step()
        if sch:
            sch.step()
    return _snapshot(opt, params), norms


def _fused_run(pkg, lr, two_groups=False, max_norm=None, sched=False, steps=3, skip=None, nan_at=None):
    p0, grads = _data()
    params = [torch.nn.Parameter(p.to(DEV)) for p in p0]
    opt = pkg.FusedAdamW(_groups(params, lr, TWO_GROUPS if two_groups else None), lr=lr, betas=BETAS, weight_decay=WD,
                         max_grad_norm=max_norm)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 0.5 ** s) if sched else None
    norms = []
    for t in range(steps):
        for i, p in enumerate(params):
            g = grads[t][i].clone()
            if nan_at == (t, i):
                g.view(-1)[g.numel() // 2] = float("nan")
            if skip == (t, i):
                p.grad = None
            elif i in VIEWS:
                buf = torch.zeros(g.numel() + 2, device=DEV)
                buf[1:1 + g.numel()] = g.reshape(-1).to(DEV)
                p.grad = buf[1:1 + g.numel()].view(g.shape)
                assert p.grad.data_ptr() % 16 == 4 and p.grad.is_contiguous()
            else:
                p.grad = g.to(DEV)
        kept = [p.grad for p in params]
        before = [None if g is None else g.clone() for g in kept]
        opt.step()
        if sch:
            sch.step()
        norms.append(opt.grad_norm)
        for g, b in zip(kept, before):   # the gradients are read, never rewritten
            assert g is None or torch.equal(g, b) or nan_at is not None
    torch.cuda.synchronize()
    return _snapshot(opt, params), norms


def _within(ours, ref64, yard32, what):
    """The 4 x yardstick bound of the module docstring, per tensor; prints each figure first."""
    ours, yard32 = ours.detach().double().cpu(), yard32.detach().double().cpu()
    d_ours, d_yard = (ours - ref64).abs().max().item(), (yard32 - ref64).abs().max().item()
    ulp = float(np.spacing(np.float32(ref64.abs().max().item())))
    print(f"  {what:40s} ours {d_ours:.3e} yardstick {d_yard:.3e} ulp {ulp:.3e}")
    return d_ours <= max(4 * d_yard, ulp)


def _check_snapshot(ours, ref, yard, label):
    bad = []
    for i, (o, r, y) in enumerate(zip(ours, ref, yard)):
        assert o[3] == r[3] == y[3], (label, i, "step")
        if r[1] is None:
            assert o[1] is None
            continue
        for k, name in ((0, "p"), (1, "exp_avg"), (2, "exp_avg_sq")):
            if not _within(o[k], r[k], y[k], f"{label} {tuple(SHAPES[i])} {name}"):
                bad.append((i, name))
    assert not bad, bad


def _bit_equal(a, b):
    for x, y in zip(a, b):
        assert x[3] == y[3]
        for k in range(3):
            assert (x[k] is None and y[k] is None) or torch.equal(x[k], y[k])


# ---------------------------------------------------------------- 1. update parity, 3. determinism
@pytest.mark.parametrize("lr", [1e-4, 1e-2])
def test_update_parity_and_determinism(pkg, lr):
    ours, _ = _fused_run(pkg, lr)
    _check_snapshot(ours, _torch_run(torch.float64, lr)[0], _torch_run(torch.float32, lr)[0], f"lr={lr}")
    _bit_equal(ours, _fused_run(pkg, lr)[0])


def test_update_parity_two_param_groups(pkg):
    ours, _ = _fused_run(pkg, 1e-3, two_groups=True)
    _check_snapshot(ours, _torch_run(torch.float64, 1e-3, True)[0], _torch_run(torch.float32, 1e-3, True)[0], "two groups")


# ---------------------------------------------------------------- 2. norm and clip
def test_grad_norm_and_clip(pkg):
    _, norms64 = _torch_run(torch.float64, 1e-2)
    half = 0.5 * norms64[0].item()
    ours, norms = _fused_run(pkg, 1e-2, max_norm=half, steps=2)
    ref, ref_norms = _torch_run(torch.float64, 1e-2, max_norm=half, steps=2)
    yard, _ = _torch_run(torch.float32, 1e-2, max_norm=half, steps=2)
    for got, want in zip(norms, ref_norms):   # fp64 accumulation: the float64 norm, rounded once
        assert got.shape == () and got.device.type == "cuda"
        w32 = np.float32(want.item())
        print(f"grad_norm {got.item()!r} float64 {want.item()!r}")
        assert abs(np.float64(got.item()) - np.float64(w32)) <= np.spacing(w32)
    assert ref_norms[1].item() > 2 * ref_norms[0].item()   # the second step clips by another factor
    _check_snapshot(ours, ref, yard, "clipped")   # exp_avg / exp_avg_sq carry the clip in full
    unclipped = _torch_run(torch.float64, 1e-2, steps=2)[0]
    assert (unclipped[6][1] - ref[6][1]).abs().max() > 0.1 * ref[6][1].abs().max()   # the oracle itself sees the clip


def test_clip_coefficient_one_is_exact_and_nan_propagates(pkg):
    _, norms64 = _torch_run(torch.float64, 1e-2)
    big = 2.0 * max(n.item() for n in norms64)
    a, norms = _fused_run(pkg, 1e-2, max_norm=big)
    b, none = _fused_run(pkg, 1e-2, max_norm=None)
    _bit_equal(a, b)
    assert none == [None] * 3 and all(torch.isfinite(n) for n in norms)
    _, norms = _fused_run(pkg, 1e-2, max_norm=1.0, steps=1, nan_at=(0, 7))
    assert torch.isnan(norms[0])


def test_norm_is_deterministic(pkg):
    a = _fused_run(pkg, 1e-2, max_norm=1.0)[1]
    b = _fused_run(pkg, 1e-2, max_norm=1.0)[1]
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 5. skips
def test_parameter_without_grad_is_untouched(pkg):
    skip = (1, 6)
    ours, _ = _fused_run(pkg, 1e-2, steps=2, skip=skip)
    first, _ = _fused_run(pkg, 1e-2, steps=1)
    assert ours[6][3] == 1.0 and ours[5][3] == 2.0
    for k in range(3):
        assert torch.equal(ours[6][k], first[6][k])
    _check_snapshot(ours, _torch_run(torch.float64, 1e-2, steps=2, skip=skip)[0],
                    _torch_run(torch.float32, 1e-2, steps=2, skip=skip)[0], "skip")


# ---------------------------------------------------------------- packed segments through the C ABI
def test_packed_segments_at_ragged_shapes(pkg):
    """The tile path on shapes with ragged 64 x 64 tiles, two tensors sharing one pack
    at an offset that is no multiple of 8, a one-column tensor and a gradient view:
    p / m / v bit-equal to the flat path, packs equal to torch's bf16 cast, padding and
    everything outside the destinations untouched."""
    O = import_module("dct_autoencoder_amd.optim")
    L = import_module("dct_autoencoder_amd._lib")
    ctx = L.context(DEV)
    g = torch.Generator().manual_seed(5)
    shapes = [(257, 1), (130, 196), (196, 128), (52, 128), (52, 128), (128, 52), (65, 63)]
    pad = lambda k: (k + 63) // 64 * 64
    ps = [torch.randn(*s, generator=g).to(DEV) for s in shapes]
    gbuf = [torch.randn(s[0] * s[1] + 2, generator=g).to(DEV) for s in shapes]
    gs = [b[1:-1].view(s) if i in (1, 5) else b[:-2].view(s).clone() for i, (b, s) in enumerate(zip(gbuf, shapes))]
    ms = [torch.randn(*s, generator=g).to(DEV) * 0.1 for s in shapes]
    vs = [torch.rand(*s, generator=g).to(DEV) * 0.1 for s in shapes]
    flat = [[t.clone() for t in ts] for ts in (ps, ms, vs)]
    FILL = 0x1234
    w, wt, off = [], [], []
    for i, (r, c) in enumerate(shapes):
        if i == 4:      # the second (52, 128) shares the pack of the first, at row / column offset 52
            w.append(w[3]); wt.append(wt[3]); off.append(52)
            continue
        rows = 104 if i == 3 else r
        w.append(torch.full((rows, pad(c)), FILL, dtype=torch.int16, device=DEV))
        wt.append(torch.full((c, pad(rows)), FILL, dtype=torch.int16, device=DEV))
        off.append(0)

    def run(p, m, v, packed):
        tab = np.zeros(len(shapes), dtype=O._SEG_DTYPE)
        for i, (r, c) in enumerate(shapes):
            tab["p"][i], tab["g"][i], tab["exp_avg"][i], tab["exp_avg_sq"][i] = (t[i].data_ptr() for t in (p, gs, m, v))
            tab["rows"][i], tab["cols"][i] = r, c
            if packed:
                tab["w_dst"][i], tab["ldw"][i], tab["w_row_off"][i] = w[i].data_ptr(), w[i].shape[1], off[i]
                tab["wt_dst"][i], tab["ldwt"][i], tab["wt_col_off"][i] = wt[i].data_ptr(), wt[i].shape[1], off[i]
        nb, nw = C.c_int64(), C.c_int64()
        ctx.check(ctx.lib.dctae_optim_plan(ctx.h, C.c_void_p(tab.ctypes.data), len(shapes), C.byref(nb), C.byref(nw)))
        dev_tab = torch.from_numpy(tab.view(np.uint8).reshape(-1).copy()).to(DEV)
        hp = (L.OptimGroup * 1)(L.OptimGroup(1 - 1e-2 * 0.1, 0.1, 0.99, 0.01, 0.1, 0.1, 1e-8, 0.0))
        ctx.check(ctx.lib.dctae_optim_adamw_pack(ctx.h, L.ptr(dev_tab), len(shapes), nw.value, hp, 1, None,
                                                 L.stream_ptr(DEV)), "adamw_pack")
        torch.cuda.synchronize()

    run(*flat, packed=False)
    run(ps, ms, vs, packed=True)
    for a, b in zip(flat, (ps, ms, vs)):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    for i, (r, c) in enumerate(shapes):
        bits = ps[i].to(torch.bfloat16).view(torch.int16)
        assert torch.equal(w[i][off[i]:off[i] + r, :c], bits), i
        assert torch.equal(wt[i][:c, off[i]:off[i] + r], bits.t()), i
        if i not in (3, 4):
            assert (w[i][:, c:] == FILL).all() and (wt[i][:, r:] == FILL).all(), i
    assert (w[3][:, 128:] == FILL).all() and (wt[3][:, 104:] == FILL).all()


# ---------------------------------------------------------------- 6. state-dict exchange
@pytest.mark.parametrize("direction", ["fused_to_torch", "torch_to_fused"])
def test_state_dict_exchange_with_torch_adamw(pkg, direction):
    """Two steps in one optimizer, its state_dict loaded into the other (deep-copied, as a
    checkpoint read from disk is: torch's load_state_dict keeps the tensors of a live dict),
    a third step in each on the same gradients: all within the bound of the 3-step oracle."""
    lr = 1e-2
    p0, grads = _data()
    pa = [torch.nn.Parameter(p.to(DEV)) for p in p0]
    fused = pkg.FusedAdamW(pa, lr=lr, betas=BETAS, weight_decay=WD)
    plain = torch.optim.AdamW([torch.nn.Parameter(p.to(DEV)) for p in p0], lr=lr, betas=BETAS, weight_decay=WD,
                              foreach=False)
    first, second = (fused, plain) if direction == "fused_to_torch" else (plain, fused)

    def params(opt):
        return opt.param_groups[0]["params"]

    for t in range(2):
        for p, g in zip(params(first), grads[t]):
            p.grad = g.to(DEV)
        first.step()
    second.load_state_dict(copy.deepcopy(first.state_dict()))
    with torch.no_grad():
        for q, p in zip(params(second), params(first)):
            q.copy_(p)
    for opt in (first, second):
        for p, g in zip(params(opt), grads[2]):
            p.grad = g.to(DEV)
        opt.step()
    torch.cuda.synchronize()
    assert set(fused.state[pa[0]]) == {"step", "exp_avg", "exp_avg_sq"}
    st = fused.state[pa[0]]["step"]
    assert st.device.type == "cpu" and st.dtype == torch.float32 and st.shape == ()
    ref, yard = _torch_run(torch.float64, lr)[0], _torch_run(torch.float32, lr)[0]
    for opt, label in ((first, "first"), (second, "second")):
        _check_snapshot(_snapshot(opt, params(opt)), ref, yard, f"{direction} {label}")


# ---------------------------------------------------------------- 7. scheduler
def test_lambda_lr_schedule(pkg):
    ours, _ = _fused_run(pkg, 1e-2, sched=True)
    _check_snapshot(ours, _torch_run(torch.float64, 1e-2, sched=True)[0], _torch_run(torch.float32, 1e-2, sched=True)[0],
                    "LambdaLR")
    assert not torch.equal(ours[6][0], _fused_run(pkg, 1e-2)[0][6][0])


def test_step_refusals(pkg):
    p = torch.nn.Parameter(torch.zeros(8, device=DEV, dtype=torch.float16))
    with pytest.raises(NotImplementedError):
        pkg.FusedAdamW([p])
    p = torch.nn.Parameter(torch.zeros(8, 8, device=DEV).t()[:, :4])
    with pytest.raises(NotImplementedError):
        pkg.FusedAdamW([p])
    p = torch.nn.Parameter(torch.zeros(8, 4, device=DEV))
    opt = pkg.FusedAdamW([p])
    p.grad = torch.sparse_coo_tensor(torch.tensor([[0], [0]]), torch.tensor([1.0]), (8, 4)).to(DEV)
    with pytest.raises(NotImplementedError):
        opt.step()
    p.grad = torch.ones(4, 8, device=DEV).t()   # non-contiguous: made contiguous first
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(p).all() and (p != 0).all()


# ---------------------------------------------------------------- model
@pytest.fixture(scope="module")
def golden(pkg):
    d = np.load(os.path.join(HERE, "golden", "model_ref.npz"))
    w = {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w.")}
    hid, heads, inter, layers, ncb, cbs, s = [int(v) for v in d["cfg"]]
    enc = dict(hidden_size=hid, intermediate_size=inter, num_attention_heads=heads, num_hidden_layers=layers)
    cfg = pkg.DCTAutoencoderConfig(image_channels=3, patch_size=14, max_patch_h=32, max_patch_w=32,
                                   vq_codebook_size=cbs, vq_num_codebooks=ncb, vq_type="lfq", encoder_config=enc,
                                   decoder_config=enc)
    tabs = np.load(os.path.join(HERE, "golden", "patchnorm_ref.npz"))

    def make():
        m = pkg.DCTAutoencoder(cfg)
        m.load_state_dict(w, strict=False)
        m.patchnorm.median.data.copy_(torch.from_numpy(tabs["median"]))
        m.patchnorm.b.data.copy_(torch.from_numpy(tabs["b"]))
        m.patchnorm.frozen = True
        return m.to(DEV)

    t = {k: torch.from_numpy(d[k]).to(DEV) for k in d.files if not k.startswith("w.") and k != "cfg"}
    return make, t, cbs


WEIGHTS = dict(rec_loss=0.1, rec_loss_unnormalized=1.0, commit_loss=0.1, entropy_loss=0.1)   # main.py:311-314
HYPER = dict(lr=1e-4, betas=(0.9, 0.99), weight_decay=0.1)                                  # main.py:420-425


def _dp(pkg, t, patches):
    return pkg.DCTPatches(patches=patches, key_pad_mask=t["key_pad_mask"], batched_image_ids=t["batched_image_ids"],
                          patch_channels=t["patch_channels"], patch_positions=t["patch_positions"], patch_sizes=[],
                          original_sizes=[])


def _losses(pkg, m, t, cbs):
    """One training step's losses (main.py:56-93 through step_losses) and their weighted sum."""
    losses = import_module("dct_autoencoder_amd.losses")
    normalized = _dp(pkg, t, t["patches_in"])
    with torch.no_grad():
        raw = _dp(pkg, t, m.patchnorm.inverse_norm(_dp(pkg, t, t["patches_in"].clone())))
    out = losses.step_losses(m(normalized.shallow_copy()), raw, normalized, m.patchnorm, cbs)
    return out, sum(w * out[k] for k, w in WEIGHTS.items())


def _fresh_pack(pkg, m):
    return import_module("dct_autoencoder_amd.model")._Packed(m)


def _same_pack(pk, fresh):
    assert sorted(pk.w) == sorted(fresh.w) and sorted(pk.wt) == sorted(fresh.wt)
    for k in fresh.w:
        assert pk.w[k].shape == fresh.w[k].shape and torch.equal(pk.w[k], fresh.w[k]), k      # padding columns too
        assert pk.wt[k].shape == fresh.wt[k].shape and torch.equal(pk.wt[k], fresh.wt[k]), k
        assert (fresh.b[k] is None and pk.b[k] is None) or torch.equal(pk.b[k], fresh.b[k]), k


@pytest.fixture(scope="module")
def stepped(pkg, golden):
    """The golden model after one real step (losses of main.py:311-314) of FusedAdamW(model=m)."""
    make, t, cbs = golden
    m = make().train()
    opt = pkg.FusedAdamW(m.parameters(), max_grad_norm=5.0, model=m, **HYPER)
    frozen = {n: p.detach().clone() for n, p in m.named_parameters() if not p.requires_grad}
    _losses(pkg, m, t, cbs)[1].backward()
    assert all(p.grad is not None for p in m.parameters() if p.requires_grad)
    opt.step()
    torch.cuda.synchronize()
    return m, opt, frozen


def test_packs_are_maintained_by_the_step(pkg, golden, stepped):
    make, t, cbs = golden
    m, opt, frozen = stepped
    pk = m._weights()
    assert pk is opt._pk and m._weights() is pk          # no rebuild
    _same_pack(pk, _fresh_pack(pkg, m))
    assert sorted(frozen) == ["patchnorm.b", "patchnorm.median", "patchnorm.n"]
    for n, p in m.named_parameters():                    # 5. the PatchNorm tables are bit-unchanged
        if n in frozen:
            assert torch.equal(p, frozen[n]) and p not in opt.state
    m2 = copy.deepcopy(m)
    m2._packed = None                                    # rebuilt by torch ops
    a, b = _losses(pkg, m, t, cbs)[0], _losses(pkg, m2, t, cbs)[0]
    assert m._weights() is opt._pk and m2._weights() is not opt._pk
    for k in WEIGHTS:
        assert torch.isfinite(a[k]) and torch.equal(a[k], b[k]), k


def test_other_parameter_changes_still_rebuild(pkg, golden, stepped):
    m, opt, _ = stepped
    m = copy.deepcopy(m)
    assert m._weights() is not opt._pk                   # the copy's parameters live elsewhere
    m.load_state_dict({k: v + 1 if k.endswith("fc1.weight") else v for k, v in m.state_dict().items()})
    pk = m._weights()
    _same_pack(pk, _fresh_pack(pkg, m))
    with torch.no_grad():
        m.decoder.layers[1].self_attn.k_proj.weight.add_(1)
    assert m._weights() is not pk
    _same_pack(m._weights(), _fresh_pack(pkg, m))


def test_rebuild_after_in_place_change_between_steps(pkg, golden):
    """A parameter changed by other means between two optimizer steps: the forward in between
    rebuilds by torch ops, and the pack the next step installs is right for every tensor,
    also for one that step skips."""
    make, t, cbs = golden
    m = make().train()
    opt = pkg.FusedAdamW(m.parameters(), max_grad_norm=5.0, model=m, **HYPER)
    _losses(pkg, m, t, cbs)[1].backward()
    opt.step()
    skipped = m.encoder.layers[0].mlp.fc2.weight
    with torch.no_grad():
        skipped.add_(1)
    assert m._weights() is not opt._pk
    _same_pack(m._weights(), _fresh_pack(pkg, m))
    skipped.grad = None
    opt.step()
    assert m._weights() is opt._pk
    _same_pack(opt._pk, _fresh_pack(pkg, m))


def test_rebuild_after_data_add(pkg, golden, stepped):
    """``p.data.add_(1)`` on one weight: torch gives ``p.data`` a version counter of its own,
    so neither ``p._version`` nor ``p.data_ptr()`` records the write; the Linear parameters
    ``_Packed`` copies count accesses of ``.data`` instead (model._TrackedParameter), and
    ``_weights()`` rebuilds."""
    m, opt, _ = stepped
    m = copy.deepcopy(m)
    pk = m._weights()
    m.encoder.layers[0].mlp.fc1.weight.data.add_(1)
    assert m._weights() is not pk
    _same_pack(m._weights(), _fresh_pack(pkg, m))
    # the same on a model the optimizer maintains, between two steps
    make, t, cbs = golden
    m = make().train()
    opt = pkg.FusedAdamW(m.parameters(), max_grad_norm=5.0, model=m, **HYPER)
    _losses(pkg, m, t, cbs)[1].backward()
    opt.step()
    assert m._weights() is opt._pk
    m.decoder.layers[0].self_attn.v_proj.weight.data.add_(1)
    assert m._weights() is not opt._pk
    _same_pack(m._weights(), _fresh_pack(pkg, m))
    opt.step()
    assert m._weights() is opt._pk
    _same_pack(opt._pk, _fresh_pack(pkg, m))


def test_eval_after_training_steps_equals_a_fresh_model(pkg, golden):
    make, t, cbs = golden
    m = make().train()
    opt = pkg.FusedAdamW(m.parameters(), max_grad_norm=5.0, model=m, **HYPER)
    for _ in range(2):
        opt.zero_grad()
        _losses(pkg, m, t, cbs)[1].backward()
        opt.step()
    fresh = make()
    fresh.load_state_dict(m.state_dict())
    out = m.eval()(_dp(pkg, t, t["patches_in"].clone()))
    assert m._weights() is opt._pk
    ref = fresh.eval()(_dp(pkg, t, t["patches_in"].clone()))
    torch.cuda.synchronize()
    assert torch.equal(out["codes"], ref["codes"])
    assert torch.equal(out["dct_patches"].patches, ref["dct_patches"].patches)


# ---------------------------------------------------------------- 8. stale graph
def test_backward_through_a_stale_graph_raises(pkg, golden):
    make, t, cbs = golden
    m = make().train()
    opt = pkg.FusedAdamW(m.parameters(), max_grad_norm=5.0, model=m, **HYPER)
    _losses(pkg, m, t, cbs)[1].backward()
    opt.step()                                   # the optimizer's pack is now the model's
    _losses(pkg, m, t, cbs)[1].backward()        # gradients of an earlier backward
    stale = _losses(pkg, m, t, cbs)[1]           # a forward on the current pack
    opt.step()                                   # rewrites that pack in place
    with pytest.raises(RuntimeError, match="stale graph"):
        stale.backward()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 9. end to end
def _train3(pkg, golden):
    make, t, cbs = golden
    m = make().train()
    opt = pkg.FusedAdamW(m.parameters(), max_grad_norm=5.0, model=m, **HYPER)
    curve, first = [], None
    for i in range(3):
        opt.zero_grad()
        total = _losses(pkg, m, t, cbs)[1]
        curve.append(total.detach().clone())
        total.backward()
        if i == 0:
            first = ({n: p.detach().clone() for n, p in m.named_parameters()},
                     {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
        opt.step()
        if i == 0:
            first += ({n: p.detach().clone() for n, p in m.named_parameters()}, opt.grad_norm.clone())
    torch.cuda.synchronize()
    return curve, first, {n: p.detach().clone() for n, p in m.named_parameters()}


def test_three_training_steps_end_to_end(pkg, golden):
    make, t, cbs = golden
    curve, (p0, g0, p1, norm), final = _train3(pkg, golden)
    assert all(torch.isfinite(c) for c in curve)
    # the same first step with clip_grad_norm_ + torch.optim.AdamW on a twin model: identical
    # inputs, so bit-identical gradients; the twin is the yardstick, CPU float64 the oracle
    twin = make().train()
    topt = torch.optim.AdamW(twin.parameters(), **HYPER)
    _losses(pkg, twin, t, cbs)[1].backward()
    names = [n for n, p in twin.named_parameters() if p.requires_grad]
    assert sorted(g0) == sorted(names)
    for n, p in twin.named_parameters():
        assert not p.requires_grad or torch.equal(p.grad, g0[n]), n
    tnorm = torch.nn.utils.clip_grad_norm_(twin.parameters(), 5.0)
    topt.step()
    ref = {n: torch.nn.Parameter(p0[n].double().cpu()) for n in names}
    for n in names:
        ref[n].grad = g0[n].double().cpu()
    rnorm = torch.nn.utils.clip_grad_norm_(list(ref.values()), 5.0, foreach=False)
    torch.optim.AdamW(list(ref.values()), foreach=False, **HYPER).step()
    print(f"grad norm: ours {norm.item()!r} torch fp32 {tnorm.item()!r} float64 {rnorm.item()!r}")
    assert abs(np.float64(norm.item()) - np.float64(np.float32(rnorm.item()))) <= np.spacing(np.float32(rnorm.item()))
    twin_p = dict(twin.named_parameters())
    bad = [n for n in names if not _within(p1[n], ref[n].detach(), twin_p[n], n)]
    assert not bad, bad
    # the whole sequence repeats bit for bit
    curve2, _, final2 = _train3(pkg, golden)
    assert all(torch.equal(a, b) for a, b in zip(curve, curve2))
    assert all(torch.equal(final[n], final2[n]) for n in final)
