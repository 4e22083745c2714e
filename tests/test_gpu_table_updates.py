"""The Python-side caches follow in-place updates of what they copy.

PatchNorm caches the LFQ thresholds of its tables (``state(thresholds=True)``:
every codes-only encode), BatchEncoder / BatchDecoder keep the state they took
at construction, the model keeps bf16 packs of its Linear weights, and LFQ
hands its projection weights to the kernels.  A module that has already served
a codes-only encode gets new tables in each of the ways torch offers; after
each, the codes-only encode must equal, bit for bit, the codes of
``return_patches=True`` from the same module (no thresholds) and the codes of
a fresh module built with the new tables, and a BatchEncoder / BatchDecoder
made before the change must follow it.

``p.data`` has a version counter of its own: ``p.data.copy_``, an in-place op
under ``no_grad`` and ``load_state_dict`` move neither ``p.data._version`` nor
``data_ptr()``, which is what the cache was keyed on: those three cases
returned the old tables' codes before PatchNorm took tracked parameters."""
import copy

import pytest
import torch

import stale_state as ss

pytestmark = pytest.mark.gpu
DEV = ss.DEV
SIZE = (64, 96)


@pytest.fixture(scope="module")
def env(pkg):
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
    lfq = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).to(DEV).eval()
    imgs = ss.images(61, [SIZE, SIZE])
    return fe, lfq, imgs, torch.stack(imgs).contiguous()


def _new_tables(seed=7):
    return ss.tables(seed, 32, 32, 14)


def _copy_data(pn):
    med, b = _new_tables()
    pn.median.data.copy_(med)
    pn.b.data.copy_(b)


def _inplace_no_grad(pn):
    with torch.no_grad():
        pn.b.mul_(3.0)
        pn.median.add_(0.01)


def _load_state_dict(pn):
    med, b = _new_tables()
    sd = {k: v.clone() for k, v in pn.state_dict().items()}
    sd["median"], sd["b"] = med.to(DEV), b.to(DEV)
    pn.load_state_dict(sd)


def _assign_data(pn):
    med, b = _new_tables()
    pn.median.data = med.to(DEV)
    pn.b.data = b.to(DEV)


def _assign_data_twice(pn):
    """``.data = new`` twice: the second tensor may land where the first one was"""
    _assign_data(pn)
    pn.state(thresholds=True)
    med, b = _new_tables(8)
    pn.median.data = med.to(DEV)
    pn.b.data = b.to(DEV)


def _new_parameter(pn):
    med, b = _new_tables()
    pn.median = torch.nn.Parameter(med.to(DEV), requires_grad=False)
    pn.b = torch.nn.Parameter(b.to(DEV), requires_grad=False)


def _eps(pn):
    pn.eps = 0.5


def _clamp(pn):
    pn.max_val, pn.min_val = 6.0, 0.25   # every normalised value is positive now: every bit set


def _train_step(pn, env=None):
    fe, lfq, imgs, _ = env
    ((dp, _),) = fe.encode_batch(imgs, None, None, return_raw=True)
    pn.frozen = False
    pn.train()
    pn(dp)
    pn.frozen = True
    pn.eval()


# (the change, whether the codes must differ from those of the old tables: eps
# moves no sign, so there only the decoded images change)
CHANGES = [(_copy_data, True), (_inplace_no_grad, True), (_load_state_dict, True), (_assign_data, True),
           (_assign_data_twice, True), (_new_parameter, True), (_eps, False), (_clamp, True), (_train_step, True)]


def _fresh(pkg, pn):
    """a module built with pn's tables and scalars as they are now"""
    f = ss.patchnorm(pkg, pn.median.detach().clone().cpu(), pn.b.detach().clone().cpu())
    f.eps, f.max_val, f.min_val = pn.eps, pn.max_val, pn.min_val
    return f


def _codes(fe, imgs, pn, lfq, **kw):
    ((_, codes),) = fe.encode_batch(imgs, pn, lfq, **kw)
    return codes.clone()


@pytest.mark.parametrize("change,codes_move", CHANGES, ids=[c.__name__.strip("_") for c, _ in CHANGES])
def test_patchnorm_update_reaches_every_cache(pkg, ref_tables, env, change, codes_move):
    fe, lfq, imgs, x = env
    _, _, fe_mod, _ = ss.mods()
    pn = ss.patchnorm(pkg, ref_tables.median, ref_tables.b)
    before = _codes(fe, imgs, pn, lfq)                     # codes only: the thresholds are cached now
    assert torch.equal(before, _codes(fe, imgs, pn, lfq, return_patches=True))
    enc = fe_mod.BatchEncoder(fe, 2, *SIZE, pn, lfq, device=DEV)
    dec = fe_mod.BatchDecoder(enc, pn, lfq)
    out = enc(x)
    assert torch.equal(out["codes"], before.view(out["codes"].shape))
    img_before = dec(out).clone()
    # unchanged tables: the pre-planned objects keep the state they hold (no device work, no rebuild)
    held = (enc.norm, enc._ncfg, dec.norm, pn._thr_cache[1])
    enc(x), dec(out)
    now = (enc.norm, enc._ncfg, dec.norm, pn._thr_cache[1])
    assert all(a is b for a, b in zip(now, held)) and enc.norm.thr is held[3]

    if change is _train_step:
        change(pn, env)
    else:
        change(pn)

    fresh = _fresh(pkg, pn)
    want = _codes(fe, imgs, fresh, lfq)
    with_patches = _codes(fe, imgs, pn, lfq, return_patches=True)
    codes_only = _codes(fe, imgs, pn, lfq)
    ss.assert_same_bits(ss.flat(with_patches), ss.flat(want), "return_patches=True against a fresh module")
    ss.assert_same_bits(ss.flat(codes_only), ss.flat(want), "codes-only encode_batch against a fresh module")
    assert torch.equal(before, want) != codes_move, "the change of tables does not show in the codes"
    # the objects planned before the change
    f_enc = fe_mod.BatchEncoder(fe, 2, *SIZE, fresh, lfq, device=DEV)
    f_out = {k: v.clone() for k, v in f_enc(x).items()}
    got = enc(x)
    ss.assert_same_bits(ss.flat(got), ss.flat(f_out), "a BatchEncoder made before the change")
    assert torch.equal(got["codes"], want.view(got["codes"].shape))
    f_img = fe_mod.BatchDecoder(f_enc, fresh, lfq)(f_out).clone()
    img = dec(got)
    ss.assert_same_bits(ss.flat(img), ss.flat(f_img), "a BatchDecoder made before the change")
    assert not torch.equal(img, img_before), "the change of tables does not show in the decoded images"


def test_patchnorm_pickle_and_state_dict_stay_plain(pkg, ref_tables, env):
    """tracked parameters pickle, deep-copy and save as plain ones: a state dict
    or a pickle of the module loads anywhere an nn.Parameter does, and the
    copies are tracked again on their first use"""
    import pickle
    fe, lfq, imgs, _ = env
    pn = ss.patchnorm(pkg, ref_tables.median, ref_tables.b)
    want = _codes(fe, imgs, pn, lfq)
    assert {k: type(v) for k, v in pn.state_dict().items()} == {k: torch.Tensor for k in ("n", "median", "b")}
    for clone in (pickle.loads(pickle.dumps(pn)), copy.deepcopy(pn)):
        assert isinstance(clone.median, torch.nn.Parameter) and not clone.median.requires_grad
        assert torch.equal(_codes(fe, imgs, clone, lfq), want)
        _copy_data(clone)
        assert torch.equal(_codes(fe, imgs, clone, lfq), _codes(fe, imgs, _fresh(pkg, clone), lfq))
        assert torch.equal(_codes(fe, imgs, pn, lfq), want)   # the original keeps its own tables and cache
    assert type(pickle.loads(pickle.dumps(pn.median))) is torch.nn.Parameter


def test_lfq_projection_weights_follow_data_copy(pkg, ref_tables, env):
    fe, _, imgs, _ = env
    pn = ss.patchnorm(pkg, ref_tables.median, ref_tables.b)
    torch.manual_seed(5)
    lfq_p = pkg.LFQ(dim=196, codebook_size=2 ** 13, num_codebooks=16).to(DEV).eval()
    before = _codes(fe, imgs, pn, lfq_p)
    g = torch.Generator().manual_seed(9)
    lfq_p.project_in.weight.data.copy_(torch.randn(lfq_p.project_in.weight.shape, generator=g) / 14.0)
    fresh = pkg.LFQ(dim=196, codebook_size=2 ** 13, num_codebooks=16).to(DEV).eval()
    fresh.load_state_dict(lfq_p.state_dict())
    after = _codes(fe, imgs, pn, lfq_p)
    assert torch.equal(after, _codes(fe, imgs, pn, fresh)) and not torch.equal(after, before)


def test_model_pack_follows_data_copy(pkg, env):
    fe, _, imgs, _ = env
    side = dict(hidden_size=64, intermediate_size=128, num_attention_heads=1, num_hidden_layers=1)
    cfg = pkg.DCTAutoencoderConfig(patch_size=14, vq_codebook_size=2 ** 8, vq_num_codebooks=2, encoder_config=side,
                                   decoder_config=side)
    torch.manual_seed(3)
    model = pkg.DCTAutoencoder(cfg).to(DEV).eval()
    ((dp, _),) = fe.encode_batch(imgs, None, None, return_raw=True)

    def run(m):
        out = m(dp.shallow_copy())
        return ss.flat([out["codes"], out["dct_patches"].patches])

    before = run(model)
    lin = model.to_patch_embedding[0]
    g = torch.Generator().manual_seed(4)
    lin.weight.data.copy_(torch.randn(lin.weight.shape, generator=g) / 14.0)
    fresh = pkg.DCTAutoencoder(cfg).to(DEV).eval()
    fresh.load_state_dict(model.state_dict())
    after = run(model)
    ss.assert_same_bits(after, run(fresh), "the model's bf16 packs after weight.data.copy_")
    assert not torch.equal(after[0][1], before[0][1]) or not torch.equal(after[1][1], before[1][1])
