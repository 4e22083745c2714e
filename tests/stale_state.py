"""Helpers of the tests that look for results depending on something other than
the call's own inputs: stale scratch (test_gpu_stale_scratch.py), output
memory no kernel wrote (test_gpu_outputs_written.py), the context's caches
(test_gpu_context_caches.py) and the Python-side caches
(test_gpu_table_updates.py).  A plain module: no test lives here."""
import ctypes as C
from importlib import import_module

import torch

from oracle import rng
from test_gpu_options import _context, _set, _stages   # noqa: F401  (a fresh context, an option, the stage table)

DEV = "cuda"


def mods():
    """(_lib, _ops, feature_extraction, packing) of the package under test"""
    return tuple(import_module("dct_autoencoder_amd." + m) for m in ("_lib", "_ops", "feature_extraction", "packing"))


def timed(ctx):
    ctx.check(ctx.lib.dctae_set_timing(ctx.h, 1))
    return ctx


def bits(t):
    """an integer view of the tensor on the host, so that NaN payloads and -0.0 count"""
    t = t.detach().contiguous()
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    elif t.dtype.is_floating_point:
        t = t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t.cpu()


def flat(out, prefix=""):
    """[(name, integer host tensor)] of a tensor / dict / list / tuple of them (None entries skipped)"""
    if out is None:
        return []
    if torch.is_tensor(out):
        return [(prefix or "out", bits(out))]
    items = sorted(out.items()) if isinstance(out, dict) else enumerate(out)
    res = []
    for k, v in items:
        res += flat(v, f"{prefix}.{k}" if prefix else str(k))
    return res


def assert_same_bits(a, b, what):
    """a, b: results of flat().  Equal names, shapes, dtypes and every bit."""
    assert [n for n, _ in a] == [n for n, _ in b], what
    for (name, x), (_, y) in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {name} {x.shape} {x.dtype} vs {y.shape} {y.dtype}"
        if not torch.equal(x, y):
            bad = (x != y).reshape(-1).nonzero().flatten()
            raise AssertionError(f"{what}: {name} differs in {bad.numel()} of {x.numel()} words, first at flat index "
                                 f"{int(bad[0])}: {int(x.reshape(-1)[bad[0]])} vs {int(y.reshape(-1)[bad[0]])}")


def images(seed, sizes, dev=DEV):
    return [torch.from_numpy(x).to(dev) for x in rng.synth_images(seed, sizes)]


def byte_images(seed, sizes, dev=DEV):
    return [(x * 255.0).round().clamp(0, 255).to(torch.uint8) for x in images(seed, sizes, dev)]


def tables(seed, mh, mw, P):
    """PatchNorm tables of any geometry: medians around zero, b in [0.05, 1.05)"""
    g = torch.Generator().manual_seed(seed)
    med = torch.randn(3, mh, mw, P * P, generator=g) * 0.05
    b = torch.rand(3, mh, mw, P * P, generator=g) + 0.05
    return med, b


def patchnorm(pkg, med, b, dev=DEV):
    mh, mw, pp = med.shape[1:]
    pn = pkg.PatchNorm(mh, mw, int(round(pp ** 0.5)), 3).to(dev)
    with torch.no_grad():
        pn.median.copy_(med)
        pn.b.copy_(b)
    pn.frozen = True
    return pn.eval()


def encode(fe, imgs, pn, lfq, *, patches=False, raw=False, scores=False, codes_dtype=torch.int64, uint8=False,
           out=None, ks=None):
    """encode_batch's fused path for one packing plan, through _ops.encode, so
    that the caller can pass the output tensors (``out``): the dict of packed
    tensors.  LFQ with projections: the packed PatchNorm output, then the
    projection kernel, as encode_batch runs it."""
    _, ops, _, packing = mods()
    desc, dev, keep = (ops.image_set_u8 if uint8 else ops.image_set)(imgs)
    sizes = [(im.shape[1], im.shape[2]) for im in imgs]
    ks = ks or [min(fe._tokens(h, w), fe.max_seq_len) for h, w in sizes]
    max_tok = fe.max_patch_h * fe.max_patch_w * fe.channels
    (rows,) = list(packing.iter_batch_plans([(ks, list(range(len(ks))))], fe.max_seq_len, max_tok, None))
    plan = packing.layout(rows, dict(enumerate(ks)))
    proj = lfq is not None and lfq.has_projections
    want_norm = patches or proj
    norm = pn.state(thresholds=not want_norm) if pn is not None else None
    lcfg = lfq.cfg() if lfq is not None and not proj else None
    res = ops.encode(desc, dev, fe.params(), plan, plan.n_rows, fe.max_seq_len, norm, lcfg,
                     want_codes=lcfg is not None, want_patches=want_norm, want_raw=raw, want_scores=scores, out=out,
                     codes_dtype=codes_dtype)
    if proj:
        res["codes"] = lfq.project_codes(res["patches"], x_bound=max(abs(norm.min_val), abs(norm.max_val)),
                                         codes_dtype=codes_dtype)
    res["_plan"] = plan
    res["_sizes"] = sizes
    return res


def tensors(res):
    return {k: v for k, v in res.items() if torch.is_tensor(v)}


def filled_like(res, byte):
    """tensors of res's shapes and dtypes with every byte set to ``byte``"""
    out = {}
    for k, v in tensors(res).items():
        t = torch.empty_like(v)
        t.view(torch.uint8).fill_(byte)
        out[k] = t
    return out


def decode_args(fe, res):
    """what _ops.decode / decode_table take, of an encode()'s result"""
    _, _, _, packing = mods()
    plan, sizes = res["_plan"], res["_sizes"]
    S = res["key_pad_mask"].shape[1]
    return (fe.params(S), res["image_ids"], res["key_pad_mask"], res["positions"], res["channels"],
            [packing.patch_grid(*sizes[i], fe.patch_size) for i in plan.images], [tuple(sizes[i]) for i in plan.images])


def spectrum_tokens(fe, imgs, uint8=False):
    """dctae_spectrum_tokens(_u8): (tokens, scores) in flat token order"""
    lib, ops, _, _ = mods()
    dev = imgs[0].device
    ctx = lib.context(dev)
    desc, _, keep = (ops.image_set_u8 if uint8 else ops.image_set)(imgs)
    n = [fe._tokens(im.shape[1], im.shape[2]) for im in imgs]
    off = lib.i64([sum(n[:i]) for i in range(len(n))])
    PP = fe.patch_size ** 2
    tok = torch.empty((sum(n), PP), dtype=torch.float32, device=dev)
    sc = torch.empty(sum(n), dtype=torch.float32, device=dev)
    cfg = fe.params().c(fe.max_seq_len)
    name = "dctae_spectrum_tokens" + ("_u8" if uint8 else "")
    ctx.check(getattr(ctx.lib, name)(ctx.h, C.byref(cfg), C.byref(desc), C.cast(off, C.POINTER(C.c_int64)),
                                     lib.ptr(tok), lib.ptr(sc), lib.stream_ptr(dev)), name)
    return tok, sc
