"""No result depends on scratch an earlier call left behind.

The context's five scratch buffers (workspace, staging, PatchNorm statistics,
VectorQuantize, LFQ projection) keep what the previous call wrote, and the
suite encodes the same images many times: a kernel that skips part of T / T' /
Y or of the staging would read the previous, identical values and pass.  Every
case here computes its outputs three times on one fresh context:

  1. plain (the buffers hold what the previous case's larger call left);
  2. with ``ws_poison=1`` (every buffer the call asks for is filled with 0xff
     bytes before the call's first use of it);
  3. with ``ws_poison=1`` after an unrelated call on other data, larger than
     every such call before it on this context, has grown and refilled all
     five buffers (so the workspace has moved),

and the three must be equal bit for bit (integer views: NaN payloads count).
Each case also asserts, through the library's timing table, that the stages it
is named after ran in all three runs: a case must not pass by being routed
elsewhere.  The timing table names stages, not kernels: where an option only
picks another kernel for the same stage (``cols512b``, ``rows_kernel``,
``cols_wide``, ``sort_kernel``, ``gemm_h2`` / ``gemm_x3`` / ``gemm_dma`` /
``cols_dma``, the decode's kernel switches, the bitonic sort above 3072
tokens) the stage check shows the route and the option itself picks the
kernel.
Shapes are the smallest that reach the kernel."""
import dataclasses
from typing import Callable, Dict, Tuple

import pytest
import torch

import stale_state as ss
from test_gpu_vq import _make as make_vq
from test_options_host import DEFAULTS

pytestmark = pytest.mark.gpu
DEV = ss.DEV
I16 = torch.int16


class Env:
    """what the cases share: one fresh context, the modules, cached inputs"""

    def __init__(self, pkg, ref_tables, ctx):
        self.pkg, self.ctx = pkg, ctx
        self.lib, self.ops, self.fe_mod, self.packing = ss.mods()
        FE = pkg.DCTAutoencoderFeatureExtractor
        self.fe = FE(3, 14, 0.0, 32, 32, 3072)
        self.fe_drop = FE(3, 14, 0.0, 32, 32, 2000)    # a 512^2 image keeps 2000 of its 3072 tokens
        self.fe_drop_s = FE(3, 14, 0.0, 32, 32, 50)    # a 64 x 96 image keeps 50 of its 72
        self.fe2 = FE(3, 2, 0.0, 40, 40, 4800)         # 80 x 80 at P = 2: 4800 tokens, the bitonic sort
        self.pn = ss.patchnorm(pkg, ref_tables.median, ref_tables.b)
        self.pn2 = ss.patchnorm(pkg, *ss.tables(11, 40, 40, 2))
        lfq = lambda **kw: pkg.LFQ(**kw).to(DEV).eval()   # noqa: E731
        self.lfq = lfq(dim=196, codebook_size=2 ** 14, num_codebooks=14)
        self.lfq28 = lfq(dim=196, codebook_size=2 ** 7, num_codebooks=28)
        self.lfq2 = lfq(dim=4, codebook_size=4, num_codebooks=2)
        torch.manual_seed(5)
        self.lfq_p = lfq(dim=196, codebook_size=2 ** 13, num_codebooks=16)   # 196 -> 208 -> 196
        assert self.lfq_p.has_projections and not self.lfq28.has_projections and not self.lfq2.has_projections
        self._cache: Dict = {}
        self.grown = 0

    def once(self, key, fn):
        """an input made on first use; what making it launched is taken off the timing table (a case
        makes its inputs before the calls it is about)"""
        if key not in self._cache:
            self._cache[key] = fn()
            torch.cuda.synchronize()
            ss._stages(self.ctx)
        return self._cache[key]

    def imgs(self, seed, sizes, uint8=False):
        def make():
            if len(sizes) >= 16 and not uint8:   # a large uniform batch: generated on the device
                return list(self.ops.synth_images(len(sizes), *sizes[0], seed=seed))
            return (ss.byte_images if uint8 else ss.images)(seed, sizes)
        return self.once(("imgs", seed, tuple(sizes), uint8), make)

    def grow(self, images=None):
        """an unrelated call on every scratch buffer, larger than the one before:
        an encode with every sink (workspace, staging), a statistics step on its
        tokens, a VectorQuantize forward with projections and a mask, and a
        256 -> 240 LFQ projection (the largest weight the kernels take)"""
        k = self.grown
        self.grown += 1
        n, h, w = images or (3 + k // 10, 520 + 4 * k, 530 + 2 * k)
        x = self.ops.synth_images(n, h, w, seed=1000 + k)
        r = ss.encode(self.fe, list(x), self.pn, self.lfq, patches=True, raw=True, scores=True)
        med, b = ss.tables(12, 32, 32, 14)
        self.ops.norm_train_step(r["raw"], r["channels"], r["positions"], r["key_pad_mask"],
                                 torch.zeros(3, 32, 32, device=DEV), med.to(DEV), b.to(DEV), self.fe.params())
        g = torch.Generator().manual_seed(k)
        vq = self.once("grow_vq", lambda: make_vq(self.pkg, 96, 4, 700, seed=3))
        nv = 2048 + 256 * k
        vq(torch.randn(1, nv, 96, generator=g).to(DEV), mask=(torch.rand(1, nv, generator=g) > 0.2).to(DEV))
        big = self.once("grow_lfq", lambda: self.pkg.LFQ(dim=256, codebook_size=2 ** 15, num_codebooks=16).to(DEV).eval())
        big.project_codes(torch.randn(300 + k, 256, generator=g).to(DEV))
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def env(pkg, ref_tables):
    lib = ss.mods()[0]
    with ss._context(lib) as ctx:
        yield Env(pkg, ref_tables, ss.timed(ctx))


@dataclasses.dataclass
class Case:
    name: str
    run: Callable                                  # (env) -> tensors / dicts / lists of them
    stages: Dict[str, int]                         # stage name -> least number of launches in the call
    opts: Dict[str, int] = dataclasses.field(default_factory=dict)
    absent: Tuple[str, ...] = ()                   # stages that must not run
    grow: Tuple[int, int, int] = None              # (n, h, w) of the larger call where the default is too small


# ---- the encode ------------------------------------------------------------------------------------------------
def enc(sizes, seed=31, fe="fe", pn="pn", lfq="lfq", uint8=False, codes_dtype=torch.int64, edit=None):
    """codes with every other sink, then codes only (the threshold path): all of both calls' tensors"""
    def run(env):
        x = env.imgs(seed, sizes, uint8)
        if edit is not None:
            x = env.once(("edit", seed, tuple(sizes), edit.__name__), lambda: edit([t.clone() for t in x]))
        f, p, q = getattr(env, fe), getattr(env, pn), getattr(env, lfq)
        kw = dict(uint8=uint8, codes_dtype=codes_dtype)
        return [ss.tensors(ss.encode(f, x, p, q, patches=True, raw=True, scores=True, **kw)),
                ss.tensors(ss.encode(f, x, p, q, **kw))]
    return run


def _hot_and_inf(x):
    """a pixel of 40.0 leaves k_rows_fused's fixed fp16 scale, an inf pixel is not finite: both are redone"""
    x[0][1, 5, 7] = 40.0
    x[1][2, 3, 2] = float("inf")
    return x


FFT = {"fft_rows": 2, "fft_cols": 2, "sort_pack": 2}        # two calls per case
GEMM = {"rows_fused": 2, "rows_fixup": 2, "gemm_cols": 2, "tile_epilogue": 2, "sort_pack": 2, "pad_fill": 2}
NO_GEMM = ("gemm_rows", "gemm_cols", "rows_fused", "bs_rows", "bs_cols")
NO_FFT = ("fft_rows", "fft_cols", "bs_rows", "bs_cols")
S512, S224, SG = [(512, 512)] * 2, [(224, 224)] * 3, [(37, 53), (333, 517)]

ENCODE = [
    Case("512", enc(S512), FFT, absent=NO_GEMM + ("pad_fill",)),
    Case("512-cols512b=0", enc(S512), FFT, {"cols512b": 0}, NO_GEMM),
    Case("512-rows_kernel=2", enc(S512), FFT, {"rows_kernel": 2}, NO_GEMM),
    Case("512-cols_wide=1", enc(S512), FFT, {"cols_wide": 1}, NO_GEMM),
    Case("512-sort_kernel=1", enc(S512), FFT, {"sort_kernel": 1}, NO_GEMM),
    Case("512-chunks", enc([(512, 512)] * 3), {"fft_rows": 6, "fft_cols": 6}, {"chunk_bytes": 4 << 20}, NO_GEMM),
    Case("512x300+300x512", enc([(512, 300), (300, 512)]),
         {"fft_rows": 2, "fft_cols": 2, "gemm_rows": 2, "gemm_cols": 2, "fold_t": 2, "tile_epilogue": 2}),
    Case("224", enc(S224), FFT | {"pad_fill": 2}, absent=NO_GEMM),
    Case("224x98+98x224", enc([(224, 98), (98, 224)]), FFT | {"pad_fill": 2}),
    Case("gemm-small", enc([(37, 53), (15, 17), (14, 14)]), GEMM, absent=NO_FFT),
    Case("gemm-333x517", enc(SG), GEMM, absent=NO_FFT),
    Case("gemm-rows_fused=0", enc(SG), {"rgb_to_ipt": 2, "gemm_rows": 2, "gemm_cols": 2, "tile_epilogue": 2},
         {"rows_fused": 0}, NO_FFT + ("rows_fused",)),
    Case("gemm-tperm=0", enc(SG), {"rgb_to_ipt": 2, "gemm_rows": 2, "gemm_cols": 2, "tile_epilogue": 2}, {"tperm": 0},
         NO_FFT + ("rows_fused",)),   # the fused row pass writes the parity-planar T only
    Case("gemm-gemm_h2=0", enc(SG), {"gemm_cols": 2, "tile_epilogue": 2}, {"gemm_h2": 0}, NO_FFT),
    Case("gemm-gemm_x3=0", enc(SG), {"gemm_cols": 2, "tile_epilogue": 2}, {"gemm_x3": 0}, NO_FFT),
    Case("gemm-gemm_dma=0", enc(SG), GEMM, {"gemm_dma": 0}, NO_FFT),
    Case("gemm-cols_dma=0", enc(SG), GEMM, {"cols_dma": 0}, NO_FFT),
    Case("gemm-fixup", enc([(37, 53), (45, 51)], edit=_hot_and_inf), GEMM, absent=NO_FFT),
    Case("fft_generic-64x96", enc([(64, 96)] * 2), FFT, {"fft_generic": 1}, NO_GEMM),
    Case("fft_odd-45x75", enc([(45, 75)] * 2), FFT, {"fft_generic": 1, "fft_odd": 1}, NO_GEMM),
    Case("bluestein", enc([(58, 46), (46, 58), (37, 53)]), {"bs_rows": 2, "bs_cols": 2, "tile_epilogue": 2},
         {"bluestein": 1}, ("gemm_rows", "gemm_cols", "rows_fused")),
    Case("bitonic-P2", enc([(80, 80)] * 2, fe="fe2", pn="pn2", lfq="lfq2"), {"sort_pack": 2}),
    # one byte-input and one int16-code variant per kernel family instantiated on them
    Case("u8-512", enc(S512, uint8=True), FFT, absent=NO_GEMM),
    Case("u8-224", enc(S224, uint8=True), FFT, absent=NO_GEMM),
    Case("u8-gemm", enc(SG, uint8=True), GEMM, absent=NO_FFT),
    Case("c16-ncb14", enc([(512, 512), (224, 224)], codes_dtype=I16), FFT | {"pad_fill": 2}),
    Case("c16-ncb28", enc([(224, 224), (37, 53)], lfq="lfq28", codes_dtype=I16), {"sort_pack": 2, "pad_fill": 2}),
    Case("i64-ncb28", enc([(224, 224), (37, 53)], lfq="lfq28"), {"sort_pack": 2, "pad_fill": 2}),
    Case("u8-c16-gemm", enc(SG, uint8=True, codes_dtype=I16), GEMM, absent=NO_FFT),
]


def _batch_encoder(B, H, W, lfq="lfq_p", **kw):
    def run(env):
        e = env.once(("benc", B, H, W, lfq, tuple(kw.items())),
                     lambda: env.fe_mod.BatchEncoder(env.fe, B, H, W, env.pn, getattr(env, lfq), device=DEV, **kw))
        # every row full: dctae_encode_lfq_proj, not dctae_encode followed by dctae_lfq_project_in (same stages)
        assert e.proj_staged
        u8 = kw.get("input_dtype") == torch.uint8
        x = env.once(("bx", B, H, W, u8), lambda: torch.stack(env.imgs(33, [(H, W)] * B, u8)).contiguous())
        return {k: v.clone() for k, v in e(x).items()}
    return run


def _project(which):
    def run(env):
        q, ops = env.lfq_p, env.ops
        r = env.once("proj_in", lambda: ss.tensors(ss.encode(env.fe, env.imgs(34, [(224, 98), (37, 53)]), env.pn,
                                                             q, patches=True)))
        wi, bi = q._proj_w(q.project_in, r["codes"].device)
        wo, bo = q._proj_w(q.project_out, r["codes"].device)
        if which == "in":
            return [ops.lfq_project_in(r["patches"], wi, bi, q.cfg()),
                    ops.lfq_project_in(r["patches"], wi, bi, q.cfg(), x_bound=6.0),
                    ops.lfq_project_in(r["patches"], wi, bi, q.cfg(), x_bound=6.0, codes_dtype=I16)]
        if which == "out":
            return [ops.lfq_project_out(r["codes"], wo, bo, q.cfg()),
                    ops.lfq_project_out(r["codes"].to(I16), wo, bo, q.cfg())]
        return ops.lfq_project_out_inverse_norm(r["codes"], wo, bo, q.cfg(), env.pn.state(), env.fe.params(),
                                                r["channels"], r["positions"])
    return run


def _token_mode(env):
    x, x8 = env.imgs(35, [(28, 60), (46, 58), (224, 224)]), env.imgs(35, [(28, 60), (46, 58)], True)
    items = env.fe.preprocess_many(x)
    return [[it["patches"], it["positions"], it["channels"]] for it in items] + \
        [ss.spectrum_tokens(env.fe, x), ss.spectrum_tokens(env.fe, x8, True)]


def _dct2(env):
    out = []
    for x in [torch.stack(env.imgs(36, [hw] * 2)) for hw in ((37, 53), (64, 96))]:
        y = env.ops.dct2(x, inverse=False, color=True)
        out += [y, env.ops.dct2(y, inverse=True, color=True), env.ops.dct2(x, inverse=False, color=False)]
    return out


def _patch_spectrum(env):
    x = env.once("spectrum", lambda: env.ops.dct2(env.imgs(37, [(56, 70)])[0], inverse=False, color=True))
    return list(env.ops.patch_spectrum(x, env.fe.params(), 60))


ENCODE_SIDE = [
    Case("encode_lfq_proj", _batch_encoder(2, 512, 512), {"lfq_project_in": 1, "fft_rows": 1, "sort_pack": 1}),
    Case("encode_lfq_proj-u8-c16", _batch_encoder(2, 512, 512, input_dtype=torch.uint8, codes_dtype=I16),
         {"lfq_project_in": 1, "fft_rows": 1, "sort_pack": 1}),
    Case("lfq_project_in", _project("in"), {"lfq_project_in": 3}),
    Case("lfq_project_out", _project("out"), {"lfq_project_out": 2}),
    Case("lfq_project_out_inverse_norm", _project("inv"), {"lfq_project_out": 1}),
    Case("token-mode", _token_mode, {"tile_epilogue": 1, "sort_pack": 1, "fft_cols": 1}),
    Case("dct2", _dct2, {"dct2_gemm": 6, "rgb_to_ipt": 2, "ipt_to_rgb": 2}),
    Case("patch_spectrum", _patch_spectrum, {"tile_epilogue": 1, "sort_pack": 1}),
]


# ---- the decode ------------------------------------------------------------------------------------------------
def dec(sizes, src="codes", fe="fe", lfq="lfq", out_dtype=torch.float32, codes_dtype=torch.int64, edit=None):
    def run(env):
        f, q = getattr(env, fe), getattr(env, lfq)

        def inputs():
            r = ss.encode(f, env.imgs(41, sizes), env.pn, q, patches=True, raw=True, codes_dtype=codes_dtype)
            return edit(r) if edit is not None else r
        r = env.once(("dec", tuple(sizes), fe, lfq, codes_dtype, edit and edit.__name__), inputs)
        args = ss.decode_args(f, r)
        kw = {"codes": dict(codes=r["codes"], norm=env.pn.state(), lfq=q.cfg()), "patches": dict(patches=r["raw"]),
              "normed": dict(patches=r["patches"], norm=env.pn.state(), normed=True)}[src]
        return env.ops.decode(*args, out_dtype=out_dtype, **kw)
    return run


def _duplicates(r):
    """two tokens at one image place, in either order in the row (FE:639-643: the later slot wins)"""
    for a, b in ((3, 17), (40, 8)):
        r["positions"][0, a] = r["positions"][0, b]
        r["channels"][0, a] = r["channels"][0, b]
    return r


DFFT = {"dec_map": 1, "idct_cols": 1, "idct_rows": 1}
DGEMM = {"dec_map": 1, "scatter_tokens": 1, "idct_cols": 1, "idct_rows": 1, "ipt_to_rgb": 1}
RAGGED = [(37, 53), (224, 98), (15, 17), (333, 517)]
DECODE = [
    Case("dec512", dec(S512), DFFT, absent=("scatter_tokens",)),
    Case("dec512-cols=1", dec(S512), DFFT, {"dec_cols_kernel": 1}, ("scatter_tokens",)),
    Case("dec512-rows=2", dec(S512), DFFT, {"dec_rows_kernel": 2}, ("scatter_tokens",)),
    Case("dec512-cols=1-rows=2", dec(S512), DFFT, {"dec_cols_kernel": 1, "dec_rows_kernel": 2}, ("scatter_tokens",)),
    Case("dec512-patches", dec(S512, "patches"), DFFT, absent=("scatter_tokens",)),
    Case("dec512-normed", dec(S512, "normed"), DFFT, absent=("scatter_tokens",)),
    Case("dec512-u8", dec(S512, out_dtype=torch.uint8), DFFT, absent=("scatter_tokens",)),
    Case("dec512-c16", dec(S512, codes_dtype=I16), DFFT, absent=("scatter_tokens",)),
    Case("dec512-dropped", dec(S512, fe="fe_drop"), DFFT, absent=("scatter_tokens",)),
    Case("dec512-duplicates", dec(S512, edit=_duplicates), DFFT, absent=("scatter_tokens",)),
    Case("dec-ragged", dec(RAGGED), DGEMM),
    Case("dec-ragged-patches", dec(RAGGED, "patches"), DGEMM),
    Case("dec-ragged-normed", dec(RAGGED, "normed"), DGEMM | {"norm_inverse": 1}),
    Case("dec-ragged-u8", dec(RAGGED, out_dtype=torch.uint8), DGEMM),
    Case("dec-ragged-c16-u8", dec(RAGGED, codes_dtype=I16, out_dtype=torch.uint8), DGEMM),
    Case("dec-ragged-dropped", dec([(64, 96), (37, 53), (64, 96)], fe="fe_drop_s"), DGEMM),
    Case("dec-ragged-duplicates", dec(RAGGED, edit=_duplicates), DGEMM),
]


# ---- the rest --------------------------------------------------------------------------------------------------
def _tokens(env):
    return env.once("tokens", lambda: ss.tensors(ss.encode(env.fe, env.imgs(51, [(224, 98), (37, 53), (64, 96)]),
                                                           None, None, raw=True)))


def _train_step(env):
    r = _tokens(env)
    med, b = ss.tables(13, 32, 32, 14)
    n, med, b = torch.full((3, 32, 32), 2.0, device=DEV), med.to(DEV), b.to(DEV)
    y = env.ops.norm_train_step(r["raw"], r["channels"], r["positions"], r["key_pad_mask"], n, med, b, env.fe.params())
    return [y, n, med, b]


def _stats_steps(env):
    r, p = _tokens(env), env.fe.params()
    args = (r["raw"], r["channels"], r["positions"], r["key_pad_mask"])
    bn, bm = env.ops.norm_batch_stats(*args, p)
    med, b = (t.to(DEV) for t in ss.tables(13, 32, 32, 14))
    n = torch.full((3, 32, 32), 2.0, device=DEV)
    env.ops.norm_merge_(med, bm, n, bn, False)
    bb = env.ops.norm_batch_mad(*args, med, p)
    env.ops.norm_merge_(b, bb, n, bn, True)
    return [bn, bm, bb, med, b, n, env.ops.norm_batch_stats(r["raw"], r["channels"], r["positions"], None, p)]


def _vq(dim, mask):
    def run(env):
        vq = make_vq(env.pkg, dim, 4, 300, seed=2)   # a new module each time: the forward updates its batch statistics
        g = torch.Generator().manual_seed(6)
        x = torch.randn(2, 77, dim, generator=g).to(DEV)
        m = (torch.rand(2, 77, generator=g) > 0.3).to(DEV) if mask else None
        q, idx, _ = vq(x, mask=m)
        cb = vq._codebook
        return [q, idx, cb.batch_mean, cb.batch_variance, vq.get_output_from_indices(idx)]
    return run


def _entropy(env):
    g = torch.Generator().manual_seed(8)
    h = torch.randn(3, 50, 14 * 8, generator=g).to(DEV)
    mask = (torch.rand(3, 50, generator=g) > 0.25).to(DEV)
    cfg = env.once("ent_lfq", lambda: env.pkg.LFQ(dim=112, codebook_size=2 ** 8, num_codebooks=14).to(DEV)).cfg()
    avg, sc = env.ops.lfq_entropy_forward(h, mask, cfg)
    return [avg, sc, env.ops.lfq_entropy_backward(h, mask, cfg, avg, sc, torch.tensor(0.7, device=DEV))]


VQ_STAGES = {"vq_codebook": 1, "vq_assign": 1}
REST = [
    Case("norm_train_step", _train_step, {"norm_train_step": 1}),
    Case("stats-steps", _stats_steps, {"norm_batch_stats": 2, "norm_batch_mad": 1, "norm_merge": 2}),
    Case("vq", _vq(64, False), VQ_STAGES, absent=("vq_project_in",)),
    Case("vq-mask", _vq(64, True), VQ_STAGES, absent=("vq_project_in",)),
    Case("vq-proj", _vq(96, False), VQ_STAGES | {"vq_project_in": 1, "vq_project_out": 2, "vq_codes": 1}),
    Case("vq-proj-mask", _vq(96, True), VQ_STAGES | {"vq_project_in": 1, "vq_project_out": 2, "vq_codes": 1}),
    Case("lfq-entropy", _entropy, {"lfq_entropy_forward": 1, "lfq_entropy_backward": 1}),
]

# the two-stream schedules last: their batches are the largest calls of the module
SIDE = [
    Case("halves-32x224", enc([(224, 224)] * 32), {"fft_rows": 4, "fft_cols": 4, "sort_pack": 4}, {"halves": 1},
         NO_GEMM),   # the default larger call (nine images of about 760 x 650 by now) is the larger one
    Case("sort_overlap-64x512", enc([(512, 512)] * 64), {"fft_rows": 2, "fft_cols": 4, "sort_pack": 2},
         {"sort_overlap": 1}, NO_GEMM, grow=(72, 512, 512)),
]

CASES = ENCODE + ENCODE_SIDE + DECODE + REST + SIDE
assert len({c.name for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_outputs_do_not_depend_on_stale_scratch(env, case):
    ctx = env.ctx

    def run():
        ss._stages(ctx)
        out = ss.flat(case.run(env))
        torch.cuda.synchronize()
        return out, ss._stages(ctx)

    try:
        for k, v in case.opts.items():
            ss._set(ctx, k, v)
        plain, st_plain = run()
        ss._set(ctx, "ws_poison", 1)
        poisoned, st_poisoned = run()
        env.grow(case.grow)
        regrown, st_regrown = run()
    finally:
        torch.cuda.synchronize()
        for k in list(case.opts) + ["ws_poison"]:
            ss._set(ctx, k, DEFAULTS[k])
    print(f"[{case.name}] stages {st_plain}")
    for name, least in case.stages.items():
        assert st_plain.get(name, 0) >= least, f"stage {name}: {st_plain.get(name, 0)} launches, expected >= {least}"
    for name in case.absent:
        assert name not in st_plain, f"stage {name} ran: the case was routed elsewhere"
    assert st_poisoned == st_plain and st_regrown == st_plain
    ss.assert_same_bits(plain, poisoned, "plain against ws_poison=1")
    ss.assert_same_bits(plain, regrown, "plain against ws_poison=1 after a larger call regrew the buffers")
