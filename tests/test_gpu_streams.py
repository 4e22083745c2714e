"""The library driven from more than one stream (DESIGN.md "Streams and the
context's scratch").  Run on an MI355X: pytest -m gpu tests/test_gpu_streams.py

(a) Ordering harness.  A dctae_ctx owns device memory that successive calls
reuse; a call on one stream must wait for the context's previous call on
another (the OrderedCall scope, csrc/dctae_ctx.h).  For a pair
(first, second) of calls on one context the harness

  1. warms both (second, then first: the workspace, the plan buffer and the
     DCT matrices grow here, on the host-synchronising paths), times the pair
     once more with events, and synchronises the device;
  2. on stream A launches a blocker of ~100 ms, records the blocker's event,
     launches `first`, records eA;
  3. on stream B launches `second`;
  4. requires the blocker's event to be still pending: the host ran ahead of
     the parked stream, so the run is conclusive;
  5. synchronises B and requires eA: when B's work is done, `first` is done.

An unordered `second` runs to completion while `first` is still parked behind
the blocker, so the failing state never has two kernels in the same scratch.
eA is recorded on A right after the call's own event; it may trail that event
by the few microseconds a marker takes, so step 5 polls eA for at most 1/50 of
the blocker before it gives up -- an unordered pair would need the whole rest
of the blocker, fifty times as long.

The partner of every pair is dctae_lfq_project_out, which follows the protocol
and uploads no plan (two plan uploads in one pair would wait on the host for
the parked stream).  (partner, partner) proves the partner; a control pair of
two plain torch kernels proves that A and B really run side by side here (it
must come out *unordered*).  Every ORDERED row of
test_stream_contract_host.TABLE is then `first` once and `second` once.  The
calls go to the C ABI through ctypes with buffers allocated once, so warmed
and measured calls are the same call.

(b) Every public operation of the Python layer once under
``torch.cuda.stream(side)``, against the default-stream result of the same
inputs: bit equality wherever the project already asserts run-to-run bit
identity, test_gpu_vq.py's tolerances for VectorQuantize (fp64 atomics).

(c) The training arrangement as a regression check: 20 steps, stream A encodes
batch i + 1 while stream B runs the step's losses on batch i, forward and
backward, no host synchronisation in the loop; everything equals the serial
default-stream run bit for bit.
"""
import ctypes as C
import math
import time

import pytest
import torch

from conftest import golden
from test_gpu_model_train import golden as model_golden  # noqa: F401  (that module's model fixture)
from test_stream_contract_host import HARNESS_ROWS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TARGET_MS = 100.0      # the blocker
PAIR_FRACTION = 20     # a warmed pair takes less than 1 / 20 of the blocker
PARTNER = "lfq_project_out"

# (symbol, label): the harness cases, every ORDERED row at least once
CASES = [
    ("dctae_encode", "encode_gemm"), ("dctae_encode", "encode_fft512"),
    ("dctae_encode_lfq_proj", "encode_lfq_proj"), ("dctae_spectrum_tokens", "spectrum_tokens"),
    ("dctae_dct2", "dct2"), ("dctae_patch_spectrum", "patch_spectrum"),
    ("dctae_decode", "decode_gemm"), ("dctae_decode", "decode_fft512"),
    ("dctae_decode_normed", "decode_normed_gemm"), ("dctae_decode_normed", "decode_normed_fft512"),
    ("dctae_decode_backward", "decode_backward"), ("dctae_pixel_loss_forward", "pixel_loss_forward"),
    ("dctae_rec_loss_forward", "rec_loss_forward"),
    ("dctae_lfq_entropy_forward", "lfq_entropy_forward"), ("dctae_lfq_entropy_backward", "lfq_entropy_backward"),
    ("dctae_lfq_project_in", "lfq_project_in"), ("dctae_lfq_project_in_bounded", "lfq_project_in_bounded"),
    ("dctae_lfq_project_out", PARTNER), ("dctae_lfq_project_out_inverse_norm", "lfq_project_out_inverse_norm"),
    ("dctae_vq_forward", "vq_forward"), ("dctae_vq_output_from_indices", "vq_output_from_indices"),
    ("dctae_norm_batch_stats", "norm_batch_stats"), ("dctae_norm_batch_mad", "norm_batch_mad"),
    ("dctae_norm_train_step", "norm_train_step"),
]
LABELS = [label for _, label in CASES]
MEASURED = {}   # (first, second) -> ms of the warmed pair


def _ops():
    from dct_autoencoder_amd import _ops
    return _ops


def _event(timing=False):
    return torch.cuda.Event(enable_timing=timing)


def _ms(fn):
    a, b = _event(True), _event(True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


# ---------------------------------------------------------------- the blocker
class Blocker:
    """~TARGET_MS of work on the current stream that leaves the other streams
    free: torch.cuda._sleep, calibrated with events; a chain of large torch.mm
    if _sleep does not give the time asked for."""

    def __init__(self):
        self.cycles_per_ms = self._calibrate_sleep()
        self.mode = "sleep" if self.cycles_per_ms else "mm"
        if self.mode == "mm":
            self.x = torch.randn(4096, 4096, device=DEV)
            self.y = torch.empty_like(self.x)
            torch.mm(self.x, self.x, out=self.y)
            self.mm_ms = _ms(lambda: [torch.mm(self.x, self.x, out=self.y) for _ in range(8)]) / 8
        self.set_target(TARGET_MS)

    @staticmethod
    def _calibrate_sleep():
        if not hasattr(torch.cuda, "_sleep"):
            return None
        cycles = 1_000_000
        torch.cuda._sleep(1000)
        for _ in range(8):
            ms = _ms(lambda: torch.cuda._sleep(cycles))
            if ms >= 5.0:
                break
            cycles *= 4
        else:
            return None
        per_ms = cycles / ms
        check = _ms(lambda: torch.cuda._sleep(int(per_ms * 20)))
        return per_ms if 15.0 <= check <= 30.0 else None

    def set_target(self, ms):
        self.target_ms = ms
        if self.mode == "sleep":
            self.cycles = int(self.cycles_per_ms * ms)
        else:
            self.n_mm = max(1, math.ceil(ms / self.mm_ms))
        self.measured_ms = _ms(self.launch)

    def launch(self):
        if self.mode == "sleep":
            torch.cuda._sleep(self.cycles)
        else:
            for _ in range(self.n_mm):
                torch.mm(self.x, self.x, out=self.y)


class Rig:
    def __init__(self):
        torch.cuda.set_device(DEV)
        self.A, self.B = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
        self.blocker = Blocker()

    def run(self, first, second, timed=None):
        """Steps 1 - 6 of the module docstring for callables taking a stream.
        Returns (conclusive, ordered, lag of eA behind B in ms)."""
        cur = torch.cuda.current_stream(DEV)
        second(cur)
        first(cur)
        pair_ms = _ms(lambda: (second(cur), first(cur)))
        if timed is not None:
            MEASURED[timed] = pair_ms
        if pair_ms >= self.blocker.measured_ms / PAIR_FRACTION:   # launch jitter must not flip the answer
            self.blocker.set_target(2 * PAIR_FRACTION * pair_ms)
        assert pair_ms < self.blocker.measured_ms / PAIR_FRACTION, (pair_ms, self.blocker.measured_ms)
        torch.cuda.synchronize()
        e_blk, e_a = _event(), _event()
        try:
            with torch.cuda.stream(self.A):
                self.blocker.launch()
                e_blk.record()
                first(self.A)
                e_a.record()
            with torch.cuda.stream(self.B):
                second(self.B)
            conclusive = not e_blk.query()
            self.B.synchronize()
            ordered = e_a.query()
            t0 = time.perf_counter()
            limit = self.blocker.measured_ms / 50.0
            while not ordered and (time.perf_counter() - t0) * 1e3 < limit:
                ordered = e_a.query()
            lag = (time.perf_counter() - t0) * 1e3
        finally:
            torch.cuda.synchronize()
        return conclusive, ordered, lag


@pytest.fixture(scope="module")
def rig(pkg):
    return Rig()


# ---------------------------------------------------------------- the calls
def _patchnorm14(pkg):
    tabs = golden("patchnorm_ref.npz")
    pn = pkg.PatchNorm(32, 32, 14, 3)
    pn.median.data.copy_(torch.from_numpy(tabs["median"]))
    pn.b.data.copy_(torch.from_numpy(tabs["b"]))
    pn.frozen = True
    return pn.eval().to(DEV)


def _stats_batch(seed=9, shape=(3, 8, 8, 16), rows=3, seq=200):
    g = torch.Generator().manual_seed(seed)
    c, mh, mw, z = shape
    ch = torch.randint(0, c, (rows, seq), generator=g)
    pos = torch.stack([torch.randint(0, mh, (rows, seq), generator=g), torch.randint(0, mw, (rows, seq), generator=g)], -1)
    x = torch.round(torch.randn(rows, seq, z, generator=g) * 3)
    kp = torch.zeros(rows, seq, dtype=torch.bool)
    kp[:, seq - seq // 5:] = True
    x[kp] = 0
    return x, ch, pos, kp


@pytest.fixture(scope="module")
def calls(pkg):
    """label -> callable(stream) of one C ABI call on this thread's context,
    every buffer allocated here, once"""
    from dct_autoencoder_amd import _lib, packing
    from test_gpu_lfq_train import build as lfq_build, G as LG
    from test_gpu_pixel_loss import case as pixel_case
    from test_gpu_vq import _make as vq_make
    from test_rec_loss_host import case as rec_case
    ops = _ops()
    torch.cuda.set_device(DEV)
    ctx = _lib.context(DEV)
    lib, ptr = ctx.lib, _lib.ptr
    keep, out = [], {}

    def bind(label, name, *args):
        fn = getattr(lib, name)
        keep.append(args)

        def run(stream):
            ctx.check(fn(ctx.h, *args, C.c_void_p(stream.cuda_stream)), name)
        assert label in LABELS and dict((b, a) for a, b in CASES)[label] == name
        out[label] = run
        return run

    def ref(struct):
        keep.append(struct)
        return C.byref(struct)

    here = torch.cuda.current_stream(DEV)
    pn = _patchnorm14(pkg)
    norm = pn.state()
    lcfg = _lib.LFQCfg(14, 14, 1.0)
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
    keep.extend([pn, norm, fe])

    # ---- encode / decode: two ragged images in one padded row (GEMM path), one 512 x 512 image (FFT path)
    def image_batch(tag, sizes, S, seed):
        imgs = [ops.synth_images(1, h, w, seed + i)[0].contiguous() for i, (h, w) in enumerate(sizes)]
        ks = [fe._tokens(h, w) for h, w in sizes]
        plan = packing.layout([list(range(len(sizes)))], dict(enumerate(ks)))
        assert plan.row_len[0] <= S
        desc, _, k_img = ops.image_set(imgs)
        pk_arrays = [_lib.i32(a) for a in (plan.row, plan.col, plan.k, plan.local_id, plan.row_len)]
        pk = _lib.Packing(*[C.cast(a, C.POINTER(C.c_int32)) for a in pk_arrays], 1)
        t = dict(codes=torch.empty((1, S, 14), dtype=torch.long, device=DEV),
                 positions=torch.empty((1, S, 2), dtype=torch.long, device=DEV),
                 channels=torch.empty((1, S), dtype=torch.long, device=DEV),
                 image_ids=torch.empty((1, S), dtype=torch.long, device=DEV),
                 key_pad=torch.empty((1, S), dtype=torch.bool, device=DEV),
                 patches=torch.empty((1, S, 196), dtype=torch.float32, device=DEV))
        po = _lib.PackedOut(ptr(t["codes"]), ptr(t["positions"]), ptr(t["channels"]), ptr(t["image_ids"]),
                            ptr(t["key_pad"]), ptr(t["patches"]), None, None)
        p = fe.params(S)
        keep.extend([imgs, k_img, pk_arrays, t])
        enc = bind(f"encode_{tag}", "dctae_encode", ref(p.c(S)), ref(desc), ref(pk), ref(norm.c()), ref(lcfg), ref(po))
        enc(here)   # the packed batch the decodes start from
        torch.cuda.synchronize()
        tab = ops.decode_table(p, t["image_ids"], t["key_pad"], t["positions"], t["channels"],
                               [packing.patch_grid(h, w, 14) for h, w in sizes], [tuple(s) for s in sizes])
        rgb = torch.empty(tab.total, dtype=torch.float32, device=DEV)
        keep.extend([tab, rgb])
        batch = (ptr(tab.ids), ptr(tab.key_pad), ptr(tab.pos), ptr(tab.ch))
        bind(f"decode_{tag}", "dctae_decode", ref(p.c(S)), tab.R, *tab.c_args(), *batch, ref(norm.c()), ref(lcfg),
             ptr(t["codes"]), None, ptr(rgb))
        bind(f"decode_normed_{tag}", "dctae_decode_normed", ref(p.c(S)), tab.R, *tab.c_args(), *batch, ref(norm.c()),
             ptr(t["patches"]), ptr(rgb))
        return imgs, desc, pk, p

    imgs, desc, pk, p = image_batch("gemm", [(100, 77), (64, 64)], 160, 40)
    imgs5, desc5, pk5, p5 = image_batch("fft512", [(512, 512)], 3072, 50)

    # the fused projection encode needs rows without padding: the 512 x 512 image's full row
    gen = torch.Generator().manual_seed(3)
    pcfg = _lib.LFQCfg(13, 16, 1.0)   # 196 -> 16 x 13, conf/patch14-l.json
    w_in = (torch.randn(208, 196, generator=gen) / 14).to(DEV)
    b_in = (torch.randn(208, generator=gen) * 0.1).to(DEV)
    w_out = (torch.randn(196, 208, generator=gen) / 14).to(DEV)
    b_out = (torch.randn(196, generator=gen) * 0.1).to(DEV)
    tp = dict(codes=torch.empty((1, 3072, 16), dtype=torch.long, device=DEV),
              positions=torch.empty((1, 3072, 2), dtype=torch.long, device=DEV),
              channels=torch.empty((1, 3072), dtype=torch.long, device=DEV),
              image_ids=torch.empty((1, 3072), dtype=torch.long, device=DEV),
              key_pad=torch.empty((1, 3072), dtype=torch.bool, device=DEV))
    pop = _lib.PackedOut(ptr(tp["codes"]), ptr(tp["positions"]), ptr(tp["channels"]), ptr(tp["image_ids"]),
                         ptr(tp["key_pad"]), None, None, None)
    keep.extend([tp, w_in, b_in, w_out, b_out])
    bind("encode_lfq_proj", "dctae_encode_lfq_proj", ref(p5.c(3072)), ref(desc5), ref(pk5), ref(norm.c()), ref(pcfg),
         ptr(w_in), ptr(b_in), ref(pop))

    n_tok = sum(fe._tokens(h, w) for h, w in [(100, 77), (64, 64)])
    tok_off = _lib.i64([0, fe._tokens(100, 77)])
    tokens = torch.empty((n_tok, 196), dtype=torch.float32, device=DEV)
    scores = torch.empty(n_tok, dtype=torch.float32, device=DEV)
    keep.extend([tok_off, tokens, scores])
    bind("spectrum_tokens", "dctae_spectrum_tokens", ref(p.c(160)), ref(desc), C.cast(tok_off, C.POINTER(C.c_int64)),
         ptr(tokens), ptr(scores))

    x1 = imgs[0][None].contiguous()
    y1 = torch.empty_like(x1)
    keep.extend([x1, y1])
    dct2 = bind("dct2", "dctae_dct2", ptr(x1), 1, 100, 77, 0, 1, ptr(y1))
    dct2(here)
    torch.cuda.synchronize()
    spec = y1[0, :, :98, :70].contiguous()
    k = fe._tokens(98, 70)
    ps = (torch.empty((k, 196), dtype=torch.float32, device=DEV), torch.empty((k, 2), dtype=torch.long, device=DEV),
          torch.empty(k, dtype=torch.long, device=DEV))
    keep.extend([spec, ps])
    bind("patch_spectrum", "dctae_patch_spectrum", ref(fe.params().c()), ptr(spec), 98, 70, k, ptr(ps[0]), ptr(ps[1]),
         ptr(ps[2]), None)

    # ---- LFQ projections at dim 196, a few hundred tokens
    n = 300
    xin = torch.randn(n, 196, generator=gen).clamp_(-6, 6).to(DEV)
    idx_in = torch.empty((n, 16), dtype=torch.long, device=DEV)
    idx = torch.randint(0, 2 ** 13, (n, 16), generator=gen).to(DEV)
    xout = torch.empty((n, 196), dtype=torch.float32, device=DEV)
    chn = torch.randint(0, 3, (n,), generator=gen).to(DEV)
    posn = torch.randint(0, 32, (n, 2), generator=gen).to(DEV)
    keep.extend([xin, idx_in, idx, xout, chn, posn])
    bind("lfq_project_in", "dctae_lfq_project_in", ref(pcfg), ptr(xin), n, 196, ptr(w_in), ptr(b_in), ptr(idx_in))
    bind("lfq_project_in_bounded", "dctae_lfq_project_in_bounded", ref(pcfg), ptr(xin), n, 196, ptr(w_in), ptr(b_in),
         C.c_float(6.0), ptr(idx_in))
    bind(PARTNER, "dctae_lfq_project_out", ref(pcfg), ptr(idx), n, 196, ptr(w_out), ptr(b_out), ptr(xout))
    bind("lfq_project_out_inverse_norm", "dctae_lfq_project_out_inverse_norm", ref(pcfg), ptr(idx), n, 196, ptr(w_out),
         ptr(b_out), ref(norm.c()), 32, 32, ptr(chn), ptr(posn), ptr(xout))

    # ---- reconstruction loss: the fixture's "p5"
    rpn, rt, _ = rec_case(pkg, "p5", DEV)
    rnorm, rp = rpn.state(), rpn._params()
    r = {k: rt[k].float().contiguous() for k in ("out", "tn", "raw")}
    r.update({k: rt[k].long().contiguous() for k in ("ch", "pos")})
    r["kp"] = rt["key_pad"].contiguous().view(torch.uint8)
    rn = r["out"].numel() // rp.patch_size ** 2
    r["un"], r["sc"] = torch.empty_like(r["out"]), torch.empty(3, dtype=torch.float32, device=DEV)
    keep.extend([rpn, rnorm, r])
    bind("rec_loss_forward", "dctae_rec_loss_forward", ref(rnorm.c()), rp.patch_size, 32, 32, ptr(r["out"]),
         ptr(r["tn"]), ptr(r["raw"]), ptr(r["ch"]), ptr(r["pos"]), ptr(r["kp"]), rn, ptr(r["un"]), ptr(r["sc"]))

    # ---- LFQ entropy losses: the fixture's "d6"
    m = lfq_build(pkg, "d6").train()
    _, _, _, dist = m(torch.from_numpy(LG["d6_x"]).to(DEV), mask=torch.from_numpy(LG["d6_mask"]).to(DEV))
    ecfg = dist.cfg()
    hs = dist.h.detach().float().contiguous()
    ms = torch.from_numpy(LG["d6_mask"]).to(DEV).contiguous().view(torch.uint8)
    en = ms.numel()
    avg = torch.empty(2 ** ecfg.codebook_dim, dtype=torch.float32, device=DEV)
    esc = torch.empty(5, dtype=torch.float32, device=DEV)
    eg, dh = torch.ones(1, device=DEV), torch.empty_like(hs)
    keep.extend([hs, ms, avg, esc, eg, dh])
    bind("lfq_entropy_forward", "dctae_lfq_entropy_forward", ref(ecfg), ptr(hs), ptr(ms), en, 0.01, 1e-9, ptr(avg),
         ptr(esc))(here)
    bind("lfq_entropy_backward", "dctae_lfq_entropy_backward", ref(ecfg), ptr(hs), ptr(ms), en, 0.01, 1e-9, ptr(avg),
         ptr(esc), ptr(eg), ptr(dh))

    # ---- PatchNorm statistics: 600 tokens on a (3, 8, 8) grid of 4 x 4 patches
    sx, sch, spos, skp = (t.to(DEV).contiguous() for t in _stats_batch())
    sn = sx.shape[0] * sx.shape[1]
    cells = (3, 8, 8)
    bn, bm = torch.empty(cells, device=DEV), torch.empty((*cells, 16), device=DEV)
    med, bb = torch.zeros((*cells, 16), device=DEV), torch.ones((*cells, 16), device=DEV)
    n_dev, sy, mad = torch.zeros(cells, device=DEV), torch.empty_like(sx), torch.empty((*cells, 16), device=DEV)
    snorm = ops.NormState(med, bb)
    keep.extend([sx, sch, spos, skp, bn, bm, n_dev, sy, mad, snorm])
    bind("norm_batch_stats", "dctae_norm_batch_stats", 4, 3, 8, 8, ptr(sx), ptr(sch), ptr(spos), ptr(skp), sn, ptr(bn),
         ptr(bm))
    bind("norm_batch_mad", "dctae_norm_batch_mad", 4, 3, 8, 8, ptr(sx), ptr(sch), ptr(spos), ptr(skp), sn, ptr(bm),
         ptr(mad))
    bind("norm_train_step", "dctae_norm_train_step", ref(snorm.c()), ptr(n_dev), 4, 3, 8, 8, ptr(sx), ptr(sch),
         ptr(spos), ptr(skp), sn, ptr(sy))

    # ---- pixel loss and the decode's backward: the fixture's "p5"
    proc, dp, pt, _ = pixel_case(pkg, "p5")
    pp = proc.params(pt["out"].shape[1])
    d = dp(pt["out"])
    ptab = ops.decode_table(pp, d.batched_image_ids, d.key_pad_mask, d.patch_positions, d.patch_channels,
                            d.patch_sizes, d.original_sizes)
    fh, fx = (ops.decode(pp, ptab.ids, ptab.key_pad, ptab.pos, ptab.ch, None, None, patches=x, table=ptab,
                         return_flat=True)[1] for x in (pt["out"], pt["patches"]))
    lut, lut_w, n_img, hw, off, phw = ptab.c_args()
    psc = torch.empty(1 + n_img, dtype=torch.float32, device=DEV)
    pin, pg, pdp = pt["out"].float().contiguous(), torch.ones(1, device=DEV), torch.empty_like(pt["out"].float())
    keep.extend([ptab, fh, fx, psc, pin, pg, pdp])
    bind("pixel_loss_forward", "dctae_pixel_loss_forward", n_img, hw, off, ptr(fh), ptr(fx), ptr(psc))
    bind("decode_backward", "dctae_decode_backward", ref(pp.c(ptab.S)), ptab.R, lut, lut_w, n_img, hw, off, phw,
         ptr(ptab.ids), ptr(ptab.key_pad), ptr(ptab.pos), ptr(ptab.ch), ptr(pin), None, ptr(fh), ptr(fx), ptr(pg),
         ptr(pdp))

    # ---- VectorQuantize: (16, 1, 333) masked (no projections, so no plan upload); the index route
    # reaches its scratch only with projections: (40, 2, 256), one plan upload, cached after the warm call
    vq = vq_make(pkg, 16, 1, 333, seed=16 + 333)
    vcfg = vq._cfg(DEV)
    vn = 3 * 129
    vx = torch.randn(vn, 16, generator=gen).to(DEV)
    vm = (torch.rand(vn, generator=gen) > 0.3).to(torch.uint8).to(DEV)
    vq_q, vq_i = torch.empty_like(vx), torch.empty((vn, 1), dtype=torch.long, device=DEV)
    vq2 = vq_make(pkg, 40, 2, 256, seed=5)
    vcfg2 = vq2._cfg(DEV)
    vi2 = torch.randint(0, 256, (vn, 2), generator=gen).to(DEV)
    vo2 = torch.empty((vn, 40), dtype=torch.float32, device=DEV)
    keep.extend([vq, vx, vm, vq_q, vq_i, vq2, vi2, vo2])
    bind("vq_forward", "dctae_vq_forward", ref(vcfg), ptr(vx), ptr(vm), vn, ptr(vq_q), ptr(vq_i))
    bind("vq_output_from_indices", "dctae_vq_output_from_indices", ref(vcfg2), ptr(vi2), vn, ptr(vo2))

    torch.cuda.synchronize()
    assert set(out) == set(LABELS)
    out["_keep"] = keep
    return out


# ---------------------------------------------------------------- (a) the harness
def test_every_ordered_row_has_a_case():
    assert sorted({s for s, _ in CASES}) == HARNESS_ROWS


def test_blocker_is_calibrated(rig):
    b = rig.blocker
    what = f"{b.cycles_per_ms:.0f} cycles per ms" if b.mode == "sleep" else f"{b.n_mm} x mm of {b.mm_ms:.3f} ms"
    print(f"blocker: {b.mode}, {what}, asked {b.target_ms:.0f} ms, measured {b.measured_ms:.1f} ms")
    assert 0.5 * b.target_ms <= b.measured_ms <= 3.0 * b.target_ms


def _control(rig):
    """two plain torch kernels on A and B: no ordering between them exists"""
    x, y = torch.zeros(1024, device=DEV), torch.zeros(1024, device=DEV)

    def first(stream):
        with torch.cuda.stream(stream):
            x.add_(1.0)

    def second(stream):
        with torch.cuda.stream(stream):
            y.add_(1.0)
    return rig.run(first, second)


def test_control_pair_is_seen_unordered(rig):
    """the harness can tell: streams A and B are not serialised by the runtime"""
    conclusive, ordered, _ = _control(rig)
    assert conclusive, "the host was held up behind the blocker"
    assert not ordered, "two unrelated kernels on A and B came out ordered: the harness cannot see a missing order"


def test_partner_is_ordered_after_itself(rig, calls):
    conclusive, ordered, lag = rig.run(calls[PARTNER], calls[PARTNER], timed=(PARTNER, PARTNER))
    assert conclusive, "the host was held up behind the blocker: inconclusive"
    assert ordered, "dctae_lfq_project_out on B did not wait for dctae_lfq_project_out on A"


@pytest.mark.parametrize("role", ["first", "second"])
@pytest.mark.parametrize("label", [c for c in LABELS if c != PARTNER])
def test_call_is_ordered_against_the_partner(rig, calls, label, role):
    first, second = (label, PARTNER) if role == "first" else (PARTNER, label)
    conclusive, ordered, lag = rig.run(calls[first], calls[second], timed=(first, second))
    print(f"{first} on A, {second} on B: warmed pair {MEASURED[(first, second)]:.3f} ms, blocker "
          f"{rig.blocker.measured_ms:.1f} ms, conclusive {conclusive}, ordered {ordered}, eA behind B {lag:.3f} ms")
    assert conclusive, f"the host was held up behind the blocker in {second}: inconclusive"
    assert ordered, f"{second} on stream B finished while {first} on stream A had not: the pair is unordered"


def test_control_pair_is_still_seen_unordered(rig, calls):
    """as the first control, after every call (the encode's side stream included) has run"""
    conclusive, ordered, _ = _control(rig)
    assert conclusive and not ordered
    if MEASURED:
        worst = max(MEASURED, key=MEASURED.get)
        print(f"slowest warmed pair: {worst} {MEASURED[worst]:.3f} ms of {len(MEASURED)} pairs; blocker "
              f"{rig.blocker.measured_ms:.1f} ms ({rig.blocker.mode})")


def test_error_flag_crosses_streams(pkg, rig):
    """dctae_check_device_errors on B reports (and clears) the flag that an
    ordered call raises on A, although that call is still parked when the check
    is made: the check waits for it."""
    from dct_autoencoder_amd import _lib
    from test_rec_loss_host import case as rec_case
    ops = _ops()
    pn, t, _ = rec_case(pkg, "p5", DEV)
    ctx = _lib.context(DEV)
    r, s = torch.nonzero(~t["key_pad"])[0].tolist()
    bad = t["pos"].clone()
    bad[r, s, 1] = 32          # one past max_patch_w
    args = dict(norm=pn.state(), p=pn._params())
    for stream in (torch.cuda.current_stream(DEV), rig.A, rig.B):   # each stream's allocator pool warm
        with torch.cuda.stream(stream):
            ops.rec_loss_forward(t["out"], t["tn"], t["raw"], t["ch"], t["pos"], t["key_pad"], **args)
            ops.check_device_errors(DEV)
    torch.cuda.synchronize()
    e_blk = _event()
    try:
        with torch.cuda.stream(rig.A):
            rig.blocker.launch()
            e_blk.record()
            ops.rec_loss_forward(t["out"], t["tn"], t["raw"], t["ch"], bad, t["key_pad"], **args)
        assert not e_blk.query(), "the host was held up behind the blocker: inconclusive"
        with torch.cuda.stream(rig.B):
            with pytest.raises(Exception, match="out of range"):
                ops.check_device_errors(DEV)
            assert e_blk.query(), "the check returned before the parked call had run"
            ops.check_device_errors(DEV)   # read once, cleared
    finally:
        torch.cuda.synchronize()
        left = ctx.lib.dctae_check_device_errors(ctx.h, None)   # no later test inherits the flag
    assert left == 0


# ---------------------------------------------------------------- (b) side-stream plumbing
def _both(fn):
    """fn() on the default stream, then under a side stream; both results, synchronised"""
    torch.cuda.synchronize()
    base = fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        got = fn()
    side.synchronize()
    torch.cuda.synchronize()
    return base, got


def _flat(x):
    if isinstance(x, torch.Tensor):
        return [x]
    if isinstance(x, dict):
        return [t for k in sorted(x) for t in _flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in _flat(v)]
    return []


def _same_bits(a, b):
    a, b = _flat(a), _flat(b)
    assert len(a) == len(b) and len(a) > 0
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and u.dtype == v.dtype, i
        assert torch.equal(u.detach().reshape(-1).view(torch.uint8), v.detach().reshape(-1).view(torch.uint8)), \
            f"tensor {i} of {len(a)} differs between the default and the side stream"


@pytest.fixture(scope="module")
def small(pkg):
    """two ragged images, a frozen PatchNorm, LFQ 14 x 14, rows of 160 tokens"""
    ops = _ops()
    sizes = [(100, 77), (64, 64)]
    imgs = [ops.synth_images(1, h, w, 60 + i)[0].contiguous() for i, (h, w) in enumerate(sizes)]
    pn = _patchnorm14(pkg)
    lfq = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).to(DEV).eval()
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 160)
    torch.cuda.synchronize()
    return fe, pn, lfq, imgs


def _dp_tensors(dp):
    return [dp.patches, dp.key_pad_mask, dp.batched_image_ids, dp.patch_channels, dp.patch_positions]


def test_side_stream_encode_and_decode(pkg, small):
    fe, pn, lfq, imgs = small

    def run():
        ((dp, codes),) = fe.encode_batch(imgs, pn, lfq, return_patches=True, return_raw=True)
        out = fe.decode_batch(dp, codes, pn, lfq)
        raw = dp.shallow_copy()
        raw.patches = dp._data["raw_patches"]
        return _dp_tensors(dp), codes, raw.patches, out, fe.postprocess(raw)
    _same_bits(*_both(run))


def test_side_stream_fft_path(pkg):
    """one 512 x 512 image: the FFT encode with its staging buffer and the FFT decode"""
    ops = _ops()
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 3072)
    pn = _patchnorm14(pkg)
    lfq = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).to(DEV).eval()
    x = ops.synth_images(1, 512, 512, 70)

    def run():
        ((dp, codes),) = fe.encode_batch(x, pn, lfq)
        return _dp_tensors(dp)[1:], codes, fe.decode_batch(dp, codes, pn, lfq)
    _same_bits(*_both(run))


@pytest.mark.parametrize("proj", [False, True])
def test_side_stream_batch_encoder_and_decoder(pkg, proj):
    from dct_autoencoder_amd import feature_extraction as fe_mod
    ops = _ops()
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 96)
    pn = _patchnorm14(pkg)
    torch.manual_seed(0)
    lfq = (pkg.LFQ(dim=196, codebook_size=2 ** 13, num_codebooks=16) if proj else
           pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14)).to(DEV).eval()
    x = ops.synth_images(2, 64, 64, 80)
    enc = fe_mod.BatchEncoder(fe, 2, 64, 64, pn, lfq, device=DEV)
    dec = fe_mod.BatchDecoder(enc, pn, lfq)

    def run():   # the encoder and decoder reuse their output buffers: copies
        packed = enc(x)
        return {k: v.clone() for k, v in packed.items()}, dec(packed).clone()
    _same_bits(*_both(run))


def test_side_stream_patchnorm(pkg, small):
    fe, pn, lfq, imgs = small
    ((dp, _),) = fe.encode_batch(imgs, None, None, return_raw=True)

    def run():
        normed = pn(dp)
        back = dp.shallow_copy()
        back.patches = normed
        return normed, pn.inverse_norm(back)
    _same_bits(*_both(run))

    x, ch, pos, kp = (t.to(DEV) for t in _stats_batch())

    def train():
        m = pkg.PatchNorm(8, 8, 4, 3).to(DEV).train()
        outs = [m(pkg.DCTPatches(x, kp, None, None, ch, pos)), m(pkg.DCTPatches(x.flip(1), kp.flip(1), None, None,
                                                                               ch.flip(1), pos.flip(1)))]
        return outs, m.n.data, m.median.data, m.b.data
    _same_bits(*_both(train))


@pytest.mark.parametrize("name", ["d6", "proj"])
def test_side_stream_lfq(pkg, name):
    from test_gpu_lfq_train import G as LG, build as lfq_build
    x0 = torch.from_numpy(LG[f"{name}_x"]).to(DEV)
    mask = torch.from_numpy(LG[f"{name}_mask"]).to(DEV)
    model = lfq_build(pkg, name)

    def evaluate():
        q, idx, _, _ = model.eval()(x0, mask=mask)
        return q, idx, model.indices_to_codes(idx)

    def train():
        m = model.train()
        x = x0.clone().requires_grad_(True)
        xq, idx, commit, dist = m(x, mask=mask)
        ent = pkg.compute_entropy_loss(dist, mask)
        g, = torch.autograd.grad(ent + commit, x)   # what test_gpu_lfq_train.py asserts run-to-run identical
        return xq, idx, commit, ent, g
    _same_bits(*_both(evaluate))
    _same_bits(*_both(train))


@pytest.mark.parametrize("decode_pixels", [False, True])
def test_side_stream_step_losses(pkg, decode_pixels):
    from test_gpu_pixel_loss import step_setup

    def run():
        proc, dp, t, pn, tn, res = step_setup(pkg)
        d = pkg.step_losses(res, dp(t["patches"]), dp(tn), pn, 2 ** 6, decode_pixels=decode_pixels, proc=proc)
        keys = sorted(k for k in d if "loss" in k or k == "perplexity")
        total = sum(d[k] for k in keys if "loss" in k)
        g, = torch.autograd.grad(total, res["dct_patches"].patches)
        return [d[k] for k in keys], d["rec_patches_unnormalized"].patches, d.get("x_hat", []), d.get("x", []), g
    _same_bits(*_both(run))


def test_side_stream_vector_quantize(pkg):
    from test_gpu_vq import _make
    gen = torch.Generator().manual_seed(7)
    xs = [(torch.randn(3, 129, 16, generator=gen) * (1.0 + s)).to(DEV) for s in range(2)]
    masks = [(torch.rand(3, 129, generator=gen) > 0.3).to(DEV) for _ in range(2)]

    def run():
        vq = _make(pkg, 16, 1, 333, seed=16 + 333)
        outs = [vq(x, mask=m)[:2] for x, m in zip(xs, masks)]   # the second batch sees the first's statistics
        return outs, vq._codebook.batch_mean, vq._codebook.batch_variance, vq.get_codes_from_indices(outs[0][1])
    (o0, bm0, bv0, c0), (o1, bm1, bv1, c1) = _both(run)
    for a, b in ((bm0, bm1), (bv0, bv1)):   # fp64 atomics: test_gpu_vq.py's allowance
        assert torch.allclose(a, b, atol=1e-6, rtol=1e-5)
    n_bad = 0
    for (q0, i0), (q1, i1) in zip(o0, o1):
        same = i0 == i1
        n_bad += int((~same).sum())
        assert torch.allclose(q0[same], q1[same], atol=2e-5, rtol=2e-5)
    assert n_bad <= 2, n_bad   # test_gpu_vq.py: max(2, tokens / 1000) near-ties
    if n_bad == 0:
        assert torch.equal(c0, c1)


def test_side_stream_model_forward_and_train_step(pkg, model_golden):
    from test_gpu_model_train import _dp, _step
    make, t, cbs = model_golden

    def forward():
        m = make().eval()
        out = m(_dp(pkg, t, t["patches_in"].clone()))
        return out["codes"], out["dct_patches"].patches

    def step():
        m = make().train()
        opt = pkg.FusedAdamW(m.parameters(), max_grad_norm=5.0, model=m, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.1)
        out, total = _step(pkg, m, t, cbs)
        total.backward()
        opt.step()
        after = m.eval()(_dp(pkg, t, t["patches_in"].clone()))   # on the packs the step maintains
        return (total, opt.grad_norm, [p.data for p in m.parameters()], after["codes"], after["dct_patches"].patches)
    _same_bits(*_both(forward))
    _same_bits(*_both(step))


# ---------------------------------------------------------------- (c) overlap regression
def test_encode_overlaps_the_losses(pkg):
    """Stream A encodes batch i + 1 while stream B runs the step's losses on
    batch i, 20 times, no host synchronisation inside the loop; tensors change
    streams with wait_stream / record_stream, as torch requires."""
    ops = _ops()
    steps = 20
    sizes = [(100, 77), (64, 64)]
    fe = pkg.DCTAutoencoderFeatureExtractor(3, 14, 0.0, 32, 32, 160)
    pn = _patchnorm14(pkg)
    codes_lfq = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).to(DEV).eval()
    torch.manual_seed(11)
    lfq = pkg.LFQ(dim=196, codebook_size=2 ** 6, num_codebooks=3).to(DEV).train()
    batches = [[ops.synth_images(1, h, w, 100 + 2 * i + j)[0].contiguous() for j, (h, w) in enumerate(sizes)]
               for i in range(steps + 1)]

    def encode(i):
        ((dp, codes),) = fe.encode_batch(batches[i], pn, codes_lfq, return_patches=True, return_raw=True)
        return dp, codes

    def tensors_of(enc):
        dp, codes = enc
        return _dp_tensors(dp) + [codes, dp._data["raw_patches"]]

    def losses(enc):
        dp, _ = enc
        raw = dp.shallow_copy()
        raw.patches = dp._data["raw_patches"]
        x = dp.patches.clone().requires_grad_(True)
        xq, idx, commit, dist = lfq(x, mask=~dp.key_pad_mask)
        out = dp.shallow_copy()
        out.patches = xq
        d = pkg.step_losses(dict(dct_patches=out, codes=idx, commit_loss=commit, distances=dist), raw, dp, pn, 2 ** 6)
        keys = sorted(k for k in d if "loss" in k)
        g, = torch.autograd.grad(sum(d[k] for k in keys), x)
        return [d[k].detach() for k in keys], d["perplexity"], g

    torch.cuda.synchronize()
    serial = []
    for i in range(steps):
        enc = encode(i)
        serial.append((tensors_of(enc), losses(enc)))
    torch.cuda.synchronize()

    A, B = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    overlapped = []
    try:
        with torch.cuda.stream(A):
            nxt = encode(0)
        for i in range(steps):
            cur = nxt
            B.wait_stream(A)
            with torch.cuda.stream(A):
                nxt = encode(i + 1)
            with torch.cuda.stream(B):
                for t in tensors_of(cur):
                    t.record_stream(B)
                overlapped.append((tensors_of(cur), losses(cur)))
    finally:
        torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(serial, overlapped)):
        try:
            _same_bits(a, b)
        except AssertionError as e:
            raise AssertionError(f"step {i}: {e}") from None
