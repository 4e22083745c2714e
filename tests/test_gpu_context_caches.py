"""The context's caches hit, miss and are replaced without changing a result.

A context keeps the last encode plan and its key, the bytes of the last plan
upload (``plan_last`` / ``plan_last_id``: an equal upload is skipped), the DCT
matrices by (length, kept rows), the FFT and Bluestein plans with their tables
in one buffer that grows, and the workspace pointer the cached plan was built
on (``EncPlan::ws``).  On one live context a sequence of calls makes each of
them hit, miss and be replaced; after every call all outputs are compared,
bit for bit, with the same call made on a context of its own, which has no
cache to be wrong about.

Every step is ONE library call, because the context caches one encode plan:
two steps hit the plan only when they are adjacent and share
``EncCall::plan_key`` -- full, the image count, P, the caps, max_seq_len, the
number of codebooks, want_raw, want_norm, the pixel type, the plan-shaping
options, and per image its offset from the lowest image address, its size and
its packed place.  The steps below therefore reuse the same image tensors,
and ``A`` (every sink) and ``B`` (codes only) never alternate inside a group.
The library has no counter of plan hits to assert on; that two adjacent steps
share a key is by this reading of ``plan_key``."""
import pytest
import torch

import stale_state as ss

pytestmark = pytest.mark.gpu
DEV = ss.DEV
I16 = torch.int16
SMALL = [(37, 53), (224, 224), (64, 96)]
ALL = dict(patches=True, raw=True, scores=True)


@pytest.fixture(scope="module")
def env(pkg, ref_tables):
    FE = pkg.DCTAutoencoderFeatureExtractor

    class E:
        lib, ops, fe_mod, packing = ss.mods()
        fe = FE(3, 14, 0.0, 32, 32, 3072)
        fe_s1000 = FE(3, 14, 0.0, 32, 32, 1000)
        fe_weights = FE(3, 14, 0.0, 32, 32, 3072, channel_importances=(1.0, 8.0, 2.0), patch_sample_magnitude_weight=0.7)
        fe_cap = FE(3, 14, 0.0, 10, 32, 3072)   # a 500 x 500 image: both sides length 500, 140 against 448 kept rows
        pn = ss.patchnorm(pkg, ref_tables.median, ref_tables.b)
        pn_other = ss.patchnorm(pkg, *ss.tables(21, 32, 32, 14))
        pn_cap = ss.patchnorm(pkg, *ss.tables(22, 10, 32, 14))
        lfq = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14).to(DEV).eval()
        lfq_neg = pkg.LFQ(dim=196, codebook_size=2 ** 14, num_codebooks=14, codebook_scale=-1.0).to(DEV).eval()
        small = ss.images(81, SMALL)
        small_u8 = ss.byte_images(81, SMALL)
        small_u8_f32 = [u.float() / 255.0 for u in small_u8]
        big = list(ops.synth_images(8, 700, 900, seed=82))
        sq500 = ss.images(83, [(500, 500)])
        sq512 = ss.images(84, [(512, 512)])
        # inputs of the calls that go between two encodes, made here, on the shared context
        dec_in = ss.encode(fe, small, pn, lfq)
        spectrum = ops.dct2(ss.images(85, [(56, 70)])[0], inverse=False, color=True)
        wide = torch.stack(list(ops.synth_images(6, 900, 1100, seed=86)))   # dctae_dct2 of it outgrows the workspace
    return E


def _one(fe, x, pn, lfq, sinks=False, **kw):
    """one encode call: codes only (the thresholds), or with every sink"""
    return ss.tensors(ss.encode(fe, x, pn, lfq, **(ALL if sinks else {}), **kw))


def _steps(e):
    steps = []

    def add(name, fn):
        steps.append((name, fn))

    def small(sinks, fe=None, pn=None, lfq=None, x=None, **kw):
        return lambda: _one(fe or e.fe, x or e.small, pn or e.pn, lfq or e.lfq, sinks, **kw)

    def decode():
        r = e.dec_in
        return e.ops.decode(*ss.decode_args(e.fe, r), codes=r["codes"], norm=e.pn.state(), lfq=e.lfq.cfg())

    # calls that use the plan buffer (and the workspace) without being an encode: the cached plan stays
    between = [("decode", decode),
               ("dct2", lambda: e.ops.dct2(torch.stack(e.small[2:]), inverse=False, color=True)),
               ("patch_spectrum", lambda: list(e.ops.patch_spectrum(e.spectrum, e.fe.params(), 60)))]
    for sinks, tag in ((False, "B"), (True, "A")):
        add(f"{tag}", small(sinks))
        add(f"{tag} again: plan hit, upload skipped", small(sinks))
        add(f"{tag} a third time", small(sinks))
        # the same images in another packing and with another max_seq_len: misses that replace the plan
        add(f"{tag} another packing", small(sinks, ks=[5, 700, 60]))
        add(f"{tag} after another packing", small(sinks))
        add(f"{tag} another max_seq_len", small(sinks, fe=e.fe_s1000))
        add(f"{tag} after another max_seq_len", small(sinks))
        # arguments outside plan_key on the plan the step before left: each must reach the kernels anyway
        add(f"{tag} another PatchNorm table pointer", small(sinks, pn=e.pn_other))
        add(f"{tag} the first tables again", small(sinks))
        add(f"{tag} codebook_scale of the opposite sign", small(sinks, lfq=e.lfq_neg))
        add(f"{tag} positive scale again", small(sinks))
        add(f"{tag} other channel_importances / magnitude_weight", small(sinks, fe=e.fe_weights))
        add(f"{tag} the usual weights again", small(sinks))
        add(f"{tag} int16 codes", small(sinks, codes_dtype=I16))
        add(f"{tag} int64 codes again", small(sinks))
        # fp32 then uint8 input of the same bytes (the pixel type is in the key: a miss), then fp32 again
        add(f"{tag} fp32 input", small(sinks, x=e.small_u8_f32))
        add(f"{tag} uint8 input", small(sinks, x=e.small_u8, uint8=True))
        add(f"{tag} fp32 input again", small(sinks, x=e.small_u8_f32))
        # a plan hit while the plan buffer holds another call's bytes (plan_last / plan_last_id)
        for name, fn in between:
            add(f"{tag} before {name}", small(sinks))
            add(name, fn)
            add(f"{tag} after {name}: plan hit, the plan buffer holds {name}'s bytes", small(sinks))
        # token mode is an encode plan of its own: it replaces the cached one
        add("token mode (preprocess)", lambda: [[it["patches"], it["positions"]] for it in e.fe.preprocess_many(e.small)])
        add(f"{tag} after preprocess", small(sinks))
        add("token mode (dctae_spectrum_tokens)", lambda: list(ss.spectrum_tokens(e.fe, e.small)))
        add(f"{tag} after dctae_spectrum_tokens", small(sinks))
        add(f"{tag} once more", small(sinks))
    # EncPlan::ws: a key hit on a workspace that has moved.  dctae_dct2 of a large batch grows the
    # workspace and leaves the encode plan alone; the encode after it has the cached key and must rebuild
    add("B before the workspace moves", small(False))
    add("dct2 of a batch that outgrows the workspace", lambda: e.ops.dct2(e.wide, inverse=False, color=False))
    add("B after the workspace moved under the cached plan", small(False))
    add("B again", small(False))
    # the same through a much larger encode (a key miss as well)
    add("A before a much larger encode", small(True))
    add("a much larger encode", lambda: _one(e.fe, e.big, e.pn, e.lfq, True))
    add("A after the much larger encode", small(True))
    add("A again", small(True))
    # two sides of one DCT matrix length with different kept rows, then the usual corner
    for sinks in (False, True):
        add("500 x 500 keeping 140 x 448", lambda s=sinks: _one(e.fe_cap, e.sq500, e.pn_cap, e.lfq, s))
        add("500 x 500 keeping 448 x 448", lambda s=sinks: _one(e.fe, e.sq500, e.pn, e.lfq, s))
        add("500 x 500 keeping 140 x 448 again", lambda s=sinks: _one(e.fe_cap, e.sq500, e.pn_cap, e.lfq, s))
        add("512 x 512", lambda s=sinks: _one(e.fe, e.sq512, e.pn, e.lfq, s))
        add("small at the end", small(sinks))
    return steps


def _compare(e, steps, opts=()):
    """each step on the live context (the one in place), then on a context of its own"""
    for name, fn in steps:
        got = ss.flat(fn())
        torch.cuda.synchronize()
        with ss._context(e.lib) as own:
            for k, v in opts:
                ss._set(own, k, v)
            want = ss.flat(fn())
            torch.cuda.synchronize()
        ss.assert_same_bits(got, want, f"step '{name}': the live context against a context of its own")


def test_cached_state_never_changes_a_result(env):
    with ss._context(env.lib):
        _compare(env, _steps(env))


# ---- the FFT table buffer that grows -----------------------------------------------------------------------------
TAB_CAP = 1 << 20   # entries (float2) of the buffer at dctae_ctx_create


def _smooth(m):
    for r in (2, 3, 5, 7):
        while m % r == 0:
            m //= r
    return m == 1


def _bs_entries(n):
    """(table entries of the Bluestein plan of length n, its FFT length L): chirp n, b-hat L, post n (bs_plan_for)"""
    L = 256
    while L < 2 * n - 1:
        L <<= 1
    return 2 * n + L, L


def _widths():
    """The fewest lengths whose Bluestein tables cross twice the initial capacity: the largest
    tables first.  Only lengths that take nothing else from the buffer: odd ones (no Makhoul plan
    without fft_odd) and even ones whose half is not 7-smooth (the radix search fails before any
    table is made)."""
    cand = [n for n in range(1024, 31, -1) if n % 2 or not _smooth(n // 2)]
    cand.sort(key=lambda n: (-_bs_entries(n)[0], -n))
    chosen, total, seen_L = [], 0, set()
    for n in cand:
        ent, L = _bs_entries(n)
        total += ent + (0 if L in seen_L else L)
        seen_L.add(L)
        chosen.append(n)
        if total > 2 * TAB_CAP:
            return chosen, total
    raise AssertionError("not enough lengths")


def test_fft_table_growth_keeps_every_plan(env):
    widths, total = _widths()
    assert total > 2 * TAB_CAP   # and the largest tables were taken first: no fewer lengths do
    third = (len(widths) + 2) // 3
    parts = [widths[i: i + third] for i in range(0, len(widths), third)]
    # the first part alone stays below the initial capacity (with room for the four FFT lengths' own
    # tables and the small Makhoul plan of the 14-long side), the first two cross it, all three cross twice it
    sums = [sum(_bs_entries(n)[0] for n in sum(parts[:i + 1], [])) for i in range(3)]
    print(f"{len(widths)} lengths {widths[0]} .. {widths[-1]}, table entries after each part {sums}, in all {total}")
    assert sums[0] + 4096 < TAB_CAP < sums[1]
    g = torch.Generator().manual_seed(85)

    def strip_images(ws):
        flat = torch.rand(sum(3 * 14 * w for w in ws), generator=g).to(DEV)
        out, o = [], 0
        for w in ws:
            out.append(flat[o: o + 3 * 14 * w].view(3, 14, w))
            o += 3 * 14 * w
        return out

    batches = [strip_images(p) for p in parts]
    first = batches[0][:1]
    steps = [(f"part {i} of the widths", (lambda b: lambda: _one(env.fe, b, env.pn, env.lfq, True))(b))
             for i, b in enumerate(batches)]
    steps += [("the first strip again", lambda: _one(env.fe, first, env.pn, env.lfq, True)),
              ("the first strip again, codes only", lambda: _one(env.fe, first, env.pn, env.lfq)),
              ("512 x 512 after the growth", lambda: _one(env.fe, env.sq512, env.pn, env.lfq, True)),
              ("part 0 again", steps[0][1]), ("part 2 again, codes only",
                                              lambda: _one(env.fe, batches[2], env.pn, env.lfq))]
    with ss._context(env.lib) as live:
        ss.timed(live)
        ss._set(live, "bluestein", 1)
        _compare(env, steps[:1], opts=[("bluestein", 1)])
        assert "bs_rows" in ss._stages(live), "the strips did not take the Bluestein row kernel"
        _compare(env, steps[1:], opts=[("bluestein", 1)])
