"""TEST INFRASTRUCTURE ONLY — the decode backward / pixel loss cases of
tests/test_gpu_pixel_loss_shapes.py and tests/test_pixel_loss_shapes_host.py,
and the float64 / fp32 oracle they share with tests/test_pixel_loss_host.py
(which pins this recipe to the reference's recorded losses and gradients: bit
for bit in fp32, 1e-12 in float64).

A case is a packed batch built from a list of image sizes by project code
alone: ``rng.synth_images`` -> ``ref_cpu.preprocess`` -> ``ref_cpu._group`` (the
last open row included) -> ``ref_cpu.batch_groups``.  The target is the batch's
``patches``; the model output ``out`` is the target plus seeded Gaussian noise
of 5 % of the mean |patch| of the real tokens; the upstream image of image i
for the vjp is the rank-3 product ``upstream(a, u, v)`` of seeded normals.

What each case is there for (sizes are H x W; P, caps (h, w), S as in CASES;
``g1 .. g4`` are the backward's GEMMs (M, N, K) = (H, Kw, Kh), (H, W, Kw),
(H, Kw, W), (Kh, Kw, H), tiles 128 along the DCT matrix and 64 along the
per-channel operand, k chunks of 32):

  mid       several tiles both ways with ragged M, N and K tails; H = 127
            (Kh = 126), W = 257 (eight chunks + 1), H = 65 / W = 129 (one past a tile)
  p16       Kh = Kw = 128 and 64 (full tiles), K = 64 and 320 (whole chunks)
  caps      Kh = 112 << H, Kw = 168 << W; cached DCT matrices of 168 rows < N columns
  big       520 x 600 at offset 0: the vectorised colour adjoint's second
            grid-stride iteration; M = K = 1000; 521 x 97 misaligns the next image
  mixed512  512 x 512 images on the GEMM decode beside others
  sq512x2   the FFT decode with every token, the GEMM recompute in the backward
  p5        the scalar token gather (P * P % 4 != 0) at medium size
  many72    >= 64 problems per tile list: per-problem XCD dealing, padding tiles
  many300   more than 256 images: the loss's finish kernel, many ids per row
  holes     mid with tokens removed: image 0's (c = 0, 0, 0), image 1's three DC
            tokens, a seeded 30 % of the rest
  zero      the second image's output all zero (l = 0, derivative defined as 0)
"""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu, rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (patch size, (max_patch_h, max_patch_w), max_seq_len, image sizes in packing order)
MID = [(300, 262), (127, 257), (65, 129)]
CASES: Dict[str, Tuple[int, Tuple[int, int], int, List[Tuple[int, int]]]] = {
    "mid": (14, (32, 32), 3072, MID),
    "p16": (16, (32, 32), 3072, [(129, 130), (64, 65), (143, 320)]),
    "caps": (14, (8, 12), 512, [(333, 517), (200, 450)]),
    "big": (14, (32, 32), 3072, [(520, 600), (521, 97), (1000, 97)]),
    "mixed512": (14, (32, 32), 3072, [(512, 512), (100, 77), (512, 512), (224, 224)]),
    "sq512x2": (14, (32, 32), 3072, [(512, 512), (512, 512)]),
    "p5": (5, (20, 20), 1200, [(127, 161), (64, 33)]),
    "many72": (14, (6, 6), 256, rng.ragged_sizes(72, 72, 28, 90)),
    "many300": (14, (2, 3), 64, [(h, w) for (h, _), (_, w) in zip(rng.ragged_sizes(300, 300, 14, 30),
                                                                   rng.ragged_sizes(301, 300, 14, 45))]),
    "holes": (14, (32, 32), 3072, MID),
    "zero": (14, (32, 32), 3072, [(65, 129), (30, 45)]),
}
NAMES = list(CASES)


def upstream(a, u, v):
    """w[c, y, x] = fp32(sum_r a[r, c] u[r, y] v[r, x]), the sum in float64 (as gen_pixel_loss_golden.py)"""
    return torch.einsum("rc,ry,rx->cyx", a.double(), u.double(), v.double()).float()


@functools.lru_cache(maxsize=None)
def _recorded_colours():
    m = np.load(os.path.join(ROOT, "tests", "golden", "colors.npz"))
    return torch.from_numpy(m["ipt2lms"].copy()), torch.from_numpy(m["lms2rgb"].copy())


def ipt_to_rgb(x):
    """ref_cpu.ipt_to_rgb (util.py:85-97) with the colour matrices the fixtures were recorded with
    (colors.npz): ref_cpu.color_matrices() recomputes rgb2lms.inverse() in fp32 on the host it runs
    on, and another CPU gives other last bits (5.8e-5 on ragged14's vjp, measured)"""
    ipt2lms, lms2rgb = _recorded_colours()
    l = ref_cpu._channel_mult(ipt2lms, x)
    return ref_cpu._channel_mult(lms2rgb, ref_cpu._signed_pow(l, 1 / ref_cpu.IPT_GAMMA))


def oracle_images(batch, cfg, patches, per_token_loop=True):
    """FE:289-310 with ref_cpu's dtype-keeping stages"""
    b = ref_cpu.Batch(patches=patches, key_pad_mask=batch.key_pad_mask, attn_mask=None,
                      batched_image_ids=batch.batched_image_ids, patch_channels=batch.patch_channels,
                      patch_positions=batch.patch_positions, patch_sizes=batch.patch_sizes,
                      original_sizes=batch.original_sizes)
    out = []
    for img, (h, w) in zip(ref_cpu.revert_patching(b, cfg, per_token_loop=per_token_loop), batch.original_sizes):
        full = torch.zeros(cfg.channels, h, w, dtype=img.dtype)
        full[:, : img.shape[1], : img.shape[2]] = img
        out.append(ipt_to_rgb(ref_cpu.idct2(full)))
    return out


def oracle_results(batch, cfg, out, ws, dtype, per_token_loop=True):
    """The reference's pixel term (main.py:95-110) and the vjp of FE.postprocess under
    autograd in ``dtype``: ``loss``, ``grad`` (of the loss with respect to ``out``),
    ``vjp`` (of sum_i <w_i, x_hat_i>), ``mse`` and ``xmax`` (max |x_i|) per image as
    numpy arrays, and the images ``x`` (of the target) and ``x_hat`` (of ``out``).
    per_token_loop is needed only where a batch has duplicate places."""
    out = out.to(dtype).requires_grad_(True)
    with torch.no_grad():
        x = oracle_images(batch, cfg, batch.patches.to(dtype), per_token_loop)
    x_hat = oracle_images(batch, cfg, out, per_token_loop)
    mses = [F.mse_loss(a, b) for a, b in zip(x, x_hat)]
    loss = sum(mses) / len(x_hat)
    grad, = torch.autograd.grad(loss, out, retain_graph=True)
    vjp, = torch.autograd.grad(sum((w.to(dtype) * xh).sum() for w, xh in zip(ws, x_hat)), out)
    return {"loss": loss.detach().numpy(), "grad": grad.numpy(), "vjp": vjp.numpy(),
            "mse": torch.stack(mses).detach().numpy(), "xmax": torch.stack([a.abs().max() for a in x]).numpy(),
            "x": x, "x_hat": [a.detach() for a in x_hat]}


def token_image(ids, key_pad):
    """image index of every packed slot (-1 at padding): rows in order, ids ascending (FE:619-633)"""
    ids, kp = torch.as_tensor(ids).long(), torch.as_tensor(key_pad)
    img = torch.full(ids.shape, -1, dtype=torch.long)
    n = 0
    for r in range(ids.shape[0]):
        for i in torch.unique(ids[r]).tolist():
            img[r][(ids[r] == i) & ~kp[r]] = n
            n += 1
    return img


def pack(images, cfg, rows=None):
    """The packed batch of ``images`` ((3, H, W) fp32 tensors): preprocess, greedy
    first-fit rows (FE:454-513) closed by the last open one, collation.  rows: image
    indices per row instead of the greedy grouping."""
    items = [ref_cpu.preprocess(im, cfg) for im in images]
    trip = [(it["patches"], it["positions"], it["channels"]) for it in items]
    if rows is None:
        st = ref_cpu._group(trip, cfg, ref_cpu._Groups())
        groups = st.rows + ([st.cur] if st.cur else [])
    else:
        groups = [[trip[i] for i in row] for row in rows]
    return ref_cpu.batch_groups(groups, cfg, build_attn_mask=False,
                                original_sizes=[it["original_sizes"] for it in items],
                                patch_sizes=[it["patch_sizes"] for it in items])


@dataclass
class Case:
    name: str
    cfg: ref_cpu.FEConfig
    batch: ref_cpu.Batch                    # patches = the target
    out: torch.Tensor                       # the perturbed output (R, S, PP) fp32
    factors: List[Tuple[torch.Tensor, ...]]  # (a, u, v) of every image's upstream
    img: torch.Tensor                       # token_image of the batch
    zero_images: Tuple[int, ...] = ()

    @property
    def ws(self):
        return [upstream(*f) for f in self.factors]

    @property
    def sizes(self):
        return [tuple(int(v) for v in s) for s in self.batch.original_sizes]


def config(name):
    P, (mh, mw), S, _ = CASES[name]
    return ref_cpu.FEConfig(patch_size=P, max_patch_h=mh, max_patch_w=mw, max_seq_len=S)


def perturb(batch, g):
    """(out, factors): the target plus noise of 5 % of the mean |patch| of the real tokens, the upstream factors"""
    p = batch.patches
    sigma = 0.05 * p[~batch.key_pad_mask].abs().mean()
    out = p + sigma * torch.randn(p.shape, generator=g)
    factors = [(torch.randn(3, 3, generator=g), torch.randn(3, h, generator=g), torch.randn(3, w, generator=g))
               for h, w in batch.original_sizes]
    return out, factors


def _punch_holes(batch, img, g):
    """holes: pad image 0's (c = 0, 0, 0) token, image 1's three DC tokens and a seeded 30 % of the rest"""
    pos, ch = batch.patch_positions, batch.patch_channels
    dc = (pos[..., 0] == 0) & (pos[..., 1] == 0)
    gone = ((img == 0) & dc & (ch == 0)) | ((img == 1) & dc)
    assert int(gone.sum()) == 4
    gone = gone | ((img >= 0) & ~gone & (torch.rand(img.shape, generator=g) < 0.3))
    batch.key_pad_mask = batch.key_pad_mask | gone
    return torch.where(gone, torch.full_like(img, -1), img)


@functools.lru_cache(maxsize=None)
def build(name) -> Case:
    """the case ``name`` of CASES; cached, read-only"""
    cfg = config(name)
    sizes = CASES[name][3]
    seed = 7000 + NAMES.index(name if name != "holes" else "mid")
    batch = pack([torch.from_numpy(x) for x in rng.synth_images(seed, sizes)], cfg)
    g = torch.Generator().manual_seed(seed)
    img = token_image(batch.batched_image_ids, batch.key_pad_mask)
    if name == "holes":
        img = _punch_holes(batch, img, g)
    out, factors = perturb(batch, g)
    zero = ()
    if name == "zero":
        out[img == 1] = 0.0
        zero = (1,)
    n = len(sizes)
    assert int(img.max()) + 1 == n and all(bool((img == i).any()) for i in range(n)), "every image keeps a token"
    return Case(name, cfg, batch, out, factors, img, zero)


@functools.lru_cache(maxsize=None)
def results(name, dtype):
    """oracle_results of build(name); cached, read-only"""
    c = build(name)
    return oracle_results(c.batch, c.cfg, c.out, c.ws, dtype, per_token_loop=False)


# ---- the grid cap of the token gather (k_gather_tokens) -----------------------------
# A batch of R rows whose first and last rows hold a case's images and whose other
# rows are fully padded.  A fully padded row still names image id 0 (FE:619-633), so
# each gets a 14 x 14 placeholder image (3 * 14 * 14 floats: the later images keep
# their 16-byte alignment in the flat image buffer).
GRID_CAP = {"mid": 30, "p5": 150}      # case -> rows
PLACEHOLDER = (14, 14)


@functools.lru_cache(maxsize=None)
def grid_cap_case(name):
    """(two-row batch, R-row batch, out2, outR, factors): the case's first image in the first row,
    the others in the last"""
    cfg = config(name)
    sizes = CASES[name][3]
    seed = 7000 + NAMES.index(name)
    n = len(sizes)
    small = pack([torch.from_numpy(x) for x in rng.synth_images(seed, sizes)], cfg, rows=[[0], list(range(1, n))])
    g = torch.Generator().manual_seed(seed)
    out2, factors = perturb(small, g)
    R, S = GRID_CAP[name], cfg.max_seq_len
    P = cfg.patch_size
    assert PLACEHOLDER[0] >= P and PLACEHOLDER[1] >= P

    def spread(x, fill):
        y = torch.full((R, *x.shape[1:]), fill, dtype=x.dtype)
        y[0], y[R - 1] = x[0], x[1]
        return y
    ph = (PLACEHOLDER[0] // P, PLACEHOLDER[1] // P)
    big = ref_cpu.Batch(patches=spread(small.patches, 0), key_pad_mask=spread(small.key_pad_mask, True),
                        attn_mask=None, batched_image_ids=spread(small.batched_image_ids, 0),
                        patch_channels=spread(small.patch_channels, 0),
                        patch_positions=spread(small.patch_positions, 0),
                        patch_sizes=[small.patch_sizes[0]] + [ph] * (R - 2) + list(small.patch_sizes[1:]),
                        original_sizes=[small.original_sizes[0]] + [PLACEHOLDER] * (R - 2)
                        + list(small.original_sizes[1:]))
    # the padded rows' output is not zero: whatever is there must not reach the gradient
    outR = spread(out2, 1.0)
    assert S == small.patches.shape[1]
    return small, big, out2, outR, factors
