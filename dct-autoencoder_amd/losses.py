"""The reference's training losses around the quantizer (util.py:346-410):
``masked_mean``, ``compute_entropy_loss`` and ``calculate_perplexity``.

``compute_entropy_loss`` takes either the dense affinity tensor the reference
passes (b, n, c, 2**codebook_dim) -- evaluated with torch ops -- or the
``LFQDistance`` that this package's ``LFQ.forward`` returns in training mode.
On a GPU the latter runs the fused HIP path (dctae_lfq_entropy_forward /
_backward): the codebook is {-s, +s}^d, so the softmax over the codes
factorises over the bits, and loss and gradient come from the projected
features alone; the dense tensor (2**codebook_dim floats per token and
codebook, plus the softmax / log_softmax / autograd copies of it) is never
formed.

Differences from the reference, both deliberate:
  * the fused path never reads the values of masked-out tokens.  The
    reference multiplies them by the mask, so a NaN in padding poisons its
    loss; here it does not.  A NaN in a masked-in token gives a NaN loss and
    ``mask.sum() == 0`` gives NaN, as in the reference.
  * non-fp32 features are upcast to fp32 before the kernel; the reference
    first rounds the dense distance to the model dtype.

The other two terms of the reference's training step (main.py:44-93) are
here as well: ``reconstruction_losses`` (the masked L1 pair on the normalized
and the inverse-normalized output, fused HIP forward and backward on a GPU),
``masked_perplexity`` and ``step_losses``, the dict of main.py:85-93; with
``decode_pixels`` also ``pixel_loss`` (main.py:95-110), the mean per-image MSE
of the decoded images, over a differentiable decode (dctae_decode_backward).
"""
from __future__ import annotations

import torch

from . import _ops
from ._lib import LFQCfg


class LFQDistance:
    """Stand-in for ``distance = -2 * einsum('... i d, j d -> ... i j', h,
    codebook)`` (lfq.py:191), the fourth return value of ``LFQ.forward`` in
    training mode: the projected features ``h`` (b, n, c, d) with their
    autograd history, the codebook scale ``s`` and the codebook shape.
    ``shape`` / ``dtype`` are those of the dense tensor; ``materialize()``
    builds it with torch (small cases and tests)."""

    def __init__(self, h: torch.Tensor, codebook_scale: float, codebook_dim: int, num_codebooks: int):
        assert h.ndim == 4 and h.shape[2] == num_codebooks and h.shape[3] == codebook_dim
        self.h = h
        self.s = float(codebook_scale)
        self.codebook_dim = codebook_dim
        self.num_codebooks = num_codebooks

    @property
    def codebook_size(self):
        return 2 ** self.codebook_dim

    @property
    def shape(self):
        return torch.Size((*self.h.shape[:3], self.codebook_size))

    @property
    def dtype(self):
        return self.h.dtype

    @property
    def device(self):
        return self.h.device

    def codebook(self) -> torch.Tensor:
        """(2**d, d) table of +-s, dimension 0 the most significant bit"""
        d = self.codebook_dim
        bits = 2 ** torch.arange(d - 1, -1, -1, device=self.h.device)
        on = ((torch.arange(2 ** d, device=self.h.device)[:, None].int() & bits) != 0).to(self.h.dtype)
        return on * self.s * 2 - self.s

    def materialize(self) -> torch.Tensor:
        return -2 * torch.einsum("...id,jd->...ij", self.h, self.codebook())

    def cfg(self) -> LFQCfg:
        # the scale as the reference's ones_like(x) * codebook_scale holds it (lfq.py:174)
        s = self.s
        if self.h.dtype in (torch.float16, torch.bfloat16, torch.float32):
            s = float(torch.tensor(s, dtype=self.h.dtype))
        return LFQCfg(self.codebook_dim, self.num_codebooks, s)


class _FusedEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, mask, cfg, temperature, eps):
        avg, sc = _ops.lfq_entropy_forward(h, mask, cfg, temperature, eps)
        ctx.save_for_backward(h, mask, avg, sc)
        ctx.args = (cfg, temperature, eps)
        return sc[0].clone()

    @staticmethod
    def backward(ctx, grad):
        h, mask, avg, sc = ctx.saved_tensors
        cfg, temperature, eps = ctx.args
        dh = _ops.lfq_entropy_backward(h, mask, cfg, avg, sc, grad, temperature, eps)
        return dh.view(h.shape).to(h.dtype), None, None, None, None


class _FusedCommit(torch.autograd.Function):
    """commit_loss = sum_masked (h - q)^2 / (M c d), q = where(h > 0, s, -s)
    (lfq.py:195-200), from the fused forward; its gradient is element-wise."""

    @staticmethod
    def forward(ctx, h, mask, cfg):
        _, sc = _ops.lfq_entropy_forward(h, mask, cfg)
        ctx.save_for_backward(h, mask, sc)
        ctx.cfg = cfg
        return sc[3].clone()

    @staticmethod
    def backward(ctx, grad):
        h, mask, sc = ctx.saved_tensors
        s = ctx.cfg.codebook_scale
        hf = h.float()
        q = torch.where(hf > 0, s, -s)
        k = grad.float() * 2.0 / (sc[4] * float(ctx.cfg.num_codebooks * ctx.cfg.codebook_dim))
        m = mask.to(torch.bool).reshape(*mask.shape, *([1] * (h.ndim - mask.ndim)))
        dh = torch.where(m, (hf - q) * k, torch.zeros((), device=h.device))
        return dh.to(h.dtype), None, None


def fused_losses(dist: LFQDistance, mask: torch.Tensor, temperature=0.01, eps=1e-9):
    """avg_probs (2**d) and [entropy, sample_entropy, avg_entropy, commit_loss,
    M] of the fused forward, without autograd (inspection and tests)."""
    return _ops.lfq_entropy_forward(dist.h, mask, dist.cfg(), temperature, eps)


def commit_loss(dist: LFQDistance, mask: torch.Tensor) -> torch.Tensor:
    return _FusedCommit.apply(dist.h, mask, dist.cfg()).to(dist.h.dtype)


def masked_mean(x, m, dim=None):
    """util.py:346-353: the sum of x at m (m over the leading dims of x)
    divided by m.sum(); over everything, or over ``dim``."""
    mm = m.reshape(*m.shape, *([1] * (x.ndim - m.ndim)))
    x = (x * mm) / m.sum()
    return x.sum() if dim is None else x.sum(dim=dim)


def compute_entropy_loss(affinity, mask, temperature=0.01, eps=1e-9):
    """util.py:355-387: sample entropy minus the entropy of the mean code
    distribution, of softmax(affinity / temperature + eps) over the last dim.
    affinity: an ``LFQDistance`` (fused HIP path on a GPU) or a dense tensor
    (b, s, c, z); mask (b, s): False at padding.  The result has the
    affinity's dtype.  See the module docstring for the deviations of the
    fused path (padding values are never read; fp32 upcast of h)."""
    if isinstance(affinity, LFQDistance):
        if affinity.h.is_cuda:
            if affinity.codebook_dim > 16 or affinity.num_codebooks > 32:
                raise NotImplementedError("the fused LFQ entropy loss serves codebook_dim <= 16 and "
                                          "num_codebooks <= 32")
            loss = _FusedEntropy.apply(affinity.h, mask, affinity.cfg(), float(temperature), float(eps))
            return loss.to(affinity.dtype)
        affinity = affinity.materialize()
    og_dtype = affinity.dtype
    a = affinity.to(torch.float32)
    a = a.reshape(-1, *a.shape[2:])                  # (b s) c z
    m = mask.reshape(-1)
    logits = a / temperature + eps
    log_probs = torch.log_softmax(logits, dim=-1)
    probs = torch.softmax(logits, dim=-1)
    avg_probs = masked_mean(probs, m, dim=0).mean(dim=0)
    avg_entropy = -(avg_probs * torch.log(avg_probs + eps)).sum()
    sample_entropy = -masked_mean((probs * log_probs).sum(dim=-1), m)
    return (sample_entropy - avg_entropy).to(og_dtype)


class _FusedRecLoss(torch.autograd.Function):
    """rec_loss, rec_loss_unnormalized and inverse_norm(out) from one pass
    (dctae_rec_loss_forward); the backward recomputes the signs from the
    inputs (dctae_rec_loss_backward), nothing is saved per element."""

    @staticmethod
    def forward(ctx, out, tn, raw, channels, positions, key_pad, state, params, want_unnorm):
        sc, un = _ops.rec_loss_forward(out, tn, raw, channels, positions, key_pad, state, params, want_unnorm)
        ctx.save_for_backward(out, tn, raw, channels, positions, key_pad, sc)
        ctx.args = (state, params)
        ctx.set_materialize_grads(False)
        if un is not None:
            un = un.view(out.shape)
        return sc[0].clone(), sc[1].clone(), un

    @staticmethod
    def backward(ctx, g_rec, g_unn, g_patches):
        out, tn, raw, channels, positions, key_pad, sc = ctx.saved_tensors
        state, params = ctx.args
        zero = torch.zeros((), dtype=torch.float32, device=out.device)
        g = torch.stack([zero if t is None else t.float().reshape(()) for t in (g_rec, g_unn)])
        dout = _ops.rec_loss_backward(out, tn, raw, channels, positions, key_pad, state, params, sc, g, g_patches)
        return dout.view(out.shape).to(out.dtype), None, None, None, None, None, None, None, None


def _inverse_norm_torch(patchnorm, dp, x):
    """patchnorm.py:167-177 with torch ops, on x in place of dp.patches"""
    c, h, w = dp.patch_channels, dp.h_indices, dp.w_indices
    std = patchnorm.b[c, h, w] * 2 ** 0.5 + patchnorm.eps
    return x * std + patchnorm.median[c, h, w]


def reconstruction_losses(output, normalized_target, target, patchnorm, want_unnormalized=True):
    """The reconstruction terms of the reference's step_autoencoder
    (main.py:71, 79-83), arguments ``DCTPatches``, mask = ~output.key_pad_mask:

        rec_loss = F.l1_loss(output.patches[mask], normalized_target.patches[mask])
        rec_patches_unnormalized = patchnorm.inverse_norm(output)
        rec_loss_unnormalized = F.l1_loss(rec_patches_unnormalized[mask], target.patches[mask])

    Returns (rec_loss, rec_loss_unnormalized, rec_patches_unnormalized); the
    last is None unless wanted.  All three carry gradients to
    ``output.patches``.  On a GPU this is one autograd Function over the fused
    HIP kernels (dctae_rec_loss_forward / _backward): no boolean index, so no
    host synchronisation.  On CPU tensors the formula above runs with torch ops.

    Differences from the reference, both deliberate (as for the entropy loss):
      * the fused path never reads the targets of padded tokens, so a NaN there
        does not reach the losses (the reference's index drops them too); a NaN
        in a real token gives NaN and no real token at all gives NaN.
      * fp16 / bf16 tensors are upcast to fp32 before the kernel, the losses and
        rec_patches_unnormalized are fp32 and the gradient is cast back to the
        output's dtype.  The reference gets the same promotion from its fp32
        targets and tables; with half-precision targets it would compute in half."""
    import torch.nn.functional as F
    out = output.patches
    if out.is_cuda:
        return _FusedRecLoss.apply(out, normalized_target.patches, target.patches, output.patch_channels,
                                   output.patch_positions, output.key_pad_mask, patchnorm.state(),
                                   patchnorm._params(), bool(want_unnormalized))
    mask = ~output.key_pad_mask
    rec = F.l1_loss(out[mask], normalized_target.patches[mask])
    un = _inverse_norm_torch(patchnorm, output, out)
    rec_un = F.l1_loss(un[mask], target.patches[mask])
    return rec, rec_un, (un if want_unnormalized else None)


def masked_perplexity(codes, mask, codebook_size):
    """``calculate_perplexity(codes[mask], codebook_size)`` (main.py:73-76)
    without the boolean index: the codes of masked-out tokens become the null
    index.  codes (b, s, ...) integer, mask (b, s): True at real tokens."""
    m = mask.reshape(*mask.shape, *([1] * (codes.ndim - mask.ndim)))
    return calculate_perplexity(torch.where(m, codes, torch.full_like(codes, -1)), codebook_size)


class _Postprocess(torch.autograd.Function):
    """FE.postprocess with a HIP backward (dctae_decode / dctae_decode_backward):
    the images of ``patches`` and, in the backward, the vjp of the upstream
    image gradients.  Nothing is saved but the patches: the backward recomputes
    the pre-colour image with the colour-less GEMM inverse."""

    @staticmethod
    def forward(ctx, patches, table, params):
        imgs, _ = _ops.decode(params, table.ids, table.key_pad, table.pos, table.ch, None, None, patches=patches,
                              table=table, return_flat=True)
        ctx.save_for_backward(patches)
        ctx.args = (table, params)
        ctx.set_materialize_grads(False)
        return tuple(imgs)

    @staticmethod
    def backward(ctx, *grads):
        patches, = ctx.saved_tensors
        table, params = ctx.args
        if all(g is None for g in grads):
            return None, None, None
        flat = torch.zeros(table.total, dtype=torch.float32, device=patches.device)
        for view, g in zip(table.images(flat), grads):
            if g is not None:
                view.copy_(g)
        dp = _ops.decode_backward(params, table, patches, grad_rgb=flat)
        return dp.view(patches.shape).to(patches.dtype), None, None


def _decode_table(proc, dp):
    return _ops.decode_table(proc.params(dp.patches.shape[1]), dp.batched_image_ids, dp.key_pad_mask,
                             dp.patch_positions, dp.patch_channels, dp.patch_sizes, dp.original_sizes)


def differentiable_postprocess(proc, dp):
    """``proc.postprocess(dp)`` (fused path) with a grad_fn: what
    DCTAutoencoderFeatureExtractor.postprocess runs for patches that require grad."""
    return list(_Postprocess.apply(dp.patches, _decode_table(proc, dp), proc.params(dp.patches.shape[1])))


class _PixelLoss(torch.autograd.Function):
    """The two decodes, dctae_pixel_loss_forward and, in the backward,
    dctae_decode_backward in its fused form (the gradient image
    g 2 (x_hat - x) / (3 H W n_img) exists only inside the colour kernel).
    One image table (its ids.cpu() walk is the only host synchronisation)
    serves all three calls."""

    @staticmethod
    def forward(ctx, patches, target_patches, table, params):
        def dec(x):
            return _ops.decode(params, table.ids, table.key_pad, table.pos, table.ch, None, None, patches=x,
                               table=table, return_flat=True)
        x_hat, flat_hat = dec(patches)
        x, flat = dec(target_patches)
        sc = _ops.pixel_loss_forward(table, flat_hat, flat)
        ctx.save_for_backward(patches, flat_hat, flat)
        ctx.args = (table, params)
        ctx.mark_non_differentiable(*x_hat, *x)
        return (sc[0].clone(), *x_hat, *x)

    @staticmethod
    def backward(ctx, g, *_):
        patches, flat_hat, flat = ctx.saved_tensors
        table, params = ctx.args
        dp = _ops.decode_backward(params, table, patches, rgb_hat=flat_hat, rgb=flat, g=g)
        return dp.view(patches.shape).to(patches.dtype), None, None, None


def pixel_loss(output_unnormalized, target_unnormalized, proc):
    """The pixel term of the reference's step_autoencoder (main.py:96-106),
    arguments ``DCTPatches`` of un-normalised patches over the same packed batch:

        images_hat = proc.postprocess(output_unnormalized)
        images     = proc.postprocess(target_unnormalized)
        pixel_loss = mean_i F.mse_loss(images[i], images_hat[i])

    Returns (pixel_loss, images_hat, images): a 0-d fp32 device tensor and two
    lists of (3, H, W) fp32 images.  pixel_loss carries the gradient to
    ``output_unnormalized.patches`` (fused HIP forward and backward); the
    target gets none.

    Differences from the reference, all deliberate:
      * the returned images are detached: a further loss on ``images_hat``
        takes ``proc.postprocess`` of patches that require grad instead;
      * fp16 / bf16 patches are upcast to fp32 and the gradient is cast back;
      * padded tokens are never read, their gradient is exactly zero;
      * with an overridden ``_transform_image_out`` / ``revert_patching`` hook
        the staged stages run and the loss is torch ops on their images, which
        carry no grad_fn (as ``postprocess`` itself there)."""
    import torch.nn.functional as F
    out = output_unnormalized.patches
    if proc._staged_out() or not out.is_cuda:
        if not out.is_cuda:
            from ._lib import DCTAEUnavailable
            raise DCTAEUnavailable("pixel_loss: the decode has no CPU path")
        x_hat, x = proc.postprocess(output_unnormalized), proc.postprocess(target_unnormalized)
        loss = sum(F.mse_loss(a, b) for a, b in zip(x, x_hat)) / len(x_hat)
        return loss, x_hat, x
    table = _decode_table(proc, output_unnormalized)
    params = proc.params(out.shape[1])
    res = _PixelLoss.apply(out, target_unnormalized.patches.detach(), table, params)
    n = table.n_img
    return res[0], list(res[1:1 + n]), list(res[1 + n:])


def step_losses(res, batch, normalized_batch, patchnorm, codebook_size, training=True, decode_pixels=False,
                proc=None):
    """The dict the reference's step_autoencoder returns (main.py:85-112) from
    the model's output ``res`` (``dct_patches``, ``codes``, ``commit_loss``,
    ``distances``), the raw ``batch`` and the ``normalized_batch`` it was fed.
    decode_pixels (main.py:95-110, needs the feature extractor ``proc``): adds
    ``x_hat``, ``pixel_loss`` and ``x``, the target decoded from
    ``inverse_norm(normalized_batch)`` as the reference does; pixel_loss reaches
    ``res["dct_patches"].patches`` through rec_patches_unnormalized."""
    if decode_pixels and proc is None:
        raise ValueError("step_losses(decode_pixels=True) needs proc, the feature extractor that decodes the images")
    output = res["dct_patches"]
    mask = ~output.key_pad_mask
    entropy_loss = compute_entropy_loss(res["distances"], mask) if training else 0.0
    rec_loss, rec_loss_unnormalized, un = reconstruction_losses(output, normalized_batch, batch, patchnorm)
    with torch.no_grad():
        perplexity = masked_perplexity(res["codes"], mask, codebook_size)
    unnormalized = output.shallow_copy()
    unnormalized.patches = un
    out = dict(rec_patches=output, rec_patches_unnormalized=unnormalized, rec_loss=rec_loss,
               rec_loss_unnormalized=rec_loss_unnormalized, perplexity=perplexity,
               commit_loss=res["commit_loss"], entropy_loss=entropy_loss)
    if decode_pixels:
        target = normalized_batch.shallow_copy()
        with torch.no_grad():
            target.patches = patchnorm.inverse_norm(normalized_batch)
        out["pixel_loss"], out["x_hat"], out["x"] = pixel_loss(unnormalized, target, proc)
    return out


def calculate_perplexity(codes, codebook_size, null_index=-1):
    """util.py:391-410: 2 ** entropy (bits) of the code histogram over the
    non-null codes.  No host synchronisation: null codes are weighted 0
    instead of being filtered out."""
    codes = codes.flatten()
    keep = codes != null_index
    counts = torch.zeros(codebook_size, dtype=codes.dtype, device=codes.device)
    counts = counts.scatter_add_(0, torch.where(keep, codes, torch.zeros_like(codes)), keep.to(codes.dtype))
    probs = counts / keep.sum()
    logits = torch.log2(probs)
    logits = torch.where(probs == 0.0, torch.zeros_like(logits), logits)
    entropy = -torch.sum(probs * logits)
    return 2 ** entropy
