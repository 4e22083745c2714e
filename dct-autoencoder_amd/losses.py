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
