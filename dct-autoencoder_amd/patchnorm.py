"""PatchNorm — drop-in for the reference's dct_autoencoder/patchnorm.py:32-177.

Same constructor, buffers (``n``, ``median``, ``b`` as non-trainable
Parameters, so state dicts interchange), ``frozen`` flag, ``forward`` and
``inverse_norm``.  The eval forward and the inverse run as HIP kernels
(dctae_norm_forward / dctae_norm_inverse); the training update (a13) runs as
dctae_stats kernels (see stats.py).
"""
from __future__ import annotations

import torch
from torch import nn

from . import _ops
from ._ops import FEParams, NormState
from ._tracked import _param_stamp, _track
from .dct_patches import DCTPatches


class PatchNorm(nn.Module):
    def __init__(self, max_patch_h: int, max_patch_w: int, patch_size: int, channels: int, eps: float = 1e-6,
                 max_val: float = 6.0, min_val: float = -6.0):
        super().__init__()
        self.eps = eps
        self.patch_size = patch_size
        self.channels = channels
        self.max_patch_h = max_patch_h
        self.max_patch_w = max_patch_w
        self.n = nn.Parameter(torch.zeros(channels, max_patch_h, max_patch_w), requires_grad=False)
        self.median = nn.Parameter(torch.zeros(channels, max_patch_h, max_patch_w, patch_size ** 2),
                                   requires_grad=False)
        self.b = nn.Parameter(torch.ones(channels, max_patch_h, max_patch_w, patch_size ** 2), requires_grad=False)
        self.frozen = False
        self.max_val = max_val
        self.min_val = min_val

    @property
    def std(self) -> torch.Tensor:
        return self.b * 2 ** 0.5

    def _params(self) -> FEParams:
        return FEParams(channels=self.channels, patch_size=self.patch_size, max_patch_h=self.max_patch_h,
                        max_patch_w=self.max_patch_w)

    def _stamp(self):
        """What identifies the tables' current values to the caches that copy
        them (the LFQ thresholds here; BatchEncoder / BatchDecoder).  median
        and b are tracked parameters (_tracked.py): an in-place op moves
        ``_version``, a write through ``.data`` its access count, a new
        tensor the pointer; a Parameter object that is not tracked yet (a new
        one, or one from a pickle) is made so and counted.  Host work only.
        Not a pure read: it is also where an untracked Parameter becomes a
        tracked one (its ``__class__`` is swapped in place, as model.py does
        for the Linears) and ``_retracked`` counts those swaps, so that a new
        Parameter object at a reused address still moves the stamp.  A module
        from an older pickle has no ``_retracked`` yet, hence the getattr."""
        retracked = getattr(self, "_retracked", 0)
        if _track(self.median) | _track(self.b):
            retracked += 1
            self._retracked = retracked
        return (_param_stamp(self.median), _param_stamp(self.b), retracked, float(self.eps),
                float(self.min_val), float(self.max_val))

    def state(self, thresholds: bool = False) -> NormState:
        """Device view of the tables handed to the kernels.  With thresholds,
        the exact LFQ-bit thresholds (one compare per element instead of a
        subtract + divide + two table reads) are attached; they are cached
        and rebuilt whenever median / b / eps / clamp change (``_stamp``).
        The tables are taken with ``detach()``, never through ``.data``,
        which would move the stamp."""
        stamp = self._stamp()
        med = self.median.detach()
        b = self.b.detach()
        if med.dtype != torch.float32 or b.dtype != torch.float32:
            raise AssertionError("PatchNorm tables must be float32 on the MI355X path")
        st = NormState(med.contiguous(), b.contiguous(), float(self.eps), float(self.min_val), float(self.max_val))
        if thresholds and med.is_cuda:
            cache = getattr(self, "_thr_cache", None)
            if cache is None or cache[0] != stamp:
                cache = (stamp, _ops.norm_thresholds(st))
                self._thr_cache = cache
            st.thr = cache[1]
        return st

    def forward(self, dct_patches: DCTPatches) -> torch.Tensor:
        """patchnorm.py:81-165.  Training (and not frozen): update n / median /
        b from the non-pad tokens and return the raw patches with pads zeroed;
        otherwise return (x - median) / (b*sqrt(2) + eps) clamped."""
        if self.training and not self.frozen:
            from . import stats
            return stats.train_step(self, dct_patches)
        return _ops.norm_apply(dct_patches.patches, dct_patches.patch_channels, dct_patches.patch_positions,
                               self.state(), self._params(), inverse=False)

    def inverse_norm(self, dct_patches: DCTPatches) -> torch.Tensor:
        """patchnorm.py:167-177.  Differentiable in the patches: an input that
        requires grad gets the same values with a grad_fn whose backward is
        grad * std (dctae_norm_inverse_backward); the tables get no gradient
        (they are buffers).  The result is fp32, as without grad."""
        x = dct_patches.patches
        if x.requires_grad and torch.is_grad_enabled():
            return _InverseNorm.apply(x, dct_patches.patch_channels, dct_patches.patch_positions, self.state(),
                                      self._params())
        return _ops.norm_apply(x, dct_patches.patch_channels, dct_patches.patch_positions,
                               self.state(), self._params(), inverse=True)


class _InverseNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, channels, positions, state, params):
        ctx.save_for_backward(channels, positions)
        ctx.args = (state, params, x.dtype)
        return _ops.norm_apply(x, channels, positions, state, params, inverse=True)

    @staticmethod
    def backward(ctx, grad):
        channels, positions = ctx.saved_tensors
        state, params, dtype = ctx.args
        dx = _ops.norm_inverse_backward(grad, channels, positions, state, params)
        return dx.view(grad.shape).to(dtype), None, None, None, None
