"""Parameters whose in-place updates a cache can see: what model._Packed,
PatchNorm's LFQ thresholds and optim.FusedAdamW key their device copies on."""
from __future__ import annotations

import torch
from torch import nn


class _TrackedParameter(nn.Parameter):
    """An nn.Parameter that a device-side cache copies, counting accesses of ``.data``.
    torch gives ``p.data`` a version counter of its own, so ``p.data.copy_(...)`` moves
    neither ``p._version`` nor ``p.data_ptr()``; the count is the third part of
    ``_param_stamp``, so the cached copies are rebuilt after any access that may have
    been such a write (a read costs one rebuild, never a stale copy).  A tensor obtained from
    ``.data`` earlier and written later is not seen.  Pickling gives back a plain Parameter."""
    _data_reads = 0

    @property
    def data(self):
        self._data_reads += 1
        return torch.Tensor.data.__get__(self)

    @data.setter
    def data(self, value):
        self._data_reads += 1
        torch.Tensor.data.__set__(self, value)

    def __deepcopy__(self, memo):   # nn.Parameter's, without going through .data
        if id(self) in memo:
            return memo[id(self)]
        result = type(self)(self.detach().clone(memory_format=torch.preserve_format), self.requires_grad)
        memo[id(self)] = result
        return result

    def __repr__(self):
        return "Parameter containing:\n" + repr(self.detach().as_subclass(torch.Tensor))


def _param_stamp(p):
    """What identifies a parameter's current value to the caches."""
    return p.data_ptr(), p._version, getattr(p, "_data_reads", 0)


def _track(p) -> bool:
    """Make ``p`` a _TrackedParameter in place; True if it was not one (a
    plain Parameter: a new object, or one that came back from a pickle)."""
    if type(p) is _TrackedParameter or not isinstance(p, nn.Parameter):
        return False
    p.__class__ = _TrackedParameter
    return True
