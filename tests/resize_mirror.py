"""A numpy float32 mirror of the resize arithmetic of csrc/dctae_resize_math.h
(a helper, no tests): vectorised over rows and output pixels, with a loop over
the taps.  numpy rounds every float32 operation on its own and divides
correctly, so the mirror is the defined arithmetic bit for bit:

  scale = n_in / n_out, support = max(scale, 1), inv = 1 / scale (1 when scale < 1)
  center = scale * (i + 0.5)
  taps [lo, hi): lo = max(int(center - support + 0.5), 0), hi = min(int(center + support + 0.5), n_in)
  raw(j) = max(0, 1 - |(j - center + 0.5) * inv|), summed in ascending j
  out[i] = (raw(lo) / sum) * x[lo], then acc = acc + (raw(j) / sum) * x[j] in ascending j
  horizontal pass first, vertical pass over its results; a byte u is u / 255.
"""
import numpy as np

F = np.float32


def axis_windows(n_in, n_out):
    """center (n_out,) float32, lo / hi (n_out,) int64, inv float32"""
    scale = F(n_in) / F(n_out)
    down = scale >= F(1)
    support = scale if down else F(1)
    inv = F(1) / scale if down else F(1)
    i = np.arange(n_out).astype(np.float32)
    center = scale * (i + F(0.5))
    lo = np.maximum(((center - support) + F(0.5)).astype(np.int64), 0)   # astype truncates, as int() does
    hi = np.minimum(((center + support) + F(0.5)).astype(np.int64), n_in)
    assert center.dtype == np.float32 and (hi > lo).all()
    return center, lo, hi, inv


def raw_weight(j, center, inv):
    x = ((j.astype(np.float32) - center) + F(0.5)) * inv
    w = np.maximum(F(1) - np.abs(x), F(0))
    assert w.dtype == np.float32
    return w


def axis_weights(n_in, n_out):
    """lo, hi and the (taps, n_out) normalised weights of one axis (entries past hi are unused)"""
    center, lo, hi, inv = axis_windows(n_in, n_out)
    taps = int((hi - lo).max())
    s = np.zeros(n_out, np.float32)
    for t in range(taps):
        j = lo + t
        s = np.where(j < hi, s + raw_weight(j, center, inv), s)
    w = np.stack([raw_weight(lo + t, center, inv) / s for t in range(taps)])
    assert w.dtype == np.float32
    return lo, hi, w


def resize_axis(x, n_out, axis):
    """one pass of the filter along `axis` of a float32 array"""
    x = np.moveaxis(np.asarray(x), axis, -1)
    assert x.dtype == np.float32
    n_in = x.shape[-1]
    lo, hi, w = axis_weights(n_in, n_out)
    acc = None
    with np.errstate(invalid="ignore"):
        for t in range(w.shape[0]):
            j = lo + t
            p = w[t] * x[..., np.minimum(j, n_in - 1)]
            acc = p if t == 0 else np.where(j < hi, acc + p, acc)
    assert acc.dtype == np.float32
    return np.moveaxis(acc, -1, axis)


def unit_from_byte(u8):
    return np.asarray(u8).astype(np.float32) / F(255)


def resize(x, oh, ow):
    """(..., H, W) float32 or uint8 -> (..., oh, ow) float32"""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        x = unit_from_byte(x)
    return resize_axis(resize_axis(x, ow, -1), oh, -2)
