"""A NumPy restatement, in float64 and written from the formula of include/posepaf.h, of

    pp_conv3x3_dgrad_f16   s[b, i, j, c] = sum over (r, q, k) with (i + 1 - r, j + 1 - q) inside image b of
                                           dy[b, i + 1 - r, j + 1 - q, k] * w[k][r][q][c]
                           t = s where y > 0 or y is None, else slope * s;   dx = half(t)

with the |dy| |w| sums its rounding bound multiplies, the bound, and the operands of the exact (small-integer) cases of
tests/test_gpu_conv_dgrad.py.  Nothing here imports the package."""
import numpy as np

from conv_wgrad_reference import CHANNELS, INT_MAX, LARGE_SHAPE, SMALL_SHAPES, case_id, to_half  # noqa: F401  (shared shapes)

TAPS = [(r, q) for r in range(3) for q in range(3)]
SLOPE = 0.125                        # a power of two: slope * s is exact
EXACT_CASES = [(shape, c) for shape in SMALL_SHAPES for c in CHANNELS] + [(LARGE_SHAPE, (64, 64))]
SPECIALS = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x3C00, 0xBC00, 0x4500, 0xC500], np.uint16).view(np.float16)


def _sums(d, ww):
    """d: float64 (n, h, w, K); ww: float64 (K, 3, 3, C) -> s float64 (n, h, w, C)"""
    n, h, w, K = d.shape
    s = np.zeros((n, h, w, ww.shape[3]), np.float64)
    for r, q in TAPS:
        # output pixel (i, j) takes dy pixel (i + 1 - r, j + 1 - q): the output window whose source lies inside the image
        di, dj = 1 - r, 1 - q
        i0, i1, j0, j1 = max(0, -di), min(h, h - di), max(0, -dj), min(w, w - dj)
        if i1 > i0 and j1 > j0:
            s[:, i0:i1, j0:j1, :] += d[:, i0 + di:i1 + di, j0 + dj:j1 + dj, :] @ ww[:, r, q, :]
    return s


def _check(dy, w, y, shape):
    dy, w = np.asarray(dy), np.asarray(w)
    n, h, wd = shape
    assert dy.dtype == np.float16 and w.dtype == np.float16 and w.ndim == 4 and w.shape[1:3] == (3, 3)
    assert dy.shape == (n * h * wd, w.shape[0])
    if y is not None:
        y = np.asarray(y)
        assert y.dtype == np.float16 and y.shape == (n, h, wd, w.shape[3])
    return dy.astype(np.float64).reshape(n, h, wd, -1), w.astype(np.float64), y


def conv3x3_dgrad_sums(dy, w, shape):
    """(s, sum |dy| |w|) float64 (n, h, w, c_in).  dy: binary16 (n h w, c_out); w: binary16 (c_out, 3, 3, c_in)"""
    d, ww, _ = _check(dy, w, None, shape)
    return _sums(d, ww), _sums(np.abs(d), np.abs(ww))


def conv3x3_dgrad(dy, w, y, shape, slope):
    """t float64 (n, h, w, c_in), the value dx rounds.  y: binary16 (n, h, w, c_in) or None; slope as the float32 the entry receives"""
    d, ww, y = _check(dy, w, y, shape)
    s = _sums(d, ww)
    if y is None:
        return s
    return np.where(y.astype(np.float64) > 0.0, s, float(np.float32(slope)) * s)


def conv3x3_dgrad_bound(dy, w, y, shape, slope):
    """|float(dx) - t| <= E + max(2^-11 (|t| + E), 2^-25),  E = a (9 c_out 2^-23 sum |dy w| + 2^-24 |s|),  a = 1 where y > 0 (or no y)
    else slope: at most 9 c_out float32 additions of exact products in ANY order ((9 c_out - 1) 2^-24 sum |dy w| to first order) with a
    factor 2 for an accumulate that truncates (as conv_wgrad_reference.conv3x3_bounds argues), one float32 multiply (2^-24 |s|, charged to
    every element), one binary16 rounding: relative 2^-11 of the rounded value, or half a subnormal step 2^-25"""
    d, ww, y = _check(dy, w, y, shape)
    s, absprod = _sums(d, ww), _sums(np.abs(d), np.abs(ww))
    a = 1.0 if y is None else np.where(y.astype(np.float64) > 0.0, 1.0, float(np.float32(slope)))
    E = a * (9 * ww.shape[0] * 2.0 ** -23 * absprod + 2.0 ** -24 * np.abs(s))
    return E + np.maximum(2.0 ** -11 * (np.abs(a * s) + E), 2.0 ** -25)


def int_operands(case):
    """(dy (n h w, c_out), w (c_out, 3, 3, c_in), y (n, h, w, c_in)) binary16, a function of the case alone: dy and w are integers in
    -4 .. 4; y is drawn from +-0, the smallest and the largest subnormal of either sign, +-1 and +-5"""
    (n, h, w), (c_in, c_out) = case
    rng = np.random.default_rng([n, h, w, c_in, c_out, 27])
    dy = rng.integers(-INT_MAX, INT_MAX + 1, (n * h * w, c_out)).astype(np.float16)
    wt = rng.integers(-INT_MAX, INT_MAX + 1, (c_out, 3, 3, c_in)).astype(np.float16)
    y = SPECIALS[rng.integers(0, SPECIALS.size, (n, h, w, c_in))]
    return dy, wt, y
