"""NumPy restatements, in float64 and written from the formulas of include/posepaf.h, of

    pp_conv3x3_wgrad_f16   dw[k][r][s][c] = inv * sum over pixels (b, i, j) with (i + r - 1, j + s - 1) inside the image of
                                            dy[b, i, j, k] * x[b, i + r - 1, j + s - 1, c];     db[k] = inv * sum dy[., k]
    pp_head_dgrad_f16      s = g[:, :c_out] @ w;   t = s where y > 0 else slope * s;   dx = half(t)

with what their rounding bounds multiply, and the operands of the exact (small-integer) cases of tests/test_gpu_conv_wgrad.py.
Nothing here imports the package."""
import numpy as np

TAPS = [(r, s) for r in range(3) for s in range(3)]


def _windows(h, w, r, s):
    """the pixels (i, j) whose neighbour (i + r - 1, j + s - 1) lies inside an h x w image, as slices, and the neighbours' slices"""
    dr, ds = r - 1, s - 1
    i0, i1, j0, j1 = max(0, -dr), min(h, h - dr), max(0, -ds), min(w, w - ds)
    return (slice(i0, i1), slice(j0, j1)), (slice(i0 + dr, i1 + dr), slice(j0 + ds, j1 + ds)), max(0, i1 - i0) * max(0, j1 - j0)


def _wgrad(d, xx):
    n, h, w, K = d.shape
    C = xx.shape[3]
    dw = np.zeros((K, 3, 3, C), np.float64)
    for r, s in TAPS:
        (pi, pj), (qi, qj), count = _windows(h, w, r, s)
        if count:
            dw[:, r, s, :] = d[:, pi, pj, :].reshape(-1, K).T @ xx[:, qi, qj, :].reshape(-1, C)
    return dw, d.reshape(-1, K).sum(axis=0)


def conv3x3_wgrad(dy, x, inv_loss_scale=1.0):
    """dy: binary16 (n h w, c_out); x: binary16 (n, h, w, c_in) -> (dw float64 (c_out, 3, 3, c_in), db float64 (c_out,))"""
    dy, x = np.asarray(dy), np.asarray(x)
    assert dy.dtype == np.float16 and x.dtype == np.float16 and x.ndim == 4 and dy.shape[0] == x.shape[0] * x.shape[1] * x.shape[2]
    dw, db = _wgrad(dy.astype(np.float64).reshape(x.shape[:3] + (-1,)), x.astype(np.float64))
    return dw * float(inv_loss_scale), db * float(inv_loss_scale)


def conv3x3_abs_products(dy, x, inv_loss_scale=1.0):
    """(|dy|^T |x_tap| per element of dw, sum |dy| per element of db): what the rounding bound multiplies"""
    dy, x = np.asarray(dy), np.asarray(x)
    dw, db = _wgrad(np.abs(dy.astype(np.float64)).reshape(x.shape[:3] + (-1,)), np.abs(x.astype(np.float64)))
    return dw * float(inv_loss_scale), db * float(inv_loss_scale)


def contributing_pixels(n, h, w):
    """M[r][s]: the number of pixels whose neighbour of tap (r, s) lies inside its image"""
    return np.array([[n * _windows(h, w, r, s)[2] for s in range(3)] for r in range(3)], np.float64)


def conv3x3_bounds(dy, x, inv_loss_scale=1.0):
    """|device - float64| <= M * 2^-23 * inv * sum |dy| |x_tap| (tests/head_wgrad_reference.rounding_bound with the tap's own number of
    terms: (M - 1) 2^-24 for ANY order of M - 1 float32 additions of exact products, a factor 2 for an accumulate that truncates,
    the last float32 rounding of inv * A inside M against M - 1)"""
    n, h, w, _ = np.asarray(x).shape
    aw, ab = conv3x3_abs_products(dy, x, inv_loss_scale)
    return contributing_pixels(n, h, w)[None, :, :, None] * 2.0 ** -23 * aw, float(n * h * w) * 2.0 ** -23 * ab


def head_dgrad(g, w, y, c_out, slope):
    """g: binary16 (m, ldg), only [:, :c_out] is looked at; w: binary16 (c_out, c_in); y: binary16 (m, c_in) -> t float64 (m, c_in),
    the value dx rounds.  slope is taken as the float32 the entry receives"""
    g, w, y = np.asarray(g), np.asarray(w), np.asarray(y)
    assert g.dtype == np.float16 and w.dtype == np.float16 and y.dtype == np.float16 and w.shape[0] == c_out <= g.shape[1]
    s = g[:, :c_out].astype(np.float64) @ w.astype(np.float64)
    return np.where(y.astype(np.float64) > 0.0, s, float(np.float32(slope)) * s)


def to_half(t):
    with np.errstate(over="ignore"):
        return np.asarray(t).astype(np.float16)


def head_dgrad_bound(g, w, y, c_out, slope):
    """|float(dx) - t| <= E + max(2^-11 (|t| + E), 2^-25),  E = a 2^-24 (c_out sum_k |g w| + |s|),  a = 1 where y > 0 else slope:
    c_out float32 additions of exact products in one order ((c_out - 1) 2^-24 sum |g w| to first order, c_out covers the rest), one
    float32 multiply (2^-24 |s|, charged to every element), one binary16 rounding: relative 2^-11 of the rounded value, or half a
    subnormal step 2^-25"""
    g, w, y = np.asarray(g), np.asarray(w), np.asarray(y)
    absprod = np.abs(g[:, :c_out].astype(np.float64)) @ np.abs(w.astype(np.float64))
    s = g[:, :c_out].astype(np.float64) @ w.astype(np.float64)
    a = np.where(y.astype(np.float64) > 0.0, 1.0, float(np.float32(slope)))
    E = a * 2.0 ** -24 * (c_out * absprod + np.abs(s))
    return E + np.maximum(2.0 ** -11 * (np.abs(a * s) + E), 2.0 ** -25)


# ---- the exact cases: operands that are small integers, so every float32 partial sum is exact in ANY order

SMALL_SHAPES = [(1, 1, 1), (1, 1, 70), (1, 70, 1), (2, 3, 5), (1, 5, 29), (3, 8, 8)]
LARGE_SHAPE = (1, 130, 127)          # m = 16510: more chunks than workgroups; at (64, 64) only
CHANNELS = [(64, 64), (192, 128), (256, 256)]
EXACT_CASES = [(shape, c) for shape in SMALL_SHAPES for c in CHANNELS] + [(LARGE_SHAPE, (64, 64))]
INT_MAX = 4


def case_id(case):
    (n, h, w), (c_in, c_out) = case
    return f"{n}x{h}x{w}-{c_in}to{c_out}"


def int_operands(case):
    """(dy (n h w, c_out), x (n, h, w, c_in)) binary16 with integer values in -4 .. 4, a function of the case alone"""
    (n, h, w), (c_in, c_out) = case
    rng = np.random.default_rng([n, h, w, c_in, c_out])
    dy = rng.integers(-INT_MAX, INT_MAX + 1, (n * h * w, c_out)).astype(np.float16)
    x = rng.integers(-INT_MAX, INT_MAX + 1, (n, h, w, c_in)).astype(np.float16)
    return dy, x


DGRAD_MS, DGRAD_C_OUTS, DGRAD_LDGS = (1, 63, 64, 145), (1, 50, 64), (50, 64)
DGRAD_SLOPE = 0.125                  # a power of two: slope * s is exact


def dgrad_int_operands(m, c_in, c_out, ldg, seed=0):
    """(g (m, ldg) with NaN behind c_out, w (c_out, c_in), y (m, c_in)) binary16.  g and w are integers in -4 .. 4; y mixes positive and
    negative values with +0, -0 and positive and negative subnormals"""
    rng = np.random.default_rng([m, c_in, c_out, ldg, seed])
    g = np.full((m, ldg), np.nan, np.float16)
    g[:, :c_out] = rng.integers(-INT_MAX, INT_MAX + 1, (m, c_out)).astype(np.float16)
    w = rng.integers(-INT_MAX, INT_MAX + 1, (c_out, c_in)).astype(np.float16)
    special = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x3C00, 0xBC00, 0x4500, 0xC500], np.uint16).view(np.float16)
    y = special[rng.integers(0, special.size, (m, c_in))]
    return g, w, y
