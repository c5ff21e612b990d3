"""NumPy restatement of the 1 x 1 head's weight and bias gradient (pp_head_wgrad_f16, include/posepaf.h):

    dw = g[:, :c_out].T @ xs    db = g[:, :c_out].sum(0)      in float64
    xs = x, or with gains  half(float32(x) * float32(scale[m // hw]))  -- the product of two binary16 values is exact in float32,
         so the conversion is the ONE rounding (nearest even) of the exact product

and of the trainer's "auto" loss scale.  Nothing here imports the package."""
import numpy as np


def scaled_input(x, scale=None, hw=None):
    """xs (m, c_in) binary16.  x: binary16 (m, c_in); scale: binary16 (m // hw, c_in) or None"""
    x = np.asarray(x)
    assert x.dtype == np.float16 and x.ndim == 2
    if scale is None:
        return x
    scale = np.asarray(scale)
    assert scale.dtype == np.float16 and x.shape[0] % hw == 0 and scale.shape == (x.shape[0] // hw, x.shape[1])
    prod = x.astype(np.float32) * np.repeat(scale.astype(np.float32), hw, axis=0)      # exact: 11 + 11 significand bits
    with np.errstate(over="ignore"):                     # a product above 65504 becomes an infinity, as on the device
        return prod.astype(np.float16)


def head_wgrad(g, x, c_out, scale=None, hw=None, inv_loss_scale=1.0):
    """-> (dw float64 (c_out, c_in), db float64 (c_out,)).  g: binary16 (m, ldg), only [:, :c_out] is looked at"""
    g = np.asarray(g)
    assert g.dtype == np.float16 and g.ndim == 2 and g.shape[1] >= c_out
    g64 = g[:, :c_out].astype(np.float64)
    xs = scaled_input(x, scale, hw).astype(np.float64)
    return (g64.T @ xs) * float(inv_loss_scale), g64.sum(axis=0) * float(inv_loss_scale)


def abs_products(g, x, c_out, scale=None, hw=None, inv_loss_scale=1.0):
    """(|g|.T @ |xs|, sum |g|): what the rounding bound  m * 2^-23 * (.)  multiplies"""
    g64 = np.abs(np.asarray(g)[:, :c_out].astype(np.float64))
    xs = np.abs(scaled_input(x, scale, hw).astype(np.float64))
    return (g64.T @ xs) * float(inv_loss_scale), g64.sum(axis=0) * float(inv_loss_scale)


def rounding_bound(m, absprod):
    """|device - float64| <= m * 2^-23 * sum |g| |xs|:  (m - 1) * 2^-24 is the classical bound of ANY order of m - 1 float32 additions
    with round-to-nearest (the products are exact); the factor 2 covers an MFMA accumulate that truncates; the final float32
    rounding of inv_loss_scale * A (a power of two here: exact) and of the reference's float64 are inside the remaining m vs m - 1"""
    return float(m) * 2.0 ** -23 * absprod


# ---- the trainer's loss scale (posepaf/head_train.py): restated, not imported

NSTACK_WEIGHT = (1, 1, 1, 1)
SCALE_WEIGHT = (0.1, 0.2, 0.4, 1.6, 6.4)
KEYPOINT_TASK_WEIGHT = 3.0
ELEMENT_BOUND = 12.0        # |2 d f + d^2 f'| for p in [-1, 2], G in [0, 1]:  |d| <= 2, f <= 2, |f'| = 1  ->  2*2*2 + 4 = 12
HALF_MAX = 65504.0


def tw_max(batch, stages, scales=5):
    nw, sw = NSTACK_WEIGHT[:stages], SCALE_WEIGHT[:scales]
    return max(nw) / sum(nw) * max(sw) / sum(sw) / batch


def auto_loss_scale(batch, stages, scales=5):
    """the largest power of two S with S * tw_max * 3.0 * 12 <= 65504"""
    limit = HALF_MAX / (tw_max(batch, stages, scales) * KEYPOINT_TASK_WEIGHT * ELEMENT_BOUND)
    s = 1.0
    while s * 2.0 <= limit:
        s *= 2.0
    while s > limit:
        s /= 2.0
    return s
