"""NumPy float64 restatement of the multi-scale focal-L2 validation loss, written from the contract with plain
loops: no torch, nothing shared with posepaf.val_loss or csrc/posepaf_loss.hip.

    terms[t][s][b] = sum over c, y, x of  (p - G)^2 * |1 - st| * M * cw[c]

G: adaptive average pooling with the general window formula, float64 sum / float64 count, rounded once to float32.
st: p where G >= float32(0.01) (compared in float32), 1 - p elsewhere.   M: bilinear, align_corners = False, float64, < 0.5 -> 0.
cw: multi_task_weight for channel 48, keypoint_task_weight for channels 30..47, 1 otherwise.
"""
import math

import numpy as np

NSTACK_WEIGHT = (1, 1, 1, 1)
SCALE_WEIGHT = (0.1, 0.2, 0.4, 1.6, 6.4)
MULTI_TASK_WEIGHT, KEYPOINT_TASK_WEIGHT = 0.1, 3.0
HEAT_START, BKG_START = 30, 48
FG = np.float32(0.01)


def windows(n_in, n_out):
    """[(start, end)] of adaptive pooling's n_out windows over n_in cells: floor(i n_in / n_out) .. ceil((i + 1) n_in / n_out)"""
    return [((i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)) for i in range(n_out)]


def pool_target(g, h, w):
    """g (C, H, W) float16 / float32 -> (C, h, w) float32: the exact mean of each window, rounded once"""
    C, H, W = g.shape
    planes = g.astype(np.float64).tolist()                   # Python floats: float64, added in row-major order
    out = np.zeros((C, h, w), np.float32)
    for i, (r0, r1) in enumerate(windows(H, h)):
        for j, (c0, c1) in enumerate(windows(W, w)):
            cells = float((r1 - r0) * (c1 - c0))
            for c in range(C):
                total = 0.0
                for r in range(r0, r1):
                    for v in planes[c][r][c0:c1]:
                        total += v
                out[c, i, j] = np.float32(total / cells)
    return out


def pool_scales(target, sizes):
    """[s][b] -> pool_target(target[b], *sizes[s]): what focal_l2_terms takes as `pooled`, for callers that score several
    predictions against one target"""
    return [[pool_target(target[b], h, w) for b in range(target.shape[0])] for (h, w) in sizes]


def taps(n_in, n_out):
    """[(first tap, second tap, weight of the second)] of bilinear resampling with align_corners = False"""
    res = []
    for i in range(n_out):
        src = max((i + 0.5) * n_in / n_out - 0.5, 0.0)
        i0 = min(int(math.floor(src)), n_in - 1)
        res.append((i0, min(i0 + 1, n_in - 1), src - i0))
    return res


def resample_mask(m, h, w, threshold=True):
    """m (H, W) float32 -> (h, w) float64; threshold: values < 0.5 become 0"""
    H, W = m.shape
    m64 = m.astype(np.float32).astype(np.float64)
    out = np.zeros((h, w), np.float64)
    for i, (y0, y1, ly) in enumerate(taps(H, h)):
        for j, (x0, x1, lx) in enumerate(taps(W, w)):
            v = (1.0 - ly) * ((1.0 - lx) * m64[y0, x0] + lx * m64[y0, x1]) + ly * ((1.0 - lx) * m64[y1, x0] + lx * m64[y1, x1])
            out[i, j] = 0.0 if (threshold and v < 0.5) else v
    return out


def channel_weights(n_ch=50, multi_task_weight=MULTI_TASK_WEIGHT, keypoint_task_weight=KEYPOINT_TASK_WEIGHT):
    cw = np.ones(n_ch, np.float64)
    cw[n_ch - 2] = multi_task_weight
    cw[HEAT_START:BKG_START] = keypoint_task_weight
    return cw


def focal_l2_terms(preds, target, mask=None, multi_task_weight=MULTI_TASK_WEIGHT, keypoint_task_weight=KEYPOINT_TASK_WEIGHT,
                   plain_l2=False, pooled=None):
    """preds[t][s]: (B, 50, h_s, w_s) arrays (float16 / float32); target (B, 50, H, W); mask (B, H, W) float32 or None;
    pooled: pool_scales(target, sizes) when the caller already has it.  -> float64 (T, K, B)"""
    T, K = len(preds), len(preds[0])
    B, C, H, W = target.shape
    cw = channel_weights(C, multi_task_weight, keypoint_task_weight)
    terms = np.zeros((T, K, B), np.float64)
    for s in range(K):
        h, w = preds[0][s].shape[2:]
        for b in range(B):
            G = pool_target(target[b], h, w) if pooled is None else pooled[s][b]
            assert G.shape == (C, h, w) and G.dtype == np.float32
            M = np.ones((h, w), np.float64) if mask is None else resample_mask(mask[b], h, w)
            fg = G >= FG                                     # float32 against float32
            G64 = G.astype(np.float64)
            for t in range(T):
                p = np.asarray(preds[t][s][b]).astype(np.float64)
                v = (p - G64) ** 2
                if not plain_l2:
                    v = v * np.abs(1.0 - np.where(fg, p, 1.0 - p))
                v = v * M[None] * cw[:, None, None]
                total = 0.0
                for c in range(C):                           # channel by channel; any order of a float64 sum of N non-negative
                    total += float(v[c].sum())               # terms is within N 2^-53 of any other
                terms[t, s, b] = total
    return terms


def combine(terms, nstack_weight=NSTACK_WEIGHT, scale_weight=SCALE_WEIGHT, n_images=None):
    """sum_s scale_weight[s] * (sum_t nstack_weight[t] * sum_b terms[t][s][b] / sum nstack_weight) / sum scale_weight / n_images"""
    T, K, B = terms.shape
    n_images = B if n_images is None else n_images
    total = 0.0
    for s in range(K):
        per_scale = 0.0
        for t in range(T):
            per_scale += nstack_weight[t] * float(terms[t, s].sum())
        total += scale_weight[s] * (per_scale / float(sum(nstack_weight[:T])))
    return total / float(sum(scale_weight[:K])) / n_images


def near_threshold_cells(target, sizes, eps=1e-6):
    """pooled cells of multi-cell windows within eps of 0.01 (there the float32 accumulation order of a pooling decides the side)"""
    n = 0
    B, C, H, W = target.shape
    for (h, w) in sizes:
        multi = np.array([[(r1 - r0) * (c1 - c0) > 1 for (c0, c1) in windows(W, w)] for (r0, r1) in windows(H, h)])
        for b in range(B):
            G = pool_target(target[b], h, w).astype(np.float64)
            n += int(np.count_nonzero((np.abs(G - 0.01) < eps) & multi[None]))
    return n


def near_half_mask_values(mask, sizes, eps=1e-6):
    """resampled mask values within eps of 0.5 that are not exactly 0.5-representable results (exact 0.5 is exact in any order)"""
    n = 0
    for (h, w) in sizes:
        for b in range(mask.shape[0]):
            M = resample_mask(mask[b], h, w, threshold=False)
            n += int(np.count_nonzero((np.abs(M - 0.5) < eps) & (M != 0.5)))
    return n
