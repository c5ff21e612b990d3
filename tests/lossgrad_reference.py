"""NumPy float64 restatement of the gradient of the multi-scale focal-L2 loss with respect to the predictions,
written from the contract with plain loops over tests/loss_reference.py's pool_target / resample_mask: no torch, nothing shared with
posepaf.val_loss or csrc/posepaf_loss.hip.

Given upstream weights tw[t][s][b] = dL / dterms[t][s][b], for every element p of preds[t][s][b] (widened from its stored value):

    d = p - float64(G)
    focal:  f  = |1 - st|,  st = p where G >= float32(0.01) (compared in float32), 1 - p elsewhere
            f' = -sgn(1 - p) where G >= float32(0.01), sgn(p) elsewhere; sgn(0) = +0.0 in both (torch's abs has derivative 0 at 0)
            e  = (2.0 * d) * f + (d * d) * f'
    plain:  e  = 2.0 * d
    g64  = tw[t][s][b] * (cw[c] * (M * e))
    grad = float32(g64), then, for binary16 predictions, float16 of that float32    (both round to nearest even)

float64 in exactly this association.  There is no gradient with respect to the target or the mask.
"""
import os

import numpy as np

import loss_reference as lr


def load_case(golden, name):
    """tests/golden/lossgrad_<name>.npz (and loss_<name>.npz where the gradient fixture reuses its inputs) -> dict of target, mask,
    preds[t][s], sizes, grads[t][s] (the reference's float32 gradients of its scalar), kinks (elements on a kink)"""
    g = np.load(os.path.join(golden, f"lossgrad_{name}.npz"))
    src = g if "target" in g.files else np.load(os.path.join(golden, f"loss_{name}.npz"))
    sizes = [tuple(int(v) for v in hw) for hw in g["sizes"]]
    assert sizes == [tuple(int(v) for v in hw) for hw in src["sizes"]]
    preds = [[src[f"pred_{t}_{s}"] for s in range(5)] for t in range(2)]
    grads = [[g[f"grad_{t}_{s}"] for s in range(5)] for t in range(2)]
    return dict(target=src["target"], mask=src["mask"], preds=preds, sizes=sizes, grads=grads, kinks=int(g["kink_elements"]))


def sgn(x):
    """+1 / -1 / +0.0, elementwise (never -0.0)"""
    return np.where(x > 0.0, 1.0, np.where(x < 0.0, -1.0, 0.0))


def element_gradient(p, G, M, cw, tw, plain_l2=False):
    """p (C, h, w) float64, G (C, h, w) float32, M (h, w) float64, cw (C,) float64, tw a float -> g64 (C, h, w) float64"""
    d = p - G.astype(np.float64)
    e = 2.0 * d
    if not plain_l2:
        fg = G >= lr.FG                                      # float32 against float32
        f = np.abs(1.0 - np.where(fg, p, 1.0 - p))
        fd = np.where(fg, np.where(1.0 - p > 0.0, -1.0, np.where(1.0 - p < 0.0, 1.0, 0.0)), sgn(p))
        e = e * f + (d * d) * fd
    return np.float64(tw) * (cw[:, None, None] * (M[None] * e))


def focal_l2_grad(preds, target, term_weights, mask=None, multi_task_weight=lr.MULTI_TASK_WEIGHT, keypoint_task_weight=lr.KEYPOINT_TASK_WEIGHT,
                  plain_l2=False, pooled=None, rounded=True):
    """preds[t][s]: (B, 50, h_s, w_s) float16 / float32 arrays; target (B, 50, H, W); term_weights (T, K, B) float64; mask (B, H, W)
    float32 or None; pooled: lr.pool_scales(target, sizes) when the caller has it.
    -> grads[t][s]: arrays of the predictions' shape and dtype (rounded=False: the float64 values before the roundings)"""
    T, K = len(preds), len(preds[0])
    B, C, H, W = target.shape
    cw = lr.channel_weights(C, multi_task_weight, keypoint_task_weight)
    tw = np.asarray(term_weights, np.float64)
    assert tw.shape == (T, K, B)
    grads = [[None] * K for _ in range(T)]
    for s in range(K):
        h, w = preds[0][s].shape[2:]
        for t in range(T):
            grads[t][s] = np.zeros((B, C, h, w), preds[t][s].dtype if rounded else np.float64)
        for b in range(B):
            G = lr.pool_target(target[b], h, w) if pooled is None else pooled[s][b]
            assert G.shape == (C, h, w) and G.dtype == np.float32
            M = np.ones((h, w), np.float64) if mask is None else lr.resample_mask(mask[b], h, w)
            for t in range(T):
                p = np.asarray(preds[t][s][b]).astype(np.float64)
                g64 = element_gradient(p, G, M, cw, tw[t, s, b], plain_l2)
                if not rounded:
                    grads[t][s][b] = g64
                    continue
                g32 = g64.astype(np.float32)                 # nearest even
                grads[t][s][b] = g32.astype(np.float16) if preds[t][s].dtype == np.float16 else g32
    return grads


def combine_weights(T, K, B, nstack_weight=lr.NSTACK_WEIGHT, scale_weight=lr.SCALE_WEIGHT, n_images=None):
    """d combine(terms) / d terms[t][s][b] = sw[s] / sum(sw) * nw[t] / sum(nw) / n_images  -> (T, K, B) float64"""
    n = B if n_images is None else n_images
    tw = np.zeros((T, K, B), np.float64)
    for t in range(T):
        for s in range(K):
            tw[t, s, :] = scale_weight[s] / float(sum(scale_weight[:K])) * (nstack_weight[t] / float(sum(nstack_weight[:T]))) / n
    return tw


def kink_elements(preds, target, sizes, pooled=None):
    """[t][s] boolean arrays: the elements at which |1 - st| has no derivative (p == 1 on the foreground, p == 0 elsewhere)"""
    T, K = len(preds), len(preds[0])
    out = [[None] * K for _ in range(T)]
    for s, (h, w) in enumerate(sizes):
        G = np.stack([lr.pool_target(target[b], h, w) if pooled is None else pooled[s][b] for b in range(target.shape[0])])
        fg = G >= lr.FG
        for t in range(T):
            p = preds[t][s].astype(np.float64)
            out[t][s] = np.where(fg, p == 1.0, p == 0.0)
    return out
