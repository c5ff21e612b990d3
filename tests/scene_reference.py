"""Float64 restatement of the reference's training-target recipe (py_cocodata_server/py_data_heatmapper.py:105-257): the
yardstick of the scene renderers (posepaf/synth.py on the host, pp_render_scenes on the device).  Written from the recipe, one
pixel formula at a time, independent of both: no float32 anywhere, no accumulation-order rules, no NumPy slicing tricks.

    keypoint channel 30 + k   max over annotated people of exp(-((gx - x)^2 + (gy - y)^2) / 162), gx = 4 i + 1.5, inside the
                              cells round(x / 4) - 7 .. round(x / 4) + 7 (likewise y), clipped to the map; skipped when the
                              window's upper bound is negative                                        (:117-164)
    limb channel l            inside the cells round((min - 4) / 4) .. round((max + 4) / 4) of the end points (same clipping and
                              skipping, zero-length limb skipped): g = exp(-d^2 / 98), d = the distance to the LINE through
                              the end points with the reference's + 1e-6 in the denominator; g <= 0.015 becomes 0.01; the
                              mean of the contributions where there is one                            (:178-244, :326-357)
    clip to [0, 1]

`round` is Python's (ties to even).  tests/golden/scene_*.npz (made by tests/golden/make_golden_scenes.py from the reference's own
Heatmapper) pin this file to the reference.

The limb floor is a step: a contribution within a few ulp of 0.015 legitimately lands on either side in a float32 / other-libm
implementation.  render() therefore also returns, for the limb channels, the mask of pixels where some contribution lies within
0.015 * (1 +- FLOOR_BAND); comparisons skip those pixels and tests cap their share at MASK_CAP of a scene's limb pixels.
"""
import math

import numpy as np

NUM_PART, NUM_LIMB, NUM_CH = 18, 30, 50
LIMB_FROM = [1, 1, 1, 1, 1, 0, 0, 14, 15, 1, 2, 3, 1, 5, 6, 1, 8, 9, 1, 11, 12, 0, 0, 2, 8, 5, 11, 16, 17, 8]
LIMB_TO = [0, 14, 15, 16, 17, 14, 15, 16, 17, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 2, 5, 8, 12, 11, 9, 2, 5, 11]
FLIP_HEAT = [0, 1, 5, 6, 7, 2, 3, 4, 11, 12, 13, 8, 9, 10, 15, 14, 17, 16, 18, 19]
FLIP_LIMB = [0, 2, 1, 4, 3, 6, 5, 8, 7, 12, 13, 14, 9, 10, 11, 18, 19, 20, 15, 16, 17, 22, 21, 25, 26, 23, 24, 28, 27, 29]
FLOOR, FLOOR_VALUE, FLOOR_BAND = 0.015, 0.01, 1e-4
MASK_CAP = 1e-4          # at most this share of a scene's limb pixels may sit on the floor's step
TOL = 1e-6               # |implementation - restatement| outside the mask (values <= 1: ~16 float32 half-ulps at 1)


def _cells(lo: int, hi: int, n: int):
    """the map cells lo .. hi (inclusive) as the reference's slice leaves them, or None when it skips the item"""
    if hi < 0:
        return None
    return range(max(lo, 0), min(hi, n - 1) + 1)


def render(joints, h: int, w: int, reverse_kp: bool = False):
    """joints (P, 18, 3): x, y in image pixels, flag < 2 = annotated.  -> (maps float64 (50, h, w), mask bool (30, h, w))"""
    joints = np.asarray(joints, np.float64).reshape(-1, NUM_PART, 3)
    maps = np.zeros((NUM_CH, h, w), np.float64)
    mask = np.zeros((NUM_LIMB, h, w), bool)
    for k in range(NUM_PART):
        for x, y, flag in joints[:, k]:
            if not flag < 2:
                continue
            cx, cy = int(round(x / 4)), int(round(y / 4))
            xs, ys = _cells(cx - 7, cx + 7, w), _cells(cy - 7, cy + 7, h)
            if xs is None or ys is None:
                continue
            for i in ys:
                for j in xs:
                    v = math.exp(-((4 * j + 1.5 - x) ** 2) / 162.0) * math.exp(-((4 * i + 1.5 - y) ** 2) / 162.0)
                    maps[NUM_LIMB + k, i, j] = max(maps[NUM_LIMB + k, i, j], v)
    for l, (a, b) in enumerate(zip(LIMB_FROM, LIMB_TO)):
        total = np.zeros((h, w), np.float64)
        count = np.zeros((h, w), np.int64)
        for person in joints:
            x1, y1, f1 = person[a]
            x2, y2, f2 = person[b]
            if not (f1 < 2 and f2 < 2):
                continue
            dx, dy = x2 - x1, y2 - y1
            if dx * dx + dy * dy == 0:
                continue
            norm = math.sqrt(dx * dx + dy * dy)
            xs = _cells(int(round((min(x1, x2) - 4) / 4)), int(round((max(x1, x2) + 4) / 4)), w)
            ys = _cells(int(round((min(y1, y2) - 4) / 4)), int(round((max(y1, y2) + 4) / 4)), h)
            if xs is None or ys is None:
                continue
            for i in ys:
                for j in xs:
                    d = abs(dx * (y1 - (4 * i + 1.5)) - (x1 - (4 * j + 1.5)) * dy) / (norm + 1e-6)
                    g = math.exp(-(d * d) / 98.0)
                    if abs(g - FLOOR) <= FLOOR * FLOOR_BAND:
                        mask[l, i, j] = True
                    total[i, j] += FLOOR_VALUE if g <= FLOOR else g
                    count[i, j] += 1
        maps[l] = np.where(count > 0, total / np.maximum(count, 1), 0.0)
    if reverse_kp:
        maps[NUM_CH - 1] = maps[NUM_LIMB:NUM_LIMB + NUM_PART].max(axis=0)
    return np.clip(maps, 0.0, 1.0), mask


def mirror(maps):
    """what the network would output for the W-mirrored image: out1[c] = mirror_W(out0[flip_ord[c]])"""
    order = list(FLIP_LIMB) + [NUM_LIMB + c for c in FLIP_HEAT]
    return np.ascontiguousarray(maps[order][:, :, ::-1])


def full_mask(mask):
    """limb mask (30, h, w) -> (50, h, w) (keypoint and background channels have no step)"""
    out = np.zeros((NUM_CH,) + mask.shape[1:], bool)
    out[:NUM_LIMB] = mask
    return out


def mirror_mask(mask50):
    return mirror(mask50)


def masked_share(mask) -> float:
    return float(mask.sum()) / float(mask.size)


def max_err_outside(got, want, mask50) -> float:
    """max |got - want| over the pixels outside the mask (float64)"""
    err = np.abs(np.asarray(got, np.float64) - want)
    err[mask50] = 0.0
    return float(err.max()) if err.size else 0.0
