"""Shared by tests/test_draw_limbs_cpu.py and tests/test_gpu_draw_limbs.py: a per-pixel restatement of
utils.draw.draw_limbs_original (the form the HIP kernel pp_draw_limbs_u8 evaluates) and the per-instance parameters both ways.

The restatement: draw.py takes instance after instance (limb types of DRAW_LIST outside, persons inside), paints two rings and
an ellipse into a copy inside bounding boxes and blends the WHOLE canvas 0.4 / 0.6 with the copy.  Here every pixel folds, in
the same order, over the instances that hit it -- no bounding box at all, only the three tests:
    ring     9 <= (x - rx)^2 + (y - ry)^2 <= 25                                                  (integers)
    ellipse  u = (x - cx) c + (y - cy) s;  v = (-(x - cx)) s + (y - cy) c;  (u / a)^2 + (v / 3)^2 <= 1    (float64)
    hit      px = clip(rint(px 0.4 + cur 0.6), 0, 255),  cur = the ellipse's colour where it hits, black where only a ring does
Both give the same canvas iff a pixel nothing hits keeps its value under draw.py's blend and draw.py's boxes cut no primitive;
test_draw_limbs_cpu.py checks both."""
import math

import numpy as np

COLOR_BOARD = [0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21]      # utils/draw.py:103


def instances_drawpy(persons, cand):
    """the instances of draw_limbs_original(canvas, persons, cand, LIMB_PAIRS, DRAW_LIST) in draw order, each with the
    parameters draw.py itself forms (`** 0.5` on NumPy scalars, math.atan2): (ring0, ring1, centre, a, k, colour)"""
    from posepaf import skeleton as sk
    from utils import draw
    out = []
    for t, i in enumerate(sk.DRAW_LIST):
        for person in persons:
            ids = person[np.asarray(sk.LIMB_PAIRS[i]), 0].astype(int)
            if -1 in ids:
                continue
            xs, ys = cand[ids, 0], cand[ids, 1]
            length = float(((ys[0] - ys[1]) ** 2 + (xs[0] - xs[1]) ** 2) ** 0.5)
            k = int(math.degrees(math.atan2(ys[0] - ys[1], xs[0] - xs[1])))
            out.append(((int(xs[0]), int(ys[0])), (int(xs[1]), int(ys[1])), (int(np.mean(xs)), int(np.mean(ys))),
                        max(float(int(length / 2)), 0.5), k, tuple(draw.LimbColors[COLOR_BOARD[t % 18]])))
    return out


def instances_device(rec, lib):
    """the same list as the kernel forms it from a record: peak_id < 0 absent, coordinates widened to double, math.sqrt,
    pp_limb_angle_deg, truncation towards zero"""
    from posepaf import _lib, skeleton as sk
    from utils import draw
    is_float = bool(int(rec["status"]) & _lib.ST_FLOAT_COORDS)
    out = []
    nh = min(max(int(rec["n_humans"]), 0), _lib.MAX_HUMANS)
    for t, i in enumerate(sk.DRAW_LIST):
        pa, pb = sk.LIMB_PAIRS[i]
        for hid in range(nh):
            hm = rec["humans"][hid]
            if hm["peak_id"][pa] < 0 or hm["peak_id"][pb] < 0:
                continue
            xs, ys = (hm["x"].view(np.float32), hm["y"].view(np.float32)) if is_float else (hm["x"], hm["y"])
            x0, y0, x1, y1 = float(xs[pa]), float(ys[pa]), float(xs[pb]), float(ys[pb])
            dy, dx = y0 - y1, x0 - x1
            length = math.sqrt(dy * dy + dx * dx)
            out.append(((int(x0), int(y0)), (int(x1), int(y1)), (int((x0 + x1) / 2), int((y0 + y1) / 2)),
                        max(float(int(length / 2)), 0.5), int(lib.pp_limb_angle_deg(dy, dx)), tuple(draw.LimbColors[COLOR_BOARD[t]])))
    return out


def fold(canvas, instances):
    """-> a new canvas: every pixel folded over the instances that hit it, in order; no bounding boxes"""
    h, w = canvas.shape[:2]
    out = canvas.copy()
    yi, xi = np.mgrid[0:h, 0:w]
    yf, xf = yi.astype(np.float64), xi.astype(np.float64)
    for (r0, r1, (cx, cy), a, k, colour) in instances:
        rings = np.zeros((h, w), bool)
        for rx, ry in (r0, r1):
            d2 = (xi - rx) ** 2 + (yi - ry) ** 2
            rings |= (d2 >= 9) & (d2 <= 25)
        c, s = math.cos(math.radians(k)), math.sin(math.radians(k))
        u = (xf - cx) * c + (yf - cy) * s
        v = -(xf - cx) * s + (yf - cy) * c
        ell = (u / a) ** 2 + (v / 3.0) ** 2 <= 1.0
        hit = rings | ell
        cur = np.where(ell[..., None], np.asarray(colour, np.float64), 0.0)
        blended = np.clip(np.rint(out.astype(np.float64) * 0.4 + cur * 0.6), 0, 255).astype(np.uint8)
        out[hit] = blended[hit]
    return out


def fractional(people, fx=0.75, fy=0.5):
    """integer people -> the same people pushed away from zero by a fraction (so that truncation brings them back)"""
    return [{p: (x + (fx if x >= 0 else -fx), y + (fy if y >= 0 else -fy)) for p, (x, y) in parts.items()} for parts in people]
