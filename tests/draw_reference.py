"""Shared by tests/test_draw_records_cpu.py and tests/test_gpu_draw.py: a per-pixel restatement of utils.draw.draw_humans (the
form the HIP kernel pp_draw_humans_u8 evaluates) and builders of hand-made person records.

The restatement: utils/draw.py paints primitive after primitive inside bounding boxes, later over earlier.  Here every pixel of
the canvas asks, walking the primitives BACKWARDS, for the first one whose test holds -- no bounding box at all, only the two
tests and the canvas bounds:
    disc   (x - cx)^2 + (y - cy)^2 <= 20.25                                           (integers)
    line   u = clip(((x - ax) dx + (y - ay) dy) / den, 0, 1), u = 0 when den == 0;    (float64, one operation at a time)
           (x - (ax + u dx))^2 + (y - (ay + u dy))^2 <= 2.25
Both give the same canvas iff draw.py's boxes never cut a primitive; test_draw_records_cpu.py checks that on random people."""
import numpy as np


def primitives(humans):
    """draw order of utils.draw.draw_humans(normalized=False): per human the discs of the present parts 0..17, then the lines
    of CocoPairsRender 0..16 -> list of ("disc", (cx, cy), None, colour) / ("line", (ax, ay), (bx, by), colour)"""
    from utils import draw
    out = []
    for human in humans:
        centers = {}
        for i in range(18):
            if i in human.body_parts:
                bp = human.body_parts[i]
                centers[i] = (int(bp.x), int(bp.y))
                out.append(("disc", centers[i], None, draw.CocoColors[i]))
        for pair_order, (a, b) in enumerate(draw.CocoPairsRender):
            if a in centers and b in centers:
                out.append(("line", centers[a], centers[b], draw.CocoColors[pair_order]))
    return out


def render_last_hit(canvas, humans):
    """-> a new canvas: every pixel takes the colour of the LAST primitive in draw order whose test holds, else keeps its own"""
    h, w = canvas.shape[:2]
    out = canvas.copy()
    open_px = np.ones((h, w), bool)
    yi, xi = np.mgrid[0:h, 0:w]
    yf, xf = yi.astype(np.float64), xi.astype(np.float64)
    for kind, a, b, colour in reversed(primitives(humans)):
        if kind == "disc":
            hit = (xi - a[0]) ** 2 + (yi - a[1]) ** 2 <= 20.25
        else:
            (ax, ay), (bx, by) = a, b
            dx, dy = bx - ax, by - ay
            den = float(dx * dx + dy * dy)
            u = np.clip(((xf - ax) * dx + (yf - ay) * dy) / den, 0.0, 1.0) if den > 0 else np.zeros_like(xf)
            hit = (xf - (ax + u * dx)) ** 2 + (yf - (ay + u * dy)) ** 2 <= 2.25
        hit &= open_px
        out[hit] = colour
        open_px &= ~hit
    return out


def random_parts(rng, lo_x, hi_x, lo_y, hi_y, p_absent=0.3, p_coincident=0.15):
    """one random person as {part: (x, y)}: integer joints in [lo, hi], some parts absent, some joints on top of another"""
    parts = {}
    for p in range(18):
        if rng.random() < p_absent:
            continue
        if parts and rng.random() < p_coincident:
            parts[p] = parts[int(rng.choice(list(parts)))]
        else:
            parts[p] = (int(rng.integers(lo_x, hi_x + 1)), int(rng.integers(lo_y, hi_y + 1)))
    return parts


def make_record(people, float_coords=False):
    """list of {part: (x, y)} (at most 128) -> one numpy record (posepaf._lib.RECORD_DTYPE).  Slots beyond n_humans and the
    coordinates of absent parts hold junk on purpose: the renderers must not look at them."""
    from posepaf import _lib
    rec = np.zeros((), _lib.RECORD_DTYPE)
    junk = np.random.default_rng(len(people)).integers(-2 ** 31, 2 ** 31 - 1, (128, 18), dtype=np.int64).astype(np.int32)
    rec["humans"]["x"], rec["humans"]["y"] = junk, junk[::-1]
    rec["humans"]["peak_id"] = 7                      # stale people beyond n_humans look alive
    rec["n_humans"] = len(people)
    rec["status"] = _lib.ST_FLOAT_COORDS if float_coords else 0
    for k, parts in enumerate(people):
        hm = rec["humans"][k]
        hm["peak_id"] = -1
        for p, (x, y) in parts.items():
            hm["peak_id"][p] = 18 * k + p
            if float_coords:
                hm["x"][p], hm["y"][p] = np.float32(x).view(np.int32), np.float32(y).view(np.int32)
            else:
                hm["x"][p], hm["y"][p] = x, y
            hm["part_score"][p] = 0.25 + p / 32
        hm["n_parts"] = len(parts)
        hm["score"] = 0.5 + k / 256
    return rec
