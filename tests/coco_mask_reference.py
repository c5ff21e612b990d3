"""NumPy / pure-Python restatement of the COCO person-mask contract (the device stage is pp_coco_masks_u8,
csrc/posepaf_segm.hip).  Test data only: the kernel is checked against it byte for byte.  It follows the published maskApi.c
(rleFrPoly, rleFrBbox, rleMerge, rleDecode) as annToMask uses it and the reference's make_mask (data/coco_masks_hdf5.py:69-107),
but it is this statement the implementation is held to, not a pycocotools run.

    vertices   X = (int)(5.0 x + 0.5), C truncation, float64 with every operation rounded on its own; the ring is closed
    edges      dense points walked literally, one per unit of max(dx, dy), in travel order; a zero-length edge gives none
    events     every consecutive pair with different u: (xd, yd) as rleFrPoly downsamples them, a = xd h + yd
    ring       pixel p = x h + y is 1 iff an odd number of events have a <= p (ring_mask); ring_mask_runs is the literal sort,
               difference and zero-run merge of the C source; ring_mask_columns keeps (x, y) apart, one parity per column
    crowd      uncompressed counts: pixel p is 1 iff it lies in an odd-indexed run
    make_mask  all = OR of the non-crowd annotations, miss = OR of those with num_keypoints <= 0, the one crowd minus what the
               non-crowd annotations BEFORE it cover; mask_miss = 255 NOT(miss OR crowd), mask_all = 255 (all OR crowd)
"""
import numpy as np


def c_int(v):
    """(int) of a double: truncation toward zero"""
    return int(v)


def ring_points(ring):
    """ring: k >= 3 (x, y) pairs -> the dense points (u, v) of rleFrPoly in travel order, as two lists of ints"""
    xy = np.asarray(ring, np.float64).reshape(-1, 2)
    k = len(xy)
    X = [c_int(np.float64(5.0) * xy[j, 0] + np.float64(0.5)) for j in range(k)]
    Y = [c_int(np.float64(5.0) * xy[j, 1] + np.float64(0.5)) for j in range(k)]
    X.append(X[0])
    Y.append(Y[0])
    us, vs = [], []
    for j in range(k):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        if dx == 0 and dy == 0:
            continue                                   # 0 / 0 in the C source; its one point's v is never read
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = np.float64(ye - ys) / np.float64(dx)
            for d in range(dx + 1):
                t = dx - d if flip else d
                us.append(t + xs)
                vs.append(c_int(np.float64(ys) + s * np.float64(t) + np.float64(0.5)))
        else:
            s = np.float64(xe - xs) / np.float64(dy)
            for d in range(dy + 1):
                t = dy - d if flip else d
                vs.append(t + ys)
                us.append(c_int(np.float64(xs) + s * np.float64(t) + np.float64(0.5)))
    return us, vs


def ring_events(ring, h, w):
    """-> the events of one ring as a list of (x, y), 0 <= x <= w - 1 and 0 <= y <= h, in the order rleFrPoly meets them"""
    us, vs = ring_points(ring)
    ev = []
    for j in range(1, len(us)):
        if us[j] == us[j - 1]:
            continue
        xd = np.float64(us[j] if us[j] < us[j - 1] else us[j] - 1)
        xd = (xd + np.float64(0.5)) / np.float64(5.0) - np.float64(0.5)
        if np.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = np.float64(min(vs[j], vs[j - 1]))
        yd = (yd + np.float64(0.5)) / np.float64(5.0) - np.float64(0.5)
        yd = np.float64(0.0) if yd < 0 else (np.float64(h) if yd > h else yd)
        ev.append((c_int(xd), c_int(np.ceil(yd))))
    return ev


def ring_mask(ring, h, w):
    """the literal linear form: pixel p = x h + y is 1 iff the number of events a = x h + y with a <= p is odd -> uint8 (h, w)"""
    a = np.array([x * h + y for x, y in ring_events(ring, h, w)], np.int64)
    counts = np.bincount(a, minlength=h * w + 1)[:h * w]
    return (np.cumsum(counts) & 1).astype(np.uint8).reshape(w, h).T.copy()


def ring_mask_runs(ring, h, w):
    """the same through rleFrPoly's own sort, difference and zero-run merge, decoded as rleDecode does -> uint8 (h, w)"""
    a = sorted([x * h + y for x, y in ring_events(ring, h, w)] + [h * w])
    p, d = 0, []
    for t in a:
        d.append(t - p)
        p = t
    b, j = [d[0]], 1
    while j < len(d):
        if d[j] > 0:
            b.append(d[j])
            j += 1
        else:
            j += 1
            if j < len(d):
                b[-1] += d[j]
                j += 1
    return rle_mask(b, h, w, pad=True)


def ring_mask_columns(ring, h, w):
    """(x, y) kept apart: pixel (x, y) is 1 iff an odd number of column x's events have y_e <= y.  -> (uint8 (h, w), every column
    holds an even number of events)"""
    t = np.zeros((w, h + 1), np.int64)
    for x, y in ring_events(ring, h, w):
        t[x, y] += 1
    even = bool((t.sum(axis=1) % 2 == 0).all())
    return (np.cumsum(t[:, :h], axis=1) & 1).astype(np.uint8).T.copy(), even


def rle_mask(counts, h, w, pad=False):
    """uncompressed counts -> uint8 (h, w): pixel p = x h + y is 1 iff it lies in an odd-indexed run.  pad: the runs may end before
    h w (rleFrPoly's do after a merge at the end); the rest is 0"""
    counts = [int(c) for c in counts]
    assert all(c >= 0 for c in counts) and (sum(counts) == h * w or (pad and sum(counts) <= h * w))
    flat = np.zeros(h * w, np.uint8)
    p = 0
    for i, c in enumerate(counts):
        if i & 1:
            flat[p:p + c] = 1
        p += c
    return flat.reshape(w, h).T.copy()


def ann_mask(ann, h, w):
    """annToMask of one annotation: the OR of its rings, or its uncompressed run-length code"""
    seg = ann["segmentation"]
    if isinstance(seg, dict):
        assert list(seg["size"]) == [h, w]
        return rle_mask(seg["counts"], h, w)
    m = np.zeros((h, w), np.uint8)
    for ring in seg:
        m |= ring_mask(ring, h, w)
    return m


def combine(anns, masks, h, w):
    """make_mask's combination (coco_masks_hdf5.py:69-107) of the annotations' 0 / 1 masks, in annotation order
    -> (mask_miss, mask_all) uint8 0 / 255.  More than one crowd raises, as the reference does."""
    mask_all, mask_miss = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    mask_crowd, flag = None, 0
    for p, m in zip(anns, masks):
        if p["iscrowd"] == 1:
            mask_crowd = m - np.bitwise_and(mask_all, m)
            flag += 1
            continue
        mask_all = np.bitwise_or(m, mask_all)
        if p["num_keypoints"] <= 0:
            mask_miss = np.bitwise_or(m, mask_miss)
    if flag > 1:
        raise ValueError("crowd segments > 1")
    if flag == 1:
        mask_miss = np.bitwise_or(mask_miss, mask_crowd)
        mask_all = np.bitwise_or(mask_all, mask_crowd)
    return (255 * (1 - mask_miss)).astype(np.uint8), (255 * mask_all).astype(np.uint8)


def make_mask(anns, h, w):
    """one image's annotations -> (mask_miss, mask_all) uint8 (h, w)"""
    return combine(anns, [ann_mask(p, h, w) for p in anns], h, w)
