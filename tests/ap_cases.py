"""Inputs of the keypoint-evaluation tests (tests/test_oks_ranges_cpu.py, tests/test_gpu_ap_device.py): pp_record arrays
fabricated on the host, the ground truth that goes with them, and the host-side expectations, each computed once."""
import functools

import numpy as np

from posepaf import coco, oks_eval as oe, skeleton as sk
from posepaf._lib import MAX_HUMANS, RECORD_DTYPE

SEED, SEEDED_BATCH = 20240611, 64
MARGIN = 1e-9
FIXED_COUNTS = {0: (3, 0), 1: (0, 4), 2: (8, 25), 3: (0, 0)}    # (people, detections) of the seeded images that pin the extremes


def make_record(dets, float_coords=False, n_humans=None):
    """dets: list of (xy (17, 2) numbers in COCO order, present (17,) bool, score) -> one pp_record; the humans take the first
    len(dets) slots.  float_coords: x / y are stored as float32 bit patterns (PP_ST_FLOAT_COORDS)."""
    rec = np.zeros((), RECORD_DTYPE)
    rec["humans"]["peak_id"][:] = -1
    assert len(dets) <= MAX_HUMANS
    pid = 0
    for h, (xy, present, score) in enumerate(dets):
        hm = rec["humans"][h]
        for k, part in enumerate(sk.ORDER_COCO):
            if not present[k]:
                continue
            hm["peak_id"][part] = pid
            pid += 1
            if float_coords:
                hm["x"][part] = np.float32(xy[k][0]).view(np.int32)
                hm["y"][part] = np.float32(xy[k][1]).view(np.int32)
            else:
                hm["x"][part], hm["y"][part] = int(xy[k][0]), int(xy[k][1])
            hm["part_score"][part] = 0.5
        hm["score"] = np.float32(score)
        hm["n_parts"] = int(np.sum(present))
    rec["n_humans"] = len(dets) if n_humans is None else n_humans
    rec["n_peaks"] = pid
    if float_coords:
        rec["status"] = 32
    return rec


def host_rows(rec):
    """coco.humans_from_record + coco.coco_results of one record -> (n, 52) float64 rows; as evaluate.py, a PP_ST_FLOAT_COORDS
    record is rounded with np.rint first and n_humans beyond the record's capacity means its capacity."""
    rec = rec.copy()
    rec["n_humans"] = min(max(int(rec["n_humans"]), 0), MAX_HUMANS)
    if int(rec["status"]) & 32:
        fx, fy = rec["humans"]["x"].view(np.float32), rec["humans"]["y"].view(np.float32)
        rec["humans"]["x"], rec["humans"]["y"] = np.rint(fx).astype(np.int32), np.rint(fy).astype(np.int32)
    res = coco.coco_results(0, coco.humans_from_record(rec))
    return np.array([list(r["keypoints"]) + [r["score"]] for r in res], np.float64).reshape(len(res), 52)


def dts_of_record(rec):
    return [{"keypoints": list(r[:51]), "score": float(r[51])} for r in host_rows(rec)]


def gt_ann(xy, v, area, bbox=None, iscrowd=0, num_keypoints=None):
    kp = np.zeros((17, 3))
    kp[:, :2], kp[:, 2] = xy, v
    g = {"keypoints": kp.reshape(-1).tolist(), "area": float(area), "num_keypoints": int(np.sum(np.asarray(v) > 0)) if num_keypoints is None else num_keypoints,
         "iscrowd": iscrowd}
    if bbox is not None:
        g["bbox"] = [float(t) for t in bbox]
    return g


def grid_pose(x0, y0, step=6):
    """17 integer keypoints on a slanted line starting at (x0, y0)"""
    k = np.arange(17)
    return np.stack([x0 + k * step, y0 + k * (step // 2)], axis=1).astype(np.float64)


def _random_image(rng, n_people=None, n_dets=None):
    """0-8 people with continuous coordinates, 0-25 integer detections around them or anywhere"""
    gts = []
    for _ in range(int(rng.integers(0, 9)) if n_people is None else n_people):
        size = float(np.exp(rng.uniform(np.log(18.0), np.log(320.0))))     # areas below 32^2, medium and large all occur
        cx, cy = rng.uniform(40, 600, 2)
        xy = np.stack([cx + rng.uniform(-0.5, 0.5, 17) * size, cy + rng.uniform(-0.5, 0.5, 17) * size], axis=1)
        if gts and gts[-1]["num_keypoints"] > 0 and rng.uniform() < 0.35:   # a near twin of the previous person: the two compete
            prev = np.asarray(gts[-1]["keypoints"]).reshape(17, 3)[:, :2]
            size = float(np.sqrt(gts[-1]["area"]))
            xy = prev + rng.normal(0, 0.03, (17, 2)) * size
        v = rng.choice([0, 1, 2], 17, p=[0.2, 0.2, 0.6])
        kind = rng.uniform()
        x0, y0 = xy.min(axis=0)
        w, h = xy.max(axis=0) - xy.min(axis=0)
        area = w * h * rng.uniform(0.4, 0.9)
        if kind < 0.12:       # no labelled keypoint: ignored, OKS from the doubled box.  A small box: a detection with all
            # 17 joints inside the doubled box would have an OKS of exactly 1, without a margin to 1 - 1e-10
            w, h = rng.uniform(6, 14, 2)
            area = w * h * rng.uniform(0.4, 0.9)
            gts.append(gt_ann(np.zeros((17, 2)), np.zeros(17), area, (x0, y0, w, h), 0, 0))
        elif kind < 0.24:     # crowd region
            gts.append(gt_ann(xy, v, area, (x0, y0, w, h), 1))
        else:
            if not (v > 0).any():
                v[int(rng.integers(0, 17))] = 2
            gts.append(gt_ann(xy, v, area, (x0, y0, w, h)))
    dets = []
    for _ in range(int(rng.integers(0, 26)) if n_dets is None else n_dets):
        if gts and rng.uniform() < 0.75:
            g = gts[int(rng.integers(0, len(gts)))]
            kp = np.asarray(g["keypoints"]).reshape(17, 3)
            if g["num_keypoints"] == 0:
                bx, by, bw, bh = g["bbox"]
                # around the doubled box, some joints outside it (all inside would be an OKS of exactly 1, no margin to 1 - 1e-10)
                xy = np.stack([rng.uniform(bx - 1.4 * bw, bx + 2.4 * bw, 17), rng.uniform(by - 1.4 * bh, by + 2.4 * bh, 17)], axis=1)
            else:
                xy = kp[:, :2] + rng.normal(0, 0.04, (17, 2)) * np.sqrt(g["area"]) * rng.uniform(0.2, 3.0)
        else:
            xy = rng.uniform(0, 640, (17, 2))
        xy = np.clip(np.rint(xy), 1, 2000)
        present = rng.uniform(size=17) < 0.85
        present[int(rng.integers(0, 17))] = True
        dets.append((xy, present, np.float32(rng.uniform(0.05, 1.0))))
    return make_record(dets), gts


@functools.lru_cache(maxsize=None)
def seeded_cases():
    """-> (records (64,), gts {image id: annotations}, dts {image id: detections}), image ids 0..63"""
    rng = np.random.default_rng(SEED)
    recs, gts = np.zeros(SEEDED_BATCH, RECORD_DTYPE), {}
    for i in range(SEEDED_BATCH):
        recs[i], gts[i] = _random_image(rng, *FIXED_COUNTS.get(i, (None, None)))
    recs.setflags(write=False)
    dts = {i: dts_of_record(recs[i]) for i in range(SEEDED_BATCH)}
    return recs, gts, dts


@functools.lru_cache(maxsize=None)
def hand_cases():
    """-> (records, gts, dts): one image per rule that can go wrong"""
    P = grid_pose
    full = np.ones(17, bool)
    v2 = np.full(17, 2)
    images = []
    # 0: equal scores keep record order; the first of two identical detections gets the ground truth
    images.append(([(P(100, 100), full, 0.5), (P(100, 100), full, 0.5), (P(400, 300), full, 0.5), (P(101, 100), full, 0.75)],
                   [gt_ann(P(100, 100), v2, 96 * 48, (100, 100, 96, 48))]))
    # 1: a crowd region absorbs three detections; a real person next to it
    images.append(([(P(300, 300), full, 0.9), (P(300, 300), full, 0.8), (P(301, 300), full, 0.7), (P(100, 100), full, 0.6)],
                   [gt_ann(P(300, 300), v2, 9000.0, (300, 300, 96, 48), 1), gt_ann(P(100, 100), v2, 5000.0, (100, 100, 96, 48))]))
    # 2: num_keypoints == 0 with a box: the doubled-box branch (inside: OKS 1; far outside: 0), and one without a box (OKS 0)
    images.append(([(P(300, 300), full, 0.9), (P(1300, 300), full, 0.8), (P(100, 100), full, 0.7)],
                   [gt_ann(np.zeros((17, 2)), np.zeros(17), 4608.0, (300, 300, 96, 48), 0, 0),
                    gt_ann(np.zeros((17, 2)), np.zeros(17), 4608.0, None, 0, 0), gt_ann(P(100, 100), v2, 5000.0, (100, 100, 96, 48))]))
    # 3: 128 ground truths, each with its own detection (scores descending along the record)
    many = [P(10 + 7 * (g % 16), 10 + 60 * (g // 16), 4) for g in range(128)]
    images.append(([(many[g], full, 1.0 - g / 256.0) for g in range(0, 128, 5)],
                   [gt_ann(many[g], v2, 2000.0 + g, (many[g][0, 0], many[g][0, 1], 64, 32)) for g in range(128)]))
    # 4: detections and no ground truth; 5: the reverse
    images.append(([(P(100, 100), full, 0.9), (P(10, 10, 2), full, 0.4)], []))
    images.append(([], [gt_ann(P(100, 100), v2, 5000.0, (100, 100, 96, 48))]))
    # 6: areas exactly on the range ends; an unmatched detection outside `large`, a matched one outside `medium`
    small_det = (P(500, 20, 2), full, 0.3)          # box 32 x 16 = 512 < 32^2, far from everyone
    images.append(([(P(100, 100), full, 0.9), (P(100, 300), full, 0.8), small_det],
                   [gt_ann(P(100, 100), v2, 32.0 ** 2, (100, 100, 96, 48)), gt_ann(P(100, 300), v2, 96.0 ** 2, (100, 300, 96, 48))]))
    recs = np.zeros(len(images), RECORD_DTYPE)
    gts = {}
    for i, (dets, g) in enumerate(images):
        recs[i], gts[i] = make_record(dets), g
    recs.setflags(write=False)
    return recs, gts, {i: dts_of_record(recs[i]) for i in range(len(images))}


@functools.lru_cache(maxsize=None)
def stage_a(which):
    """host stage A of every image of seeded_cases / hand_cases, computed once and shared"""
    recs, gts, dts = seeded_cases() if which == "seeded" else hand_cases()
    return [oe.match_image(gts[i], dts[i]) for i in range(len(recs))]
