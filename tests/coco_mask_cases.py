"""Annotation fixtures shared by the COCO mask tests: rings that exercise every branch of the rasteriser, crowd run-length codes and
a small annotation file with images.  Test data only."""
import json
import os

import numpy as np


def rle_counts(mask):
    """0 / 1 (h, w) -> uncompressed COCO counts: runs over the column-major order, the first one of zeros"""
    flat = np.asarray(mask, np.uint8).T.reshape(-1)
    edges = np.flatnonzero(np.diff(flat)) + 1
    runs = np.diff(np.concatenate([[0], edges, [len(flat)]])).tolist()
    return runs if flat[0] == 0 else [0] + runs


def crowd(h, w, y0, y1, x0, x1, holes=()):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = 1
    for (a, b, c, d) in holes:
        m[a:b, c:d] = 0
    return {"segmentation": {"size": [h, w], "counts": rle_counts(m)}, "iscrowd": 1, "num_keypoints": 0}


def person(rings, num_keypoints):
    return {"segmentation": [list(map(float, r)) for r in rings], "iscrowd": 0, "num_keypoints": num_keypoints}


def polygon(n, cx, cy, r, phase=0.1):
    t = phase + 2 * np.pi * np.arange(n) / n
    return np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], axis=1).reshape(-1)


def zigzag(x0, x1, y_top, y_bottom, teeth):
    """teeth up and down between two rows, closed along the bottom: 2 * teeth steep edges of 5 (y_bottom - y_top) dense points each"""
    xs = np.linspace(x0, x1, 2 * teeth + 1)
    ys = np.where(np.arange(2 * teeth + 1) % 2 == 0, y_bottom, y_top)
    return np.concatenate([np.stack([xs, ys], axis=1).reshape(-1), [x1, y_bottom + 2.5, x0, y_bottom + 2.5]])


SIZES = ((37, 53), (70, 150), (64, 64))
SLOT = (96, 160)


def everything(h=70, w=150):
    """one image's annotations with every kind of ring, a crowd between persons it overlaps, and persons without keypoints"""
    return [
        person([[10.3, 5.7, 60.2, 12.9, 31.4, 50.1]], 5),                                         # a fractional triangle
        person([[70, 10, 120, 10, 120, 60, 95, 25, 70, 60]], 0),                                  # concave, no keypoints
        person([polygon(300, 100.0, 35.0, 30.0)], 3),                                             # more vertices than threads
        crowd(h, w, 20, 66, 40, 140, holes=((30, 40, 60, 80),)),                                  # overlaps earlier and later ones
        person([zigzag(5.0, 145.0, 4.0, 66.0, 8)], 7),                                            # 16 x 310 > 4 096 dense points
        person([[20, 30, 50, 30, 50, 55, 20, 55], [35.5, 40.5, 80.5, 40.5, 80.5, 68.5, 35.5, 68.5]], 0),      # two overlapping rings
        person([[-20, 10, 15, 12, 12, 30, -25.5, 33], [130, 20, 170, 25, 165, 45, 128.5, 40],      # across the left and right edges
                [60, -15, 90, -12, 85, 8.5, 62, 6], [100, 60, 125, 62, 130, 90, 98, 85]], 4),     # across the top and bottom edges
        person([[-50, 10, -20, 10, -30, 40], [160, 5, 200, 5, 180, 60], [20, -40, 60, -40, 40, -5],       # wholly outside, each side
                [20, 80, 60, 80, 40, 120]], 2),
        person([[20, 60, 50, 60, 35, 60], [90.2, 3.2, 90.2, 3.2, 90.2, 3.2]], 6),                 # zero area
        person([[-30, -30, 200, -30, 200, 2.5, -30, 2.5]], 0),                                    # a band along the top, no keypoints
    ]


def batches():
    """two batches of three images (SIZES): [[annotations of image 0, 1, 2], ...]"""
    first = [[], everything(), [crowd(64, 64, 0, 64, 10, 50)]]                                    # nothing / everything / a crowd alone
    second = [[person([[5, 5, 30.5, 8, 28, 30, 3.5, 25.5]], 9), crowd(37, 53, 10, 37, 20, 53), person([[25, 12, 50, 14, 45, 36]], 0)],
              [], [person([polygon(7, 30.0, 30.0, 25.0)], 4)]]
    return first, second


def wide(h=70, w=300):
    """an image of two column tiles: rings across the tile border at x = 256, a crowd on both sides of it"""
    return [person([[200.5, 10, 290, 20.5, 260, 65, 210, 50]], 3), person([polygon(40, 256.0, 35.0, 20.0)], 0),
            crowd(h, w, 5, 60, 240, 280), person([[250, 0, 262, 0, 262, 70, 250, 70]], 1)]


def keypoints_in(h, w, n_labelled, seed):
    rng = np.random.default_rng(seed)
    kp = np.zeros((17, 3))
    idx = rng.permutation(17)[:n_labelled]
    kp[idx, 0], kp[idx, 1], kp[idx, 2] = rng.uniform(2, w - 2, len(idx)).round(1), rng.uniform(2, h - 2, len(idx)).round(1), 2
    return kp.reshape(-1).tolist()


def write_annotation_fixture(root):
    """3 PNG images and a person_keypoints file with segmentations, one crowd and one person without keypoints
    -> (ann_file, img_dir, doc)"""
    from PIL import Image
    img_dir = os.path.join(root, "images")
    os.makedirs(img_dir, exist_ok=True)
    rng = np.random.default_rng(5)
    sizes = ((96, 128), (80, 112), (128, 96))
    images, anns, aid = [], [], 1

    def add(iid, h, w, ring, n_kp, seed, bbox, area):
        nonlocal aid
        anns.append({"id": aid, "image_id": iid, "category_id": 1, "iscrowd": 0, "segmentation": [ring], "num_keypoints": n_kp,
                     "keypoints": keypoints_in(h, w, n_kp, seed) if n_kp else [0] * 51, "bbox": bbox, "area": area})
        aid += 1
    for k, (h, w) in enumerate(sizes):
        iid = 2000 + 3 * k
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(img_dir, f"{iid:012d}.png"))
        images.append({"id": iid, "file_name": f"{iid:012d}.png", "height": h, "width": w})
        add(iid, h, w, [10.5, 8, 70, 12, 66.5, 75, 8, 70], 11, 10 * k, [8, 8, 62, 67], 3600.0)
        add(iid, h, w, [60, 30, w - 4, 28.5, w - 6, h - 5, 58, h - 8], 8, 10 * k + 1, [58, 28.5, w - 62, h - 36.5], 2500.0)
        if k == 0:
            add(iid, h, w, [30, 50, 60, 52, 55, 90, 28, 88], 0, 0, [28, 50, 32, 40], 1200.0)          # segmented, no keypoints
        if k == 1:
            c = crowd(h, w, 40, 78, 5, 60)
            anns.append(dict(c, id=aid, image_id=iid, category_id=1, keypoints=[0] * 51, bbox=[5, 40, 55, 38], area=2090.0))
            aid += 1
    doc = {"images": images, "annotations": anns, "categories": [{"id": 1, "name": "person"}]}
    ann_file = os.path.join(root, "person_keypoints_segm.json")
    with open(ann_file, "w") as f:
        json.dump(doc, f)
    return ann_file, img_dir, doc
