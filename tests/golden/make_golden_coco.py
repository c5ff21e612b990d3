#!/usr/bin/env python3
"""Generate tests/golden/coco_instances.json and coco_instances.npz from the REFERENCE's own data/coco_masks_hdf5.py (run in the build
container only).

    python tests/golden/make_golden_coco.py

What runs: process_image and make_mask of data/coco_masks_hdf5.py, imported from /root/reference with stub modules for cv2, h5py,
pycocotools and matplotlib (scipy is present for cdist).  cv2.imread returns zeros of the annotated size, and coco.annToMask returns
the masks of tests/coco_mask_reference.py: pycocotools is not installed, so the RASTERISER is not part of this fixture (its contract
is INTEGRATION section 19) -- make_mask's combination and process_image's selection are.  No reference source or bytecode is written.

The fixture is DATA:
  coco_instances.json   images (id, height, width, file_name), annotations per image in order (bbox, area, num_keypoints, iscrowd,
                        keypoints, segmentation), and per image the instances process_image yields: people_index, numOtherPeople,
                        objpos, scale_provided, joints (the reference's (17, 3) rows: x, y, 1 visible / 0 hidden / 2 absent)
  coco_instances.npz    m{i}_miss, m{i}_all uint8 (h, w): make_mask's two planes of image i
The annotations hold the stale-index case both ways (image 0: a second main person only because the side is the LAST annotation's;
image 2: a person refused for the same reason), a segmented person without keypoints, and one crowd between two persons it overlaps.
"""
import contextlib
import io
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import coco_mask_cases as cases  # noqa: E402
import coco_mask_reference as cr  # noqa: E402

SIZES = {}        # image id -> (h, w), for the cv2.imread stub


def import_reference():
    for n in ("cv2", "h5py", "pycocotools", "pycocotools.coco", "matplotlib", "matplotlib.pyplot"):
        if n not in sys.modules:
            m = types.ModuleType(n)
            m.__path__ = []
            sys.modules[n] = m
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["pycocotools.coco"].COCO = object
    sys.modules["cv2"].imread = lambda path: np.zeros(SIZES[int(os.path.basename(path).split(".")[0])] + (3,), np.uint8)
    sys.path.insert(0, os.path.join(REF, "data"))
    import coco_masks_hdf5
    sys.path.remove(os.path.join(REF, "data"))
    return coco_masks_hdf5


class StubCoco:
    def __init__(self, h, w):
        self.h, self.w = h, w

    def annToMask(self, ann):
        return cr.ann_mask(ann, self.h, self.w)


def ann(seg, bbox, area, n_kp, seed, h, w, iscrowd=0):
    return {"segmentation": seg, "bbox": bbox, "area": area, "num_keypoints": n_kp, "iscrowd": iscrowd,
            "keypoints": cases.keypoints_in(h, w, n_kp, seed) if n_kp else [0] * 51}


def fixture_annotations():
    images = [{"id": 11, "height": 64, "width": 80, "file_name": "%012d.jpg" % 11},
              {"id": 12, "height": 60, "width": 72, "file_name": "%012d.jpg" % 12},
              {"id": 13, "height": 96, "width": 128, "file_name": "%012d.jpg" % 13}]
    a0 = [ann([[5, 5, 45, 6.5, 44, 55, 6, 54]], [5, 5, 40, 50], 2000.0, 10, 1, 64, 80),
          ann([[20, 10, 50, 11, 49.5, 54, 21, 53]], [20, 10, 30, 44], 1300.0, 8, 2, 64, 80),       # 10.2 px from the first centre
          ann([[60, 40, 70, 40.5, 69, 52, 61, 51]], [60, 40, 10, 12], 100.0, 0, 3, 64, 80)]        # last: side 12, no keypoints
    c = cases.crowd(60, 72, 15, 55, 20, 60, holes=((30, 40, 30, 40),))
    a1 = [ann([[4, 4, 40, 5, 38.5, 50, 5, 48]], [4, 4, 36, 46], 1500.0, 6, 4, 60, 72),
          dict(c, bbox=[20, 15, 40, 40], area=1500.0, keypoints=[0] * 51),
          ann([[35, 20, 68, 22, 66, 58, 36.5, 57]], [35, 20, 33, 38], 1100.0, 3, 5, 60, 72)]
    a2 = [ann([[10, 10, 50, 12, 48, 80, 12, 78]], [10, 10, 40, 70], 2600.0, 12, 6, 96, 128),
          ann([[40, 12, 75, 14, 74, 70, 42, 68]], [40, 12, 35, 58], 1900.0, 9, 7, 96, 128),        # 29 px away: refused by 0.3 * 120
          ann([[2, 2, 122, 3, 120, 20, 3, 18]], [2, 2, 120, 18], 1800.0, 2, 8, 96, 128)]           # last: side 120
    return images, [a0, a1, a2]


def main():
    ref = import_reference()
    assert ref.image_size == 512
    images, anns = fixture_annotations()
    doc = {"images": images, "annotations": anns, "instances": []}
    store = {}
    with tempfile.TemporaryDirectory() as d:
        for i, (meta, img_anns) in enumerate(zip(images, anns)):
            h, w = meta["height"], meta["width"]
            SIZES[meta["id"]] = (h, w)
            open(os.path.join(d, meta["file_name"]), "w").close()
            with contextlib.redirect_stdout(io.StringIO()):
                got = list(ref.process_image(meta, meta["id"], i, img_anns, "COCO"))
                _, both = ref.make_mask(d, meta["id"], img_anns, StubCoco(h, w))
            doc["instances"].append([{"people_index": g["people_index"], "numOtherPeople": g["numOtherPeople"], "objpos": g["objpos"],
                                      "scale_provided": g["scale_provided"], "joints": g["joints"]} for g in got])
            store[f"m{i}_miss"], store[f"m{i}_all"] = both[:, :, 0].astype(np.uint8), both[:, :, 1].astype(np.uint8)
    with open(os.path.join(HERE, "coco_instances.json"), "w") as f:
        json.dump(doc, f)
    np.savez_compressed(os.path.join(HERE, "coco_instances.npz"), **store)
    print("instances per image:", [len(x) for x in doc["instances"]],
          {k: os.path.getsize(os.path.join(HERE, k)) for k in ("coco_instances.json", "coco_instances.npz")})


if __name__ == "__main__":
    main()
