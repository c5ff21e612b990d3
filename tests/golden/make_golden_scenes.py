#!/usr/bin/env python3
"""Generate tests/golden/scene_*.npz from the REFERENCE's own training-target code (run in the build container only).

    python tests/golden/make_golden_scenes.py

What runs: py_cocodata_server/py_data_heatmapper.py Heatmapper.put_joints + put_limbs + np.clip(0, 1) -- create_heatmaps without
its two background channels (cv2.erode of a segmentation mask, which the scenes here do not have) -- imported from
/root/reference with empty stub modules for cv2 and matplotlib, which those functions never touch.  The config object is the
reference's GetConfig("Canonical") with width / height / parts_shape set for the shape at hand before the Heatmapper caches its
grids.  No reference source or bytecode is written anywhere.

The fixtures are DATA: joints in, the 48 limb + keypoint channels out.
  scene_heatmap_test_128x128.npz   the joints of the reference's own heatmap_test.npz (2 people, one far outside the frame)
  scene_edge_16x24.npz, scene_edge_33x47.npz   tests/scene_cases.py edge_people: borders, ties, skips, coincident limbs
maps are float32 (h, w, 48 -> stored planar (48, h, w)); the 128 x 128 one is stored as float16 only if its compressed float32
form would pass the size the other fixtures keep to (600 kB).
"""
import contextlib
import io
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
PKG = os.path.join(ROOT, "improved-body-parts_amd")
SIZE_LIMIT = 600_000

import numpy as np  # noqa: E402


def import_heatmapper():
    for n in ("cv2", "matplotlib", "matplotlib.pyplot"):
        if n not in sys.modules:
            m = types.ModuleType(n)
            m.__path__ = []
            sys.modules[n] = m
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.path.insert(0, REF)
    from config.config import GetConfig
    from py_cocodata_server.py_data_heatmapper import Heatmapper
    sys.path.remove(REF)
    for n in [n for n in sys.modules if n == "config" or n.startswith("config.")]:
        del sys.modules[n]                       # the product package has a config/ of its own
    return GetConfig, Heatmapper


def reference_maps(GetConfig, Heatmapper, joints, h, w):
    with contextlib.redirect_stdout(io.StringIO()):   # GetConfig prints its layer table
        cfg = GetConfig("Canonical")
    cfg.width, cfg.height = 4 * w, 4 * h
    cfg.parts_shape = (h, w, cfg.num_layers)
    hm = Heatmapper(cfg)
    maps = np.zeros(cfg.parts_shape, dtype=np.float32)
    with contextlib.redirect_stdout(io.StringIO()):   # "Parts are too close to each other" for the zero-length limb
        hm.put_joints(maps, joints)
        hm.put_limbs(maps, joints)
    maps = np.clip(maps, 0.0, 1.0)
    assert cfg.paf_start == 0 and cfg.heat_start == 30 and cfg.paf_layers == 30 and cfg.num_parts == 18
    return np.ascontiguousarray(maps.transpose(2, 0, 1)[:48])


def main():
    GetConfig, Heatmapper = import_heatmapper()
    sys.path.insert(0, PKG)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scene_cases
    cases = {"heatmap_test_128x128": (np.load(os.path.join(REF, "heatmap_test.npz"))["joints"].astype(np.float32), 128, 128),
             "edge_16x24": (scene_cases.edge_people(16, 24), 16, 24),
             "edge_33x47": (scene_cases.edge_people(33, 47), 33, 47)}
    for name, (joints, h, w) in cases.items():
        maps = reference_maps(GetConfig, Heatmapper, joints, h, w)
        path = os.path.join(HERE, f"scene_{name}.npz")
        np.savez_compressed(path, joints=joints, maps=maps, h=h, w=w)
        if os.path.getsize(path) > SIZE_LIMIT:
            np.savez_compressed(path, joints=joints, maps=maps.astype(np.float16), h=h, w=w)
        print(f"{os.path.basename(path)}: {joints.shape[0]} people, {h}x{w}, {np.load(path)['maps'].dtype}, "
              f"{os.path.getsize(path)} bytes, max {maps.max():.6f}, nonzero {np.count_nonzero(maps)}")


if __name__ == "__main__":
    main()
