#!/usr/bin/env python3
"""coco_mask_probe.py -- measurements of the device mask rasteriser pp_coco_masks_u8 (csrc/posepaf_segm.hip) for DESIGN.md section 6.

    python tools/coco_mask_probe.py --out profiles/r19_coco_masks.json [--reps 15] [--batch 128]

Device events around single calls of coco_masks.masks_device (tables on the device, outputs and workspace preallocated, so a call is
the two launches) after a warm-up, median (min, max) of --reps.  The shape: --batch images of 480 x 640 with 8 people of one ring of
40 vertices each (a wobbling circle of radius 40..120 px around a centre anywhere in the frame, so rings leave the frame), every
fourth person without keypoints and a crowd rectangle in every second image.  Against the floor of writing both planes once, at the
8 TB/s peak DESIGN uses for MI355X and at the 6.3 TB/s the microarchitecture notes give as achievable, and against the pure-Python /
NumPy restatement (tests/coco_mask_reference.py) on the first --ref_images images of the same batch (which the device output must equal).
Needs an MI355X; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "improved-body-parts_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

HBM_PEAK_GBS, HBM_ACHIEVABLE_GBS = 8000.0, 6300.0
H, W, PEOPLE, VERTS = 480, 640, 8, 40


def annotations(batch, seed=19):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(batch):
        anns = []
        for p in range(PEOPLE):
            cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(40, 120)
            t = 2 * np.pi * np.arange(VERTS) / VERTS
            rad = r * (1 + 0.3 * rng.uniform(-1, 1, VERTS))
            ring = np.stack([cx + rad * np.cos(t), cy + rad * np.sin(t)], axis=1).round(2).reshape(-1).tolist()
            anns.append({"segmentation": [ring], "iscrowd": 0, "num_keypoints": 0 if p % 4 == 3 else 10})
        if i % 2:
            m = np.zeros((H, W), np.uint8)
            y, x = int(rng.integers(0, H - 100)), int(rng.integers(0, W - 150))
            m[y:y + 100, x:x + 150] = 1
            flat = m.T.reshape(-1)
            edges = np.flatnonzero(np.diff(flat)) + 1
            counts = np.diff(np.concatenate([[0], edges, [len(flat)]])).tolist()
            anns.insert(4, {"segmentation": {"size": [H, W], "counts": counts}, "iscrowd": 1, "num_keypoints": 0})
        out.append(anns)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--ref_images", type=int, default=4)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "coco_mask_probe.py needs the MI355X"
    import coco_mask_reference as cr
    from posepaf import coco_masks
    B = a.batch
    dev = torch.device("cuda", 0)
    anns = annotations(B)
    t0 = time.perf_counter()
    host = coco_masks.pack_segmentations(anns, [(H, W)] * B)
    pack_ms = (time.perf_counter() - t0) * 1e3
    packed = coco_masks.to_device(host, dev)
    out = tuple(torch.empty((B, H, W), dtype=torch.uint8, device=dev) for _ in range(2))
    work = torch.empty(coco_masks.workspace_bytes(len(host["verts"])), dtype=torch.uint8, device=dev)

    def call():
        coco_masks.masks_device(packed, (H, W), out=out, workspace=work)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = statistics.median(times)
    n_ref = min(a.ref_images, B)
    t0 = time.perf_counter()
    want = [cr.make_mask(anns[i], H, W) for i in range(n_ref)]
    ref_ms = (time.perf_counter() - t0) * 1e3 / n_ref
    got = (out[0][:n_ref].cpu().numpy(), out[1][:n_ref].cpu().numpy())
    equal = all(np.array_equal(got[0][i], want[i][0]) and np.array_equal(got[1][i], want[i][1]) for i in range(n_ref))
    written = 2 * B * H * W
    table_bytes = sum(int(v.nbytes) for v in host.values())
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_gbs": HBM_PEAK_GBS, "hbm_achievable_gbs": HBM_ACHIEVABLE_GBS,
           "geometry": f"{B} images of {H} x {W}, {PEOPLE} people of one ring of {VERTS} vertices, a crowd in every second image",
           "timing": f"device events around one call, median (min, max) of {a.reps} after 3 warm-up calls",
           "ms": ms, "min_ms": min(times), "max_ms": max(times), "bytes_written": written, "table_bytes_per_batch": table_bytes,
           "floor_ms_at_8TBs": written / HBM_PEAK_GBS / 1e6, "floor_ms_at_6_3TBs": written / HBM_ACHIEVABLE_GBS / 1e6,
           "times_the_floor_at_8TBs": ms / (written / HBM_PEAK_GBS / 1e6), "times_the_floor_at_6_3TBs": ms / (written / HBM_ACHIEVABLE_GBS / 1e6),
           "gbs": written / ms / 1e6, "images_per_ms": B / ms, "host_pack_ms_per_batch": pack_ms,
           "restatement_ms_per_image": ref_ms, "restatement_images": n_ref, "device_equals_restatement": bool(equal),
           "times_faster_than_restatement_per_image": ref_ms / (ms / B)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    assert equal, "the device masks differ from the restatement"


if __name__ == "__main__":
    main()
