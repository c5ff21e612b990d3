#!/usr/bin/env python3
"""augment_probe.py -- measurements of the device data transformer pp_augment_batch (csrc/posepaf_augment.hip) for DESIGN.md section 6.

    python tools/augment_probe.py --out profiles/r16_augment.json [--reps 15] [--batch 128]

Device events around single calls of augment.augment_device (outputs and the parameter tensor preallocated, so a call is the two
launches) after a warm-up, median (min, max) of --reps.  The shape: --batch sources of 480 x 640 (h x w) with both masks, outputs of
512 x 512, a rotation of 40 degrees about the source centre at scale ~1, 6 people per image.  Against the floor of reading every
source byte once (5 bytes per source pixel: image + two masks) and writing every output byte once, at the 8 TB/s peak DESIGN uses
for MI355X and at the 6.3 TB/s the microarchitecture notes give as achievable.  Variants: fp16 image output; the same draw without
rotation (rows of the source read in order: what the gather of a rotated read costs); no masks (the image alone).
Needs an MI355X; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "improved-body-parts_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

HBM_PEAK_GBS, HBM_ACHIEVABLE_GBS = 8000.0, 6300.0
SRC_H, SRC_W, OUT = 480, 640, 512


def median_ms(torch, fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return {"ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=128)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "augment_probe.py needs the MI355X"
    from posepaf import augment
    B, P = a.batch, 6
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(16)
    images = torch.randint(0, 256, (B, SRC_H, SRC_W, 3), dtype=torch.uint8, device=dev, generator=g)
    mask_miss = (torch.rand((B, SRC_H // 16, SRC_W // 16), device=dev, generator=g) > 0.1).to(torch.uint8).mul_(255)
    mask_all = (torch.rand((B, SRC_H // 16, SRC_W // 16), device=dev, generator=g) > 0.7).to(torch.uint8).mul_(255)
    mask_miss = mask_miss.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()      # 16 x 16 blocks
    mask_all = mask_all.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()
    rng = np.random.default_rng(17)
    joints = np.zeros((B, P, 18, 3))
    joints[..., 0], joints[..., 1], joints[..., 2] = rng.uniform(0, SRC_W, (B, P, 18)), rng.uniform(0, SRC_H, (B, P, 18)), 1.0
    joints, n_people = torch.from_numpy(joints).to(dev), torch.full((B,), P, dtype=torch.int32, device=dev)

    def params(degree):
        sel = augment.AugmentSelection(False, False, degree, (0, 0), 1.0)
        m = augment.affine_matrix(sel, (SRC_W / 2, SRC_H / 2), 0.6, OUT, OUT)[0]
        return torch.from_numpy(augment.pack_params([m] * B, [False] * B, OUT, OUT)).to(dev)
    rotated, straight = params(40.0), params(0.0)
    outs = {dt: {"image": torch.empty((B, OUT, OUT, 3), dtype=dt, device=dev), "mask_miss": torch.empty((B, OUT // 4, OUT // 4), device=dev),
                 "fg": torch.empty((B, OUT // 4, OUT // 4), device=dev), "joints": torch.empty((B, P, 18, 3), device=dev)}
            for dt in (torch.float32, torch.float16)}

    def call(par, dt, masks=True):
        return lambda: augment.augment_device(images, mask_miss if masks else None, mask_all if masks else None, None, joints, n_people, par,
                                              (OUT, OUT), dtype=dt, out=outs[dt])
    src_bytes = B * SRC_H * SRC_W * 5
    small = B * (OUT // 4) ** 2 * 8 + B * P * 18 * 3 * (8 + 4)
    out_bytes = {torch.float32: B * OUT * OUT * 12 + small, torch.float16: B * OUT * OUT * 6 + small}
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_gbs": HBM_PEAK_GBS, "hbm_achievable_gbs": HBM_ACHIEVABLE_GBS,
           "geometry": f"{B} sources of {SRC_H} x {SRC_W} uint8 with two masks, outputs {OUT} x {OUT}, rotation 40 degrees, {P} people per image",
           "source_bytes": src_bytes, "output_bytes_fp32": out_bytes[torch.float32], "output_bytes_fp16": out_bytes[torch.float16],
           "timing": f"device events around one call, median (min, max) of {a.reps} after 3 warm-up calls"}
    for name, par, dt, masks in (("rotated_fp32", rotated, torch.float32, True), ("rotated_fp16", rotated, torch.float16, True),
                                 ("straight_fp32", straight, torch.float32, True), ("rotated_fp32_no_masks", rotated, torch.float32, False)):
        r = median_ms(torch, call(par, dt, masks), a.reps)
        moved = (src_bytes if masks else src_bytes * 3 // 5) + out_bytes[dt]
        r["bytes_moved_once"] = moved
        r["floor_ms_at_8TBs"], r["floor_ms_at_6_3TBs"] = moved / HBM_PEAK_GBS / 1e6, moved / HBM_ACHIEVABLE_GBS / 1e6
        r["times_the_floor_at_8TBs"], r["times_the_floor_at_6_3TBs"] = r["ms"] / r["floor_ms_at_8TBs"], r["ms"] / r["floor_ms_at_6_3TBs"]
        r["gbs"] = moved / r["ms"] / 1e6
        r["output_pixels_per_us"] = B * OUT * OUT / r["ms"] / 1e3
        res[name] = r
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
