#!/usr/bin/env python3
"""Cost of keeping the feature maps in device memory (HIP events via pp_time_kernels / pp_time_map_prepass); GPU only.

  A/B   128 x 128 fp16, B = 128: PP_MAPS_AUTO (maps staged in LDS) against PP_MAPS_HBM on a shape both paths take
  large 272 x 480 fp16, B = 32 (a padded Full-HD frame), the large-map path alone: microseconds per launch of the three
        kernels and achieved bytes/s against the algorithmic bytes (every input byte once; the pre-pass
        also writes, and K_A / K_B read, the 48 flip-averaged planes)

Each figure is the median of `--reps` repetitions of `--iters` back-to-back launches after an untimed pass.  One JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "improved-body-parts_amd")]


def measure(post, dev, img_h, iters, reps):
    rows = []
    for _ in range(reps):
        ms = post.time_kernels(dev, img_h, True, iters=iters)
        ms["k_flip_average_maps"] = post.time_map_prepass(dev, True, iters=iters)
        rows.append(ms)
    return {k: {"median_us": 1e3 * statistics.median(r[k] for r in rows), "min_us": 1e3 * min(r[k] for r in rows),
                "max_us": 1e3 * max(r[k] for r in rows)} for k in rows[0]}


def main():
    import numpy as np
    import torch
    from posepaf import synth
    from posepaf.api import PosePostProcessor
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    people = (1, 2, 3, 4, 5, 6, 8, 10, 12, 15, 20, 30, 2, 4, 6, 3)                  # bench.py's mix
    out = {"iters": a.iters, "reps": a.reps, "device": torch.cuda.get_device_name(0)}

    B = 128
    post = PosePostProcessor(max_batch=B, max_h=128, max_w=128, max_peaks_per_part=64)
    dev = torch.from_numpy(np.stack([synth.make_net_output(people[i % 16], 9000 + i % 16, dtype=np.float16) for i in range(B)])).cuda()
    for mode in ("auto", "hbm"):
        post.set_map_residency(mode)
        out[f"128x128_f16_b128_{mode}"] = measure(post, dev, 512, a.iters, a.reps)
    post.close()

    B, h, w = 32, 272, 480
    post = PosePostProcessor(max_batch=B, max_h=h, max_w=w, max_peaks_per_part=64)
    scenes = [synth.make_net_output(people[i % 16], 9100 + i, h=h, w=w, dtype=np.float16) for i in range(8)]
    dev = torch.from_numpy(np.stack([scenes[i % 8] for i in range(B)])).cuda()
    res = measure(post, dev, 4 * h, a.iters, a.reps)
    plane = h * w * 2
    algo = {"k_flip_average_maps": B * 48 * plane * 3,       # two samples read, one plane written
            "k_heat_peaks": B * 18 * plane,                  # every part plane once
            "k_limb_connect": B * 30 * plane,                # upper bound: a limb plane is only sampled along candidate pairs
            "chain": B * 48 * plane * 4}
    for k, v in algo.items():
        res[k]["algorithmic_bytes"] = v
        res[k]["achieved_GBps"] = v / (res[k]["median_us"] * 1e-6) / 1e9
    out["272x480_f16_b32_hbm"] = res
    post.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
