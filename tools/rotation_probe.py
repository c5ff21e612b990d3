#!/usr/bin/env python3
"""Timing probe (GPU) of the test-time rotation search on the original path, at 512 x 512, batch 32, scales 0.5 / 1 / 1.5:

  * the one-launch accumulation unrotated (3 entries, k_accumulate_scales), with angles {0, 15} (6 entries,
    k_accumulate_scales_affine) and the same 6 entries through the per-entry chain (pp_original_accumulate[_affine]);
  * pp_preprocess_u8_affine against pp_preprocess_u8 on the scale-1 batch.

HIP events on the launch stream, after 2 warm-up iterations.  Prints one JSON line (and writes it to --out when given).

    python tools/rotation_probe.py [--iters 10] [--out profiles/r04_rotation_accumulate_b32.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "improved-body-parts_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from posepaf.api import PosePostProcessor
    from posepaf.original_path import OriginalPathProcessor
    from posepaf.pipeline import preprocess_batch
    from posepaf.rotation import input_and_map_inverses

    B, IMG, scales, angles = 32, 512, (0.5, 1.0, 1.5), (0.0, 15.0)
    g = torch.Generator(device="cuda").manual_seed(0)
    maps = {s: (torch.rand((B, 2, 50, int(IMG * s) // 4, int(IMG * s) // 4), generator=g, device="cuda") * 0.8).half()
            for s in scales}
    post = PosePostProcessor(max_batch=B, max_h=192, max_w=192, max_peaks_per_part=64)
    proc = OriginalPathProcessor(post, IMG, IMG, B)

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for k in range(a.iters + 2):
            if k == 2:
                ev[0].record()
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / a.iters

    def accumulate(entries, fused):
        def fn():
            proc.fused = fused
            proc.reset()
            for s, ang in entries:
                proc.accumulate(maps[s], 0, 0, len(entries), m_inv=input_and_map_inverses(int(IMG * s), int(IMG * s), ang)[1])
            proc._flush()
        return fn

    plain = [(s, 0.0) for s in scales]
    rotated = [(s, ang) for s in scales for ang in angles]
    res = {"probe": "rotation_search", "batch": B, "image": [IMG, IMG], "scales": list(scales), "angles": list(angles),
           "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    ms = {"fused_unrotated_3": timed(accumulate(plain, True)),
          "fused_rotated_6": timed(accumulate(rotated, True)),
          "chain_rotated_6": timed(accumulate(rotated, False))}
    imgs = torch.randint(0, 256, (B, IMG, IMG, 3), dtype=torch.uint8, device="cuda", generator=g)
    m_in = input_and_map_inverses(IMG, IMG, 15.0)[0]
    ms["preprocess_u8"] = timed(lambda: preprocess_batch(imgs, True, torch.float16))
    ms["preprocess_u8_affine"] = timed(lambda: preprocess_batch(imgs, True, torch.float16, m_inv=m_in))
    res["ms"] = ms
    res["fused_over_chain_speedup"] = ms["chain_rotated_6"] / ms["fused_rotated_6"]
    post.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
