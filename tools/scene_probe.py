#!/usr/bin/env python3
"""scene_probe.py -- measurements of the device scene renderer pp_render_scenes (csrc/posepaf_synth.hip) for DESIGN.md section 6.

    python tools/scene_probe.py --out profiles/r12_scenes.json [--reps 25] [--host-scenes 16]

Device events around single launches after a warm-up, median (min, max) of --reps, fp16, two samples:
  * the bench shape: 128 images of 128 x 128 maps, bench.py's people mix (SCENE_PEOPLE, cycled over the images), without and with
    noise; also fp32 and a single sample;
  * 32 images of 272 x 480 maps (a 1088 x 1920 image), the same mix scaled to that frame;
  * each against the floor of storing the output bytes once (the bytes / 8 TB/s of MI355X_MICROARCH.md, and a measured
    torch fill of the same tensor), and against the host renderer's seconds for the same scenes (synth.render_maps +
    mirror_sample on --host-scenes of them, one core, scaled to the batch);
  * the first image of each timed output is checked against the host renderer (1e-3: fp16).
Needs an MI355X; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "improved-body-parts_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0
SCENE_PEOPLE = (1, 2, 3, 4, 5, 6, 8, 10, 12, 15, 20, 30, 2, 4, 6, 3)   # bench.py's people per synthetic scene


def median_ms(torch, fn, reps, warm=5):
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


def shape_part(torch, batch, h, w, reps, host_scenes):
    from posepaf import synth, synth_device
    people = [synth.random_people(SCENE_PEOPLE[i % len(SCENE_PEOPLE)], np.random.default_rng(9000 + i), img_h=4 * h, img_w=4 * w)
              for i in range(batch)]
    mp = max(SCENE_PEOPLE)
    joints, n = synth_device.pack_joints(people, mp)
    joints, n = torch.from_numpy(joints).cuda(), torch.from_numpy(n).cuda()
    ids = torch.arange(batch, dtype=torch.int64, device="cuda")
    out16 = torch.empty((batch, 2, 50, h, w), dtype=torch.float16, device="cuda")
    nbytes = out16.numel() * 2
    res = {"geometry": f"{batch} x 2 x 50 x {h} x {w}", "output_bytes_fp16": nbytes, "people_per_image": f"bench mix, mean {np.mean(SCENE_PEOPLE):.1f}",
           "max_people": mp, "floor_ms_at_8TBs": nbytes / HBM_PEAK_GBS / 1e6,
           "timing": f"device events around one launch, median (min, max) of {reps} after 5 warm-up launches"}
    res["torch_fill_same_tensor"] = median_ms(torch, lambda: out16.fill_(0.5), reps)

    def run(**kw):
        return lambda: synth_device.render_scenes(joints, n, h, w, scene_ids=ids, seed=7, **kw)
    res["fp16_flip"] = median_ms(torch, run(out=out16), reps)
    first = out16[0].float().cpu().numpy()
    res["fp16_flip_noise"] = median_ms(torch, run(out=out16, noise=0.02), reps)
    out1 = torch.empty((batch, 1, 50, h, w), dtype=torch.float16, device="cuda")
    res["fp16_single_sample"] = median_ms(torch, run(out=out1, flip=False), reps)
    del out1
    out32 = torch.empty((batch, 2, 50, h, w), dtype=torch.float32, device="cuda")
    res["fp32_flip"] = median_ms(torch, run(out=out32, dtype=torch.float32), reps)
    del out32
    for k in ("fp16_flip", "fp16_flip_noise"):
        res[k]["times_the_8TBs_floor"] = res[k]["ms"] / res["floor_ms_at_8TBs"]
        res[k]["times_the_fill"] = res[k]["ms"] / res["torch_fill_same_tensor"]["ms"]
        res[k]["gbs_stored"] = nbytes / res[k]["ms"] / 1e6
    # the host renderer on the same scenes
    k = min(host_scenes, batch)
    t0 = time.perf_counter()
    host = []
    for pj in people[:k]:
        base = synth.render_maps(pj, h, w)
        host.append(np.stack([base, synth.mirror_sample(base)]).astype(np.float16))
    sec = (time.perf_counter() - t0) / k
    res["host_renderer"] = {"scenes_timed": k, "seconds_per_scene_one_core": sec, "seconds_per_batch_one_core": sec * batch,
                            "times_the_kernel": sec * batch * 1e3 / res["fp16_flip"]["ms"]}
    res["first_image_max_abs_diff_to_host_fp16"] = float(np.abs(first - host[0].astype(np.float32)).max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--host-scenes", type=int, default=16)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "scene_probe.py needs the MI355X"
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_gbs": HBM_PEAK_GBS,
           "bench_shape": shape_part(torch, 128, 128, 128, a.reps, a.host_scenes),
           "maps_272x480_x32": shape_part(torch, 32, 272, 480, a.reps, max(2, a.host_scenes // 4))}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
