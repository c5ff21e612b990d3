#!/usr/bin/env python3
"""limbs_probe.py -- measurements of the device renderer of the demo's original style, pp_draw_limbs_u8
(csrc/posepaf_limbs.hip), for DESIGN.md section 6.

    python tools/limbs_probe.py --out profiles/r11_draw_limbs.json [--batch 128]

At the bench geometry (128 images of 512 x 512) with bench.py's people mix (SCENE_PEOPLE, cycled over the images;
synth.random_people, integer joints).  HIP events around 20 back-to-back launches; one untimed pass first, then the median
(min, max) of 5 repetitions, reported per launch:
  * pp_draw_limbs_u8, two-buffer form and in place;
  * pp_draw_humans_u8 on the same records;
  * dst.copy_(src) of the same buffers: one read plus one write of the canvases at the HBM rate this device reaches -- the
    floor of the two-buffer form;
  * the canvas is checked against the NumPy renderer on a sample of images, whose host time per image is the baseline the
    kernel replaces.
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

IMG = 512
LAUNCHES, REPS = 20, 5


def records_for(batch, seed=11_000):
    from bench import SCENE_PEOPLE
    from posepaf import _lib, synth
    recs = np.zeros(batch, _lib.RECORD_DTYPE)
    for b in range(batch):
        people = SCENE_PEOPLE[b % len(SCENE_PEOPLE)]
        joints = synth.random_people(people, np.random.default_rng(seed + b), IMG, IMG)
        recs[b]["n_humans"] = people
        recs[b]["humans"]["peak_id"] = -1
        for k in range(people):
            present = joints[k, :, 2] == 1
            hm = recs[b]["humans"][k]
            hm["peak_id"] = np.where(present, np.arange(18) + 18 * k, -1)
            hm["x"], hm["y"] = joints[k, :, 0].astype(np.int32), joints[k, :, 1].astype(np.int32)
            hm["n_parts"], hm["score"] = int(present.sum()), 1.0
    return recs


def per_launch_us(torch, fn):
    """one untimed pass, then REPS timed passes of LAUNCHES launches each -> (median, min, max) microseconds per launch"""
    for _ in range(LAUNCHES):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    return {"median_us": statistics.median(out), "min_us": min(out), "max_us": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=128)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "limbs_probe.py needs an MI355X"
    from bench import SCENE_PEOPLE
    from posepaf.render import draw_limbs_record_numpy, draw_limbs_records, draw_records, limb_angle_table_dev
    batch = a.batch
    src = torch.randint(0, 256, (batch, IMG, IMG, 3), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    recs = records_for(batch)
    rec_dev = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
    limb_angle_table_dev("cuda")
    alg = 2 * batch * IMG * IMG * 3
    out = {"device": torch.cuda.get_device_name(0), "geometry": f"{batch} x {IMG} x {IMG} x 3 uint8",
           "people_per_image": f"bench.py SCENE_PEOPLE {list(SCENE_PEOPLE)}, cycled (mean {sum(SCENE_PEOPLE) / len(SCENE_PEOPLE):.1f})",
           "limb_instances_in_the_batch": int(sum(len(_instances(recs[b])) for b in range(batch))),
           "timing": f"HIP events around {LAUNCHES} launches, one untimed pass, then median (min, max) of {REPS} passes, per launch",
           "algorithmic_bytes_two_buffers": alg}
    copy = per_launch_us(torch, lambda: dst.copy_(src))
    copy["gbs"] = alg / copy["median_us"] / 1e3
    out["copy_dst_from_src"] = copy
    limbs = per_launch_us(torch, lambda: draw_limbs_records(src, rec_dev, None, out=dst))
    got = dst.cpu().numpy()
    limbs["times_the_copy"] = limbs["median_us"] / copy["median_us"]
    limbs["gbs_algorithmic"] = alg / limbs["median_us"] / 1e3
    out["pp_draw_limbs_u8"] = limbs
    work = src.clone()
    out["pp_draw_limbs_u8_in_place"] = per_launch_us(torch, lambda: draw_limbs_records(work, rec_dev, None, out=work))
    out["pp_draw_humans_u8_same_records"] = per_launch_us(torch, lambda: draw_records(src, rec_dev, None, out=dst))
    src_host = src.cpu().numpy()
    sample = list(range(min(batch, len(SCENE_PEOPLE))))           # one cycle of the people mix
    t0 = time.perf_counter()
    want = [draw_limbs_record_numpy(src_host[b], recs[b]) for b in sample]
    numpy_ms = (time.perf_counter() - t0) / len(sample) * 1e3
    out["numpy_draw_limbs_record_ms_per_image_one_core"] = numpy_ms
    out["numpy_ms_per_batch_one_core"] = numpy_ms * batch
    out[f"equal_to_numpy_on_{len(sample)}_images"] = bool(all(np.array_equal(got[b], w) for b, w in zip(sample, want)))
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


def _instances(rec):
    from posepaf import skeleton as sk
    ids = rec["humans"]["peak_id"][:int(rec["n_humans"])]
    return [(t, h) for t, i in enumerate(sk.DRAW_LIST) for h in range(len(ids))
            if ids[h][sk.LIMB_PAIRS[i][0]] >= 0 and ids[h][sk.LIMB_PAIRS[i][1]] >= 0]


if __name__ == "__main__":
    main()
