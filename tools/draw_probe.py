#!/usr/bin/env python3
"""draw_probe.py -- measurements of the device renderer pp_draw_humans_u8 (csrc/posepaf_draw.hip) for DESIGN.md section 6.

    python tools/draw_probe.py --out profiles/r08_draw.json [--batch 128] [--reps 25] [--no-engine]

At the bench geometry (128 images of 512 x 512), device events around single launches after a warm-up, median of --reps:
  * the kernel at 2, 8 and 30 people per image (synth.random_people, integer joints), two-buffer form and in place;
  * next to it a plain dst.copy_(src) of the same buffers -- the floor of the two-buffer form; algorithmic bytes 2 B h w 3,
    share of the HBM roof with the 8 TB/s of MI355X_MICROARCH.md;
  * every timed canvas is checked against the NumPy renderer on a sample of images;
  * the NumPy renderer's host time per image on the same records (the baseline the kernel replaces);
  * the engine's images/s (bench.py's step: ingest + forward + post-processing) with render=True and render=False, alternating,
    three runs each, against the spread of the render=False runs.
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
HBM_PEAK_GBS = 8000.0


def records_for(people, batch, seed):
    from posepaf import _lib, synth
    recs = np.zeros(batch, _lib.RECORD_DTYPE)
    for b in range(batch):
        joints = synth.random_people(people, np.random.default_rng(seed + b), IMG, IMG)
        recs[b]["n_humans"] = people
        for k in range(people):
            present = joints[k, :, 2] == 1
            hm = recs[b]["humans"][k]
            hm["peak_id"] = np.where(present, np.arange(18) + 18 * k, -1)
            hm["x"], hm["y"] = joints[k, :, 0].astype(np.int32), joints[k, :, 1].astype(np.int32)
            hm["n_parts"], hm["score"] = int(present.sum()), 1.0
    return recs


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
    return statistics.median(out), min(out), max(out)


def kernel_part(torch, batch, reps):
    from posepaf.render import draw_record_numpy, draw_records
    src = torch.randint(0, 256, (batch, IMG, IMG, 3), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    alg = 2 * batch * IMG * IMG * 3
    out = {"geometry": f"{batch} x {IMG} x {IMG} x 3 uint8", "algorithmic_bytes_two_buffers": alg, "hbm_peak_gbs": HBM_PEAK_GBS,
           "timing": f"device events around one launch, median (min, max) of {reps} after 5 warm-up launches"}
    m = median_ms(torch, lambda: dst.copy_(src), reps)
    out["copy_dst_from_src"] = {"ms": m[0], "min_ms": m[1], "max_ms": m[2], "gbs": alg / m[0] / 1e6, "share_of_hbm_roof": alg / m[0] / 1e6 / HBM_PEAK_GBS}
    src_host = src.cpu().numpy()
    for people in (2, 8, 30):
        recs = records_for(people, batch, 7000 + 1000 * people)
        rec_dev = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
        m = median_ms(torch, lambda: draw_records(src, rec_dev, None, out=dst), reps)
        got = dst.cpu().numpy()
        sample = list(range(0, batch, max(1, batch // 8)))
        t0 = time.perf_counter()
        want = [draw_record_numpy(src_host[b], recs[b]) for b in sample]
        numpy_ms = (time.perf_counter() - t0) / len(sample) * 1e3
        equal = all(np.array_equal(got[b], w) for b, w in zip(sample, want))
        work = src.clone()
        mi = median_ms(torch, lambda: draw_records(work, rec_dev, None, out=work), reps)
        out[f"people_{people}"] = {
            "kernel_ms": m[0], "min_ms": m[1], "max_ms": m[2], "gbs_algorithmic": alg / m[0] / 1e6,
            "share_of_hbm_roof": alg / m[0] / 1e6 / HBM_PEAK_GBS, "times_the_copy": m[0] / out["copy_dst_from_src"]["ms"],
            "in_place_kernel_ms": mi[0], "numpy_draw_humans_ms_per_image_one_core": numpy_ms,
            "numpy_ms_per_batch_one_core": numpy_ms * batch, f"equal_to_numpy_on_{len(sample)}_images": bool(equal)}
    return out


def engine_part(torch, batch, steps, runs=3):
    from bench import BENCH_CHOICE_TABLE, SCENE_PEOPLE, build_scenes
    from posepaf import fused_model
    from posepaf.api import PosePostProcessor
    from posepaf.engine import InferenceEngine
    from posepaf.fused_model import build_inference_model
    dev = torch.device("cuda", 0)
    torch.backends.cudnn.benchmark = True
    post = PosePostProcessor(max_batch=batch, max_h=IMG // 4, max_w=IMG // 4, max_peaks_per_part=64, device=0)
    _, uniq = build_scenes(len(SCENE_PEOPLE))
    model = build_inference_model(dev, fused=True)
    fused_model.load_table(), fused_model.load_table(BENCH_CHOICE_TABLE)
    engines = {}
    for render in (False, True):
        eng = InferenceEngine(model, post, batch, 0, rules="cpp", inject_scale=1e-3, max_image_hw=(IMG, IMG), n_slots=2, render=render)
        plan = eng.plan(IMG, IMG, batch)
        eng.set_bank(plan, np.stack(uniq))
        g = np.random.default_rng(1234)
        slots = []
        for _ in range(2):
            slot = eng.acquire()
            sizes, idx, imgs = slot.views(batch, IMG, IMG)
            sizes[:] = IMG
            idx[:] = np.arange(batch) % len(uniq)
            imgs[:] = g.integers(0, 256, imgs.shape, dtype=np.uint8)
            slots.append(slot)
        eng.prepare(plan)
        engines[render] = (eng, plan, slots)
    rates = {False: [], True: []}
    for _ in range(runs):
        for render in (False, True):
            eng, plan, slots = engines[render]
            for k in range(3):
                eng.submit(slots[k % 2], plan, recycle=False)
            eng.sync()
            t0 = time.perf_counter()
            for k in range(steps):
                eng.submit(slots[k % 2], plan, recycle=False)
            eng.sync()
            rates[render].append(batch * steps / (time.perf_counter() - t0))
    same = bool(torch.equal(engines[False][1].records, engines[True][1].records))
    off, on = rates[False], rates[True]
    post.close()
    return {"step": f"bench.py's step (pinned-host upload + forward + post-processing), {batch} images, {steps} steps per run after 3 warm-up steps, "
                    "render=False and render=True alternating in one process",
            "images_per_sec_render_false": off, "images_per_sec_render_true": on,
            "median_render_false": statistics.median(off), "median_render_true": statistics.median(on),
            "spread_render_false_percent": (max(off) - min(off)) / statistics.median(off) * 100,
            "render_true_vs_false_percent": (statistics.median(on) / statistics.median(off) - 1) * 100,
            "records_of_the_last_step_equal": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--no-engine", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "draw_probe.py needs an MI355X"
    out = {"device": torch.cuda.get_device_name(0), "kernel": kernel_part(torch, a.batch, a.reps)}
    out["engine"] = "not measured" if a.no_engine else engine_part(torch, a.batch, a.steps)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
