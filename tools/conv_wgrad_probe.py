#!/usr/bin/env python3
"""conv_wgrad_probe.py -- measurements of pp_head_dgrad_f16, pp_conv3x3_wgrad_f16 and HeadTrainer(train="heads+conv") (INTEGRATION
section 25) for DESIGN.md section 6, round 26.

    python tools/conv_wgrad_probe.py --out profiles/r26_conv_wgrad.json [--repeats 5] [--steps 10] [--parent_pkg DIR]

Kernel times: both kernels at the five scale shapes of 8 x 512 x 512 (maps of 128^2 ... 8^2 pixels: m = 131072 ... 512; 256 -> 256
channels, a head of 50 outputs in rows of 64), device events around one call after a warm-up, median (min, max) of 25, next to the
time of reading the inputs and writing the outputs once at 8 TB/s (the HBM rate of the other probes) and to torch's binary16
torch.nn.grad.conv2d_weight on the same tensors.  The workspace sizes are reported with them.
Step time: the `final` network, 4 stages, 8 x 512 x 512, update="device", wgrad="multi", graph=True; train="heads" and "heads+conv" are
warmed up (three steps each), then timed in --repeats rounds that ALTERNATE between the two: a host clock around --steps steps that
ends in a device synchronise.
--parent_pkg DIR (a built copy of the package directory of the commit before this change): train="heads" of this tree and of that
one are timed in child processes that alternate, the same rounds in each; reported with both spreads.
Needs an MI355X; there is no CPU path."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGES, SIDE, STAGES = 8, 512, 4
C_IN = C_OUT = 256
HEAD_K, HEAD_LDG = 50, 64
HBM_PEAK_GBS = 8000.0
TRAINER = dict(update="device", wgrad="multi", graph=True)


def summary(values, unit):
    return {f"median_{unit}": statistics.median(values), f"min_{unit}": min(values), f"max_{unit}": max(values), "n": len(values)}


def events(torch, fn, reps=25):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return summary(ts, "us")


def data(torch, dev):
    import numpy as np
    from posepaf import synth, synth_device
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.uniform(0.0, 1.0, (IMAGES, SIDE, SIDE, 3)).astype(np.float16)).to(dev)
    people = [synth.random_people(1 + i % 6, np.random.default_rng(20 + i), img_h=SIDE, img_w=SIDE) for i in range(IMAGES)]
    joints, n_people = synth_device.pack_joints(people, 6)
    target = synth_device.render_scenes(torch.from_numpy(joints).to(dev), torch.from_numpy(n_people).to(dev), SIDE // 4, SIDE // 4,
                                        dtype=torch.float16, flip=False, noise=0.0, reverse_kp=True)
    return x, target


def kernel_rows(torch, dev):
    from posepaf import _lib, fused_model
    L = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rows = {}
    for side in (128, 64, 32, 16, 8):
        m = IMAGES * side * side
        g = torch.randn((m, HEAD_LDG), device=dev).half() * 0.125
        w = torch.randn((HEAD_K, C_OUT), device=dev).half() * 0.1
        y = torch.randn((m, C_OUT), device=dev).half()
        x = torch.randn((IMAGES, side, side, C_IN), device=dev).half()
        dy = torch.empty((m, C_OUT), dtype=torch.float16, device=dev)
        need = int(L.pp_conv3x3_wgrad_workspace_bytes(IMAGES, side, side, C_IN, C_OUT))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        dw = torch.empty((C_OUT, 3, 3, C_IN), dtype=torch.float32, device=dev)
        db = torch.empty(C_OUT, dtype=torch.float32, device=dev)

        def dgrad():
            _lib.check(L.pp_head_dgrad_f16(ptr(g), HEAD_LDG, ptr(w), ptr(y), m, C_OUT, HEAD_K, fused_model.LEAK, ptr(dy), stream))

        def wgrad():
            _lib.check(L.pp_conv3x3_wgrad_f16(ptr(dy), ptr(x), IMAGES, side, side, C_IN, C_OUT, 1.0, None, ptr(ws), need, ptr(dw), ptr(db), stream))

        xt, dyt = x.permute(0, 3, 1, 2), dy.view(IMAGES, side, side, C_OUT).permute(0, 3, 1, 2)

        def torch_wgrad():
            torch.nn.grad.conv2d_weight(xt, (C_OUT, C_IN, 3, 3), dyt, stride=1, padding=1)

        row = {"m": m, "pp_head_dgrad_f16": events(torch, dgrad), "pp_conv3x3_wgrad_f16": events(torch, wgrad),
               "torch conv2d_weight, binary16": events(torch, torch_wgrad), "conv3x3_wgrad_workspace_bytes": need}
        d_bytes = m * HEAD_K * 2 + HEAD_K * C_OUT * 2 + 2 * m * C_OUT * 2
        w_bytes = m * C_OUT * 2 + m * C_IN * 2 + (dw.numel() + db.numel()) * 4
        row["pp_head_dgrad_f16"]["floor_us_at_8TBs"] = d_bytes / HBM_PEAK_GBS / 1e3
        row["pp_conv3x3_wgrad_f16"]["floor_us_at_8TBs"] = w_bytes / HBM_PEAK_GBS / 1e3
        row["pp_conv3x3_wgrad_f16"]["useful_tflops"] = 2.0 * m * 9 * C_IN * C_OUT / row["pp_conv3x3_wgrad_f16"]["median_us"] / 1e6
        rows[f"{side}x{side}"] = row
        print(json.dumps({f"{side}x{side}": row}), file=sys.stderr)
    return rows


def timed_rounds(torch, trainers, x, target, repeats, steps):
    for tr in trainers.values():
        for _ in range(3):
            tr.step(x, target)
    torch.cuda.synchronize()
    ms = {name: [] for name in trainers}
    for _ in range(repeats):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(x, target)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    return ms


def build(torch, dev, trains):
    from posepaf import head_train
    from posepaf.model_init import build_network
    torch.backends.cudnn.deterministic = True
    net, _ = build_network("final", None, 7, nstack=STAGES)
    x, target = data(torch, dev)
    trainers = {t: head_train.HeadTrainer(net, dev, **TRAINER, **({} if t == "heads" else {"train": t})) for t in trains}
    return trainers, x, target


def child(a):
    """one process of the comparison with the parent commit: train='heads' of the package on sys.path -> one JSON line of ms per step"""
    import torch
    dev = torch.device("cuda", 0)
    trainers, x, target = build(torch, dev, ["heads"])
    print(json.dumps({"ms_per_step": timed_rounds(torch, trainers, x, target, a.repeats, a.steps)["heads"]}))


def parent_rows(a):
    import tempfile
    out = {"this": [], "parent": []}
    caches = {name: tempfile.mkdtemp(prefix=f"conv_wgrad_probe_{name}_") for name in out}      # a kernel-choice cache per code version
    for turn in range(4):
        name = ("this", "parent")[turn % 2]
        pkg = os.path.join(ROOT, "improved-body-parts_amd") if name == "this" else os.path.abspath(a.parent_pkg)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--pkg", pkg, "--repeats", str(a.repeats), "--steps", str(a.steps)],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, POSEPAF_CACHE_DIR=caches[name]))
        if r.returncode != 0:
            raise SystemExit(f"the child for {name} failed ({r.returncode}):\n{r.stderr[-2000:]}")
        out[name] += json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["ms_per_step"]
        print(json.dumps({name: out[name]}), file=sys.stderr)
    rows = {name: summary(v, "ms_per_step") for name, v in out.items()}
    p = rows["parent"]
    rows["this_median_inside_the_parents_range"] = bool(p["min_ms_per_step"] <= rows["this"]["median_ms_per_step"] <= p["max_ms_per_step"])
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--parent_pkg", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "improved-body-parts_amd"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("conv_wgrad_probe.py needs an MI355X: there is no CPU path")
    if a.child:
        return child(a)
    dev = torch.device("cuda", 0)
    doc = {"shape": {"images": IMAGES, "side": SIDE, "stages": STAGES, "c_in": C_IN, "c_out": C_OUT}, "hbm_peak_gbs": HBM_PEAK_GBS,
           "kernel": kernel_rows(torch, dev)}
    trainers, x, target = build(torch, dev, ["heads", "heads+conv"])
    ms = timed_rounds(torch, trainers, x, target, a.repeats, a.steps)
    doc["step"] = {name: dict(summary(v, "ms_per_step"), graph_replays=trainers[name].graph_replays, skipped_steps=int(trainers[name].skipped_steps))
                   for name, v in ms.items()}
    doc["step"]["trainer"] = {k: str(v) for k, v in TRAINER.items()}
    doc["step"]["workspace_bytes_heads+conv"] = int(trainers["heads+conv"]._workspace.numel())
    print(json.dumps(doc["step"]), file=sys.stderr)
    del trainers
    torch.cuda.empty_cache()
    if a.parent_pkg:
        doc["heads_against_the_parent_commit"] = parent_rows(a)
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
