#!/usr/bin/env python3
"""conv_dgrad_probe.py -- measurements of pp_conv3x3_dgrad_f16 and HeadTrainer(train="heads+conv2") for
DESIGN.md section 6, round 27.

    python tools/conv_dgrad_probe.py --out profiles/r27_conv_dgrad.json [--part kernel|step|parent|all] [--repeats 5] [--steps 10]
                                     [--parent_pkg DIR]

--part kernel: pp_conv3x3_dgrad_f16 at the five scale shapes of 8 x 512 x 512 (maps of 128^2 ... 8^2 pixels, 256 -> 256 channels),
device events around one call after a warm-up, median (min, max) of 25, next to the time of reading dy, w and y and writing dx once
at 8 TB/s (the HBM rate of the other probes), to torch's binary16 torch.nn.grad.conv2d_input on the same tensors, and the useful
TFLOP/s (2 m 9 c_in c_out; the split into bfloat16 halves costs four times that on the matrix unit).
--part step: the `final` network, 4 stages, 8 x 512 x 512, update="device", wgrad="multi", graph=True; train="heads", "heads+conv" and
"heads+conv2" are warmed up (three steps each), then timed in --repeats rounds that ALTERNATE between the three: a host clock around
--steps steps that ends in a device synchronise.
--part parent (needs --parent_pkg DIR, a built copy of the package directory of the commit before this change): train="heads" and
train="heads+conv" of this tree and of that one are timed in child processes that alternate (--order, by default this, parent,
parent, this, so that a drift over the run falls on both alike), the same rounds in each.  A trainer times the forward's kernel
candidates in every process, so a pilot process does that once and every measured process of either version installs the pilot's
table (the forward's kernels are the same in both trees): the hash of the choices each process ran is reported, with the values of
every process and both spreads.
Every part merges its keys into --out, so the parts can run as separate processes.  Needs an MI355X; there is no CPU path."""
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
HBM_PEAK_GBS = 8000.0
TRAINER = dict(update="device", wgrad="multi", graph=True)
MODES = ("heads", "heads+conv", "heads+conv2")


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
        dy = torch.randn((m, C_OUT), device=dev).half() * 0.125
        w = (torch.randn((C_OUT, 3, 3, C_IN), device=dev) * 0.05).half()
        y = torch.randn((IMAGES, side, side, C_IN), device=dev).half()
        dx = torch.empty((IMAGES, side, side, C_IN), dtype=torch.float16, device=dev)

        def dgrad():
            _lib.check(L.pp_conv3x3_dgrad_f16(ptr(dy), ptr(w), ptr(y), IMAGES, side, side, C_IN, C_OUT, fused_model.LEAK, ptr(dx), stream))

        wt, dyt = w.permute(0, 3, 1, 2), dy.view(IMAGES, side, side, C_OUT).permute(0, 3, 1, 2)      # channels-last views, no copies

        def torch_dgrad():
            torch.nn.grad.conv2d_input((IMAGES, C_IN, side, side), wt, dyt, stride=1, padding=1)

        row = {"m": m, "pp_conv3x3_dgrad_f16": events(torch, dgrad), "torch conv2d_input, binary16": events(torch, torch_dgrad)}
        moved = m * C_OUT * 2 + w.numel() * 2 + 2 * m * C_IN * 2
        row["pp_conv3x3_dgrad_f16"]["floor_us_at_8TBs"] = moved / HBM_PEAK_GBS / 1e3
        row["pp_conv3x3_dgrad_f16"]["useful_tflops"] = 2.0 * m * 9 * C_IN * C_OUT / row["pp_conv3x3_dgrad_f16"]["median_us"] / 1e6
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
    """one process of the comparison with the parent commit: the modes both trees have, of the package on sys.path -> one JSON line.
    --table FILE: the forward's kernel choices are installed from FILE before anything runs (with --tune: timed here as usual, then
    saved to FILE); the hash of the table after the timed rounds says which choices this process ran"""
    import torch
    from posepaf import fused_model
    dev = torch.device("cuda", 0)
    installed = fused_model.load_table(a.table, force=True) if a.table and not a.tune else 0     # (the forward's kernels are the
    trainers, x, target = build(torch, dev, MODES[:2])                                            # same objects in both trees)
    ms = timed_rounds(torch, trainers, x, target, a.repeats, a.steps)
    if a.tune:
        fused_model.save_table(a.table)
    print(json.dumps({"ms_per_step": ms, "kernel_choices": {"installed": installed, "entries": len(fused_model.conv_choices()),
                                                            "hash": fused_model.table_hash()}}))


def parent_rows(a):
    """a pilot process of this tree times the forward's kernel candidates and saves its choices; every measured process of either
    version installs that one table, so both versions run the same forward kernels"""
    import tempfile
    table = os.path.join(tempfile.mkdtemp(prefix="conv_dgrad_probe_"), "conv_choice.json")
    order = ["pilot"] + a.order.split(",")
    extra = dict(v.split("=", 1) for v in a.extra_pkg)       # further versions --order may name, e.g. the parent's Python over this library
    runs = []
    for name in order:
        pkg = os.path.abspath(extra.get(name, a.parent_pkg)) if name in extra or name == "parent" else os.path.join(ROOT, "improved-body-parts_amd")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--pkg", pkg, "--repeats", str(a.repeats), "--steps", str(a.steps),
               "--table", table] + (["--tune"] if name == "pilot" else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"the child for {name} failed ({r.returncode}):\n{r.stderr[-2000:]}")
        got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        runs.append({"version": name, "ms_per_step": got["ms_per_step"], "kernel_choices": got["kernel_choices"]})
        print(json.dumps(runs[-1]), file=sys.stderr)
    rows = {"order": a.order, "processes": runs,
            "same_kernel_choices_in_every_process": len({r["kernel_choices"]["hash"] for r in runs}) == 1}
    for mode in MODES[:2]:
        vals = {v: [t for r in runs if r["version"] == v for t in r["ms_per_step"][mode]] for v in ("this", "parent")}
        this, parent = summary(vals["this"], "ms_per_step"), summary(vals["parent"], "ms_per_step")
        rows[mode] = {"this": this, "parent": parent, "this_median_inside_the_parents_range":
                      bool(parent["min_ms_per_step"] <= this["median_ms_per_step"] <= parent["max_ms_per_step"])}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", choices=("kernel", "step", "parent", "all"), default="all")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--parent_pkg", default=None)
    ap.add_argument("--order", default="this,parent,parent,this", help="the child processes of --part parent, in order")
    ap.add_argument("--extra_pkg", action="append", default=[], metavar="NAME=DIR",
                    help="one more package directory that --order may name (its processes are listed, not part of the condition)")
    ap.add_argument("--table", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tune", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "improved-body-parts_amd"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("conv_dgrad_probe.py needs an MI355X: there is no CPU path")
    if a.child:
        return child(a)
    if a.part == "parent" and not a.parent_pkg:
        raise SystemExit("--part parent needs --parent_pkg DIR")
    dev = torch.device("cuda", 0)
    doc = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc.update({"shape": {"images": IMAGES, "side": SIDE, "stages": STAGES, "c_in": C_IN, "c_out": C_OUT}, "hbm_peak_gbs": HBM_PEAK_GBS})
    if a.part in ("kernel", "all"):
        doc["kernel"] = kernel_rows(torch, dev)
    if a.part in ("step", "all"):
        trainers, x, target = build(torch, dev, MODES)
        ms = timed_rounds(torch, trainers, x, target, a.repeats, a.steps)
        doc["step"] = {name: dict(summary(v, "ms_per_step"), graph_replays=trainers[name].graph_replays, skipped_steps=int(trainers[name].skipped_steps))
                       for name, v in ms.items()}
        doc["step"]["trainer"] = {k: str(v) for k, v in TRAINER.items()}
        print(json.dumps(doc["step"]), file=sys.stderr)
        del trainers
        torch.cuda.empty_cache()
    if a.part in ("parent", "all") and a.parent_pkg:
        doc["against_the_parent_commit"] = parent_rows(a)
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
