#!/usr/bin/env python3
"""head_step_probe.py -- measurements of the captured head-training step for DESIGN.md section 6, round 25.

    python tools/head_step_probe.py --out profiles/r25_head_step.json [--repeats 5] [--steps 10] [--no_finetune]

Everything at 8 images of 512 x 512, 4 stages, in one process on one card.
Step time: three HeadTrainers on one network -- today's path (update="torch", wgrad="device"), update="device" + wgrad="multi" eager,
and the same with graph=True -- are warmed up (three steps each: the eager first one, the capture, one replay), then timed in
--repeats rounds that ALTERNATE between them: a host clock around --steps steps that ends in a device synchronise.  Median, minimum
and maximum of the rounds, in ms per step.  Two more trainers run the first and the last form with torch.backends.cudnn.deterministic
off (times only: such steps are not reproducible bit for bit).
Kernel time, device events around one call after a warm-up, median (min, max) of 25: the twenty heads of a step through one
pp_head_wgrad_multi_f16 call against twenty pp_head_wgrad_f16 calls on the same captured tensors, and pp_head_update_f32 against
opt.step() + the masked restore + the 80 copies; the three HIP forms also as a replay of a graph that holds just that call.
Fine-tune (child processes that share one kernel-choice cache, a 3-step run first): finetune.py --model plain --train heads, --model
fused as today, and --model fused --graph --wgrad multi; steady-state steps per second from the JSON line.
Needs an MI355X; there is no CPU path."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "improved-body-parts_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

IMAGES, SIDE, STAGES = 8, 512, 4
CONFIGS = {"today (update torch, wgrad device)": dict(update="torch", wgrad="device"),
           "update device, wgrad multi, eager": dict(update="device", wgrad="multi"),
           "update device, wgrad multi, graph": dict(update="device", wgrad="multi", graph=True)}
# the same two ends with torch.backends.cudnn.deterministic OFF (the layers without a fused kernel then run MIOpen's tuned solvers; steps
# are no longer reproducible bit for bit, so these rows are times only): what the flag costs, and what the capture gains without it
FLAG_OFF = {"today, cudnn.deterministic off": dict(update="torch", wgrad="device"),
            "update device, wgrad multi, graph, cudnn.deterministic off": dict(update="device", wgrad="multi", graph=True)}


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


def replayed(torch, fn):
    """fn captured alone into a graph -> a thunk that replays it"""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


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


def step_rows(torch, trainers, x, target, repeats, steps):
    for name, tr in trainers.items():
        torch.backends.cudnn.deterministic = name not in FLAG_OFF
        for _ in range(3):
            tr.step(x, target)
    torch.cuda.synchronize()
    ms = {name: [] for name in trainers}
    for _ in range(repeats):
        for name, tr in trainers.items():
            torch.backends.cudnn.deterministic = name not in FLAG_OFF
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(x, target)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    rows = {name: summary(v, "ms_per_step") for name, v in ms.items()}
    for name, tr in trainers.items():
        rows[name].update({"graph_replays": tr.graph_replays, "skipped_steps": int(tr.skipped_steps)})
    torch.backends.cudnn.deterministic = True
    return rows


def kernel_rows(torch, trainers):
    today, multi = trainers["today (update torch, wgrad device)"], trainers["update device, wgrad multi, eager"]
    inv = 1.0 / multi.loss_scale_for(IMAGES)

    def twenty_single():
        for key, (g2, ldg, x2, scale) in multi.last_inputs.items():
            today._wgrad(key, g2, ldg, x2, scale, inv)

    forms = {"wgrad: twenty pp_head_wgrad_f16 calls": twenty_single, "wgrad: one pp_head_wgrad_multi_f16 call": lambda: multi._wgrad_multi(inv),
             "update: pp_head_update_f32": multi._device_update}
    rows = {name: {"eager": events(torch, fn), "in a graph replay": events(torch, replayed(torch, fn))} for name, fn in forms.items()}
    rows["update: opt.step() + masked restore + 80 copies"] = {"eager": events(torch, today._torch_update),
                                                              "in a graph replay": "not measured: torch.optim.SGD.step() is not captured here"}
    return rows


def finetune_rows():
    out = {}
    with tempfile.TemporaryDirectory() as cache:
        env = dict(os.environ, POSEPAF_CACHE_DIR=cache)
        base = [sys.executable, os.path.join(PKG, "finetune.py"), "--train", "heads", "--synthetic", "64", "--batch", str(IMAGES), "--sizes",
                f"{SIDE}x{SIDE}", "--stages", str(STAGES)]
        for name, extra in (("plain", ["--model", "plain"]), ("fused, today", ["--model", "fused"]),
                            ("fused, --graph --wgrad multi", ["--model", "fused", "--graph", "--wgrad", "multi"])):
            for steps in (3, 22):
                r = subprocess.run(base + extra + ["--steps", str(steps)], capture_output=True, text=True, env=env, timeout=900)
                if r.returncode != 0:
                    raise SystemExit(f"finetune.py {' '.join(extra)} failed:\n{r.stderr[-2000:]}")
                res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            out[name] = {k: res.get(k) for k in ("steps", "seconds", "steps_per_s", "loss_first", "loss_last", "graph_replays", "skipped_steps")}
            print(json.dumps({name: out[name]}), file=sys.stderr)
    for name in list(out):
        if name != "plain":
            out[name]["steps_per_s_over_plain"] = out[name]["steps_per_s"] / out["plain"]["steps_per_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no_finetune", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("head_step_probe.py needs an MI355X: there is no CPU path")
    from posepaf import head_train
    from posepaf.model_init import build_network
    dev = torch.device("cuda", 0)
    torch.backends.cudnn.deterministic = True
    net, _ = build_network("posenet", None, 7, nstack=STAGES)
    x, target = data(torch, dev)
    trainers = {name: head_train.HeadTrainer(net, dev, **kw) for name, kw in {**CONFIGS, **FLAG_OFF}.items()}
    doc = {"shape": {"images": IMAGES, "side": SIDE, "stages": STAGES}, "repeats": max(5, a.repeats), "steps_per_repeat": a.steps,
           "step": step_rows(torch, trainers, x, target, max(5, a.repeats), a.steps)}
    today = doc["step"]["today (update torch, wgrad device)"]
    graph = doc["step"]["update device, wgrad multi, graph"]
    doc["graph_faster_than_today_by_more_than_todays_spread"] = bool(
        today["median_ms_per_step"] - graph["median_ms_per_step"] > today["max_ms_per_step"] - today["min_ms_per_step"])
    print(json.dumps(doc["step"]), file=sys.stderr)
    doc["kernel"] = kernel_rows(torch, trainers)
    print(json.dumps(doc["kernel"]), file=sys.stderr)
    if not a.no_finetune:
        doc["finetune"] = finetune_rows()
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
