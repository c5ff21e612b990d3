#!/usr/bin/env python3
"""head_step_trace.py -- where the time of ONE replay of the captured head-training step goes.
A kernel trace slows the host, so it is a run of its own, apart from tools/head_step_probe.py:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o step -- python tools/head_step_trace.py            # prints REPLAY_MS [...]
    python tools/head_step_trace.py --summarise DIR --replay_ms MS > profiles/r25_replay_trace.json

The first form runs HeadTrainer(update="device", wgrad="multi", graph=True) at 8 x 512 x 512, 4 stages: four steps (eager, capture, two
replays), then three replays timed by device events.  The second reads the trace and keeps the kernels that started within MS
(the last replay's event time) of the end of the last kernel: their number, their summed time, the gaps between them and the time
per kernel name."""
import argparse
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "improved-body-parts_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def run():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("head_step_trace.py needs an MI355X: there is no CPU path")
    import head_step_probe as hp
    from posepaf import head_train
    from posepaf.model_init import build_network
    dev = torch.device("cuda", 0)
    net, _ = build_network("posenet", None, 7, nstack=hp.STAGES)
    x, target = hp.data(torch, dev)
    tr = head_train.HeadTrainer(net, dev, update="device", wgrad="multi", graph=True)
    for _ in range(4):
        tr.step(x, target)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.step(x, target)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    print("REPLAY_MS", json.dumps(ts))


def short_name(name):
    """a kernel's name without its argument list and return type, at most 90 characters.  The library's kernels live in an anonymous
    namespace, whose '(anonymous namespace)::' is not the argument list: it is taken out before the cut at the first '('"""
    name = re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", "")).strip()
    return re.sub(r"^void\s+", "", name)[:90]


def summarise(directory, replay_ms):
    rows = []
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows.sort()
    end = max(r[1] for r in rows)
    win = [r for r in rows if r[0] >= end - replay_ms * 1e6]
    by = {}
    for s, e, name in win:
        t = by.setdefault(short_name(name), [0, 0])
        t[0] += e - s
        t[1] += 1
    gaps = sorted(win[i + 1][0] - win[i][1] for i in range(len(win) - 1))
    return {"window_ms": replay_ms, "kernels_in_window": len(win), "kernel_busy_ms": sum(e - s for s, e, _ in win) / 1e6,
            "first_to_last_ms": (win[-1][1] - win[0][0]) / 1e6, "median_gap_us": gaps[len(gaps) // 2] / 1e3,
            "sum_positive_gaps_ms": sum(g for g in gaps if g > 0) / 1e6,
            "top": [{"kernel": k, "ms": v[0] / 1e6, "launches": v[1]} for k, v in sorted(by.items(), key=lambda kv: -kv[1][0])[:25]]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise", default=None, help="the directory rocprofv3 wrote")
    ap.add_argument("--replay_ms", type=float, default=None)
    a = ap.parse_args()
    if a.summarise:
        print(json.dumps(summarise(a.summarise, a.replay_ms), indent=1))
    else:
        run()
