#!/usr/bin/env python3
"""head_wgrad_probe.py -- measurements of pp_head_wgrad_f16 (csrc/posepaf_headgrad.hip) and of finetune.py --model fused for DESIGN.md
section 6, round 20.

    python tools/head_wgrad_probe.py --out profiles/r20_head_wgrad.json [--reps 25] [--no_finetune]

Kernel: the five head shapes of 8 images of 512 x 512 (hw = 16384, 4096, 1024, 256, 64; m = 8 hw, c_in = 256, c_out = 50, ldg = 64,
SE gains given).  Device events around single calls (two launches; workspace and outputs preallocated) after a warm-up, median (min,
max) of --reps.  Against the floor of reading the 50 gradient channels and the 256 input channels once, at the 8 TB/s peak DESIGN uses
for MI355X and at the 6.3 TB/s the microarchitecture notes give as achievable, and against the torch formulation on the same
tensors: pp_channel_scale_f16 followed by a binary16 matmul with float32 output (torch.mm(..., out_dtype=float32) where this torch
has it, else the binary16 product widened afterwards -- the JSON says which) plus the column sum for db.
Fine-tune: finetune.py --model fused --train heads against --model plain --train heads at --batch 8 --sizes 512x512 --synthetic 64, as
child processes that share one kernel-choice cache; a 3-step run first (it tunes the layer shapes), then --steps 20: steps per second
from the JSON line's `seconds`.  Needs an MI355X; there is no CPU path."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "improved-body-parts_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS, HBM_ACHIEVABLE_GBS = 8000.0, 6300.0
IMAGES, C_IN, C_OUT, LDG = 8, 256, 50, 64


def timed(torch, fn, reps):
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
    return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)}


def kernel_rows(reps):
    import torch
    from posepaf import _lib, fused_model
    L = _lib.load()
    dev = torch.device("cuda", 0)
    rows, form = [], None
    for hw in (16384, 4096, 1024, 256, 64):
        m = IMAGES * hw
        gen = torch.Generator(device=dev).manual_seed(hw)
        g = (torch.randn((m, LDG), generator=gen, device=dev) * 0.125).half()
        x = torch.randn((IMAGES, hw, 1, C_IN), generator=gen, device=dev).half().permute(0, 3, 1, 2)     # channels-last (N, C, hw, 1)
        scale = (torch.rand((IMAGES, C_IN), generator=gen, device=dev) + 0.5).half()
        need = int(L.pp_head_wgrad_workspace_bytes(m, C_IN, C_OUT))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        dw, db = torch.empty((C_OUT, C_IN), dtype=torch.float32, device=dev), torch.empty(C_OUT, dtype=torch.float32, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def device():
            _lib.check(L.pp_head_wgrad_f16(C.c_void_p(g.data_ptr()), LDG, C.c_void_p(x.data_ptr()), C.c_void_p(scale.data_ptr()), m, hw, C_IN,
                                           C_OUT, 1.0, C.c_void_p(ws.data_ptr()), need, C.c_void_p(dw.data_ptr()), C.c_void_p(db.data_ptr()), st))

        gt = g[:, :C_OUT].t()

        def torch_form(out_dtype):
            xs = fused_model.channel_scale(x, scale).permute(0, 2, 3, 1).reshape(m, C_IN)
            w = torch.mm(gt, xs, out_dtype=torch.float32) if out_dtype else torch.mm(gt, xs).float()
            return w, g[:, :C_OUT].float().sum(dim=0)

        if form is None:
            try:
                torch_form(True)
                form = "channel_scale + torch.mm(binary16, binary16, out_dtype=float32)"
            except (TypeError, RuntimeError):
                form = "channel_scale + torch.mm(binary16, binary16).float()"
        with_out = "out_dtype" in form
        device()
        want = torch_form(with_out)[0]
        agree = float((dw - want).abs().max() / want.abs().max())
        floor_bytes = m * (C_OUT + C_IN) * 2
        row = {"hw": hw, "m": m, "workgroups": min(L.pp_head_wgrad_max_workgroups(), -(-m // L.pp_head_wgrad_chunk_pixels())),
               "workspace_bytes": need, "device": timed(torch, device, reps), "torch": timed(torch, lambda: torch_form(with_out), reps),
               "floor_bytes": floor_bytes, "floor_us_at_8TBs": floor_bytes / HBM_PEAK_GBS * 1e-3,
               "floor_us_at_6.3TBs": floor_bytes / HBM_ACHIEVABLE_GBS * 1e-3, "max_rel_difference_to_torch": agree}
        row["device_over_floor_8TBs"] = row["device"]["median_us"] / row["floor_us_at_8TBs"]
        row["torch_over_device"] = row["torch"]["median_us"] / row["device"]["median_us"]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return rows, form


def finetune_rows():
    out = {}
    with tempfile.TemporaryDirectory() as cache:
        env = dict(os.environ, POSEPAF_CACHE_DIR=cache)
        base = [sys.executable, os.path.join(PKG, "finetune.py"), "--train", "heads", "--synthetic", "64", "--batch", "8", "--sizes", "512x512"]
        for model in ("fused", "plain"):
            for steps in (3, 20):
                r = subprocess.run(base + ["--model", model, "--steps", str(steps)], capture_output=True, text=True, env=env, timeout=900)
                if r.returncode != 0:
                    raise SystemExit(f"finetune.py --model {model} failed:\n{r.stderr[-2000:]}")
                res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            out[model] = {"steps": res["steps"], "seconds": res["seconds"], "steps_per_second": res["steps"] / res["seconds"],
                          "loss_first": res["loss_first"], "loss_last": res["loss_last"], "losses": res["losses"]}
            if model == "fused":
                out[model].update({k: res[k] for k in ("loss_scale", "skipped_steps", "wgrad")})
            print(json.dumps({model: out[model]}), file=sys.stderr)
    out["fused_over_plain_steps_per_second"] = out["fused"]["steps_per_second"] / out["plain"]["steps_per_second"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--no_finetune", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("head_wgrad_probe.py needs an MI355X: there is no CPU path")
    rows, form = kernel_rows(max(20, a.reps))
    doc = {"shape": {"images": IMAGES, "c_in": C_IN, "c_out": C_OUT, "ldg": LDG, "scale": True}, "reps": max(20, a.reps),
           "torch_formulation": form, "kernel": rows}
    if not a.no_finetune:
        doc["finetune_batch8_512x512_heads"] = finetune_rows()
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
