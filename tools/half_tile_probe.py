#!/usr/bin/env python3
"""Tuner times (posepaf.fused_model._timed: median of five single launches) of plain-convolution variants 104 and 106 on the 3x3
layers of the bench geometry whose C_out is 64 mod 128 -- the shapes with a half-empty last channel tile -- at 256 samples.

    python tools/half_tile_probe.py [out.json] [repeats]

The two variants are timed alternately `repeats` times (default 3); the outputs of the last pair are compared bit for bit."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "improved-body-parts_amd")]
import torch  # noqa: E402

SHAPES = [(64, 256, 256), (64, 128, 128), (192, 64, 64), (192, 32, 32), (320, 16, 16)]   # (C = K, H, W)
N = 256


def main():
    from posepaf import fused_model as fm
    out = sys.argv[1] if len(sys.argv) > 1 else None
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for c, h, w in SHAPES:
        conv = torch.nn.Conv2d(c, c, 3, 1, 1)
        f = fm.FConv(conv, None, True).cuda().half()
        f._w()
        x = torch.randn((N, h, w, c), generator=g, device="cuda").half().permute(0, 3, 1, 2)
        ys = {cfg: f._out(x, h, w) for cfg in (104, 106)}
        times = {104: [], 106: []}
        for _ in range(reps):
            for cfg in (104, 106):
                rc = f._fused_launch(cfg, x, None, 0, ys[cfg])
                assert rc == 0, (cfg, c, h, w, rc)
                times[cfg].append(fm._timed(lambda: f._fused_launch(cfg, x, None, 0, ys[cfg])))
        torch.cuda.synchronize()
        row = {"shape": f"{c}->{c} 3x3 at {h}x{w}, {N} samples", "ms_104": times[104], "ms_106": times[106],
               "bit_equal": bool(torch.equal(ys[104], ys[106])),
               "gflop": 2.0 * N * h * w * c * c * 9 / 1e9}
        row["ratio_106_over_104_of_medians"] = sorted(times[106])[reps // 2] / sorted(times[104])[reps // 2]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, ys
    if out:
        with open(out, "w") as fh:
            json.dump({"command": "tools/half_tile_probe.py", "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
