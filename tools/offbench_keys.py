"""Census of the layer keys of image geometries off the bench's 512 x 512: writes profiles/conv_keys_offbench.json.

Per row (architecture, padded image height x width, samples) one eager forward of a random-init model on an EMPTY kernel-choice
table: the first forward at a new input shape runs every scale and tunes every layer shape it meets (fused_model.USE_PRUNED_SCALES),
so the keys it leaves are complete for all_preds as well.  Nothing is timed -- fused_model._timed is replaced with a constant,
so every fused form stays on its separate path (whose inner plain convolutions are keys of their own) and the recorded choices
mean nothing: the file is a LIST OF KEYS for tests/test_gpu_offbench_shapes.py, never a table the product loads.

The file has the format of profiles/conv_choice_b128.json ({"library", "entries": [[key, choice], ...]}), with two more fields:
"rows" (the rows below, in order) and "lookups" (per entry, the indices of the rows whose forward looks the key up).  A key that
several rows or both architectures share appears once.

    python tools/offbench_keys.py [--out profiles/conv_keys_offbench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "improved-body-parts_amd")]

# (arch, padded image height, width, samples: an image and its mirror are 2) -- what each reaches is worked out in
# tests/test_gpu_offbench_shapes.py from csrc/posepaf_conv_own.hip: halo_geometry
POSENET = [(64, 64, 1), (64, 64, 2), (64, 64, 3), (64, 256, 2), (64, 256, 4), (128, 192, 2), (128, 192, 44), (192, 128, 2),
           (128, 256, 2), (128, 256, 4), (256, 320, 2), (384, 384, 2),
           # added: scale 1 is 32 x 48, the only map of the set whose HALF-resolution input (the collapsed upsample convolution's
           # grid) is cut into unstacked 16-wide tiles; scale 0 (64 x 96) is 3 x 4 tiles of the 32-wide instance
           (256, 384, 2)]
FINAL = [(64, 64, 2), (128, 192, 2), (128, 256, 2), (384, 384, 2)]
ROWS = [("posenet",) + r for r in POSENET] + [("final",) + r for r in FINAL]


class Recording(dict):
    """the choice table, noting every key that is looked up"""

    def __init__(self):
        super().__init__()
        self.looked_up = set()

    def get(self, key, default=None):
        self.looked_up.add(key)
        return super().get(key, default)


def census(rows=ROWS, log=print):
    """-> (entries {key: choice}, lookups {key: [row index, ...]})"""
    import torch
    from posepaf import fused_model as fm
    saved = (fm._conv_choice, fm._conv_timing, fm._conv_calls, fm._timed)
    entries, lookups, models = {}, {}, {}
    try:
        fm._timed = lambda fn: 1.0
        for i, (arch, h, w, n) in enumerate(rows):
            if arch not in models:
                models[arch] = fm.build_inference_model("cuda", arch=arch)
            table = Recording()
            fm._conv_choice, fm._conv_timing, fm._conv_calls = table, {}, {}
            x = torch.rand((n, h, w, 3), generator=torch.Generator(device="cuda").manual_seed(1), device="cuda").half()
            with torch.no_grad():
                y = models[arch](x)
            torch.cuda.synchronize()
            assert y.shape == (n, 50, h // 4, w // 4), y.shape
            for key, choice in table.items():
                entries.setdefault(key, int(choice))
                lookups.setdefault(key, []).append(i)
            log(f"row {i}: {arch} {h}x{w} n = {n}: {len(table)} keys, {len(entries)} in all")
    finally:
        fm._conv_choice, fm._conv_timing, fm._conv_calls, fm._timed = saved
    return entries, lookups


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_keys_offbench.json"))
    a = ap.parse_args()
    from posepaf import fused_model as fm
    entries, lookups = census()
    keys = sorted(entries, key=lambda k: repr(fm._key_to_json(k)))
    doc = {"library": fm.library_hash(),
           "rows": [{"arch": arch, "image": [h, w], "n": n} for arch, h, w, n in ROWS],
           "entries": [[fm._key_to_json(k), entries[k]] for k in keys],
           "lookups": [lookups[k] for k in keys]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{name}": ' + (json.dumps(v) if name == "library" else
                                                      "[\n  " + ",\n  ".join(json.dumps(e) for e in v) + "\n ]")
                                   for name, v in doc.items()) + "\n}\n")
    print(f"{len(keys)} keys of {len(ROWS)} rows -> {a.out}")


if __name__ == "__main__":
    main()
