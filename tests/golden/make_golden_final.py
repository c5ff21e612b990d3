#!/usr/bin/env python3
"""Generate the G8 fixtures from the REFERENCE's published variant itself (run in the build container only, never on the GPU
machine):

    python tests/golden/make_golden_final.py

* g8_final_state_dict_manifest.json: key -> shape of the reference's own models/posenet_final.NetworkEval, for nstack 4 and 3
  ({"4": {...}, "3": {...}}).
* g8_final_model_forward.npz: made like G5 (make_golden.py): weights from posepaf.model_init.deterministic_init(model, seed=7)
  at nstack 4, input default_rng(42).random((2, 64, 128, 3)); stores x, last_stage_scale0, last_stage_scale4,
  first_stage_scale0 and n_params.

The reference is imported as make_golden.py imports it: EMPTY stub modules stand in for the third-party imports that are absent
here (cv2, torchvision incl. torchvision.models.densenet, thop); nothing of them is called.  No reference source or bytecode is
written anywhere (sys.dont_write_bytecode).  The fixtures are DATA: arrays and JSON only."""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import PKG, REF, ROOT, _stub  # noqa: E402
sys.path.remove(HERE)

import numpy as np  # noqa: E402


def import_reference_final():
    """-> (the reference's models.posenet_final, its config.config): only the reference tree is on the path while they load"""
    for n in ("cv2", "torchvision", "torchvision.models", "torchvision.models.densenet", "torchvision.transforms", "thop",
              "configobj", "tqdm", "PIL", "PIL.Image"):
        _stub(n)
    if not hasattr(sys.modules["thop"], "profile"):
        sys.modules["thop"].profile = None
    if not hasattr(sys.modules["configobj"], "ConfigObj"):
        sys.modules["configobj"].ConfigObj = None
    sys.path.insert(0, REF)
    import importlib
    cfg = importlib.import_module("config.config")
    net = importlib.import_module("models.posenet_final")
    for name, mod in (("config.config", cfg), ("models.posenet_final", net),
                      ("models.layers_transposed_final", sys.modules["models.layers_transposed_final"])):
        assert mod.__file__.startswith(REF), f"{name} resolved to {mod.__file__}, not the reference"
    return net, cfg


def main():
    net, cfg = import_reference_final()
    sys.path.append(ROOT)
    sys.path.append(PKG)
    import torch
    from posepaf.model_init import deterministic_init
    config = cfg.GetConfig("Canonical")
    manifest, models = {}, {}
    for nstack in (4, 3):
        opt = cfg.TrainingOpt()
        opt.nstack = nstack
        models[nstack] = net.NetworkEval(opt, config, bn=True).eval()
        manifest[str(nstack)] = {k: list(v.shape) for k, v in models[nstack].state_dict().items()}
    with open(os.path.join(HERE, "g8_final_state_dict_manifest.json"), "w") as f:
        json.dump(manifest, f, separators=(",", ":"), sort_keys=True)
    model = models[4]
    deterministic_init(model, seed=7)
    x = torch.from_numpy(np.random.default_rng(42).random((2, 64, 128, 3), dtype=np.float32))
    with torch.no_grad():
        out = model(x)
    np.savez_compressed(os.path.join(HERE, "g8_final_model_forward.npz"), x=x.numpy(),
                        last_stage_scale0=out[-1][0].numpy(), last_stage_scale4=out[-1][4].numpy(),
                        first_stage_scale0=out[0][0].numpy(),
                        n_params=np.int64(sum(p.numel() for p in model.parameters())))
    print("final model: keys", {k: len(v) for k, v in manifest.items()}, "params", sum(p.numel() for p in model.parameters()),
          "out", tuple(out[-1][0].shape), "abs mean", float(out[-1][0].abs().mean()))


if __name__ == "__main__":
    main()
