#!/usr/bin/env python3
"""Network-only forward speed of either architecture: the loop of test_inference_speed.py (the reference's
test_inference_speed.py:91-120 -- one `torch.cuda.synchronize()` per batch, its `Test: [i/n] Time .. Speed ..` line and running
average) with the architecture as an argument.  test_inference_speed.py itself keeps the reference script's surface and the
development variant (models/posenet.py); this script adds

    --arch {posenet,final,auto}     final: models/posenet_final.py, the published 3- / 4-stage IMHN; auto: from the checkpoint's keys

`-p` goes through posepaf.model_init.build_network (strict load; on a mismatch the error names the architecture the keys belong
to), and the JSON line names the architecture and the class that ran.

    python inference_speed.py --arch final [--batch 8] [--iters 50] [-p checkpoint.pth] [--plain] [--no_graph] [--json]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


from test_inference_speed import AverageMeter  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkpoint_path", "-p", default=None, help="reference checkpoint (.pth with a 'weights' entry)")
    ap.add_argument("--arch", choices=("posenet", "final", "auto"), default="posenet",
                    help="network architecture: posenet = models/posenet.py (the development variant, default), final = models/posenet_final.py "
                         "(the published 3- / 4-stage IMHN), auto = decided from the checkpoint's keys")
    ap.add_argument("--batch", type=int, default=8, help="images per batch (config/config.py batch_size of the reference: 8)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3, help="untimed batches (kernel-choice tuning happens in the first)")
    ap.add_argument("--size", type=int, nargs=2, default=[512, 512], metavar=("H", "W"))
    ap.add_argument("--plain", action="store_true", help="the nn.Module on PyTorch-ROCm instead of the fused model")
    ap.add_argument("--no_graph", action="store_true")
    ap.add_argument("--json", action="store_true", help="one JSON summary line at the end")
    for flag in ("--opt-level", "--keep-batchnorm-fp32", "--loss-scale", "--output", "--max_grad_norm"):   # reference flags, unused
        ap.add_argument(flag, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--resume", "-r", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("inference_speed.py needs the GPU (there is no CPU path)")
    from posepaf import fused_model as fm
    dev = torch.device("cuda", 0)
    arch = a.arch
    if a.checkpoint_path or arch == "auto":
        from posepaf.model_init import build_network
        try:
            net, arch = build_network(arch, a.checkpoint_path)   # :70-71 (strict)
        except ValueError as e:
            raise SystemExit(str(e))
        model = net if a.plain else fm.FusedIMHN.from_network(net).eval()
        model = model.to(device=dev, dtype=torch.float16).to(memory_format=torch.channels_last)
    else:
        model = fm.build_inference_model(dev, fused=not a.plain, arch=arch)
    h, w = a.size
    g = torch.Generator(device="cpu").manual_seed(0)
    images = torch.rand(a.batch, h, w, 3, generator=g).to(dev).half()          # the loader's normalised NHWC images (:95-97)
    with torch.no_grad():
        if not a.plain and fm.load_table():
            print("kernel-choice table", fm.table_hash(), "loaded", file=sys.stderr)
        for _ in range(max(1, a.warmup)):
            model(images)
        torch.cuda.synchronize()
        run = model
        if not a.no_graph:
            run = fm.GraphedForward(model, images, warmup=1)
        batch_time = AverageMeter()
        torch.cuda.synchronize()
        end = time.time()
        for i in range(a.iters):
            run(images)
            torch.cuda.synchronize()            # :104: the reference times each batch to its completion
            batch_time.update(time.time() - end)
            end = time.time()
            print("==================>Test: [{0}/{1}]\tTime {bt.val:.3f} ({bt.avg:.3f})\tSpeed {2:.3f} ({3:.3f})\t".format(
                i, a.iters, a.batch / batch_time.val, a.batch / batch_time.avg, bt=batch_time))
    if a.json:
        print(json.dumps({"metric": "network-only forward images/sec", "value": a.batch / batch_time.avg, "batch": a.batch,
                          "size": [h, w], "iters": a.iters, "arch": arch, "model": "nn.Module (PyTorch-ROCm)" if a.plain else type(model).__name__,
                          "launch": "eager" if a.no_graph else "hipGraph replay", "dtype": "f16",
                          "conv_table": None if a.plain else fm.table_hash()}))
    return a.batch / batch_time.avg


if __name__ == "__main__":
    main()
