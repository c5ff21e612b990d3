#!/usr/bin/env python3
"""finetune.py -- a small fine-tune loop on the MI355X: joints -> targets -> loss -> gradients -> optimizer step.

    python finetune.py --synthetic 64 --batch 8 --sizes 128x128 --steps 20 \\
        [--stages 4] [--train all|heads] [--lr 2.5e-5] [--loss device|torch] [-p weights.pth] [--seed 0] [--save out.pth]

Per step: a batch of synthetic images (random uint8 pixels, divided by 255 on the device by pp_preprocess_u8) and their
synth.random_people joints; the targets rendered from the joints by pp_render_scenes (one sample, no noise, reverse_kp, as
evaluate.py --val_loss renders them); the plain models/posenet.PoseNet in float32 (key-compatible: --save writes a checkpoint
evaluate.py -p loads); val_loss.focal_l2_terms -> combine -> backward() (pp_focal_l2_terms, pp_focal_l2_grad) -> SGD with momentum
0.9 and weight decay 1e-4, as the reference's train.py:59.  Only the module's own layers run on torch.

  --train all     every parameter is updated.  Batch normalisation stays in eval mode (the stored statistics): a fine-tune at these
                  batch sizes, and the same function of the weights in both --train modes
  --train heads   everything but the 1 x 1 heads (posenet.outs) runs under no_grad; only the heads are updated
  --loss torch    a torch formulation of the same contract (windows summed in float64 and rounded once to
                  float32, the foreground test in float32, everything behind in float64) differentiated by torch -- for A/B
  -p              a reference checkpoint (.pth with a 'weights' entry); without one the deterministic initialisation

Prints one JSON line: losses (per step), loss_first, loss_last, grad_norm_first (L2 norm of the updated parameters' gradients at
step 0), seconds, loss, train, images_per_step.  Combinations it does not support end with a message before the GPU is touched.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

PEOPLE = (1, 2, 3, 4, 5, 6)          # people of image i: PEOPLE[i mod 6]
MOMENTUM, WEIGHT_DECAY = 0.9, 1e-4   # train.py:59 of the reference


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--synthetic", type=int, default=0, help="number of synthetic images; step k takes every ceil(N / batch)-th from image k")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--sizes", default="128x128", help="image size HxW: one size, both sides multiples of 64")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--stages", type=int, default=4, help="hourglass stages of the network (a checkpoint must hold as many)")
    ap.add_argument("--train", choices=("all", "heads"), default="all")
    ap.add_argument("--lr", type=float, default=2.5e-5)
    ap.add_argument("--loss", choices=("device", "torch"), default="device")
    ap.add_argument("-p", "--checkpoint_path", default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", default=None, help="write {'weights': state_dict} here after the last step")
    return ap.parse_args(argv)


def refusals(a):
    """what this script does not do, as messages; empty when the arguments are fine (nothing here touches the GPU)"""
    from posepaf._lib import LOSS_MAX_STACKS
    out = []
    if a.synthetic < 1:
        out.append("--synthetic N (N >= 1) is the only data source: the data transformer of the reference is not part of this script")
    if a.batch < 1 or a.steps < 1:
        out.append("--batch and --steps must be at least 1")
    sizes = a.sizes.split(",")
    try:
        h, w = (int(v) for v in sizes[0].lower().split("x"))
    except ValueError:
        h = w = 0
    if len(sizes) != 1:
        out.append("--sizes takes one size: a step is one batch of equally sized images")
    elif h < 64 or w < 64 or h % 64 or w % 64:
        out.append(f"--sizes {a.sizes}: both sides must be positive multiples of 64 (the coarsest of the five scales is 1/64 of the image)")
    if not 1 <= a.stages <= LOSS_MAX_STACKS:
        out.append(f"--stages must be 1..{LOSS_MAX_STACKS} (the loss kernel walks at most {LOSS_MAX_STACKS} stacks)")
    if not (a.lr > 0 and a.lr == a.lr and a.lr != float("inf")):
        out.append("--lr must be a positive number")
    if a.checkpoint_path and not os.path.isfile(a.checkpoint_path):
        out.append(f"-p {a.checkpoint_path}: no such file")
    if a.save and not os.path.isdir(os.path.dirname(os.path.abspath(a.save))):
        out.append(f"--save {a.save}: its directory does not exist")
    return out


def torch_terms(torch, preds, target):
    """the contract of pp_focal_l2_terms on stock operators, without a mask -> (T, K, B) float64 that torch differentiates"""
    import torch.nn.functional as F
    from posepaf.val_loss import KEYPOINT_TASK_WEIGHT, MULTI_TASK_WEIGHT
    cw = torch.ones(50, dtype=torch.float64, device=target.device)
    cw[48], cw[30:48] = MULTI_TASK_WEIGHT, KEYPOINT_TASK_WEIGHT
    t64 = target.double()
    rows = []
    for t, stack in enumerate(preds):
        row = []
        for pred in stack:
            G = F.adaptive_avg_pool2d(t64, pred.shape[-2:]).float()          # float64 window sums, one rounding
            fg = torch.ge(G, 0.01)                                            # float32 against the scalar, as the reference
            p = pred.double()
            d = p - G.double()
            v = d * d * torch.abs(1.0 - torch.where(fg, p, 1.0 - p)) * cw[None, :, None, None]
            row.append(v.sum(dim=(1, 2, 3)))
        rows.append(torch.stack(row))
    return torch.stack(rows)


def forward(pn, x, heads_only):
    """models/posenet.PoseNet.forward; heads_only: everything but pn.outs under no_grad (the chain to the next stage runs on the
    detached predictions), then the heads alone with grad"""
    import torch
    if not heads_only:
        return pn(x)
    feats_of = []
    with torch.no_grad():
        y = pn.pre(x.permute(0, 3, 1, 2))
        caches = None
        for t in range(pn.num_stages):
            hg = pn.hourglass[t](y)
            if caches is not None:
                hg = [a + c for a, c in zip(hg, caches)]
            feats = pn.features[t](hg)
            feats_of.append(feats)
            if t != pn.num_stages - 1:
                caches = [pn.merge_preds[t][s](pn.outs[t][s](feats[s])) + pn.merge_features[t][s](feats[s]) for s in range(pn.num_scales)]
                y = y + caches[0]
    return [[head(f) for head, f in zip(pn.outs[t], feats_of[t])] for t in range(pn.num_stages)]


def main(argv=None):
    a = parse(argv)
    bad = refusals(a)
    if bad:
        raise SystemExit("finetune.py: " + "; ".join(bad))
    import torch
    from posepaf import _lib, synth, synth_device, val_loss
    from posepaf.model_init import build_network
    try:
        net, _ = build_network("posenet", a.checkpoint_path, 7 + a.seed, nstack=a.stages)
    except (ValueError, KeyError, RuntimeError) as e:
        raise SystemExit(f"finetune.py: -p {a.checkpoint_path}: {e}")
    if not torch.cuda.is_available():
        raise SystemExit("finetune.py needs an MI355X: there is no CPU path")
    dev = torch.device("cuda", 0)
    L = _lib.load()
    H, W = (int(v) for v in a.sizes.lower().split("x"))
    B, N = a.batch, a.synthetic
    net = net.float().to(dev).eval()
    pn = net.posenet
    heads = a.train == "heads"
    for name, p in pn.named_parameters():
        p.requires_grad_(name.startswith("outs.") or not heads)
    params = [p for p in pn.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=a.lr, momentum=MOMENTUM, weight_decay=WEIGHT_DECAY)

    # the data: N images and their people, staged on the device once
    images = np.stack([np.frombuffer(np.random.default_rng(10_000 + 1000 * a.seed + i).bytes(H * W * 3), np.uint8).reshape(H, W, 3)
                       for i in range(N)])
    people = [synth.random_people(PEOPLE[i % len(PEOPLE)], np.random.default_rng(20_000 + 1000 * a.seed + i), img_h=H, img_w=W) for i in range(N)]
    joints, n_people = synth_device.pack_joints(people, max(PEOPLE))
    images, joints, n_people = torch.from_numpy(images).to(dev), torch.from_numpy(joints).to(dev), torch.from_numpy(n_people).to(dev)

    # step k takes images k, k + ceil(N / B), k + 2 ceil(N / B) ...: the people of an image rise with its index (PEOPLE), so consecutive
    # images in one batch would make the batches, and their losses, as different as 1 + 2 people are from 3 + 4; ceil(N / B) steps see all
    per_pass = -(-N // B)
    losses, grad_norm_first = [], None
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for step in range(a.steps):
        idx = (step + torch.arange(B, device=dev) * per_pass) % N
        raw, x = images[idx], torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
        _lib.check(L.pp_preprocess_u8(C.c_void_p(raw.data_ptr()), C.c_void_p(x.data_ptr()), _lib.PP_F32, B, H, W, 64, 0, 0,
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        target = synth_device.render_scenes(joints[idx], n_people[idx], H // 4, W // 4, dtype=torch.float16, flip=False, noise=0.0,
                                            reverse_kp=True)
        preds = forward(pn, x, heads)
        terms = val_loss.focal_l2_terms(preds, target) if a.loss == "device" else torch_terms(torch, preds, target[:, 0])
        loss = val_loss.combine(terms, (1,) * a.stages)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if step == 0:
            grad_norm_first = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params))
        opt.step()
        losses.append(loss.detach())
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    losses = [float(v) for v in losses]
    if a.save:
        torch.save({"weights": {k: v.detach().cpu() for k, v in net.state_dict().items()}}, a.save)
    print(json.dumps({"losses": losses, "loss_first": losses[0], "loss_last": losses[-1], "grad_norm_first": float(grad_norm_first),
                      "seconds": dt, "loss": a.loss, "train": a.train, "images_per_step": B, "steps": a.steps, "stages": a.stages, "lr": a.lr}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
