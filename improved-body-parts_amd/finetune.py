#!/usr/bin/env python3
"""finetune.py -- a small fine-tune loop on the MI355X: joints -> targets -> loss -> gradients -> optimizer step.

    python finetune.py --synthetic 64 --batch 8 --sizes 128x128 --steps 20 \\
        [--stages 4] [--train all|heads] [--lr 2.5e-5] [--loss device|torch] [-p weights.pth] [--seed 0] [--save out.pth]
        [--augment [--src_sizes HxW[,HxW...]]]
    python finetune.py --model fused --train heads --synthetic 64 --batch 8 --sizes 512x512 --steps 20 \\
        [--arch posenet|final|auto] [-p weights.pth] [--stages 4] [--loss_scale auto|N|dynamic] [--wgrad device|multi|torch]
        [--update torch|device] [--graph] [--growth_interval 2000]
    python finetune.py --ann_file person_keypoints_train2017.json --img_dir train2017 [--limit N] --batch 8 --sizes 512x512 --steps 20 ...

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
  --augment       the reference's data transformer on the device (posepaf/augment.py, pp_augment_batch) in front of every step: per
                  step and image an AugmentSelection.random drawn from random.Random seeded by --seed and the step (tint_prob = 0:
                  the colour distortion is out of scope) warps the raw uint8 image and its two masks to --sizes, maps the joints, and
                  the loss takes mask = mask_miss (--loss torch takes the same mask).  --src_sizes gives the source sizes (image i
                  has the (i mod n)-th; default: --sizes), ragged in one slot.  Synthetic masks: mask_miss is 255 with a few seeded
                  zero rectangles, mask_all 255 inside each person's joint bounding box; objpos is the centre of person 0's box and
                  scale_provided that box's height over the output height.  The targets are rendered from the transformed joints
                  and channel 48 receives the eroded mask_all plane after the render (the renderer zeroes that channel)

  --ann_file F --img_dir D [--limit N]   real data instead of --synthetic (implies --augment): the person annotations of the first N
                  images that have one (all without --limit), read with `json`; the images decoded with PIL (RGB -> BGR), ragged in
                  one slot.  posepaf/coco_masks.py restates the reference's data/coco_masks_hdf5.py on the way: training_instances
                  picks the main persons (each is one instance: objpos and scale_provided of the main person drive the matrix, the
                  joints of everyone with keypoints are rendered), and mask_miss / mask_all are rasterised on the device from the
                  polygons and the crowd's run-length code (pp_coco_masks_u8) into the slots the transformer
                  reads.  An image with more than one crowd annotation is skipped and counted, as is an instance with more people
                  than the renderer takes.  Step k takes instances k, k + ceil(n / batch), ..., as --synthetic takes images

  --model fused   (needs --train heads) the fused fp16 forward (posepaf/fused_model.py, prediction-merge fold off) takes the place of
                  the float32 module: posepaf/head_train.HeadTrainer runs the forward under no_grad, pp_focal_l2_terms /
                  pp_focal_l2_grad with the term weights times --loss_scale, pp_head_wgrad_f16 per head and
                  the same SGD on float32 masters of the twenty heads.  --loss_scale auto | a power of two (auto: the largest that
                  keeps a binary16 gradient finite for predictions in [-1, 2]); --wgrad torch forms dw / db from the same captured
                  tensors with a float64 matmul, for A/B; --arch as evaluate.py's.  The data path (--synthetic, --augment, --ann_file)
                  is the same; --save writes {'weights': HeadTrainer.state_dict()}, which evaluate.py -p loads.  The JSON line gains
                  "model": "fused", "wgrad", "loss_scale" and "skipped_steps" (steps whose gradient was not finite: no update)
  --update device (with --model fused) pp_head_update_f32 in place of torch.optim.SGD.step(), the masked restore and the fp16 copies;
                  --wgrad multi: every head's gradient in one pp_head_wgrad_multi_f16 call; --loss_scale dynamic (needs --update device
                  and --wgrad multi or torch): apex's dynamic scaler on the device, doubling after --growth_interval finite steps;
                  --graph (implies --update device): the first step eager, the second captured into one graph, the rest replayed, the
                  losses read once after the last step.  The JSON line gains "graph", "update",
                  "graph_replays" and "loss_scale_last"
  --train heads+conv (with --model fused --arch final | auto) the 3 x 3 convolution in front of every head is trained as well:
                  pp_head_dgrad_f16 and pp_conv3x3_wgrad_f16 per layer, float32 masters of the folded weight and bias in the same
                  flat tensors, update, scale and capture as the heads
  --train heads+conv2 (the same preconditions) the 3 x 3 convolution in front of that one as well: pp_conv3x3_dgrad_f16 takes the
                  gradient through the upper convolution, --update device goes through pp_layer_update_f32

Prints one JSON line: losses (per step), loss_first, loss_last, grad_norm_first (L2 norm of the updated parameters' gradients at
step 0), seconds, steps_per_s (steady state: from the second step on, with --graph from the third, so without the first step's set-up
and the capture; null when no such step was made), loss, train, images_per_step (and "augment": true with --augment; with --ann_file
also "source": "annotations", instances, instances_skipped, images_skipped_multi_crowd).  Combinations it does not support end with a
message before the GPU is touched.
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
    ap.add_argument("--train", choices=("all", "heads", "heads+conv", "heads+conv2"), default="all",
                    help="heads+conv (with --model fused --arch final | auto): the 3 x 3 convolution in front of every head as well; "
                         "heads+conv2: both 3 x 3 convolutions below every head")
    ap.add_argument("--lr", type=float, default=2.5e-5)
    ap.add_argument("--loss", choices=("device", "torch"), default="device")
    ap.add_argument("-p", "--checkpoint_path", default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", default=None, help="write {'weights': state_dict} here after the last step")
    ap.add_argument("--augment", action="store_true", help="run the device data transformer in front of every step")
    ap.add_argument("--src_sizes", default=None, help="with --augment: source sizes HxW[,HxW...] (default: --sizes)")
    ap.add_argument("--ann_file", default=None, help="COCO person_keypoints JSON with segmentations: real data (implies --augment)")
    ap.add_argument("--img_dir", default=None, help="directory of the annotation's images")
    ap.add_argument("--limit", type=int, default=0, help="with --ann_file: only the first N images that have a person annotation")
    ap.add_argument("--model", choices=("plain", "fused"), default="plain", help="fused: train the heads on the fused fp16 forward")
    ap.add_argument("--arch", choices=("posenet", "final", "auto"), default="posenet", help="with --model fused: the architecture")
    ap.add_argument("--loss_scale", default="auto", help="with --model fused: 'auto', a power of two or 'dynamic'")
    ap.add_argument("--wgrad", choices=("device", "torch", "multi"), default="device",
                    help="with --model fused: pp_head_wgrad_f16 per head, the torch A/B form, or pp_head_wgrad_multi_f16 once")
    ap.add_argument("--update", choices=("torch", "device"), default=None, help="with --model fused: torch.optim.SGD (default) or pp_head_update_f32")
    ap.add_argument("--graph", action="store_true", help="with --model fused: capture the step in a graph (implies --update device)")
    ap.add_argument("--growth_interval", type=int, default=None, help="with --loss_scale dynamic: finite steps before the scale doubles (2000)")
    a = ap.parse_args(argv)
    if a.ann_file:
        a.augment = True
    a.update_given, a.growth_given = a.update is not None, a.growth_interval is not None
    if a.update is None:
        a.update = "device" if a.graph else "torch"
    if a.growth_interval is None:
        a.growth_interval = 2000
    return a


def parse_src_sizes(text):
    """'80x96,64x64' -> [(80, 96), (64, 64)], None when it is not such a list"""
    try:
        sizes = [tuple(int(v) for v in item.lower().split("x")) for item in text.split(",")]
    except ValueError:
        return None
    if not sizes or any(len(s) != 2 or not (8 <= s[0] <= 32768 and 8 <= s[1] <= 32768) for s in sizes):
        return None
    return sizes


def refusals(a):
    """what this script does not do, as messages; empty when the arguments are fine (nothing here touches the GPU)"""
    from posepaf._lib import LOSS_MAX_STACKS
    out = []
    if a.ann_file and a.synthetic:
        out.append("--synthetic and --ann_file are two data sources: give one")
    elif a.ann_file:
        if not os.path.isfile(a.ann_file):
            out.append(f"--ann_file {a.ann_file}: no such file")
        if not a.img_dir:
            out.append("--ann_file needs --img_dir")
        elif not os.path.isdir(a.img_dir):
            out.append(f"--img_dir {a.img_dir}: no such directory")
        if a.src_sizes is not None:
            out.append("--src_sizes belongs to --synthetic: with --ann_file the images have their own sizes")
        if a.limit < 0:
            out.append("--limit must be at least 0")
    elif a.img_dir or a.limit:
        out.append("--img_dir and --limit belong to --ann_file")
    elif a.synthetic < 1:
        out.append("a data source is needed: --synthetic N (N >= 1), or --ann_file F --img_dir D (the reference's HDF5 dataset "
                   "reader is not part of this script)")
    if a.batch < 1 or a.steps < 1:
        out.append("--batch and --steps must be at least 1")
    if a.model == "fused":
        from posepaf.head_train import is_power_of_two
        if a.train not in ("heads", "heads+conv", "heads+conv2"):
            out.append("--model fused trains the heads, or with --train heads+conv the convolution in front of each as well (the fused "
                       "model has no other backward): pass --train heads or --train heads+conv (heads+conv2: both convolutions)")
        if a.train in ("heads+conv", "heads+conv2") and a.arch not in ("final", "auto"):
            out.append(f"--train {a.train} needs --arch final (or auto): on posenet an SE block stands between the convolution and the head")
        if a.loss != "device":
            out.append("--model fused takes the loss gradient from pp_focal_l2_grad: --loss torch belongs to --model plain")
        if a.loss_scale not in ("auto", "dynamic") and not is_power_of_two(a.loss_scale):
            out.append(f"--loss_scale {a.loss_scale}: 'auto', 'dynamic' or a power of two (2^-24 .. 2^24)")
        if a.graph and a.update != "device":
            out.append("--graph captures the device update: it does not go with --update torch")
        if a.loss_scale == "dynamic" and (a.update != "device" or a.wgrad == "device"):
            out.append("--loss_scale dynamic needs --update device (or --graph) and --wgrad multi or torch: pp_head_wgrad_f16 takes its "
                       "factor from the host")
        if a.growth_interval < 0:
            out.append("--growth_interval must be at least 0")
        elif a.growth_given and a.loss_scale != "dynamic":
            out.append("--growth_interval belongs to --loss_scale dynamic")
    elif a.train in ("heads+conv", "heads+conv2"):
        out.append(f"--train {a.train} belongs to --model fused (--arch final | auto)")
    elif a.arch != "posenet" or a.loss_scale != "auto" or a.wgrad != "device" or a.graph or a.update_given or a.growth_given:
        out.append("--arch, --loss_scale, --wgrad, --update, --graph and --growth_interval belong to --model fused")
    sizes = a.sizes.split(",")
    try:
        h, w = (int(v) for v in sizes[0].lower().split("x"))
    except ValueError:
        h = w = 0
    if len(sizes) != 1:
        out.append("--sizes takes one size: a step is one batch of equally sized images")
    elif h < 64 or w < 64 or h % 64 or w % 64:
        out.append(f"--sizes {a.sizes}: both sides must be positive multiples of 64 (the coarsest of the five scales is 1/64 of the image)")
    if a.ann_file:
        pass                                                         # the sources have the images' own sizes
    elif a.src_sizes is not None and not a.augment:
        out.append("--src_sizes belongs to --augment: without it the images have the one size of --sizes")
    elif a.augment and parse_src_sizes(a.src_sizes if a.src_sizes is not None else a.sizes) is None:
        out.append(f"--src_sizes {a.src_sizes}: a comma-separated list of HxW with both sides in 8..32768")
    if not 1 <= a.stages <= LOSS_MAX_STACKS:
        out.append(f"--stages must be 1..{LOSS_MAX_STACKS} (the loss kernel walks at most {LOSS_MAX_STACKS} stacks)")
    if not (a.lr > 0 and a.lr == a.lr and a.lr != float("inf")):
        out.append("--lr must be a positive number")
    if a.checkpoint_path and not os.path.isfile(a.checkpoint_path):
        out.append(f"-p {a.checkpoint_path}: no such file")
    if a.save and not os.path.isdir(os.path.dirname(os.path.abspath(a.save))):
        out.append(f"--save {a.save}: its directory does not exist")
    return out


def torch_terms(torch, preds, target, mask=None):
    """the contract of pp_focal_l2_terms on stock operators -> (T, K, B) float64 that torch differentiates.  mask: float32 (B, H, W)
    or None, resampled bilinearly (align_corners = False) in float64 with values < 0.5 set to 0"""
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
            if mask is not None:
                M = F.interpolate(mask[:, None].double(), size=tuple(pred.shape[-2:]), mode="bilinear", align_corners=False)
                v = v * torch.where(M < 0.5, torch.zeros_like(M), M)
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


def augment_data(a, H, W):
    """--augment's N synthetic samples on the host: uint8 images and masks in one slot, sizes (2, N), float64 joints, n_people, objpos,
    scale_provided.  Image i has the (i mod n)-th source size; its people are synth.random_people of that size."""
    from posepaf import synth, synth_device
    src = parse_src_sizes(a.src_sizes if a.src_sizes is not None else a.sizes)
    N = a.synthetic
    slot_h, slot_w = max(s[0] for s in src), max(s[1] for s in src)
    images, mask_miss = np.zeros((N, slot_h, slot_w, 3), np.uint8), np.zeros((N, slot_h, slot_w), np.uint8)
    mask_all, sizes = np.zeros((N, slot_h, slot_w), np.uint8), np.zeros((2, N), np.int32)
    people, objpos, scale_provided = [], [], []
    for i in range(N):
        h, w = src[i % len(src)]
        sizes[:, i] = h, w
        images[i, :h, :w] = np.frombuffer(np.random.default_rng(10_000 + 1000 * a.seed + i).bytes(h * w * 3), np.uint8).reshape(h, w, 3)
        pj = synth.random_people(PEOPLE[i % len(PEOPLE)], np.random.default_rng(20_000 + 1000 * a.seed + i), img_h=h, img_w=w)
        people.append(pj)
        rng = np.random.default_rng(30_000 + 1000 * a.seed + i)
        mask_miss[i, :h, :w] = 255
        for _ in range(3):                                       # a few zero rectangles: regions without annotation
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            mask_miss[i, y:min(h, y + int(rng.integers(4, 1 + max(4, h // 4)))), x:min(w, x + int(rng.integers(4, 1 + max(4, w // 4))))] = 0
        boxes = []
        for p in pj:
            xy = p[p[:, 2] < 2, :2]
            if len(xy) == 0:
                continue
            x0, y0, x1, y1 = xy[:, 0].min(), xy[:, 1].min(), xy[:, 0].max(), xy[:, 1].max()
            boxes.append((x0, y0, x1, y1))
            mask_all[i, max(0, int(np.floor(y0))):min(h, int(np.ceil(y1)) + 1), max(0, int(np.floor(x0))):min(w, int(np.ceil(x1)) + 1)] = 255
        x0, y0, x1, y1 = boxes[0] if boxes else (0.0, 0.0, float(w), float(h))
        objpos.append(((x0 + x1) / 2, (y0 + y1) / 2))
        scale_provided.append(max(float(y1 - y0), 1.0) / H)
    joints = np.zeros((N, max(PEOPLE), 18, 3), np.float64)
    joints, n_people = synth_device.pack_joints(people, max(PEOPLE), joints_out=joints)
    return images, mask_miss, mask_all, sizes, joints, n_people, objpos, scale_provided


def read_bgr(path):
    """cv2.imread(path) as evaluate.py reads it: PIL, RGB -> BGR uint8 (H, W, 3)"""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))[:, :, ::-1]


def annotation_data(a, dev):
    """--ann_file's data, staged on the device once: the images ragged in one slot, mask_miss / mask_all rasterised into the same slots
    by pp_coco_masks_u8, sizes (2, images); per INSTANCE (coco_masks.training_instances) its image, float64 joints, n_people, and the
    main person's objpos and scale_provided.
    -> (images, mask_miss, mask_all, sizes, joints, n_people, objpos, scale_provided, image_of, stats)"""
    import torch
    from posepaf import coco_masks, synth_device
    doc = json.load(open(a.ann_file))
    person = [c["id"] for c in doc.get("categories", []) if c.get("name") == "person"] or [1]
    by_image = {}
    for ann in doc.get("annotations", []):
        if ann.get("category_id") in person:
            by_image.setdefault(ann["image_id"], []).append(ann)
    metas = {im["id"]: im for im in doc["images"]}
    ids = sorted(by_image)
    if a.limit:
        ids = ids[:a.limit]
    kept, multi_crowd = [], 0
    for i in ids:
        if sum(1 for ann in by_image[i] if int(ann.get("iscrowd", 0)) == 1) > 1:
            multi_crowd += 1                 # the reference's make_mask raises on such an image
        else:
            kept.append(i)
    images_meta, anns = [metas[i] for i in kept], [by_image[i] for i in kept]
    instances, skipped = coco_masks.training_instances(images_meta, anns) if kept else ([], 0)
    if not instances:
        raise SystemExit(f"finetune.py: --ann_file {a.ann_file}: no training instance (a person with 5 keypoints and an area of "
                         f"32 x 32) in {len(ids)} images")
    hw = [(int(m["height"]), int(m["width"])) for m in images_meta]
    try:
        packed = coco_masks.pack_segmentations(anns, hw, names=kept)
    except coco_masks.PosePafError as e:
        raise SystemExit(f"finetune.py: --ann_file {a.ann_file}: {e}")
    slot_h, slot_w = max(h for h, _ in hw), max(w for _, w in hw)
    images = np.zeros((len(kept), slot_h, slot_w, 3), np.uint8)
    for k, (m, (h, w)) in enumerate(zip(images_meta, hw)):
        im = read_bgr(os.path.join(a.img_dir, m["file_name"]))
        if im.shape[:2] != (h, w):
            raise SystemExit(f"finetune.py: {m['file_name']}: decoded size {im.shape[:2]} != annotation {(h, w)}")
        images[k, :h, :w] = im
    packed = coco_masks.to_device(packed, dev)
    mask_miss, mask_all = coco_masks.masks_device(packed, (slot_h, slot_w))
    most = max(len(inst["joints"]) for inst in instances)
    joints, n_people = synth_device.pack_joints([inst["joints"] for inst in instances], most,
                                                joints_out=np.zeros((len(instances), most, 18, 3), np.float64))
    stats = {"source": "annotations", "instances": len(instances), "instances_skipped": skipped, "images_skipped_multi_crowd": multi_crowd}
    return (images, mask_miss, mask_all, packed["sizes"], joints, n_people, [inst["objpos"][0] for inst in instances],
            [inst["scale_provided"][0] for inst in instances], torch.tensor([inst["image"] for inst in instances], device=dev), stats)


def main(argv=None):
    a = parse(argv)
    bad = refusals(a)
    if bad:
        raise SystemExit("finetune.py: " + "; ".join(bad))
    import torch
    from posepaf import _lib, synth, synth_device, val_loss
    from posepaf.model_init import build_network
    fused = a.model == "fused"
    try:
        net, _ = build_network(a.arch if fused else "posenet", a.checkpoint_path, 7 + a.seed, nstack=a.stages)
    except (ValueError, KeyError, RuntimeError) as e:
        raise SystemExit(f"finetune.py: -p {a.checkpoint_path}: {e}")
    if not torch.cuda.is_available():
        raise SystemExit("finetune.py needs an MI355X: there is no CPU path")
    dev = torch.device("cuda", 0)
    L = _lib.load()
    H, W = (int(v) for v in a.sizes.lower().split("x"))
    B, N = a.batch, a.synthetic
    image_of, stats = None, {}
    heads = a.train == "heads"
    if fused:
        from posepaf import head_train
        try:
            tr = head_train.HeadTrainer(net, dev, lr=a.lr, momentum=MOMENTUM, weight_decay=WEIGHT_DECAY, wgrad=a.wgrad,
                                        loss_scale=a.loss_scale if a.loss_scale in ("auto", "dynamic") else float(a.loss_scale),
                                        update=a.update, graph=a.graph, growth_interval=a.growth_interval, train=a.train)
        except _lib.PosePafError as e:
            raise SystemExit(f"finetune.py: --model fused: {e}")
        a.stages = tr.T
        # the per-shape kernel choices are timed on the first forward: runs that share POSEPAF_CACHE_DIR execute the same kernels
        from posepaf import fused_model
        fused_model.load_table()
        # the few layer shapes no fused kernel takes (3 x 3 on a 1 x 1 map) run on MIOpen, whose default solver there does not add
        # in a fixed order: with this flag a step is the same bits from run to run
        torch.backends.cudnn.deterministic = True
    else:
        net = net.float().to(dev).eval()
        pn = net.posenet
        for name, p in pn.named_parameters():
            p.requires_grad_(name.startswith("outs.") or not heads)
        params = [p for p in pn.parameters() if p.requires_grad]
        opt = torch.optim.SGD(params, lr=a.lr, momentum=MOMENTUM, weight_decay=WEIGHT_DECAY)

    # the data: N images and their people, staged on the device once
    if a.augment:
        import random
        from posepaf import augment
        if a.ann_file:                                            # N counts the instances; image_of[i] is the image of instance i
            images, mask_miss, mask_all, sizes, joints, n_people, objpos, scale_provided, image_of, stats = annotation_data(a, dev)
            N = len(objpos)
        else:
            images, mask_miss, mask_all, sizes, joints, n_people, objpos, scale_provided = augment_data(a, H, W)
            mask_miss, mask_all, sizes = torch.from_numpy(mask_miss).to(dev), torch.from_numpy(mask_all).to(dev), torch.from_numpy(sizes).to(dev)
        draw_params = augment.TransformParams(tint_prob=0.0)      # the colour distortion is out of scope: never drawn
    else:
        images = np.stack([np.frombuffer(np.random.default_rng(10_000 + 1000 * a.seed + i).bytes(H * W * 3), np.uint8).reshape(H, W, 3)
                           for i in range(N)])
        people = [synth.random_people(PEOPLE[i % len(PEOPLE)], np.random.default_rng(20_000 + 1000 * a.seed + i), img_h=H, img_w=W) for i in range(N)]
        joints, n_people = synth_device.pack_joints(people, max(PEOPLE))
    images, joints, n_people = torch.from_numpy(images).to(dev), torch.from_numpy(joints).to(dev), torch.from_numpy(n_people).to(dev)

    # step k takes images k, k + ceil(N / B), k + 2 ceil(N / B) ...: the people of an image rise with its index (PEOPLE), so consecutive
    # images in one batch would make the batches, and their losses, as different as 1 + 2 people are from 3 + 4; ceil(N / B) steps see all
    per_pass = -(-N // B)
    losses, grad_norm_first = [], None
    unsteady, t_steady = (2 if a.graph else 1), None      # steps in front of the steady state: the eager first one, and the capture
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for step in range(a.steps):
        if step == unsteady:
            torch.cuda.synchronize(dev)
            t_steady = time.perf_counter()
        idx = (step + torch.arange(B, device=dev) * per_pass) % N
        mask = None
        if a.augment:
            # raw uint8 slots -> (x, target, mask) on the device; the draws and the matrices are the only host work
            rng = random.Random(1_000_003 * a.seed + step)
            host_idx = [(step + i * per_pass) % N for i in range(B)]
            augs = [augment.AugmentSelection.random(draw_params, rng) for _ in range(B)]
            im = idx if image_of is None else image_of[idx]
            x, mask, fg, moved = augment.transform_batch(images[im], mask_miss[im], mask_all[im], sizes[:, im].contiguous(), joints[idx],
                                                         n_people[idx], augs, [objpos[i] for i in host_idx],
                                                         [scale_provided[i] for i in host_idx], (H, W))
            target = synth_device.render_scenes(moved, n_people[idx], H // 4, W // 4, dtype=torch.float16, flip=False, noise=0.0,
                                                reverse_kp=True)
            target[:, 0, 48].copy_(fg)                            # after the render, on the same stream: the renderer zeroes channel 48
        else:
            raw, x = images[idx], torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
            _lib.check(L.pp_preprocess_u8(C.c_void_p(raw.data_ptr()), C.c_void_p(x.data_ptr()), _lib.PP_F32, B, H, W, 64, 0, 0,
                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            target = synth_device.render_scenes(joints[idx], n_people[idx], H // 4, W // 4, dtype=torch.float16, flip=False, noise=0.0,
                                                reverse_kp=True)
        if fused:
            losses.append(tr.step(x, target, mask))
            if step == 0:
                grad_norm_first = tr.grad_norm()
            continue
        preds = forward(pn, x, heads)
        terms = val_loss.focal_l2_terms(preds, target, mask=mask) if a.loss == "device" else torch_terms(torch, preds, target[:, 0], mask)
        loss = val_loss.combine(terms, (1,) * a.stages)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if step == 0:
            grad_norm_first = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params))
        opt.step()
        losses.append(loss.detach())
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    dt = t1 - t0
    losses = [float(v) for v in losses]
    if fused:
        fused_model.save_table()
    if a.save:
        torch.save({"weights": {k: v.detach().cpu() for k, v in (tr if fused else net).state_dict().items()}}, a.save)
    result = {"losses": losses, "loss_first": losses[0], "loss_last": losses[-1], "grad_norm_first": float(grad_norm_first),
              "seconds": dt, "loss": a.loss, "train": a.train, "images_per_step": B, "steps": a.steps, "stages": a.stages, "lr": a.lr}
    if fused:
        result.update({"model": "fused", "wgrad": a.wgrad, "loss_scale": "dynamic" if tr.dynamic else tr.loss_scale_for(B),
                       "skipped_steps": int(tr.skipped_steps), "graph": bool(a.graph), "update": a.update, "graph_replays": tr.graph_replays,
                       "loss_scale_last": float(tr.loss_scale_now())})
    result["steps_per_s"] = (a.steps - unsteady) / (t1 - t_steady) if t_steady is not None else None
    if a.augment:
        result["augment"] = True
    result.update(stats)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
