#!/usr/bin/env python3
"""loss_probe.py -- measurements of the validation-loss kernel pp_focal_l2_terms (csrc/posepaf_loss.hip) for DESIGN.md section 6.

    python tools/loss_probe.py --out profiles/r13_val_loss.json [--reps 15] [--batch 128]
    python tools/loss_probe.py --backward --out profiles/r15_loss_grad.json     # the gradient kernel pp_focal_l2_grad, see backward()

Device events around single calls after a warm-up, median (min, max) of --reps.  The shape: --batch images of 512 x 512 (128 x 128
maps), 4 stacks x 5 scales of fp16 predictions in the pixel-major 64-channel layout the fused heads write, an fp16 target rendered
by pp_render_scenes (bench.py's people mix), no mask.  Against
  * the floor of reading those bytes once -- every stored prediction byte (64 channels per pixel) and the target once -- at the
    8 TB/s DESIGN uses for MI355X;
  * the torch formulation of the reference's models/loss_model.py (adaptive_avg_pool2d, interpolate, expand.clone, two in-place scales,
    where, abs, three multiplies, a 5-D sum per scale) on the same values as float32 planes -- the conversion to planes is NOT timed;
  * the same kernel on planar fp16 predictions.
The kernel's scalar is reported next to the torch formulation's.  They are not expected to agree closely: the target is a rendered
scene, full of 0.01f plateaus, and torch's float32 pooling order puts many of those cells on the background side (INTEGRATION
section 15).  Needs an MI355X; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "improved-body-parts_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0
SCENE_PEOPLE = (1, 2, 3, 4, 5, 6, 8, 10, 12, 15, 20, 30, 2, 4, 6, 3)   # bench.py's people per synthetic scene
NSTACK_WEIGHT, SCALE_WEIGHT = (1, 1, 1, 1), (0.1, 0.2, 0.4, 1.6, 6.4)


def median_ms(torch, fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return {"ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def torch_loss(torch, preds, target, mask):
    """models/loss_model.py:23-81, :133-161 on stock operators.  preds[s]: (T, B, 50, h, w) float32; target (B, 50, H, W); mask (B, 1, H, W)"""
    import torch.nn.functional as F
    losses = []
    for s, pred in enumerate(preds):
        gt = F.adaptive_avg_pool2d(target, output_size=pred.shape[-2:])
        mm = F.interpolate(mask, size=pred.shape[-2:], mode="bilinear")
        mm[mm < 0.5] = 0
        sxing = gt[None]
        m = mm[None].expand_as(sxing).clone()
        m[:, :, -2, :, :] *= 0.1
        m[:, :, 30:48, :, :] *= 3
        st = torch.where(torch.ge(sxing, 0.01), pred, 1 - pred)
        factor = torch.abs(1.0 - st)
        out = (pred - sxing) ** 2 * factor * m
        per_stack = out.sum(dim=(1, 2, 3, 4))
        losses.append(sum(per_stack[t] * NSTACK_WEIGHT[t] for t in range(len(NSTACK_WEIGHT))) / sum(NSTACK_WEIGHT) * SCALE_WEIGHT[s])
    return sum(losses) / sum(SCALE_WEIGHT) / target.shape[0]


def backward(a, torch, val_loss, views, planes, target, sizes, padded):
    """--backward: pp_focal_l2_grad alone (the C entry into preallocated 64-stride buffers), terms + gradients together (the Python
    entries: focal_l2_terms into out / workspace, then focal_l2_grad, which allocates the gradients and zeroes their padding
    channels), and forward + backward of the torch formulation on float32 planes -- the last two ALTERNATING, call by call, after a
    warm-up of both.  The floor: every stored prediction byte and the target read once, every gradient byte of the 50 channels
    written once, at 8 TB/s.  The gate: terms + gradients take less time than the torch formulation's forward + backward."""
    import ctypes as C
    from posepaf import _lib
    L = _lib.load()
    B, T, H, W = a.batch, len(views), target.shape[2], target.shape[3]
    # d combine / d terms: what torch_loss weighs a term with, so that the two gradients can be compared
    sw = torch.tensor(SCALE_WEIGHT, dtype=torch.float64, device="cuda")
    tw = (sw / sw.sum() / float(sum(NSTACK_WEIGHT)) / B)[None, :, None].expand(T, 5, B).contiguous()
    out = torch.empty((T, 5, B), dtype=torch.float64, device="cuda")
    work = torch.empty(val_loss.workspace_bytes(B, T, sizes), dtype=torch.uint8, device="cuda")
    gbuf = [[torch.zeros_like(buf) for buf in stack] for stack in padded]
    table = (C.c_void_p * (T * 5))(*[padded[t][s].data_ptr() for t in range(T) for s in range(5)])
    gtable = (C.c_void_p * (T * 5))(*[gbuf[t][s].data_ptr() for t in range(T) for s in range(5)])
    hs, ws = (C.c_int * 5)(*[h for h, _ in sizes]), (C.c_int * 5)(*[w for _, w in sizes])

    def raw():
        _lib.check(L.pp_focal_l2_grad(table, _lib.PP_F16, 64, C.c_void_p(target.data_ptr()), _lib.PP_F16, 50 * H * W, None, B, H, W, T, 5, hs, ws,
                                      0.1, 3.0, 0, C.c_void_p(tw.data_ptr()), gtable, C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def ours():
        val_loss.focal_l2_terms(views, target, out=out, workspace=work)
        return val_loss.focal_l2_grad(views, target, tw)

    t32 = target.float()
    ones = torch.ones((B, 1, H, W), dtype=torch.float32, device="cuda")
    stacked = [torch.stack([planes[t][s].float() for t in range(T)]).requires_grad_(True) for s in range(5)]

    def theirs():
        for p in stacked:
            p.grad = None
        torch_loss(torch, stacked, t32, ones).backward()

    pred_bytes = sum(buf.numel() * 2 for stack in padded for buf in stack)
    grad_bytes = pred_bytes * 50 // 64
    floor_ms = (pred_bytes + target.numel() * 2 + grad_bytes) / HBM_PEAK_GBS / 1e6
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_gbs": HBM_PEAK_GBS,
           "geometry": f"{B} images, {H} x {W} maps, {T} stacks x 5 scales, fp16 predictions and gradients (64 elements per pixel), fp16 target, no mask",
           "prediction_bytes_stored": pred_bytes, "gradient_bytes_of_the_50_channels": grad_bytes, "target_bytes": target.numel() * 2,
           "floor_ms_read_once_write_once_at_8TBs": floor_ms,
           "timing": f"device events around one call, median (min, max) of {a.reps}; terms + gradients and the torch formulation alternate"}
    res["pp_focal_l2_grad"] = median_ms(torch, raw, a.reps)
    res["pp_focal_l2_grad"]["times_the_floor"] = res["pp_focal_l2_grad"]["ms"] / floor_ms
    res["pp_focal_l2_grad"]["share_of_the_floor"] = floor_ms / res["pp_focal_l2_grad"]["ms"]
    for fn in (ours, theirs, ours, theirs):
        fn()
    torch.cuda.synchronize()
    samples = {"terms_and_gradients": [], "torch_formulation_forward_backward": []}
    for _ in range(a.reps):
        for key, fn in (("terms_and_gradients", ours), ("torch_formulation_forward_backward", theirs)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            samples[key].append(e0.elapsed_time(e1))
    for key, v in samples.items():
        res[key] = {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
    res["torch_formulation_forward_backward"]["times_terms_and_gradients"] = (res["torch_formulation_forward_backward"]["ms"] /
                                                                              res["terms_and_gradients"]["ms"])
    # the two gradients of one prediction, for the record: the torch side pools in float32 and differs on the 0.01f plateaus, and
    # this side rounds to binary16
    mine = ours()[0][0].float()
    theirs()
    diff = (mine - stacked[0].grad[0]).abs()
    res["gradient_of_pred_0_0"] = {"largest": float(mine.abs().max()), "largest_difference_to_torch": float(diff.max()),
                                   "elements_differing_by_more_than_1e-3_of_the_largest": int((diff > 1e-3 * mine.abs().max()).sum()),
                                   "elements": mine.numel()}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    assert res["terms_and_gradients"]["ms"] < res["torch_formulation_forward_backward"]["ms"], "the gate: terms + gradients against torch"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--backward", action="store_true", help="measure pp_focal_l2_grad instead (profiles/r15_loss_grad.json)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=128)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "loss_probe.py needs the MI355X"
    from posepaf import synth, synth_device, val_loss
    B, H, W, T = a.batch, 128, 128, 4
    sizes = [(H >> s, W >> s) for s in range(5)]
    people = [synth.random_people(SCENE_PEOPLE[i % len(SCENE_PEOPLE)], np.random.default_rng(9000 + i), img_h=4 * H, img_w=4 * W) for i in range(B)]
    joints, n = synth_device.pack_joints(people, max(SCENE_PEOPLE))
    target = synth_device.render_scenes(torch.from_numpy(joints).cuda(), torch.from_numpy(n).cuda(), H, W, dtype=torch.float16, flip=False,
                                        reverse_kp=True)[:, 0].contiguous()
    g = torch.Generator(device="cuda").manual_seed(5)
    padded = [[torch.zeros((B, h, w, 64), dtype=torch.float16, device="cuda") for (h, w) in sizes] for _ in range(T)]
    for stack in padded:
        for s, buf in enumerate(stack):   # something between noise and the target, so that both branches of the focal factor occur
            pooled = torch.nn.functional.adaptive_avg_pool2d(target.float(), sizes[s]).permute(0, 2, 3, 1)
            buf[..., :50] = (0.5 * pooled + 0.2 * torch.rand(pooled.shape, generator=g, device="cuda")).half()
    views = [[buf.permute(0, 3, 1, 2)[:, :50] for buf in stack] for stack in padded]
    assert val_loss._layout(views[0][0]) == 64
    planes = [[v.contiguous() for v in stack] for stack in views]
    if a.backward:
        return backward(a, torch, val_loss, views, planes, target, sizes, padded)
    out = torch.empty((T, 5, B), dtype=torch.float64, device="cuda")
    work = torch.empty(val_loss.workspace_bytes(B, T, sizes), dtype=torch.uint8, device="cuda")
    pred_bytes = sum(buf.numel() * 2 for stack in padded for buf in stack)
    used_bytes = pred_bytes * 50 // 64
    target_bytes = target.numel() * 2
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_gbs": HBM_PEAK_GBS,
           "geometry": f"{B} images, {H} x {W} maps, {T} stacks x 5 scales, fp16 predictions (64 elements per pixel), fp16 target, no mask",
           "prediction_bytes_stored": pred_bytes, "prediction_bytes_of_the_50_channels": used_bytes, "target_bytes": target_bytes,
           "workspace_bytes": work.numel(),
           "floor_ms_reading_stored_bytes_once_at_8TBs": (pred_bytes + target_bytes) / HBM_PEAK_GBS / 1e6,
           "timing": f"device events around one call, median (min, max) of {a.reps} after 3 warm-up calls"}
    res["kernel_pixel_major_64"] = median_ms(torch, lambda: val_loss.focal_l2_terms(views, target, out=out, workspace=work), a.reps)
    ours = float(val_loss.combine(out))
    res["kernel_planes"] = median_ms(torch, lambda: val_loss.focal_l2_terms(planes, target, out=out, workspace=work), a.reps)
    ours_planes = float(val_loss.combine(out))
    for k in ("kernel_pixel_major_64", "kernel_planes"):
        res[k]["times_the_floor"] = res[k]["ms"] / res["floor_ms_reading_stored_bytes_once_at_8TBs"]
        res[k]["gbs_of_stored_bytes"] = (pred_bytes + target_bytes) / res[k]["ms"] / 1e6
    res["combine_ms"] = median_ms(torch, lambda: val_loss.combine(out), a.reps)
    # the torch formulation on float32 planes (the reference's tensors); building them is not timed
    t32 = target.float()
    ones = torch.ones((B, 1, H, W), dtype=torch.float32, device="cuda")
    stacked = [torch.stack([planes[t][s].float() for t in range(T)]) for s in range(5)]
    res["torch_formulation_fp32_planes"] = median_ms(torch, lambda: torch_loss(torch, stacked, t32, ones), max(3, a.reps // 3), warm=1)
    theirs = float(torch_loss(torch, stacked, t32, ones))
    res["torch_formulation_fp32_planes"]["times_the_kernel"] = res["torch_formulation_fp32_planes"]["ms"] / res["kernel_pixel_major_64"]["ms"]
    res["scalar"] = {"kernel": ours, "kernel_planes": ours_planes, "torch_formulation": theirs, "relative_difference": abs(ours - theirs) / abs(theirs)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    assert abs(ours - ours_planes) <= 1e-12 * ours, (ours, ours_planes)        # two orders of one float64 sum
    assert abs(ours - theirs) <= 0.1 * abs(theirs), (ours, theirs)            # a sanity bound only, see above


if __name__ == "__main__":
    main()
