#!/usr/bin/env python3
"""Generate tests/golden/loss_*.npz from the REFERENCE's own validation loss (run in the build container only).

    python tests/golden/make_golden_loss.py

What runs: models/loss_model.py MultiTaskLoss (forward, _loss_per_scale, focal_l2_loss) imported from /root/reference, on the CPU in
float32, with nstack = 2 and the reference's own weights (config/config.py:17-20) and channel starts (:131-132).  The per-stack sums
the reference prints are obtained exactly (not parsed from its 8-digit print): _loss_per_scale with nstack_weight = one-hot returns
stack t's sum over the batch, sum_b terms[t][s][b].  No reference source or bytecode is written anywhere.

The fixtures are DATA: target, mask and fp16-valued predictions in; the reference's per-(stack, scale) sums and its scalar out.
  loss_16x16_binary.npz   16 x 16 -> 16, 8, 4, 2, 1 (square), binary mask
  loss_20x28_soft.npz     20 x 28 -> (20, 28), (10, 14), (5, 7), (2, 3), (1, 1), soft mask (values in [0, 1])
  loss_20x28_ones.npz     the same sizes, mask of ones
Each target has NO pooled cell within 1e-6 of 0.01 in a window of more than one cell, and each mask NO resampled value within 1e-6 of
0.5 other than 0.5 itself (asserted below with tests/loss_reference.py, allowed count zero): there the float32 accumulation order
of torch's pooling / interpolation decides on which side of the comparison a cell lands, not the formula.
"""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
SIZE_LIMIT = 600_000

import numpy as np  # noqa: E402
import torch  # noqa: E402


def import_reference():
    sys.path.insert(0, REF)
    from config.config import GetConfig, TrainingOpt
    from models.loss_model import MultiTaskLoss
    sys.path.remove(REF)
    for n in [n for n in sys.modules if n in ("config", "models") or n.startswith(("config.", "models."))]:
        del sys.modules[n]                       # the product package has a config/ and a models/ of its own
    return GetConfig, TrainingOpt, MultiTaskLoss


def make_case(rng, H, W, sizes, mask_kind, B=2, T=2):
    # target: sparse responses in (0, 1] as binary16 values, zeros elsewhere, and a limb-like plateau of 0.01f that no multi-cell
    # window pools alone (a single-cell window, scale 0, compares 0.01f with itself: exact in every order)
    target = np.where(rng.random((B, 50, H, W)) < 0.3, rng.random((B, 50, H, W)), 0.0).astype(np.float16).astype(np.float32)
    target[:, 3, 1, 1:4] = np.float32(0.01)
    if mask_kind == "binary":
        mask = (rng.random((B, H, W)) < 0.8).astype(np.float32)
    elif mask_kind == "soft":
        mask = rng.random((B, H, W)).astype(np.float32)
    else:
        mask = np.ones((B, H, W), np.float32)
    preds = [[(rng.random((B, 50, h, w)) * 1.2 - 0.1).astype(np.float16) for (h, w) in sizes] for _ in range(T)]
    return target, mask, preds


def reference_values(GetConfig, TrainingOpt, MultiTaskLoss, target, mask, preds):
    with contextlib.redirect_stdout(io.StringIO()):   # GetConfig prints its layer table
        cfg = GetConfig("Canonical")
    opt = TrainingOpt()
    T, B = len(preds), target.shape[0]
    opt.nstack, opt.batch_size, opt.nstack_weight = T, B, [1] * T
    assert (cfg.heat_start, cfg.bkg_start) == (30, 48) and list(opt.scale_weight) == [0.1, 0.2, 0.4, 1.6, 6.4]
    assert (opt.multi_task_weight, opt.keypoint_task_weight) == (0.1, 3)
    loss = MultiTaskLoss(opt, cfg)
    pred_t = [[torch.from_numpy(p.astype(np.float32)) for p in stack] for stack in preds]
    tgt = (torch.from_numpy(mask)[:, None], torch.from_numpy(target))
    sums = np.zeros((T, 5), np.float64)
    with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():   # the per-stack prints
        scalar = float(loss(pred_t, tgt))
        for s in range(5):
            stacked = torch.cat([pred_t[t][s][None] for t in range(T)], dim=0)
            for t in range(T):
                loss.nstack_weight = [1 if k == t else 0 for k in range(T)]
                sums[t, s] = float(loss._loss_per_scale(stacked, tgt))
    return sums, scalar


def main():
    GetConfig, TrainingOpt, MultiTaskLoss = import_reference()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import loss_reference as lr
    sq = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    rect = [(20, 28), (10, 14), (5, 7), (2, 3), (1, 1)]
    cases = {"16x16_binary": (16, 16, sq, "binary", 101), "20x28_soft": (20, 28, rect, "soft", 102), "20x28_ones": (20, 28, rect, "ones", 103)}
    for name, (H, W, sizes, kind, seed) in cases.items():
        target, mask, preds = make_case(np.random.default_rng(seed), H, W, sizes, kind)
        assert lr.near_threshold_cells(target, sizes) == 0, name
        assert lr.near_half_mask_values(mask, sizes) == 0, name
        sums, scalar = reference_values(GetConfig, TrainingOpt, MultiTaskLoss, target, mask, preds)
        terms = lr.focal_l2_terms(preds, target, mask)
        rel = np.abs(terms.sum(axis=2) - sums) / np.where(sums > 0, sums, 1.0)   # (a fully masked scale: 0 against 0)
        path = os.path.join(HERE, f"loss_{name}.npz")
        arrays = {f"pred_{t}_{s}": preds[t][s] for t in range(len(preds)) for s in range(5)}
        np.savez_compressed(path, target=target, mask=mask, per_stack_scale=sums, scalar=np.float64(scalar),
                            sizes=np.array(sizes, np.int32), **arrays)
        assert os.path.getsize(path) <= SIZE_LIMIT, (path, os.path.getsize(path))
        print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, scalar {scalar:.9g}, restatement {lr.combine(terms, (1, 1)):.9g}, "
              f"largest relative difference of a (stack, scale) sum {rel.max():.3e}, "
              f"of the scalar {abs(lr.combine(terms, (1, 1)) - scalar) / scalar:.3e}")


if __name__ == "__main__":
    main()
