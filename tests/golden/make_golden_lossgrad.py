#!/usr/bin/env python3
"""Generate tests/golden/lossgrad_*.npz from the REFERENCE's own loss under autograd (run in the build container only).

    python tests/golden/make_golden_lossgrad.py

What runs: models/loss_model.py MultiTaskLoss imported from /root/reference the way make_golden_loss.py imports it, on the CPU in
float32, nstack = 2, the reference's own weights; the predictions are float32 leaves that require grad, loss(preds, target).backward()
as train.py:141 does, and pred[t][s].grad of the scalar is stored.  No reference source or bytecode is written anywhere.

The fixtures are DATA: the reference's gradients (float32) and, for the new case, the inputs.
  lossgrad_16x16_binary.npz   the inputs of the existing loss_16x16_binary.npz (read, not rewritten); gradients only
  lossgrad_12x20_soft.npz     make_case(default_rng(104), 12, 20, [(12, 20), (6, 10), (3, 5), (2, 3), (1, 1)], "soft"): target, soft mask,
                              fp16-valued predictions, gradients
Asserted for seed 104 (allowed count zero / exact): no pooled cell of a multi-cell window within 1e-6 of 0.01, no resampled mask
value within 1e-6 of 0.5 other than 0.5 itself, and 47 prediction elements equal to 0 or 1 -- the two values at which |1 - st| can
have a kink; 20 of them lie on the side where it has one (p == 1 on the foreground, p == 0 elsewhere), and there torch's abs backward
gives 0.  (The 16 x 16 case: 39 and 16.)

The generator prints, per case, the largest difference between tests/lossgrad_reference.py (float64, unrounded) and the reference's
float32 gradients divided by each tensor's largest |gradient|, and asserts it below 1e-6: about 6 x the reference's float32 rounding
(measured 1.2e-7 .. 1.5e-7 on the three loss_*.npz fixtures) and far below one wrong sign at a kink.
Measured when these fixtures were written:
  lossgrad_16x16_binary.npz: 1.263e-07     lossgrad_12x20_soft.npz: 3.041e-07
"""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SIZE_LIMIT = 600_000
BOUND = 1e-6

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from make_golden_loss import import_reference, make_case  # noqa: E402


def reference_gradients(GetConfig, TrainingOpt, MultiTaskLoss, target, mask, preds):
    with contextlib.redirect_stdout(io.StringIO()):   # GetConfig prints its layer table
        cfg = GetConfig("Canonical")
    opt = TrainingOpt()
    T, B = len(preds), target.shape[0]
    opt.nstack, opt.batch_size, opt.nstack_weight = T, B, [1] * T
    assert (cfg.heat_start, cfg.bkg_start) == (30, 48) and list(opt.scale_weight) == [0.1, 0.2, 0.4, 1.6, 6.4]
    assert (opt.multi_task_weight, opt.keypoint_task_weight) == (0.1, 3)
    loss = MultiTaskLoss(opt, cfg)
    pred_t = [[torch.from_numpy(p.astype(np.float32)).requires_grad_(True) for p in stack] for stack in preds]
    tgt = (torch.from_numpy(mask)[:, None], torch.from_numpy(target))
    with contextlib.redirect_stdout(io.StringIO()):   # the per-stack prints
        scalar = loss(pred_t, tgt)
        scalar.backward()
    return [[p.grad.numpy().copy() for p in stack] for stack in pred_t], float(scalar.detach())


def main():
    GetConfig, TrainingOpt, MultiTaskLoss = import_reference()
    import loss_reference as lr
    import lossgrad_reference as lg
    sq = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    small = [(12, 20), (6, 10), (3, 5), (2, 3), (1, 1)]
    old = np.load(os.path.join(HERE, "loss_16x16_binary.npz"))
    assert [tuple(v) for v in old["sizes"]] == sq
    cases = {"16x16_binary": (old["target"], old["mask"], [[old[f"pred_{t}_{s}"] for s in range(5)] for t in range(2)], sq, None, False),
             "12x20_soft": make_case(np.random.default_rng(104), 12, 20, small, "soft") + (small, 47, True)}
    for name, (target, mask, preds, sizes, kinks, with_inputs) in cases.items():
        assert lr.near_threshold_cells(target, sizes) == 0, name
        assert lr.near_half_mask_values(mask, sizes) == 0, name
        n_kinks = sum(int(k.sum()) for stack in lg.kink_elements(preds, target, sizes) for k in stack)
        at_0_or_1 = sum(int(((p.astype(np.float64) == 0.0) | (p.astype(np.float64) == 1.0)).sum()) for stack in preds for p in stack)
        assert kinks is None or at_0_or_1 == kinks, (name, at_0_or_1)
        assert 0 < n_kinks <= at_0_or_1, (name, n_kinks)
        grads, scalar = reference_gradients(GetConfig, TrainingOpt, MultiTaskLoss, target, mask, preds)
        T, B = len(preds), target.shape[0]
        want = lg.focal_l2_grad(preds, target, lg.combine_weights(T, 5, B, (1,) * T), mask, rounded=False)
        worst = max(float(np.abs(want[t][s] - grads[t][s].astype(np.float64)).max() / (np.abs(grads[t][s]).max() or 1.0))
                    for t in range(T) for s in range(5))   # (a fully masked scale: 0 against 0)
        arrays = {f"grad_{t}_{s}": grads[t][s] for t in range(T) for s in range(5)}
        if with_inputs:
            arrays.update({f"pred_{t}_{s}": preds[t][s] for t in range(T) for s in range(5)})
            arrays.update(target=target, mask=mask)
        path = os.path.join(HERE, f"lossgrad_{name}.npz")
        np.savez_compressed(path, scalar=np.float64(scalar), sizes=np.array(sizes, np.int32), kink_elements=np.int64(n_kinks), **arrays)
        assert os.path.getsize(path) <= SIZE_LIMIT, (path, os.path.getsize(path))
        print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes, scalar {scalar:.9g}, {n_kinks} kink elements, largest difference "
              f"restatement - reference / largest |gradient| of the tensor {worst:.3e}")
        assert worst < BOUND, (name, worst)


if __name__ == "__main__":
    main()
