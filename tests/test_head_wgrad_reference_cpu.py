"""CPU: the NumPy restatement tests/head_wgrad_reference.py against torch autograd; the binary16 product rounding; the trainer's
"auto" loss scale; and finetune.py --model fused's refusals, which end before a GPU is looked for."""
import os
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

import head_wgrad_reference as ref
from conftest import PKG


def test_restatement_equals_autograd_of_a_float64_conv():
    rng = np.random.default_rng(3)
    B, h, w, c_in, c_out = 2, 3, 4, 64, 50                      # m = 2 * 12
    m = B * h * w
    g = np.full((m, 64), np.nan, np.float16)
    g[:, :c_out] = (rng.standard_normal((m, c_out)) * 0.125).astype(np.float16)
    x = rng.standard_normal((m, c_in)).astype(np.float16)
    scale = rng.uniform(0.5, 1.5, (B, c_in)).astype(np.float16)
    for sc in (None, scale):
        dw, db = ref.head_wgrad(g, x, c_out, sc, h * w)
        xs = torch.from_numpy(ref.scaled_input(x, sc, h * w).astype(np.float64)).view(B, h, w, c_in).permute(0, 3, 1, 2)
        conv = torch.nn.Conv2d(c_in, c_out, 1).double()
        up = torch.from_numpy(g[:, :c_out].astype(np.float64)).view(B, h, w, c_out).permute(0, 3, 1, 2)
        F.conv2d(xs, conv.weight, conv.bias).backward(up)
        gw, gb = conv.weight.grad.numpy()[:, :, 0, 0], conv.bias.grad.numpy()
        assert np.abs(dw - gw).max() <= 1e-12 * np.abs(gw).max() and np.abs(db - gb).max() <= 1e-12 * np.abs(gb).max()
    dw2, db2 = ref.head_wgrad(g, x, c_out, scale, h * w, inv_loss_scale=2.0 ** -12)
    assert np.array_equal(dw2, dw * 2.0 ** -12) and np.array_equal(db2, db * 2.0 ** -12)


def test_product_rounding_is_one_rounding_of_the_exact_product():
    every = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    every = every[np.isfinite(every)]
    for s in (0.5, 1.0, 1.5, 3.0, 0.333251953125, 1.2998046875, 6.103515625e-05, 1024.0):
        sv = np.float16(s)
        assert float(sv) == s
        got = ref.scaled_input(every[:, None], np.full((every.size, 1), sv), 1)[:, 0]
        want = (torch.from_numpy(every).float() * torch.tensor(float(sv))).half().numpy()
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
        with np.errstate(over="ignore"):                       # and the exact product in float64, rounded once
            exact = (every.astype(np.float64) * float(sv)).astype(np.float16)
        assert np.array_equal(got.view(np.uint16), exact.view(np.uint16))


def test_auto_loss_scale():
    from posepaf import head_train
    # B = 1, 2, 8, 128 at four stages: tw_max = 1/4 * 6.4/8.7 / B;  65504 / (tw_max * 36) = 9894.4 B  ->  2^13, 2^14, 2^16, 2^20
    for B, want in ((1, 2.0 ** 13), (2, 2.0 ** 14), (8, 2.0 ** 16), (128, 2.0 ** 20)):
        s = head_train.auto_loss_scale(B, 4)
        assert s == want == ref.auto_loss_scale(B, 4)
        tw_max = ref.tw_max(B, 4)
        assert s * tw_max * 36.0 <= 65504.0 < 2.0 * s * tw_max * 36.0
    assert head_train.auto_loss_scale(2, 2) == ref.auto_loss_scale(2, 2) == 2.0 ** 13
    assert head_train.is_power_of_two(0.5) and head_train.is_power_of_two("4096") and not head_train.is_power_of_two(3)
    assert not head_train.is_power_of_two(0) and not head_train.is_power_of_two("x") and not head_train.is_power_of_two(float("inf"))


def _finetune(*args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, os.path.join(PKG, "finetune.py"), *args], capture_output=True, text=True, env=env, timeout=300)


def test_finetune_fused_refusals_need_no_gpu():
    base = ["--model", "fused", "--synthetic", "4", "--batch", "2", "--sizes", "64x64", "--stages", "2", "--steps", "2"]
    r = _finetune(*base, "--train", "all")
    assert r.returncode != 0 and "--train heads" in r.stderr and "MI355X" not in r.stderr
    r = _finetune(*base, "--train", "heads", "--loss_scale", "3000")
    assert r.returncode != 0 and "power of two" in r.stderr and "MI355X" not in r.stderr
    r = _finetune(*base, "--train", "heads", "--loss", "torch")
    assert r.returncode != 0 and "--loss torch" in r.stderr and "MI355X" not in r.stderr
    r = _finetune("--synthetic", "4", "--train", "heads", "--wgrad", "torch")
    assert r.returncode != 0 and "belong to --model fused" in r.stderr
