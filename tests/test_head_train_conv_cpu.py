"""CPU: the pieces of HeadTrainer(train="heads+conv") and finetune.py --train heads+conv that need no GPU -- the BN statistics that
state_dict() writes fold to the identity in float32, so fused_model._fold returns a master's own bits; the refusals end before the
GPU is looked for."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

PKG = os.path.join(ROOT, "improved-body-parts_amd")


def bits(t):
    return t.detach().contiguous().view(torch.int32).numpy()


@pytest.mark.parametrize("eps", [1e-5, 1e-3, 1e-4, 2e-5, 1e-7])
def test_identity_bn_folds_a_master_to_its_own_bits(eps):
    from posepaf import fused_model, head_train
    v = head_train.identity_bn_var(eps)
    assert np.float32(v) == v and abs(v - (1.0 - eps)) <= 8 * 2.0 ** -24
    assert float(torch.sqrt(torch.tensor(v, dtype=torch.float32) + eps)) == 1.0
    g = torch.Generator().manual_seed(int(eps * 1e9))
    for trial in range(3):
        k, c = 64, 32
        w = torch.randn((k, 3, 3, c), generator=g) * 10.0 ** (trial - 2)           # the master's order
        b = torch.randn(k, generator=g) * 10.0 ** (2 - trial)
        w.view(-1)[:4] = torch.tensor([0.0, 1e-40, -3e-39, 65504.0])                # a zero, float32 subnormals, a large value
        conv = torch.nn.Conv2d(c, k, 3, padding=1, bias=False)
        bn = torch.nn.BatchNorm2d(k, eps=eps)
        with torch.no_grad():
            conv.weight.copy_(w.permute(0, 3, 1, 2))
            bn.weight.fill_(1.0), bn.bias.copy_(b), bn.running_mean.zero_(), bn.running_var.fill_(v)
        fw, fb = fused_model._fold(conv, bn)
        assert np.array_equal(bits(fw.permute(0, 2, 3, 1)), bits(w)) and np.array_equal(bits(fb), bits(b))
        assert np.array_equal(fw.half().view(torch.int16).numpy(), conv.weight.detach().half().view(torch.int16).numpy())


def test_dividing_by_the_old_scale_would_not_be_exact():
    """why state_dict() does not keep the old BN: w / s * s is not w for most scales"""
    g = torch.Generator().manual_seed(3)
    w, s = torch.randn(4096, generator=g), torch.rand(4096, generator=g) + 0.5
    assert not torch.equal(w / s * s, w)


@pytest.fixture()
def finetune():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import finetune
    return finetune


BASE = ["--synthetic", "4", "--batch", "2", "--steps", "1", "--sizes", "64x64"]


def test_finetune_refuses_before_the_gpu(finetune, monkeypatch):
    def never(*a, **k):
        raise AssertionError("reached past the refusals")
    from posepaf import model_init
    monkeypatch.setattr(model_init, "build_network", never)
    monkeypatch.setattr(torch.cuda, "is_available", never)
    cases = [
        (["--train", "heads+conv"], "belongs to --model fused"),
        (["--train", "heads+conv", "--model", "plain"], "belongs to --model fused"),
        (["--train", "heads+conv", "--model", "fused"], "--arch final"),
        (["--train", "heads+conv", "--model", "fused", "--arch", "posenet"], "--arch final"),
        (["--train", "all", "--model", "fused", "--arch", "final"], "--train heads"),
    ]
    for extra, text in cases:
        with pytest.raises(SystemExit) as e:
            finetune.main(BASE + extra)
        assert text in str(e.value), (extra, str(e.value))
    for arch in ("final", "auto"):
        a = finetune.parse(BASE + ["--train", "heads+conv", "--model", "fused", "--arch", arch, "--graph", "--wgrad", "multi",
                                   "--loss_scale", "dynamic"])
        assert finetune.refusals(a) == [] and a.train == "heads+conv"
    assert finetune.refusals(finetune.parse(BASE + ["--train", "heads", "--model", "fused"])) == []


def test_heads_conv_is_refused_on_posenet_and_for_unknown_values():
    from posepaf import head_train
    from posepaf._lib import PosePafError
    from posepaf.model_init import build_network
    net, _ = build_network("posenet", None, 7, nstack=1)
    with pytest.raises(PosePafError, match="final"):
        head_train.HeadTrainer(net, "cuda:0", train="heads+conv")          # before the fused model is built: no GPU is needed
    with pytest.raises(PosePafError, match="train"):
        head_train.HeadTrainer(net, "cuda:0", train="conv")
