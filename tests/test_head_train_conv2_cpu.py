"""CPU: the pieces of HeadTrainer(train="heads+conv2") and finetune.py --train heads+conv2 that need no GPU: the refusals end before
the GPU is looked for, with the messages of --train heads+conv."""
import os
import sys

import pytest
import torch

from conftest import ROOT

PKG = os.path.join(ROOT, "improved-body-parts_amd")
BASE = ["--synthetic", "4", "--batch", "2", "--steps", "1", "--sizes", "64x64"]


@pytest.fixture()
def finetune():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import finetune
    return finetune


def test_finetune_refuses_before_the_gpu(finetune, monkeypatch):
    def never(*a, **k):
        raise AssertionError("reached past the refusals")
    from posepaf import model_init
    monkeypatch.setattr(model_init, "build_network", never)
    monkeypatch.setattr(torch.cuda, "is_available", never)
    cases = [
        (["--train", "heads+conv2"], "--train heads+conv2 belongs to --model fused"),
        (["--train", "heads+conv2", "--model", "plain"], "--train heads+conv2 belongs to --model fused"),
        (["--train", "heads+conv2", "--model", "fused"], "--train heads+conv2 needs --arch final"),
        (["--train", "heads+conv2", "--model", "fused", "--arch", "posenet"], "--train heads+conv2 needs --arch final"),
        (["--train", "heads+conv2", "--model", "fused", "--arch", "final", "--loss_scale", "dynamic"], "--loss_scale dynamic needs --update device"),
    ]
    for extra, text in cases:
        with pytest.raises(SystemExit) as e:
            finetune.main(BASE + extra)
        assert text in str(e.value), (extra, str(e.value))
    for arch in ("final", "auto"):
        a = finetune.parse(BASE + ["--train", "heads+conv2", "--model", "fused", "--arch", arch, "--graph", "--wgrad", "multi",
                                   "--loss_scale", "dynamic"])
        assert finetune.refusals(a) == [] and a.train == "heads+conv2"
    with pytest.raises(SystemExit):
        finetune.parse(BASE + ["--train", "heads+conv3"])


def test_heads_conv2_is_refused_on_posenet_and_the_message_lists_all_three():
    from posepaf import head_train
    from posepaf._lib import PosePafError
    from posepaf.model_init import build_network
    net, _ = build_network("posenet", None, 7, nstack=1)
    with pytest.raises(PosePafError, match="final"):
        head_train.HeadTrainer(net, "cuda:0", train="heads+conv2")         # before the fused model is built: no GPU is needed
    with pytest.raises(PosePafError) as e:
        head_train.HeadTrainer(net, "cuda:0", train="conv2")
    assert all(f"'{v}'" in str(e.value) for v in ("heads", "heads+conv", "heads+conv2"))
