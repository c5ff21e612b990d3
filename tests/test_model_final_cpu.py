"""CPU: the published IMHN variant (models/posenet_final.py) against the reference's own module -- golden vectors G8, made by
tests/golden/make_golden_final.py from the reference's models/posenet_final.py: identical state_dict keys / shapes for nstack 4 and
3 (so the published checkpoint loads with strict=True), the same forward result under a shared deterministic init, the
architecture detection of posepaf.model_init, and the algebra of the fused form in float64."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN


def _net(arch, nstack=4):
    from config.config import GetConfig, TrainingOpt
    from posepaf.model_init import network_class
    opt = TrainingOpt()
    opt.nstack = nstack
    return network_class(arch)(opt, GetConfig("Canonical"), bn=True).eval()


@pytest.fixture(scope="module")
def model():
    from posepaf.model_init import deterministic_init
    m = _net("final")
    deterministic_init(m, seed=7)
    return m


@pytest.fixture(scope="module")
def manifest():
    return json.load(open(os.path.join(GOLDEN, "g8_final_state_dict_manifest.json")))


def test_state_dict_manifest_nstack4(model, manifest):
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert len(got) == 1236
    assert got == manifest["4"]
    assert list(got)[0] == "posenet.pre.conv1.weight"
    assert sum(p.numel() for p in model.parameters()) == 227066536


def test_state_dict_manifest_nstack3(manifest):
    got = {k: list(v.shape) for k, v in _net("final", 3).state_dict().items()}
    assert len(got) == 930
    assert got == manifest["3"]


def test_forward_matches_reference_module(model):
    g = np.load(os.path.join(GOLDEN, "g8_final_model_forward.npz"))
    assert int(g["n_params"]) == 227066536
    with torch.no_grad():
        out = model(torch.from_numpy(g["x"]))
    assert len(out) == 4 and len(out[0]) == 5
    for name, t in (("last_stage_scale0", out[-1][0]), ("last_stage_scale4", out[-1][4]), ("first_stage_scale0", out[0][0])):
        want = g[name]
        assert t.shape == want.shape
        # the bound of tests/test_model_cpu.py for G5: same ops in the same order on the same CPU kernels
        assert np.allclose(t.numpy(), want, rtol=1e-4, atol=1e-5), name
    assert float(np.abs(g["last_stage_scale0"]).mean()) > 1e-3  # the fixture is not degenerate


def test_train_mode_is_refused(model):
    model.train()
    with pytest.raises(ValueError):
        model(torch.zeros(1, 64, 64, 3))
    model.eval()


def test_arch_of_state_dict(manifest):
    from posepaf.model_init import arch_of_state_dict
    assert arch_of_state_dict(manifest["4"]) == ("final", 4)
    assert arch_of_state_dict(manifest["3"]) == ("final", 3)
    dev = json.load(open(os.path.join(GOLDEN, "g5_state_dict_manifest.json")))
    assert arch_of_state_dict(dev) == ("posenet", 4)
    assert arch_of_state_dict(["module." + k for k in manifest["3"]]) == ("final", 3)    # a DataParallel checkpoint's prefix
    with pytest.raises(ValueError):
        arch_of_state_dict({"posenet.pre.conv1.weight": 0, "posenet.hourglass.0.hg.0.0.conv.weight": 0})
    with pytest.raises(ValueError):
        arch_of_state_dict(list(dev) + list(manifest["4"]))


def test_the_two_architectures_refuse_each_others_weights():
    """strict loading, both ways; posepaf.model_init.load_weights names the architecture the keys belong to and the flag"""
    from posepaf.model_init import load_weights
    dev, fin = _net("posenet", 3), _net("final", 3)
    with pytest.raises(RuntimeError):
        fin.load_state_dict(dev.state_dict())
    with pytest.raises(RuntimeError):
        dev.load_state_dict(fin.state_dict())
    with pytest.raises(RuntimeError, match=r"--arch posenet with nstack 3"):
        load_weights(fin, dev.state_dict(), "final")
    with pytest.raises(RuntimeError, match=r"--arch final with nstack 3"):
        load_weights(dev, fin.state_dict(), "posenet")
    load_weights(fin, _net("final", 3).state_dict(), "final")
    with pytest.raises(RuntimeError, match=r"--arch final with nstack 3"):     # right architecture, wrong depth
        load_weights(_net("final", 4), fin.state_dict(), "final")


# ---- the fused form (posepaf/fused_model.py FusedIMHNFinal) checked as ALGEBRA in float64 on the CPU, where every kernel's torch
# ---- twin runs; the kernels themselves are compared with torch in tests/test_gpu_model_final.py
@pytest.fixture(scope="module")
def small():
    """a narrow 3-stage final network (32 + 16 s channels, 10 outputs) in float64, BatchNorm statistics away from the identity"""
    from models.posenet_final import PoseNet
    from posepaf.model_init import deterministic_init

    class Wrap(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.posenet = PoseNet(3, 32, 10, bn=True, increase=16, init_weights=False)

        def forward(self, x):
            return self.posenet(x)

    net = Wrap().eval()
    deterministic_init(net, seed=11)
    return net.double()


def _fold64(conv, bn):
    """conv + eval-mode BatchNorm as one affine map, in float64"""
    w = conv.weight.detach().double().flatten(1)
    b = conv.bias.detach().double() if conv.bias is not None else torch.zeros(w.shape[0], dtype=torch.float64)
    if bn is not None:
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        w, b = w * s[:, None], (b - bn.running_mean.detach().double()) * s + bn.bias.detach().double()
    return w, b


def test_folded_prediction_merge_is_the_same_linear_map_for_the_final_module(small):
    """merge_features(f) + merge_preds(outs(f)) (models/posenet_final.py: both 1x1, no activation between head and merge) == ONE 1x1
    convolution with W' = Wf + Wp Wh, b' = bf + bp + Wp bh, for every stage and scale of the final module: in float64 to 1e-12, and
    the convolution FusedIMHNFinal holds after its load-time fold to 1e-6 (posepaf.fused_model._fold forms the weights in fp32 by
    design: 2^-24 per weight, a few of them per output)."""
    from posepaf import fused_model as fm
    assert fm.USE_FOLDED_MERGE
    fused = fm.FusedIMHN.from_network(small).double()
    assert isinstance(fused, fm.FusedIMHNFinal) and fused.folded_merge
    p = small.posenet
    g = torch.Generator().manual_seed(6)
    conv = lambda t, w, b: torch.einsum("nchw,kc->nkhw", t, w) + b[None, :, None, None]
    with torch.no_grad():
        for t in range(2):
            for s in range(5):
                f = torch.randn(2, 32, 4, 6, generator=g, dtype=torch.float64)
                want = p.merge_features[t][s](f) + p.merge_preds[t][s](p.outs[t][s](f))
                assert want.shape == (2, 32 + 16 * s, 4, 6)
                (wf, bf), (wp, bp) = _fold64(p.merge_features[t][s].conv.conv, p.merge_features[t][s].conv.bn), \
                    _fold64(p.merge_preds[t][s].conv.conv, p.merge_preds[t][s].conv.bn)
                wh, bh = _fold64(p.outs[t][s].conv, None)
                got = conv(f, wf + wp @ wh, bf + bp + wp @ bh)
                assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item(), (t, s)
                got = fused.mfeat[t][s](f)
                assert got.shape == want.shape
                assert (got - want).abs().max().item() <= 1e-6 * want.abs().max().item(), (t, s)


@pytest.mark.parametrize("folded", [True, False])
def test_fused_final_forward_is_the_module_in_float64(small, folded, monkeypatch):
    """every stage's scale-0 prediction of the fused form == the module's, evaluated in float64: BN folding, the residual add before
    the activation, SE gains and cache entering the compress convolution, the (folded) merges, the skipped heads of the last stage.
    Bound: the fused weights are fp32 roundings (posepaf.fused_model._fold, 2^-24 relative each) and a prediction of the third stage
    lies behind about 90 convolutions in sequence: 90 * 2^-24 = 5.4e-6 if every layer's error lined up, so 1e-5 of the stage's scale;
    a structural mistake (an add on the wrong side of an activation, a missing cache) shows at 1e-2 and more."""
    from posepaf import fused_model as fm
    monkeypatch.setattr(fm, "USE_FOLDED_MERGE", folded)
    fused = fm.FusedIMHN.from_network(small).double().eval()
    x = torch.rand(2, 64, 128, 3, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    with torch.no_grad():
        want = small(x)
        got = fused(x, stage_preds=True)
        last = fused(x)
    assert len(got) == 3
    for t in range(3):
        scale = want[t][0].abs().max().item()
        assert scale > 1e-3
        assert (got[t] - want[t][0]).abs().max().item() <= 1e-5 * scale, t
    assert torch.equal(last, got[-1])


def test_from_network_keeps_the_development_variant_on_its_class():
    from models.posenet import PoseNet
    from posepaf import fused_model as fm

    class Wrap(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.posenet = PoseNet(2, 256, 50, bn=True, increase=128, init_weights=False)

    assert type(fm.FusedIMHN.from_network(Wrap().eval())) is fm.FusedIMHN


@pytest.mark.parametrize("prefix", ["", "module."])
def test_build_network_reads_architecture_and_depth_off_a_checkpoint(tmp_path, monkeypatch, prefix):
    """The user's path, posepaf.model_init.build_network("auto", path): torch.load of a .pth with a 'weights' entry, architecture and
    nstack read off its keys, strict load -- on a narrow configuration (32 + 16 s channels) so that the file stays small; also for a
    checkpoint saved from a DataParallel wrapper (`module.` in front of every key).  The wrong explicit architecture fails with the
    hint, and `auto` without a checkpoint is refused."""
    from config.config import TrainingOpt
    from posepaf.model_init import build_network, deterministic_init
    monkeypatch.setattr(TrainingOpt, "hourglass_inp_dim", 32)
    monkeypatch.setattr(TrainingOpt, "increase", 16)
    src = _net("final", 3)
    deterministic_init(src, seed=3)
    path = str(tmp_path / "final3.pth")
    torch.save({"weights": {prefix + k: v for k, v in src.state_dict().items()}}, path)
    net, arch = build_network("auto", path)
    assert arch == "final" and net.posenet.nstack == 3 and not net.training
    assert all(torch.equal(v, net.state_dict()[k]) for k, v in src.state_dict().items())
    net, arch = build_network("final", path, nstack=3)
    assert arch == "final" and torch.equal(net.state_dict()["posenet.pre.conv1.weight"], src.state_dict()["posenet.pre.conv1.weight"])
    with pytest.raises(RuntimeError, match=r"--arch final with nstack 3"):
        build_network("posenet", path)
    with pytest.raises(ValueError, match="checkpoint"):
        build_network("auto", None)
