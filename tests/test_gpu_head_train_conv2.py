"""GPU: HeadTrainer(train="heads+conv2") -- the heads and both 3 x 3 convolutions below each -- on the synthetic `final` network of
tests/test_gpu_head_train_conv.py (2 stages, batch 2, 64 x 64 input: maps of 16^2, 8^2, 4^2, 2^2 and 1^2 pixels).

The heads' and the ("conv", t, s) gradients are those of a "heads+conv" trainer bit for bit.  dY2 and the ("conv2", t, s) gradients
are held (a) to the derived bounds of tests/conv_dgrad_reference.py and tests/conv_wgrad_reference.py on the tensors the calls read,
and (b) to an independent float64 autograd replica of the cut (convolution -> LeakyReLU -> convolution -> LeakyReLU -> head -> the
loss on stock operators, from c2's captured input and the binary16 weights).  The device result passes through binary16 activations,
predictions, g, dY and dY2, so its distance to (b) cannot be derived: the threshold is twice the largest per-layer relative error
|dW - dW_ref| / |dW_ref| of the wgrad="torch" formulation over three batches in the same run, which uses none of the kernels under
test; both are printed.  The update paths -- update="device" goes through pp_layer_update_f32 here --,
the captured step, a skipped step and state_dict() are held to bit equality."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_dgrad_reference as dref
import conv_wgrad_reference as ref
from conftest import PKG
from test_gpu_head_train_conv import B, DEV, LR, SEEDS, STAGES, batch, bits, same

pytestmark = pytest.mark.gpu

KINDS = ("conv", "conv2")


@pytest.fixture(scope="module")
def data():
    from posepaf import head_train
    from posepaf.model_init import build_network
    keep = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    net, arch = build_network("final", None, 7, nstack=STAGES)
    assert arch == "final"
    batches = [batch(seed) for seed in SEEDS]
    head_train.HeadTrainer(net, DEV, lr=LR).gradients(*batches[0])      # times the forward's kernel candidates of these shapes
    yield dict(net=net, batches=batches)
    torch.backends.cudnn.deterministic = keep


def make(data, **kw):
    from posepaf import head_train
    kw.setdefault("train", "heads+conv2")
    return head_train.HeadTrainer(data["net"], DEV, lr=LR, **kw)


@pytest.fixture(scope="module")
def device_trainer(data):
    tr = make(data, wgrad="device")
    assert len(tr.convs) == 2 * 5 * STAGES and [k[0] for k in tr.convs] == ["conv"] * 5 * STAGES + ["conv2"] * 5 * STAGES
    return tr


# ------------------------------------------------------------------------------------------------ gradients

def test_upper_layers_gradients_are_those_of_a_heads_conv_trainer(data, device_trainer):
    upper_tr = make(data, train="heads+conv", wgrad="device")
    upper = upper_tr.gradients(*data["batches"][0])
    both = device_trainer.gradients(*data["batches"][0])
    assert sorted(map(str, both)) == sorted(map(str, list(upper) + [("conv2", t, s) for t, s in device_trainer.heads]))
    for key, (dw, db) in upper.items():
        assert same(dw, both[key][0]) and same(db, both[key][1]), key
    n_upper = upper_tr._flat.numel()                             # the new masters lie behind: the ranges of the existing keys stay
    assert same(device_trainer._flat[:n_upper], upper_tr._flat) and device_trainer._flat.numel() > n_upper
    for t, s in device_trainer.heads:
        dw, db = both[("conv2", t, s)]
        assert tuple(dw.shape) == (256, 3, 3, 256) and tuple(db.shape) == (256,) and bool(torch.isfinite(dw).all()) and float(dw.abs().max()) > 0


def test_kernels_within_the_derived_bounds(data, device_trainer):
    from posepaf import fused_model
    tr = device_trainer
    got = tr.gradients(*data["batches"][0])
    inv = 1.0 / tr.loss_scale_for(B)
    kept = {key: tuple(None if v is None or isinstance(v, int) else v.clone() for v in val) for key, val in tr.last_inputs.items()}
    via_torch = tr.gradients_from_last("torch")
    worst = 0.0
    for key in (k for k in tr.convs if k[0] == "conv2"):
        _, y_mid, dy = kept[("conv",) + key[1:]]
        w16, x_in, dy2 = kept[key]
        dy2_t = tr.last_inputs[key][2]
        n, h, w, c = x_in.shape
        assert same(w16.permute(0, 3, 1, 2), tr.convs[("conv",) + key[1:]].weight)          # c3's own binary16 weight, (K, 3, 3, C)
        assert dy2.dtype == torch.float16 and tuple(dy2.shape) == (n * h * w, 256) and tuple(y_mid.shape) == (n, h, w, 256)
        dyn, wn, yn = dy.cpu().numpy(), w16.cpu().numpy(), y_mid.cpu().numpy()
        # pp_conv3x3_dgrad_f16 on what it read
        t64 = dref.conv3x3_dgrad(dyn, wn, yn, (n, h, w), fused_model.LEAK)
        bound = dref.conv3x3_dgrad_bound(dyn, wn, yn, (n, h, w), fused_model.LEAK)
        err = np.abs(dy2.cpu().numpy().astype(np.float64).reshape(t64.shape) - t64)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (key, float((err / bound).max()))
        # the torch form of the same step, on ITS dY (which may differ from pp_head_dgrad_f16's in the last binary16 bit)
        dy_t = tr.last_inputs[("conv",) + key[1:]][2].cpu().numpy()
        t64_t, bound_t = dref.conv3x3_dgrad(dy_t, wn, yn, (n, h, w), fused_model.LEAK), dref.conv3x3_dgrad_bound(dy_t, wn, yn, (n, h, w), fused_model.LEAK)
        assert (np.abs(dy2_t.cpu().numpy().astype(np.float64).reshape(t64.shape) - t64_t) <= bound_t).all(), key
        # pp_conv3x3_wgrad_f16 on what it read
        d2n, xn = dy2.cpu().numpy(), x_in.cpu().numpy()
        want_w, want_b = ref.conv3x3_wgrad(d2n, xn, inv)
        bw, bb = ref.conv3x3_bounds(d2n, xn, inv)
        dw, db = got[key][0].cpu().numpy().astype(np.float64), got[key][1].cpu().numpy().astype(np.float64)
        assert (np.abs(dw - want_w) <= bw).all() and (np.abs(db - want_b) <= bb).all(), key
        # against wgrad='torch': its dY and dY2 may differ from the kernels' in the last binary16 bit; the difference of the dY2 that
        # the two weight gradients read, carried through the convolution's sum, and torch's float32 rounding of its result are added
        diff = np.abs(d2n.astype(np.float64) - dy2_t.cpu().numpy().astype(np.float64)).reshape(xn.shape[:3] + (-1,))
        carry_w, carry_b = ref._wgrad(diff, np.abs(xn.astype(np.float64)))
        tw, tb = via_torch[key][0].cpu().numpy().astype(np.float64), via_torch[key][1].cpu().numpy().astype(np.float64)
        assert (np.abs(dw - tw) <= bw + inv * carry_w + 2.0 ** -22 * np.abs(tw)).all(), key
        assert (np.abs(db - tb) <= bb + inv * carry_b + 2.0 ** -22 * np.abs(tb)).all(), key
    print(f"largest |dY2 - ref| / bound over {5 * STAGES} layers = {worst:.4f}")


def replica_dw(tr, key, x_in, target):
    """dW of c2 of the unscaled loss by float64 autograd on the CPU: c2's captured input, the binary16 weights as they are"""
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import finetune
    from posepaf import fused_model, head_train
    _, t, s = key
    c2, c3, head = tr.convs[key], tr.convs[("conv", t, s)], tr.heads[(t, s)]
    leak = float(np.float32(fused_model.LEAK))
    w = c2.weight.detach().double().cpu().contiguous().requires_grad_(True)
    b = c2.bias.detach().double().cpu().requires_grad_(True)
    y1 = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(x_in.double().cpu().permute(0, 3, 1, 2), w, b, padding=1), leak)
    y2 = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(y1, c3.weight.detach().double().cpu().contiguous(),
                                                                    c3.bias.detach().double().cpu(), padding=1), leak)
    pred = torch.nn.functional.conv2d(y2, head.weight.detach().double().cpu().view(head.k_real, -1, 1, 1), head.bias.detach().double().cpu())
    terms = finetune.torch_terms(torch, [[pred]], target[:, 0].cpu())
    weight = head_train.term_weights(B, tr.T, tr.K, tr.nstack_weight)[t][s]
    dw, db = torch.autograd.grad((terms[0, 0] * weight).sum(), (w, b))
    return dw.permute(0, 2, 3, 1).contiguous(), db


def test_against_a_float64_autograd_replica_of_the_cut(data, device_trainer):
    tr = device_trainer
    keys = [k for k in tr.convs if k[0] == "conv2"]
    rel = {"torch": [], "device": []}
    for x, target in data["batches"]:
        dev = tr.gradients(x, target)
        inputs = {key: tr.last_inputs[key][1].clone() for key in keys}
        tor = tr.gradients_from_last("torch")
        for key in keys:
            want, _ = replica_dw(tr, key, inputs[key], target)
            norm = float(want.norm())
            assert norm > 0
            for name, grads in (("torch", tor), ("device", dev)):
                rel[name].append(float((grads[key][0].double().cpu() - want).norm()) / norm)
    worst_torch, worst_device = max(rel["torch"]), max(rel["device"])
    print(f"relative error of c2's dW against the float64 replica over {len(SEEDS)} batches x {len(keys)} layers: torch formulation "
          f"max {worst_torch:.3e} (median {np.median(rel['torch']):.3e}), kernels max {worst_device:.3e} (median {np.median(rel['device']):.3e})")
    assert worst_device <= 2.0 * worst_torch


# ------------------------------------------------------------------------------------------------ steps

def state(tr):
    out = [bits(tr._flat), bits(tr._flat_buf)]
    for h in tr.heads.values():
        out += [bits(h.weight), bits(h.bias), bits(h.wpad), bits(h.bpad)]
    for c in tr.convs.values():
        out += [bits(c.weight), bits(c.bias)]
    return out


def pointers(tr):
    return [(c.weight.data_ptr(), c.bias.data_ptr()) for c in list(tr.convs.values()) + list(tr.heads.values())]


def steps(tr, batches, n):
    out, ptrs, first = [], pointers(tr), bits(tr._flat).copy()
    for step in range(n):
        loss = tr.step(*batches[step % 2])
        assert loss.dtype == torch.float64 and loss.dim() == 0
        print(f"step {step}: loss {float(loss):.6f}, gradient norm {float(tr.grad_norm()):.4e}, skipped {int(tr.skipped_steps)}")
        out.append((state(tr), loss.detach().cpu().numpy().view(np.int64)))
        assert pointers(tr) == ptrs, step
        for key, conv in tr.convs.items():         # the fused layer runs the rounded master: bit for bit, in place
            w, b = tr.masters[key]
            assert same(conv.weight.permute(0, 2, 3, 1), w.detach().half()) and same(conv.bias, b.detach().half()), (step, key)
    assert int(tr.skipped_steps) == 0 and not np.array_equal(first, bits(tr._flat))
    return out


def assert_same_steps(a, b):
    assert len(a) == len(b)
    for step, ((sa, la), (sb, lb)) in enumerate(zip(a, b)):
        assert np.array_equal(la, lb), (step, "loss")
        assert len(sa) == len(sb) == 2 + (4 + 2 * 2) * 5 * STAGES
        for i, (u, v) in enumerate(zip(sa, sb)):
            assert np.array_equal(u, v), (step, i)


def test_torch_update_equals_device_update(data):
    a = steps(make(data, wgrad="device", update="torch"), data["batches"], 3)
    dev = make(data, wgrad="device", update="device")
    assert dev._segments                                          # pp_layer_update_f32, also on this 30-layer network
    b = steps(dev, data["batches"], 3)
    assert_same_steps(a, b)
    assert not np.array_equal(a[0][0][0], a[2][0][0])
    n_conv2 = sum(w.numel() + b_.numel() for k, (w, b_) in dev.masters.items() if k[0] == "conv2")
    assert not np.array_equal(a[0][0][0][-n_conv2:], a[2][0][0][-n_conv2:])      # c2's masters moved


def test_graph_equals_eager_and_set_lr(data):
    kw = dict(wgrad="multi", update="device", loss_scale="dynamic", init_scale=2.0 ** 10)
    eager, graphed = make(data, **kw), make(data, graph=True, **kw)
    a, b = steps(eager, data["batches"][:1] * 2, 3), steps(graphed, data["batches"][:1] * 2, 3)
    for tr in (eager, graphed):
        tr.set_lr(LR / 4)                                          # the replay reads the device block
    a, b = a + steps(eager, data["batches"][:1] * 2, 1), b + steps(graphed, data["batches"][:1] * 2, 1)
    assert graphed.graph_replays > 0 and eager.graph_replays == 0
    assert_same_steps(a, b)


def test_an_infinite_prediction_skips_the_step(data):
    tr = make(data, wgrad="multi", update="device")
    tr.step(*data["batches"][0])
    before = state(tr)

    def poison(mod, args, out):
        out[0, 0, 0, 0] = float("inf")
    handle = tr.heads[(0, 0)].register_forward_hook(poison)
    try:
        tr.step(*data["batches"][1])
    finally:
        handle.remove()
    assert int(tr.skipped_steps) == 1 and not bool(torch.isfinite(tr._flat_grad).all())
    for i, (u, v) in enumerate(zip(before, state(tr))):
        assert np.array_equal(u, v), i
    tr.step(*data["batches"][1])
    assert int(tr.skipped_steps) == 1 and not np.array_equal(before[0], bits(tr._flat))


def test_state_dict_rebuilds_the_trainers_model(data, tmp_path):
    from posepaf import fused_model
    from posepaf.model_init import build_network
    tr = make(data, wgrad="device")
    for i in range(2):
        tr.step(*data["batches"][i])
    sd = {k: v.detach().cpu() for k, v in tr.state_dict().items()}
    assert sorted(sd) == sorted(data["net"].state_dict())
    assert all(v.dtype == data["net"].state_dict()[k].dtype and v.shape == data["net"].state_dict()[k].shape for k, v in sd.items())
    path = tmp_path / "heads_conv2.pth"
    torch.save({"weights": sd}, str(path))
    net2, arch = build_network("auto", str(path), 7)            # evaluate.py's loader (strict)
    assert arch == "final" and net2.posenet.nstack == STAGES
    fresh = fused_model.FusedIMHN.from_network(net2, folded_merge=False).eval().to(DEV).half().to(memory_format=torch.channels_last)
    for (t, s), head in tr.heads.items():
        for kind, name in zip(KINDS, ("c3", "c2")):
            mine, theirs = tr.convs[(kind, t, s)], getattr(fresh.feat[t][s], name)
            assert mine is getattr(tr.model.feat[t][s], name)
            assert same(theirs.weight, mine.weight) and same(theirs.bias, mine.bias), (kind, t, s)
        hf = fresh.head[t][s]
        assert same(hf.weight, head.weight) and same(hf.bias, head.bias) and same(hf.wpad, head.wpad) and same(hf.bpad, head.bpad), (t, s)
    x = data["batches"][0][0]
    with torch.no_grad():
        got, want = fresh(x, all_preds=True), tr.model(x, all_preds=True)
    for t in range(STAGES):
        for s in range(5):
            assert same(got[t][s], want[t][s]), (t, s)


def test_argument_refusals_raise_before_any_launch(data):
    from posepaf import head_train
    from posepaf._lib import PosePafError
    from posepaf.model_init import build_network
    net, _ = build_network("posenet", None, 7, nstack=1)
    with pytest.raises(PosePafError, match="final"):
        head_train.HeadTrainer(net, DEV, train="heads+conv2")
    with pytest.raises(PosePafError, match="heads\\+conv2"):
        make(data, train="conv2")
    with pytest.raises(PosePafError, match="dynamic"):
        make(data, loss_scale="dynamic", update="torch")
    with pytest.raises(PosePafError, match="graph"):
        make(data, graph=True, update="torch")


def test_finetune_runs_to_the_end(tmp_path):
    """finetune.py --train heads+conv2 --graph --wgrad multi --loss_scale dynamic as a child process: a small synthetic set at 128 x 128"""
    env = dict(os.environ, POSEPAF_CACHE_DIR=str(tmp_path / "cache"))
    out = tmp_path / "conv2.pth"
    cmd = [sys.executable, os.path.join(PKG, "finetune.py"), "--model", "fused", "--arch", "final", "--train", "heads+conv2", "--graph", "--wgrad",
           "multi", "--loss_scale", "dynamic", "--synthetic", "4", "--batch", "2", "--sizes", "128x128", "--stages", "2", "--steps", "4",
           "--lr", "1e-3", "--save", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    print(res["losses"], res["steps_per_s"], res["skipped_steps"])
    assert res["train"] == "heads+conv2" and res["graph"] is True and res["graph_replays"] >= 2 and res["update"] == "device"
    assert len(res["losses"]) == 4 and all(np.isfinite(v) for v in res["losses"])
    from posepaf.model_init import build_network
    net, arch = build_network("auto", str(out), 7)                # evaluate.py -p's loader
    assert arch == "final" and net.posenet.nstack == 2
