"""GPU: HeadTrainer(train="heads+conv") -- the heads and the 3 x 3 convolution in front of each -- on a synthetic `final` network with
2 stages, batch 2, 64 x 64 input: the convolutions see maps of 16^2, 8^2, 4^2, 2^2 and 1^2 pixels.

The kernels' gradients are held (a) to the derived bounds of tests/conv_wgrad_reference.py on the tensors the calls read, (b) to the
wgrad="torch" formulation of the same captured tensors, and (c) to an independent float64 autograd replica of the cut (convolution
-> LeakyReLU -> head -> the loss on stock operators, from the captured convolution input and the binary16 weights).  The device
result passes through binary16 y, predictions, g and dY, so its distance to (c) cannot be derived: the threshold is twice the
largest per-layer relative error  |dW - dW_ref| / |dW_ref|  of the wgrad="torch" formulation over three batches, which uses none of
the kernels under test.  Measured on the MI355X (printed by the test): torch formulation max 5.632e-03,
kernels max 5.632e-03 in one run, 2.885e-02 and 2.885e-02 in another (the forward's kernel choices are timed per process).
The update paths, the captured step, the in-place write-back, a skipped step and state_dict() are held to bit equality."""
import os
import sys

import numpy as np
import pytest
import torch

import conv_wgrad_reference as ref
from conftest import PKG

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
STAGES, B, H, W = 2, 2, 64, 64
LR = 1e-3              # at 1e-2 (the heads' tests) four steps on one batch ran into a non-finite gradient and a skipped step
SEEDS = (1, 2, 3)


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def batch(seed):
    from posepaf import synth, synth_device
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.uniform(0.0, 1.0, (B, H, W, 3)).astype(np.float16)).to(DEV)
    people = [synth.random_people(1 + i + seed, np.random.default_rng(20 + 10 * seed + i), img_h=H, img_w=W) for i in range(B)]
    joints, n_people = synth_device.pack_joints(people, 8)
    target = synth_device.render_scenes(torch.from_numpy(joints).to(DEV), torch.from_numpy(n_people).to(DEV), H // 4, W // 4,
                                        dtype=torch.float16, flip=False, noise=0.0, reverse_kp=True)
    return x, target


@pytest.fixture(scope="module")
def data():
    """the network, three batches, and one warm-up forward that times the kernel candidates of these shapes (cudnn.deterministic: the
    3 x 3 convolution on the 1 x 1 map runs on MIOpen, see tests/test_gpu_head_train.py::data)"""
    from posepaf import head_train
    from posepaf.model_init import build_network
    keep = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    net, arch = build_network("final", None, 7, nstack=STAGES)
    assert arch == "final"
    batches = [batch(seed) for seed in SEEDS]
    head_train.HeadTrainer(net, DEV, lr=LR).gradients(*batches[0])
    yield dict(net=net, batches=batches)
    torch.backends.cudnn.deterministic = keep


def make(data, **kw):
    from posepaf import head_train
    kw.setdefault("train", "heads+conv")
    return head_train.HeadTrainer(data["net"], DEV, lr=LR, **kw)


@pytest.fixture(scope="module")
def device_trainer(data):
    tr = make(data, wgrad="device")
    assert len(tr.convs) == 5 * STAGES and all(k[0] == "conv" for k in tr.convs)
    return tr


# ------------------------------------------------------------------------------------------------ gradients

def test_head_gradients_are_those_of_a_heads_trainer(data, device_trainer):
    heads = make(data, train="heads", wgrad="device").gradients(*data["batches"][0])
    both = device_trainer.gradients(*data["batches"][0])
    assert sorted(map(str, both)) == sorted(map(str, list(heads) + [("conv", t, s) for t, s in heads]))
    for key, (dw, db) in heads.items():
        assert same(dw, both[key][0]) and same(db, both[key][1]), key
    for t, s in heads:
        dw, db = both[("conv", t, s)]
        assert tuple(dw.shape) == (256, 3, 3, 256) and tuple(db.shape) == (256,) and bool(torch.isfinite(dw).all()) and float(dw.abs().max()) > 0


def test_kernels_within_the_derived_bounds_and_against_the_torch_formulation(data, device_trainer):
    from posepaf import fused_model
    tr = device_trainer
    got = tr.gradients(*data["batches"][0])
    inv = 1.0 / tr.loss_scale_for(B)
    kept = {key: tuple(None if v is None or isinstance(v, int) else v.clone() for v in val) for key, val in tr.last_inputs.items()}
    via_torch = tr.gradients_from_last("torch")
    for key in tr.convs:
        g2, ldg, y2, scale = kept[key[1:]]
        w16, x_in, dy = kept[key]
        dy_t = tr.last_inputs[key][2]                                 # the torch formulation's binary16 dY
        assert scale is None and dy.dtype == torch.float16 and tuple(dy.shape) == tuple(y2.shape) == (x_in.shape[0] * x_in.shape[1] * x_in.shape[2], 256)
        g, w, y = g2.cpu().numpy(), w16.cpu().numpy(), y2.cpu().numpy()
        # pp_head_dgrad_f16 on what it read
        t64, bound = ref.head_dgrad(g, w, y, g.shape[1], fused_model.LEAK), ref.head_dgrad_bound(g, w, y, g.shape[1], fused_model.LEAK)
        err = np.abs(dy.cpu().numpy().astype(np.float64) - t64)
        assert (err <= bound).all(), (key, float((err / bound).max()))
        assert (np.abs(dy_t.cpu().numpy().astype(np.float64) - t64) <= bound).all(), key      # and the torch form of the same step
        # pp_conv3x3_wgrad_f16 on what it read
        dyn, xn = dy.cpu().numpy(), x_in.cpu().numpy()
        want_w, want_b = ref.conv3x3_wgrad(dyn, xn, inv)
        bw, bb = ref.conv3x3_bounds(dyn, xn, inv)
        dw, db = got[key][0].cpu().numpy().astype(np.float64), got[key][1].cpu().numpy().astype(np.float64)
        assert (np.abs(dw - want_w) <= bw).all() and (np.abs(db - want_b) <= bb).all(), key
        # against wgrad='torch': its dY may differ from the kernel's where the float32 sum rounds to the other binary16 neighbour;
        # that difference, carried through the convolution's sum, and torch's float32 rounding of its own result are added
        diff = np.abs(dyn.astype(np.float64) - dy_t.cpu().numpy().astype(np.float64)).reshape(xn.shape[:3] + (-1,))
        carry_w, carry_b = ref._wgrad(diff, np.abs(xn.astype(np.float64)))
        tw, tb = via_torch[key][0].cpu().numpy().astype(np.float64), via_torch[key][1].cpu().numpy().astype(np.float64)
        assert (np.abs(dw - tw) <= bw + inv * carry_w + 2.0 ** -22 * np.abs(tw)).all(), key
        assert (np.abs(db - tb) <= bb + inv * carry_b + 2.0 ** -22 * np.abs(tb)).all(), key
        print(f"{key}: dY differs from the torch form in {int((diff > 0).sum())} of {diff.size} elements")


def replica_dw(tr, key, x_in, target):
    """dW of the unscaled loss by float64 autograd on the CPU: the captured convolution input, the binary16 weights as they are"""
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import finetune
    from posepaf import fused_model, head_train
    _, t, s = key
    c3, head = tr.convs[key], tr.heads[(t, s)]
    w = c3.weight.detach().double().cpu().contiguous().requires_grad_(True)
    b = c3.bias.detach().double().cpu().requires_grad_(True)
    y = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(x_in.double().cpu().permute(0, 3, 1, 2), w, b, padding=1),
                                       float(np.float32(fused_model.LEAK)))
    pred = torch.nn.functional.conv2d(y, head.weight.detach().double().cpu().view(head.k_real, -1, 1, 1), head.bias.detach().double().cpu())
    terms = finetune.torch_terms(torch, [[pred]], target[:, 0].cpu())
    weight = head_train.term_weights(B, tr.T, tr.K, tr.nstack_weight)[t][s]
    dw, db = torch.autograd.grad((terms[0, 0] * weight).sum(), (w, b))
    return dw.permute(0, 2, 3, 1).contiguous(), db


def test_against_a_float64_autograd_replica_of_the_cut(data, device_trainer):
    tr = device_trainer
    rel = {"torch": [], "device": []}
    for x, target in data["batches"]:
        dev = tr.gradients(x, target)
        inputs = {key: tr.last_inputs[key][1].clone() for key in tr.convs}
        tor = tr.gradients_from_last("torch")
        for key in tr.convs:
            want, want_b = replica_dw(tr, key, inputs[key], target)
            norm = float(want.norm())
            assert norm > 0
            for name, grads in (("torch", tor), ("device", dev)):
                rel[name].append(float((grads[key][0].double().cpu() - want).norm()) / norm)
    worst_torch, worst_device = max(rel["torch"]), max(rel["device"])
    print(f"relative error of dW against the float64 replica over {len(SEEDS)} batches x {len(tr.convs)} layers: torch formulation "
          f"max {worst_torch:.3e} (median {np.median(rel['torch']):.3e}), kernels max {worst_device:.3e} (median {np.median(rel['device']):.3e})")
    assert worst_device <= 2.0 * worst_torch


# ------------------------------------------------------------------------------------------------ steps

def state(tr):
    out = [bits(tr._flat), bits(tr._flat_buf)]
    for h in tr.heads.values():
        out += [bits(h.weight), bits(h.bias)]
    for c in tr.convs.values():
        out += [bits(c.weight), bits(c.bias)]
    return out


def pointers(tr):
    return [(c.weight.data_ptr(), c.bias.data_ptr()) for c in tr.convs.values()] + [(h.weight.data_ptr(), h.bias.data_ptr()) for h in tr.heads.values()]


def steps(tr, batches, n):
    out, ptrs, first = [], pointers(tr), bits(tr._flat).copy()
    for step in range(n):
        loss = tr.step(*batches[step % 2])
        assert loss.dtype == torch.float64 and loss.dim() == 0
        print(f"step {step}: loss {float(loss):.6f}, gradient norm {float(tr.grad_norm()):.4e}, skipped {int(tr.skipped_steps)}")
        out.append((state(tr), loss.detach().cpu().numpy().view(np.int64), None))
        assert pointers(tr) == ptrs, step
        for key, c3 in tr.convs.items():          # the fused layer runs the rounded master: bit for bit, in place
            w, b = tr.masters[key]
            assert same(c3.weight.permute(0, 2, 3, 1), w.detach().half()) and same(c3.bias, b.detach().half()), (step, key)
    assert int(tr.skipped_steps) == 0 and not np.array_equal(first, bits(tr._flat))
    return out


def assert_same_steps(a, b):
    assert len(a) == len(b)
    for step, ((sa, la, _), (sb, lb, _)) in enumerate(zip(a, b)):
        assert np.array_equal(la, lb), (step, "loss")
        assert len(sa) == len(sb) == 2 + 4 * 5 * STAGES
        for i, (u, v) in enumerate(zip(sa, sb)):
            assert np.array_equal(u, v), (step, i)


def test_torch_update_equals_device_update(data):
    a = steps(make(data, wgrad="device", update="torch"), data["batches"], 3)
    b = steps(make(data, wgrad="device", update="device"), data["batches"], 3)
    assert_same_steps(a, b)
    assert not np.array_equal(a[0][0][0], a[2][0][0])


def test_graph_equals_eager(data):
    eager = make(data, wgrad="multi", update="device", loss_scale="dynamic", init_scale=2.0 ** 10)
    graphed = make(data, wgrad="multi", update="device", loss_scale="dynamic", init_scale=2.0 ** 10, graph=True)
    a, b = steps(eager, data["batches"][:1] * 2, 4), steps(graphed, data["batches"][:1] * 2, 4)
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
    path = tmp_path / "heads_conv.pth"
    torch.save({"weights": sd}, str(path))
    net2, arch = build_network("auto", str(path), 7)            # evaluate.py's loader (strict)
    assert arch == "final" and net2.posenet.nstack == STAGES
    fresh = fused_model.FusedIMHN.from_network(net2, folded_merge=False).eval().to(DEV).half().to(memory_format=torch.channels_last)
    for (t, s), head in tr.heads.items():
        c3, c3f, hf = tr.convs[("conv", t, s)], fresh.feat[t][s].c3, fresh.head[t][s]
        assert same(c3f.weight, c3.weight) and same(c3f.bias, c3.bias), (t, s)
        assert same(hf.weight, head.weight) and same(hf.bias, head.bias) and same(hf.wpad, head.wpad) and same(hf.bpad, head.bpad), (t, s)
    x = data["batches"][0][0]
    with torch.no_grad():
        got, want = fresh(x, all_preds=True), tr.model(x, all_preds=True)
    for t in range(STAGES):
        for s in range(5):
            assert same(got[t][s], want[t][s]), (t, s)
