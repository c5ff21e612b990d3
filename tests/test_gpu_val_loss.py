"""GPU: the validation loss on the device (pp_focal_l2_terms, posepaf.val_loss, FusedIMHN.forward(all_preds=True), evaluate.py
--val_loss) against the NumPy float64 restatement tests/loss_reference.py.

Bound of a term [t][s][b]: relative 1e-9.  The terms are non-negative for a mask in [0, 1]; a float64 sum of N <= 50 * 128 * 128 of them
in any order is within N * 2^-53 = 9e-11 of any other order, and the few roundings of one term are below that.  The targets here hold
only 0 and values in [2^-17, 1] and no window holds more than 2^13 cells, so every window sum is exact in float64 and G itself does not
depend on the order (asserted on the host).  (The 20 x 28 -> 1 x 1 case pools the whole map, 560 cells: exactness holds up to 2^13 cells
for such values -- every value is a multiple of 2^-40 -- and that is what the host side asserts.)"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import loss_reference as lr
from conftest import PKG

pytestmark = pytest.mark.gpu

REL = 1e-9
SHAPES = {"32x48": (32, 48, [(32, 48), (16, 24), (8, 12), (4, 6), (2, 3)]),
          "20x28": (20, 28, [(20, 28), (10, 14), (5, 7), (2, 3), (1, 1)])}
# (prediction dtype, target dtype, mask, plain L2)
COMBOS = {"p16_t16_nomask": ("f16", "f16", None, False), "p32_t32_binary": ("f32", "f32", "binary", False),
          "p16_t32_soft": ("f16", "f32", "soft", False), "p32_t16_plain": ("f32", "f16", None, True)}
T_ALL, B_ALL = 4, 3
F = np.float32(0.01)


def make_target(H, W, dtype, rng):
    """0 or values in [2^-10, 1], plus plateaus of the renderer's floor: one aligned to the 2 x 2 / 4 x 4 blocks of the dividing
    scales, one not.  float32: 0.01f itself; float16: binary16(0.01) = 0.0100021, also >= 0.01f"""
    t = np.where(rng.random((B_ALL, 50, H, W)) < 0.25, rng.uniform(2.0 ** -10, 1.0, (B_ALL, 50, H, W)), 0.0).astype(np.float32)
    t[:, 0:4, 0:8, 0:12] = F
    t[:, 4:8, 3:13, 5:17] = F
    t[1, 31] = F                                              # a whole plane of the floor: every window of every scale
    if dtype == "f16":
        t = t.astype(np.float16)
    nz = t[t != 0].astype(np.float64)
    assert nz.min() >= 2.0 ** -17 and nz.max() <= 1.0
    return t


@pytest.fixture(scope="module")
def cases():
    """per shape: the inputs of every combination and the restatement's terms (T_ALL, 5, B_ALL), computed once; a launch with fewer
    stacks / scales / images is compared with a slice (a term depends on its own prediction, target image and mask image only)"""
    out = {}
    for name, (H, W, sizes) in SHAPES.items():
        rng = np.random.default_rng(1000 + H)
        # exact window sums: every value is a multiple of 2^-40 (a float32 >= 2^-17), so a partial sum of n values <= 1 is a multiple
        # of 2^-40 below n -- exact in float64 while n <= 2^13.  The largest windows here: 16 x 16 = 256 cells (32 x 48 -> 2 x 3) and
        # the whole 20 x 28 = 560-cell map (-> 1 x 1)
        largest = max((r1 - r0) * (c1 - c0) for (h, w) in sizes for r0, r1 in lr.windows(H, h) for c0, c1 in lr.windows(W, w))
        assert largest == (256 if name == "32x48" else 560) and largest <= 2 ** 13
        targets = {d: make_target(H, W, d, rng) for d in ("f16", "f32")}
        pooled = {d: lr.pool_scales(t, sizes) for d, t in targets.items()}
        for d in pooled:   # the plateaus pool to themselves: foreground at every scale
            floor = targets[d][1, 31, 0, 0]
            assert all((pooled[d][s][1][31] == np.float32(floor)).all() and floor >= F for s in range(5))
        p16 = [[(rng.random((B_ALL, 50, h, w)) * 1.2 - 0.1).astype(np.float16) for (h, w) in sizes] for _ in range(T_ALL)]
        p32 = [[(rng.random((B_ALL, 50, h, w)) * 1.2 - 0.1).astype(np.float32) for (h, w) in sizes] for _ in range(T_ALL)]
        masks = {None: None, "binary": (rng.random((B_ALL, H, W)) < 0.7).astype(np.float32), "soft": rng.random((B_ALL, H, W)).astype(np.float32)}
        assert lr.near_half_mask_values(masks["soft"], sizes) == 0
        for cname, (pd, td, mk, plain) in COMBOS.items():
            preds = p16 if pd == "f16" else p32
            want = lr.focal_l2_terms(preds, targets[td], masks[mk], plain_l2=plain, pooled=pooled[td])
            assert np.isfinite(want).all() and (want[:, :4] > 0).all() and (want >= 0).all()   # (the coarsest scale may be masked away)
            out[(name, cname)] = dict(H=H, W=W, sizes=sizes, preds=preds, target=targets[td], mask=masks[mk], plain=plain, want=want)
    return out


def lay_out(p, layout):
    """host (B, 50, h, w) -> the device tensor the kernel reads: planes, or pixel-major with 64 / 50 elements per pixel (the padding
    channels hold NaN: they are never part of a sum)"""
    t = torch.from_numpy(p).cuda()
    if layout == "planes":
        return t.contiguous()
    stride = 64 if layout == "px64" else 50
    buf = torch.full((t.shape[0], t.shape[2], t.shape[3], stride), float("nan"), dtype=t.dtype, device="cuda")
    buf[..., :50] = t.permute(0, 2, 3, 1)
    return buf


GUARD = 64


def launch(case, layout, stacks=range(T_ALL), scales=range(5), images=range(B_ALL), sample_pair=False, twice=True):
    """pp_focal_l2_terms on a sub-problem of `case` -> host float64 (T, K, B).  Outputs and workspace start as NaN bytes with sentinel
    guards behind them; with `twice` the launch is repeated into fresh NaN-filled buffers and must give the same bits."""
    from posepaf import _lib
    L = _lib.load()
    stacks, scales, images = list(stacks), list(scales), list(images)
    T, K, B = len(stacks), len(scales), len(images)
    H, W = case["H"], case["W"]
    sizes = [case["sizes"][s] for s in scales]
    held = [[lay_out(np.ascontiguousarray(case["preds"][t][s][images]), layout) for s in scales] for t in stacks]
    pd = held[0][0].dtype
    target = torch.from_numpy(np.ascontiguousarray(case["target"][images])).cuda()
    image_stride = 50 * H * W
    if sample_pair:   # sample 0 of a (B, 2, 50, H, W) buffer whose sample 1 holds NaN
        pair = torch.full((B, 2, 50, H, W), float("nan"), dtype=target.dtype, device="cuda")
        pair[:, 0] = target
        target, image_stride = pair, 2 * 50 * H * W
    mask = torch.from_numpy(np.ascontiguousarray(case["mask"][images])).cuda() if case["mask"] is not None else None
    hs, ws = (C.c_int * K)(*[h for h, _ in sizes]), (C.c_int * K)(*[w for _, w in sizes])
    need = L.pp_focal_l2_workspace_bytes(B, T, K, hs, ws)
    assert need > 0 and need % 8 == 0
    table = (C.c_void_p * (T * K))(*[held[t][s].data_ptr() for t in range(T) for s in range(K)])
    results = []
    for _ in range(2 if twice else 1):
        terms = torch.full((T * K * B + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        terms[T * K * B:] = 12345.6789
        work = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        work[need:] = 0xA5
        rc = L.pp_focal_l2_terms(table, 1 if pd == torch.float16 else 0, {"planes": 0, "px64": 64, "px50": 50}[layout],
                                 C.c_void_p(target.data_ptr()), 1 if target.dtype == torch.float16 else 0, image_stride,
                                 C.c_void_p(mask.data_ptr()) if mask is not None else None, B, H, W, T, K, hs, ws, 0.1, 3.0,
                                 1 if case["plain"] else 0, C.c_void_p(work.data_ptr()), C.c_void_p(terms.data_ptr()),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
        torch.cuda.synchronize()
        got = terms.cpu().numpy()
        assert (got[T * K * B:] == 12345.6789).all() and (work[need:].cpu().numpy() == 0xA5).all(), "a guard was overwritten"
        assert np.isfinite(got[: T * K * B]).all(), "a term was not stored"
        results.append(got[: T * K * B].reshape(T, K, B).copy())
    if twice:
        assert results[0].tobytes() == results[1].tobytes(), "two launches differ"
    return results[0]


def close(got, want):
    return (np.abs(got - want) <= REL * np.abs(want)).all()


@pytest.mark.parametrize("layout", ["planes", "px64", "px50"])
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_terms_match_the_restatement(cases, shape, combo, layout):
    case = cases[(shape, combo)]
    got = launch(case, layout)
    rel = np.abs(got - case["want"]) / np.where(case["want"] > 0, case["want"], 1.0)
    print(f"{shape} {combo} {layout}: largest relative difference of a term {rel.max():.3e}")
    assert close(got, case["want"]), rel


@pytest.mark.parametrize("layout", ["planes", "px64", "px50"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fewer_stacks_scales_and_images(cases, shape, layout):
    """T = 1, n_scales = 1 (each scale alone, so also a coarse scale as the only one) and B = 1; an image launched alone is BIT-equal
    to the same image in the batch of 3, in every slot"""
    case = cases[(shape, "p16_t32_soft")]
    full = launch(case, layout, twice=False)
    one_stack = launch(case, layout, stacks=[2], twice=False)
    assert one_stack.tobytes() == full[2:3].tobytes() and close(one_stack, case["want"][2:3])
    for s in range(5):
        alone = launch(case, layout, scales=[s], twice=False)
        assert alone.tobytes() == full[:, s:s + 1].tobytes()
    for b in range(B_ALL):
        alone = launch(case, layout, images=[b], twice=False)
        assert alone.shape == (T_ALL, 5, 1) and alone.tobytes() == full[:, :, b:b + 1].tobytes(), b
        assert close(alone, case["want"][:, :, b:b + 1])
    swapped = launch(case, layout, images=[2, 0, 1], twice=False)
    assert swapped.tobytes() == full[:, :, [2, 0, 1]].tobytes()


@pytest.mark.parametrize("combo", ["p16_t16_nomask", "p32_t32_binary"])
def test_target_read_as_sample_0_of_a_pair_buffer(cases, combo):
    case = cases[("32x48", combo)]
    got = launch(case, "px64", sample_pair=True)
    assert got.tobytes() == launch(case, "px64", twice=False).tobytes() and close(got, case["want"])


def test_unaligned_runs_give_the_same_bits(cases):
    """the 16-byte loads and the element-by-element walk add the same elements in the same order: predictions 2 bytes off a 16-byte
    boundary (legal: aligned to their element) give the bits of the aligned launch"""
    from posepaf import _lib
    L = _lib.load()
    case = cases[("32x48", "p16_t16_nomask")]
    H, W, sizes = case["H"], case["W"], case["sizes"]
    hs, ws = (C.c_int * 5)(*[h for h, _ in sizes]), (C.c_int * 5)(*[w for _, w in sizes])
    need = L.pp_focal_l2_workspace_bytes(B_ALL, 1, 5, hs, ws)
    target = torch.from_numpy(case["target"]).cuda()
    outs = []
    for shift in (0, 1):
        held = []
        for s in range(5):
            flat = lay_out(case["preds"][0][s], "px64").reshape(-1)
            buf = torch.zeros(flat.numel() + 8, dtype=flat.dtype, device="cuda")
            buf[shift:shift + flat.numel()] = flat
            held.append((buf, buf.data_ptr() + 2 * shift))
        table = (C.c_void_p * 5)(*[p for _, p in held])
        terms = torch.full((5 * B_ALL,), float("nan"), dtype=torch.float64, device="cuda")
        work = torch.empty(need, dtype=torch.uint8, device="cuda")
        assert L.pp_focal_l2_terms(table, 1, 64, C.c_void_p(target.data_ptr()), 1, 50 * H * W, None, B_ALL, H, W, 1, 5, hs, ws, 0.1, 3.0, 0,
                                   C.c_void_p(work.data_ptr()), C.c_void_p(terms.data_ptr()), None) == 0
        torch.cuda.synchronize()
        outs.append(terms.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes() and close(outs[0].reshape(1, 5, B_ALL), case["want"][:1])


def test_refused_arguments_launch_nothing(cases):
    """every refusal returns its code and leaves terms and workspace as they were"""
    from posepaf import _lib
    L = _lib.load()
    case = cases[("20x28", "p16_t16_nomask")]
    H, W, sizes = case["H"], case["W"], case["sizes"]
    held = [[lay_out(case["preds"][t][s], "planes") for s in range(5)] for t in range(T_ALL)]
    target = torch.from_numpy(case["target"]).cuda()
    terms = torch.full((T_ALL * 5 * B_ALL,), 777.0, dtype=torch.float64, device="cuda")
    work = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda")

    def call(**over):
        k = dict(preds=[held[t][s].data_ptr() for t in range(T_ALL) for s in range(5)], dtype=1, stride=0, target=target.data_ptr(), tdtype=1,
                 timg=50 * H * W, mask=None, batch=B_ALL, H=H, W=W, T=T_ALL, K=5, hs=[h for h, _ in sizes], ws=[w for _, w in sizes],
                 work=work.data_ptr(), terms=terms.data_ptr())
        k.update(over)
        table = (C.c_void_p * len(k["preds"]))(*k["preds"]) if k["preds"] is not None else None
        hs = (C.c_int * len(k["hs"]))(*k["hs"])
        ws = (C.c_int * len(k["ws"]))(*k["ws"])
        return L.pp_focal_l2_terms(table, k["dtype"], k["stride"], k["target"], k["tdtype"], k["timg"], k["mask"], k["batch"], k["H"], k["W"],
                                   k["T"], k["K"], hs, ws, 0.1, 3.0, 0, k["work"], k["terms"], None)

    ptrs = [held[t][s].data_ptr() for t in range(T_ALL) for s in range(5)]
    refused = [(dict(T=0), -2), (dict(T=9, preds=ptrs * 3), -6), (dict(K=0), -2), (dict(K=6, hs=[20] * 6, ws=[28] * 6, preds=ptrs * 2), -6),
               (dict(batch=0), -2), (dict(batch=65536), -3), (dict(hs=[20, 10, 5, 2, 0]), -2), (dict(hs=[21, 10, 5, 2, 1]), -2),
               (dict(ws=[28, 29, 7, 3, 1]), -2), (dict(preds=None), -2), (dict(preds=ptrs[:-1] + [0]), -2),
               (dict(preds=ptrs[:-1] + [ptrs[-1] + 1]), -2), (dict(target=None), -2), (dict(target=target.data_ptr() + 1), -2),
               (dict(mask=work.data_ptr() + 2), -2), (dict(work=None), -2), (dict(work=work.data_ptr() + 4), -2), (dict(terms=None), -2),
               (dict(terms=terms.data_ptr() + 4), -2), (dict(dtype=2), -2), (dict(tdtype=3), -2), (dict(stride=1), -2), (dict(stride=49), -2),
               (dict(stride=-1), -2), (dict(timg=50 * H * W - 1), -2)]
    for over, want in refused:
        assert call(**over) == want, over
    torch.cuda.synchronize()
    assert (terms == 777.0).all() and (work == 0x5A).all()
    assert call() == 0                                       # and the unmodified call is taken
    torch.cuda.synchronize()
    assert close(terms.cpu().numpy().reshape(T_ALL, 5, B_ALL), case["want"])


# ---------------------------------------------------------------------------------------------- combine / ValLossMeter
def test_combine_and_meter_match_the_formula():
    from posepaf import val_loss
    rng = np.random.default_rng(8)
    a, b = rng.random((4, 5, 3)) * 100, rng.random((4, 5, 4)) * 100
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    got = val_loss.combine(ta)
    assert got.dim() == 0 and got.dtype == torch.float64 and got.is_cuda
    want = lr.combine(a)
    assert abs(got.item() - want) <= 1e-12 * want
    nw, sw = (1, 2, 3, 4), (0.5, 0.25, 1, 2, 4)
    assert abs(val_loss.combine(ta, nw, sw).item() - lr.combine(a, nw, sw)) <= 1e-12 * lr.combine(a, nw, sw)
    meter = val_loss.ValLossMeter()
    meter.update(ta)
    meter.update(tb, n_valid=2)                              # a padded last batch: its first two images count
    out = meter.summary()
    both = np.concatenate([a, b[:, :, :2]], axis=2)
    want = lr.combine(both)
    assert out["images"] == 5 and abs(out["val_loss"] - want) <= 1e-12 * want
    pss = both.sum(axis=2) / 5
    assert np.allclose(np.array(out["per_stack_scale"]), pss, rtol=1e-12, atol=0)
    for t in range(4):
        w = lr.combine(both[t:t + 1], (1,))
        assert abs(out["per_stack"][t] - w) <= 1e-12 * w
    for s in range(5):
        w = lr.combine(both[:, s:s + 1], scale_weight=(1,))
        assert abs(out["per_scale"][s] - w) <= 1e-12 * w
    # val_loss is the weighted combination of per_stack_scale
    w = sum(lr.SCALE_WEIGHT[s] * sum(out["per_stack_scale"][t][s] for t in range(4)) / 4 for s in range(5)) / sum(lr.SCALE_WEIGHT)
    assert abs(out["val_loss"] - w) <= 1e-12 * w


def test_python_surface_refuses_bad_arguments(cases):
    from posepaf import val_loss
    from posepaf._lib import PosePafError
    case = cases[("20x28", "p16_t16_nomask")]
    preds = [[torch.from_numpy(p).cuda() for p in stack] for stack in case["preds"]]
    target = torch.from_numpy(case["target"]).cuda()
    ok = val_loss.focal_l2_terms(preds, target)
    assert ok.shape == (T_ALL, 5, B_ALL) and close(ok.cpu().numpy(), case["want"])
    bad = [dict(preds=[]), dict(preds=[[p.cpu() for p in s] for s in preds]), dict(target=target.cpu()), dict(target=target[:2]),
           dict(target=target.double()), dict(mask=torch.ones(B_ALL, 20, 28)), dict(mask=torch.ones(B_ALL, 20, 27, device="cuda")),
           dict(preds=[preds[0], preds[1][:4]]), dict(preds=[[p.float() if i == 2 else p for i, p in enumerate(preds[0])]]),
           dict(out=torch.empty(T_ALL, 5, B_ALL, device="cuda")), dict(workspace=torch.empty(8, dtype=torch.uint8, device="cuda")),
           dict(preds=[[torch.zeros(B_ALL, 50, 21, 28, dtype=torch.float16, device="cuda")]]), dict(preds=preds * 3)]
    for over in bad:
        k = dict(preds=preds, target=target)
        k.update(over)
        with pytest.raises(PosePafError):
            val_loss.focal_l2_terms(**k)


# ---------------------------------------------------------------------------------------------- the fused forward's 20 predictions
def _nets(arch):
    from config.config import GetConfig, TrainingOpt
    from posepaf.fused_model import FusedIMHN
    from posepaf.model_init import deterministic_init, network_class
    net = network_class(arch)(TrainingOpt(), GetConfig("Canonical"), bn=True).eval()
    deterministic_init(net, 7)
    x = torch.from_numpy(np.random.default_rng(3).random((2, 128, 192, 3), dtype=np.float32))
    with torch.no_grad():
        want = [[o.float().cpu() for o in stage] for stage in net.cuda()(x.cuda())]
        fused = FusedIMHN.from_network(net).eval().cuda().half().to(memory_format=torch.channels_last)
    return fused, x.cuda().half(), want


def before_all_after(arch):
    """fused(x), fused(x, all_preds=True), fused(x) again.  The bit-equality of the two plain calls is about all_preds leaving nothing
    behind (tuner keys, cached tensors, weights), so torch's own convolutions are pinned to their deterministic algorithms for these
    three calls: at this geometry the development variant runs some 1 x 1 skip convolutions of 4 x 6 maps through
    torch.nn.functional.conv2d (FConv.conv_only), and MIOpen's default choice there is not reproducible from one call to the next
    -- measured on the MI355X, with or without all_preds in between: five plain fused(x) calls gave five different outputs (first
    differing layer: conv_only (2, 512, 4, 6) -> (2, 640, 4, 6), 2e-3), and with the flag every one of 424 layer outputs was
    bit-equal.  The library's own kernels are deterministic either way; the published variant needs no flag."""
    fused, x, want = _nets(arch)
    pinned = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.no_grad():
            before = fused(x).clone()
            preds = fused(x, all_preds=True)
            after = fused(x).clone()
    finally:
        torch.backends.cudnn.deterministic = pinned
    return fused, x, want, before, preds, after


@pytest.fixture(scope="module")
def posenet_run():
    return before_all_after("posenet")


def check_all_preds(want, before, preds, after):
    assert len(preds) == len(want) == 4 and all(len(p) == 5 for p in preds)
    report = []
    for t in range(4):
        for s in range(5):
            g, w = preds[t][s].float().cpu(), want[t][s]
            assert g.shape == w.shape == (2, 50, 32 >> s, 48 >> s) and torch.isfinite(g).all()
            err, scale = (g - w).abs().max().item(), w.abs().max().item()
            report.append((t, s, round(err / scale, 5)))
            assert err < 0.03 * scale, (t, s, err, scale)
    print("all_preds errors / output max:", report)
    assert torch.equal(before, after), "fused(x) changed after an all_preds call"
    assert torch.equal(before, preds[-1][0])


def test_all_preds_of_the_development_variant(posenet_run):
    _, _, want, before, preds, after = posenet_run
    check_all_preds(want, before, preds, after)


def test_all_preds_of_the_published_variant():
    _, _, want, before, preds, after = before_all_after("final")
    check_all_preds(want, before, preds, after)


def test_loss_of_the_fused_models_own_outputs_against_rendered_targets(posenet_run):
    """val_loss.focal_l2_terms on the tensors all_preds hands over (64-channel views where the heads took their fast path, whatever
    torch returned elsewhere) and a render_scenes target, read as sample 0 of the two-sample buffer and as a plain tensor, against
    the restatement on host copies"""
    from posepaf import synth, synth_device, val_loss
    _, _, _, _, preds, _ = posenet_run
    people = [synth.random_people(3, np.random.default_rng(40), img_h=128, img_w=192), synth.random_people(1, np.random.default_rng(41), img_h=128, img_w=192)]
    joints, n_people = synth_device.pack_joints(people, 4)
    pair = synth_device.render_scenes(torch.from_numpy(joints).cuda(), torch.from_numpy(n_people).cuda(), 32, 48, dtype=torch.float16,
                                      flip=True, reverse_kp=True)
    single = pair[:, 0].contiguous()
    assert {val_loss._layout(p) for stage in preds for p in stage} >= {64}
    got_pair = val_loss.focal_l2_terms(preds, pair)
    got_single = val_loss.focal_l2_terms(preds, single)
    assert got_pair.dtype == torch.float64 and got_pair.shape == (4, 5, 2) and torch.equal(got_pair, got_single)
    host_preds = [[p.float().cpu().numpy().astype(np.float16) for p in stage] for stage in preds]
    host_target = single.cpu().numpy()
    nz = host_target[host_target != 0].astype(np.float64)
    assert nz.min() >= 2.0 ** -17
    want = lr.focal_l2_terms(host_preds, host_target)
    rel = np.abs(got_pair.cpu().numpy() - want) / want
    print(f"fused outputs against a rendered target: largest relative difference of a term {rel.max():.3e}")
    assert close(got_pair.cpu().numpy(), want), rel
    mask = (torch.rand(2, 32, 48, generator=torch.Generator().manual_seed(2)) < 0.8).float().cuda()
    got_masked = val_loss.focal_l2_terms(preds, pair, mask=mask, plain_l2=True)
    assert close(got_masked.cpu().numpy(), lr.focal_l2_terms(host_preds, host_target, mask.cpu().numpy(), plain_l2=True))


# ---------------------------------------------------------------------------------------------- evaluate.py --val_loss
def test_evaluate_val_loss_prints_one_json_line():
    r = subprocess.run([sys.executable, os.path.join(PKG, "evaluate.py"), "--val_loss", "--synthetic", "6", "--batch", "4", "--sizes", "128x192"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["images"] == 6 and out["mask_miss"] == "none" and out["seconds"] > 0
    assert len(out["per_stack"]) == 4 and len(out["per_scale"]) == 5
    pss = np.array(out["per_stack_scale"])
    assert pss.shape == (4, 5)
    assert np.isfinite(pss).all() and np.isfinite(out["per_stack"]).all() and np.isfinite(out["per_scale"]).all() and np.isfinite(out["val_loss"])
    sw = np.array(lr.SCALE_WEIGHT)
    want = float((sw * pss.mean(axis=0)).sum() / sw.sum())
    assert out["val_loss"] > 0 and abs(out["val_loss"] - want) <= 1e-12 * want
