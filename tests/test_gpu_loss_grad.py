"""GPU: the gradient of the focal-L2 loss on the device (pp_focal_l2_grad, val_loss.focal_l2_grad, the autograd node behind
val_loss.focal_l2_terms, finetune.py) against the NumPy float64 restatement tests/lossgrad_reference.py.

Bound, kernel against restatement: none -- the contract fixes the float64 expression and its association and both roundings, so the
stored gradients are BIT-equal (compared as unsigned integers, so also the sign of a zero).
Shapes: the fixtures' own (tests/golden/lossgrad_*.npz): 16 x 16 and 12 x 20 pyramids down to 1 x 1, T = 2, B = 2 (3 for the slot
test).  They hold non-dividing pooling windows (12 x 20 -> 2 x 3), a tile boundary (12 x 20 = 240 pixels = one 128-pixel tile + 112),
a 1 x 1 scale, kink elements and masked cells.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import loss_reference as lr
import lossgrad_reference as lg
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

CASES = ["16x16_binary", "12x20_soft"]
LAYOUTS = ["planes", "px50", "px64", "odd"]      # odd: planes one element off a 16-byte boundary (predictions and gradients)
GUARD = 64
SENTINEL = 123.0
T, K = 2, 5


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want))


@pytest.fixture(scope="module")
def cases():
    """per fixture: predictions as binary16 and as float32 (the binary16 values plus a float32 perturbation that leaves the elements
    at 0 and 1 where they are), the target as float32 and as binary16, each one's pooled scales, and a random tw with zeros"""
    out = {}
    for name in CASES:
        c = lg.load_case(GOLDEN, name)
        rng = np.random.default_rng(len(name))
        p16 = c["preds"]
        p32 = [[np.where((p == 0) | (p == 1), p.astype(np.float32),
                         p.astype(np.float32) + rng.uniform(-1e-4, 1e-4, p.shape).astype(np.float32)) for p in stack] for stack in p16]
        targets = {"f32": c["target"], "f16": c["target"].astype(np.float16)}
        assert (targets["f16"].astype(np.float32) != targets["f32"]).any()        # (the 0.01f plateau is no binary16 value)
        pooled = {d: lr.pool_scales(t, c["sizes"]) for d, t in targets.items()}
        tw = rng.uniform(-2.0, 2.0, (T, K, 2))
        tw[0, 1, 0] = tw[1, 3, 1] = tw[1, 0, 0] = 0.0
        kinks = lg.kink_elements(p16, c["target"], c["sizes"], pooled["f32"])
        assert sum(int(k.sum()) for stack in kinks for k in stack) == c["kinks"] > 0
        out[name] = dict(sizes=c["sizes"], H=c["target"].shape[2], W=c["target"].shape[3], preds={"f16": p16, "f32": p32}, targets=targets,
                         pooled=pooled, mask=c["mask"], tw=tw, wanted={})
    return out


def want_of(case, pd, td, masked, plain, tw=None):
    """the restatement's gradients, computed once per combination"""
    key = (pd, td, masked, plain, None if tw is None else tw.tobytes())
    if key not in case["wanted"]:
        case["wanted"][key] = lg.focal_l2_grad(case["preds"][pd], case["targets"][td], case["tw"] if tw is None else tw,
                                               case["mask"] if masked else None, plain_l2=plain, pooled=case["pooled"][td])
    return case["wanted"][key]


def lay_out(p, layout, fill):
    """host (B, 50, h, w) -> (the device buffer, the address of its first element, the pixel stride the entry takes).  The buffer is
    a flat allocation with GUARD elements behind the tensor; padding channels and guards hold `fill`"""
    t = torch.from_numpy(p)
    B, _, h, w = t.shape
    if layout in ("planes", "odd"):
        lead = 1 if layout == "odd" else 0
        buf = torch.full((lead + t.numel() + GUARD,), fill, dtype=t.dtype)
        buf[lead:lead + t.numel()] = t.reshape(-1)
        buf = buf.cuda()
        return buf, buf.data_ptr() + lead * t.element_size(), 0
    stride = 64 if layout == "px64" else 50
    px = torch.full((B, h, w, stride), fill, dtype=t.dtype)
    px[..., :50] = t.permute(0, 2, 3, 1)
    buf = torch.full((px.numel() + GUARD,), fill, dtype=t.dtype)
    buf[:px.numel()] = px.reshape(-1)
    buf = buf.cuda()
    return buf, buf.data_ptr(), stride


def read_back(buf, shape, layout):
    """-> (host (B, 50, h, w), everything else of the buffer as a flat host array: padding channels, lead, guards)"""
    B, _, h, w = shape
    host = buf.cpu().numpy()
    if layout in ("planes", "odd"):
        lead, n = (1 if layout == "odd" else 0), B * 50 * h * w
        return host[lead:lead + n].reshape(shape).copy(), np.concatenate([host[:lead], host[lead + n:]])
    stride = 64 if layout == "px64" else 50
    n = B * h * w * stride
    px = host[:n].reshape(B, h, w, stride)
    return np.ascontiguousarray(px[..., :50].transpose(0, 3, 1, 2)), np.concatenate([px[..., 50:].reshape(-1), host[n:]])


def launch(case, pd, td, layout, masked, plain, tw, images=(0, 1), expect=0, grad_fill=SENTINEL):
    """pp_focal_l2_grad on the images `images` (a slot may repeat an image) -> host gradients [t][s].  The gradient buffers start
    as `grad_fill`; what is not an element of channels 0..49 must still hold it afterwards."""
    from posepaf import _lib
    L = _lib.load()
    images = list(images)
    B, H, W, sizes = len(images), case["H"], case["W"], case["sizes"]
    held = [[lay_out(np.ascontiguousarray(case["preds"][pd][t][s][images]), layout, float("nan")) for s in range(K)] for t in range(T)]
    grads = [[lay_out(np.full((B, 50) + sizes[s], grad_fill, case["preds"][pd][t][s].dtype), layout, grad_fill) for s in range(K)] for t in range(T)]
    target = torch.from_numpy(np.ascontiguousarray(case["targets"][td][images])).cuda()
    mask = torch.from_numpy(np.ascontiguousarray(case["mask"][images])).cuda() if masked else None
    twd = torch.from_numpy(np.ascontiguousarray(tw)).cuda()
    assert twd.shape == (T, K, B) and twd.dtype == torch.float64
    table = (C.c_void_p * (T * K))(*[held[t][s][1] for t in range(T) for s in range(K)])
    gtable = (C.c_void_p * (T * K))(*[grads[t][s][1] for t in range(T) for s in range(K)])
    hs, ws = (C.c_int * K)(*[h for h, _ in sizes]), (C.c_int * K)(*[w for _, w in sizes])
    rc = L.pp_focal_l2_grad(table, 1 if pd == "f16" else 0, held[0][0][2], C.c_void_p(target.data_ptr()), 1 if td == "f16" else 0,
                            50 * H * W, C.c_void_p(mask.data_ptr()) if masked else None, B, H, W, T, K, hs, ws, 0.1, 3.0, 1 if plain else 0,
                            C.c_void_p(twd.data_ptr()), gtable, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == expect, rc
    torch.cuda.synchronize()
    out = [[None] * K for _ in range(T)]
    for t in range(T):
        for s in range(K):
            out[t][s], rest = read_back(grads[t][s][0], (B, 50) + sizes[s], layout)
            assert (rest == np.asarray(grad_fill, rest.dtype)).all(), ("a padding channel or a guard was written", t, s, layout)
    return out


# ---------------------------------------------------------------------------------------------- kernel against restatement
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("td", ["f16", "f32"])
@pytest.mark.parametrize("pd", ["f16", "f32"])
@pytest.mark.parametrize("name", CASES)
def test_gradients_are_bit_equal_to_the_restatement(cases, name, pd, td, layout):
    """with a mask and without, focal and plain; tw random with zeros"""
    case = cases[name]
    for masked in (True, False):
        for plain in (False, True):
            got = launch(case, pd, td, layout, masked, plain, case["tw"])
            want = want_of(case, pd, td, masked, plain)
            for t in range(T):
                for s in range(K):
                    diff = int((bits(got[t][s]) != bits(want[t][s])).sum())
                    assert same_bits(got[t][s], want[t][s]), (masked, plain, t, s, diff)
            assert (got[0][1][0] == 0).all() and (got[1][3][1] == 0).all() and (got[0][0] != 0).any()   # a zero tw: a zero gradient


def test_the_fixture_gradients_of_the_reference_are_met(cases):
    """the reference's own float32 gradients (autograd on the CPU) against the kernel's, float32 predictions holding the binary16
    values: within the fixtures' 1e-6 of each tensor's largest |gradient| plus the kernel's own rounding to float32 (2^-24 relative)"""
    for name in CASES:
        c = lg.load_case(GOLDEN, name)
        case = dict(cases[name])
        case["preds"] = {"f32": [[p.astype(np.float32) for p in stack] for stack in c["preds"]]}
        got = launch(case, "f32", "f32", "planes", True, False, lg.combine_weights(T, K, 2, (1, 1)))
        for t in range(T):
            for s in range(K):
                want = c["grads"][t][s].astype(np.float64)
                top = np.abs(want).max() or 1.0
                assert np.abs(got[t][s].astype(np.float64) - want).max() <= (1e-6 + 2.0 ** -24) * top, (name, t, s)


# ---------------------------------------------------------------------------------------------- slot independence
@pytest.mark.parametrize("layout", ["planes", "px64"])
def test_an_images_gradients_do_not_depend_on_batch_or_slot(cases, layout):
    """image 0 alone, in each slot of a batch of 3 next to image 1, and in two runs: the same bytes; launch() checks that the padding
    channels of the 64-stride buffers and the bytes behind the last element keep their sentinel"""
    case = cases["12x20_soft"]
    tw0 = case["tw"][:, :, 0:1]
    alone = launch(case, "f16", "f16", layout, True, False, np.ascontiguousarray(tw0), images=[0])
    again = launch(case, "f16", "f16", layout, True, False, np.ascontiguousarray(tw0), images=[0])
    want = want_of(case, "f16", "f16", True, False)
    for t in range(T):
        for s in range(K):
            assert alone[t][s].tobytes() == again[t][s].tobytes()
            assert same_bits(alone[t][s][0], want[t][s][0])
    for slot in range(3):
        images = [1, 1, 1]
        images[slot] = 0
        tw = np.repeat(case["tw"][:, :, 1:2], 3, axis=2)
        tw[:, :, slot] = tw0[:, :, 0]
        got = launch(case, "f16", "f16", layout, True, False, tw, images=images)
        for t in range(T):
            for s in range(K):
                assert got[t][s][slot].tobytes() == alone[t][s][0].tobytes(), (slot, t, s)
                assert all(same_bits(got[t][s][o], want[t][s][1]) for o in range(3) if o != slot)


# ---------------------------------------------------------------------------------------------- refusals
def test_refused_arguments_launch_nothing(cases):
    """every refusal returns its code and leaves the gradient buffers as they were"""
    from posepaf import _lib
    L = _lib.load()
    case = cases["16x16_binary"]
    H, W, sizes, B = case["H"], case["W"], case["sizes"], 2
    held = [[torch.from_numpy(case["preds"]["f16"][t][s]).cuda() for s in range(K)] for t in range(T)]
    grads = [[torch.full_like(held[t][s], 777.0) for s in range(K)] for t in range(T)]
    target = torch.from_numpy(case["targets"]["f16"]).cuda()
    twd = torch.from_numpy(case["tw"]).cuda()
    ptrs = [held[t][s].data_ptr() for t in range(T) for s in range(K)]
    gptrs = [grads[t][s].data_ptr() for t in range(T) for s in range(K)]

    def call(**over):
        k = dict(preds=ptrs, dtype=1, stride=0, target=target.data_ptr(), tdtype=1, timg=50 * H * W, mask=None, batch=B, H=H, W=W, T=T, K=K,
                 hs=[h for h, _ in sizes], ws=[w for _, w in sizes], tw=twd.data_ptr(), grads=gptrs)
        k.update(over)
        table = (C.c_void_p * len(k["preds"]))(*k["preds"]) if k["preds"] is not None else None
        gtable = (C.c_void_p * len(k["grads"]))(*k["grads"]) if k["grads"] is not None else None
        hs, ws = (C.c_int * len(k["hs"]))(*k["hs"]), (C.c_int * len(k["ws"]))(*k["ws"])
        return L.pp_focal_l2_grad(table, k["dtype"], k["stride"], k["target"], k["tdtype"], k["timg"], k["mask"], k["batch"], k["H"], k["W"],
                                  k["T"], k["K"], hs, ws, 0.1, 3.0, 0, k["tw"], gtable, None)

    refused = [(dict(T=0), -2), (dict(T=9, preds=ptrs * 8, grads=gptrs * 8), -6), (dict(K=0), -2),
               (dict(K=6, hs=[16] * 6, ws=[16] * 6, preds=ptrs * 2, grads=gptrs * 2), -6), (dict(batch=0), -2), (dict(batch=65536), -3),
               (dict(hs=[16, 8, 4, 2, 0]), -2), (dict(hs=[17, 8, 4, 2, 1]), -2), (dict(ws=[16, 17, 4, 2, 1]), -2), (dict(preds=None), -2),
               (dict(preds=ptrs[:-1] + [0]), -2), (dict(preds=ptrs[:-1] + [ptrs[-1] + 1]), -2), (dict(target=None), -2),
               (dict(target=target.data_ptr() + 1), -2), (dict(mask=twd.data_ptr() + 2), -2), (dict(dtype=2), -2), (dict(tdtype=3), -2),
               (dict(stride=1), -2), (dict(stride=49), -2), (dict(stride=-1), -2), (dict(timg=50 * H * W - 1), -2),
               # the gradient entry's own
               (dict(tw=None), -2), (dict(tw=twd.data_ptr() + 4), -2), (dict(grads=None), -2), (dict(grads=gptrs[:-1] + [0]), -2),
               (dict(grads=[gptrs[0] + 1] + gptrs[1:]), -2), (dict(grads=gptrs[:3] + [ptrs[3]] + gptrs[4:]), -2)]
    for over, want in refused:
        assert call(**over) == want, over
    torch.cuda.synchronize()
    assert all((g == 777.0).all() for stack in grads for g in stack)
    assert all(torch.equal(held[t][s], torch.from_numpy(case["preds"]["f16"][t][s]).cuda()) for t in range(T) for s in range(K))
    assert call() == 0                                       # and the unmodified call is taken
    torch.cuda.synchronize()
    want = want_of(case, "f16", "f16", False, False)
    assert all(same_bits(grads[t][s].cpu().numpy(), want[t][s]) for t in range(T) for s in range(K))


# ---------------------------------------------------------------------------------------------- the Python surface and autograd
def device_inputs(case, pd, how):
    """leaves that require grad, laid out `how`, and the tensors handed to focal_l2_terms (the leaves, or views of them)"""
    leaves, preds = [], []
    for stack in case["preds"][pd]:
        row = []
        for p in stack:
            t = torch.from_numpy(p).cuda()
            if how == "channels_last":
                leaf = t.contiguous(memory_format=torch.channels_last).requires_grad_(True)
                view = leaf
            elif how == "permuted":                          # stored (B, 50, w, h): no layout the kernel takes
                leaf = t.transpose(2, 3).contiguous().requires_grad_(True)
                view = leaf.transpose(2, 3)
            elif how == "px64":                              # the [:, :50] view of a 64-channel pixel-major tensor
                base = torch.zeros((t.shape[0], t.shape[2], t.shape[3], 64), dtype=t.dtype, device="cuda")
                base[..., :50] = t.permute(0, 2, 3, 1)
                leaf = base.requires_grad_(True)
                view = leaf.permute(0, 3, 1, 2)[:, :50]
            else:
                leaf = t.contiguous().requires_grad_(True)
                view = leaf
            leaves.append(leaf)
            row.append(view)
        preds.append(row)
    return leaves, preds


def grad_as_planes(leaf, how):
    g = leaf.grad
    if how == "permuted":
        g = g.transpose(2, 3)
    elif how == "px64":
        assert (g[..., 50:] == 0).all()                      # nothing flows into the padding channels
        g = g.permute(0, 3, 1, 2)[:, :50]
    return g.contiguous().cpu().numpy()


@pytest.mark.parametrize("how,pd", [("contiguous", "f32"), ("channels_last", "f16"), ("permuted", "f32"), ("px64", "f16")])
@pytest.mark.parametrize("name", CASES)
def test_backward_through_combine_is_bit_equal_to_the_restatement(cases, name, how, pd):
    """combine(focal_l2_terms(preds)).backward(): tw is what torch hands the node, d combine / d terms -- read off terms.grad and
    held against sw[s] / sum sw * nw[t] / sum nw / n_images to 4 float64 roundings -- and .grad is the restatement with that tw"""
    from posepaf import val_loss
    case = cases[name]
    leaves, preds = device_inputs(case, pd, how)
    target, mask = torch.from_numpy(case["targets"]["f16"]).cuda(), torch.from_numpy(case["mask"]).cuda()
    terms = val_loss.focal_l2_terms(preds, target, mask)
    assert terms.grad_fn is not None and terms.requires_grad
    terms.retain_grad()
    val_loss.combine(terms, (1, 1)).backward()
    tw = terms.grad.cpu().numpy()
    formula = lg.combine_weights(T, K, 2, (1, 1))
    assert (np.abs(tw - formula) <= 4 * 2.0 ** -53 * formula).all()
    want = lg.focal_l2_grad(case["preds"][pd], case["targets"]["f16"], tw, case["mask"], pooled=case["pooled"]["f16"])
    for t in range(T):
        for s in range(K):
            leaf = leaves[t * K + s]
            assert leaf.grad is not None and leaf.grad.dtype == leaf.dtype and leaf.grad.shape == leaf.shape
            assert same_bits(grad_as_planes(leaf, how), want[t][s]), (t, s)


def test_raw_gradients_keep_the_predictions_geometry(cases):
    from posepaf import val_loss
    case = cases["12x20_soft"]
    target, twd = torch.from_numpy(case["targets"]["f32"]).cuda(), torch.from_numpy(case["tw"]).cuda()
    want = want_of(case, "f16", "f32", False, True)
    for how in ("contiguous", "channels_last", "px64", "permuted"):
        _, preds = device_inputs(case, "f16", how)
        with torch.no_grad():
            grads = val_loss.focal_l2_grad(preds, target, twd, plain_l2=True)
        for t in range(T):
            for s in range(K):
                g, p = grads[t][s], preds[t][s]
                assert g.shape == p.shape and g.dtype == p.dtype and not g.requires_grad
                if how == "permuted":
                    assert g.is_contiguous()
                elif min(p.shape[2:]) > 1:                  # (strides of extent-1 dimensions say nothing)
                    assert g.stride() == p.stride(), (how, t, s)
                assert same_bits(g.contiguous().cpu().numpy(), want[t][s]), (how, t, s)
    from posepaf._lib import PosePafError
    _, preds = device_inputs(case, "f16", "contiguous")
    for bad in (twd.float(), twd[:, :4], twd.cpu(), None):
        with pytest.raises(PosePafError):
            val_loss.focal_l2_grad(preds, target, bad)


def test_nothing_changes_without_grad(cases):
    """under no_grad, and with no input requiring grad, the result has no grad_fn and holds the bytes of the library call itself;
    the node's forward holds them too.  out= with grad, and a target or mask that requires grad, are refused"""
    from posepaf import _lib, val_loss
    from posepaf._lib import PosePafError
    L = _lib.load()
    case = cases["12x20_soft"]
    H, W, sizes = case["H"], case["W"], case["sizes"]
    target, mask = torch.from_numpy(case["targets"]["f16"]).cuda(), torch.from_numpy(case["mask"]).cuda()
    plain = [[torch.from_numpy(p).cuda() for p in stack] for stack in case["preds"]["f32"]]
    hs, ws = (C.c_int * K)(*[h for h, _ in sizes]), (C.c_int * K)(*[w for _, w in sizes])
    work = torch.empty(L.pp_focal_l2_workspace_bytes(2, T, K, hs, ws), dtype=torch.uint8, device="cuda")
    direct = torch.empty((T, K, 2), dtype=torch.float64, device="cuda")
    table = (C.c_void_p * (T * K))(*[plain[t][s].data_ptr() for t in range(T) for s in range(K)])
    assert L.pp_focal_l2_terms(table, 0, 0, C.c_void_p(target.data_ptr()), 1, 50 * H * W, C.c_void_p(mask.data_ptr()), 2, H, W, T, K, hs, ws,
                               0.1, 3.0, 0, C.c_void_p(work.data_ptr()), C.c_void_p(direct.data_ptr()), None) == 0
    torch.cuda.synchronize()
    a = val_loss.focal_l2_terms(plain, target, mask)
    assert a.grad_fn is None and not a.requires_grad and torch.equal(a, direct)
    out = torch.empty_like(direct)
    assert val_loss.focal_l2_terms(plain, target, mask, out=out) is out and torch.equal(out, direct)
    tracked = [[p.clone().requires_grad_(True) for p in stack] for stack in plain]
    with torch.no_grad():
        b = val_loss.focal_l2_terms(tracked, target, mask, out=out)
    assert b is out and b.grad_fn is None and torch.equal(b, direct)
    c = val_loss.focal_l2_terms(tracked, target, mask)
    assert c.grad_fn is not None and torch.equal(c.detach(), direct)
    only_one = [[p for p in stack] for stack in plain]
    only_one[1][2] = tracked[1][2]                            # one prediction that requires grad is enough
    d = val_loss.focal_l2_terms(only_one, target, mask)
    d.sum().backward()
    assert tracked[1][2].grad is not None and tracked[0][0].grad is None
    with pytest.raises(PosePafError, match="out="):
        val_loss.focal_l2_terms(tracked, target, mask, out=out)
    with pytest.raises(PosePafError, match="target or the mask"):
        val_loss.focal_l2_terms(tracked, target.float().requires_grad_(True), mask)
    with pytest.raises(PosePafError, match="target or the mask"):
        val_loss.focal_l2_terms(tracked, target, mask.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="once_differentiable"):
        e = val_loss.focal_l2_terms(tracked, target, mask)
        w = torch.ones_like(e, requires_grad=True)           # an upstream gradient that itself requires grad
        (g,) = torch.autograd.grad((e * w).sum(), tracked[0][0], create_graph=True)
        g.sum().backward()                                   # no double backward: the node is once differentiable


# ---------------------------------------------------------------------------------------------- graph capture
def test_terms_and_gradients_in_one_graph_replayed_over_two_input_sets(cases):
    from posepaf import val_loss
    case = cases["12x20_soft"]
    sets = []
    for order in ([0, 1], [1, 0]):
        preds = [[torch.from_numpy(np.ascontiguousarray(p[order])).cuda() for p in stack] for stack in case["preds"]["f16"]]
        sets.append(dict(preds=preds, target=torch.from_numpy(np.ascontiguousarray(case["targets"]["f16"][order])).cuda(),
                         mask=torch.from_numpy(np.ascontiguousarray(case["mask"][order])).cuda(),
                         tw=torch.from_numpy(np.ascontiguousarray(case["tw"][:, :, order] * (1.0 + order[0]))).cuda()))
    eager = []
    with torch.no_grad():
        for k in sets:
            eager.append((val_loss.focal_l2_terms(k["preds"], k["target"], k["mask"]).clone(),
                          [[g.clone() for g in stack] for stack in val_loss.focal_l2_grad(k["preds"], k["target"], k["tw"], k["mask"])]))
    static = dict(preds=[[p.clone() for p in stack] for stack in sets[0]["preds"]], target=sets[0]["target"].clone(),
                  mask=sets[0]["mask"].clone(), tw=sets[0]["tw"].clone())

    def both():
        with torch.no_grad():
            return (val_loss.focal_l2_terms(static["preds"], static["target"], static["mask"]),
                    val_loss.focal_l2_grad(static["preds"], static["target"], static["tw"], static["mask"]))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        terms, grads = both()
    for rep in range(4):
        k = sets[rep % 2]
        for t in range(T):
            for s in range(K):
                static["preds"][t][s].copy_(k["preds"][t][s])
        static["target"].copy_(k["target"])
        static["mask"].copy_(k["mask"])
        static["tw"].copy_(k["tw"])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(terms, eager[rep % 2][0]), rep
        assert all(torch.equal(grads[t][s], eager[rep % 2][1][t][s]) for t in range(T) for s in range(K)), rep
    want = lg.focal_l2_grad([[p[[1, 0]] for p in stack] for stack in case["preds"]["f16"]], case["targets"]["f16"][[1, 0]],
                            case["tw"][:, :, [1, 0]] * 2.0, case["mask"][[1, 0]])
    assert all(same_bits(eager[1][1][t][s].cpu().numpy(), want[t][s]) for t in range(T) for s in range(K))


# ---------------------------------------------------------------------------------------------- finetune.py
FT_LR = "4e-3"
FT_BOUND = 2.0 ** -23        # one float32 ulp, relative: 5.6 x the largest difference measured (below)


def run_finetune(loss):
    r = subprocess.run([sys.executable, os.path.join(PKG, "finetune.py"), "--synthetic", "4", "--batch", "2", "--sizes", "64x64", "--stages", "2",
                        "--train", "heads", "--steps", "6", "--lr", FT_LR, "--loss", loss], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_finetune_descends_and_its_first_step_agrees_with_the_torch_formulation():
    """finetune.py --train heads, 2 stages, 2 x 64 x 64, 6 steps, as a child process, with --loss device and --loss torch.
    Step 0 runs on the same weights, so loss_first and grad_norm_first agree within float32 rounding of the torch side: both sides
    evaluate the contract in float64 from the same float32 predictions and round the gradient once to float32.  Measured on the
    MI355X over eight pairs of runs: loss up to 9.5e-9, gradient norm up to 2.1e-8 -- the size of what two runs of one side differ
    by between themselves (torch 6e-9, device 2.4e-8 over six runs each: MIOpen's convolutions are not bit-reproducible from process
    to process).  Bound: 2^-23 = 1.2e-7, one float32 ulp, 5.6 x the largest measured.
    loss_last < loss_first in both runs.  The 4 images make two batches, (image 0, image 2) and (image 1, image 3), which
    alternate, so the comparison is between the first batch before any update and the second after five.  --lr 4e-3 was chosen
    on the torch run (which uses none of the new code): 37.97, 66.28, 24.43, 42.38, 32.55, 35.84; the device run gives the same to
    8 digits.  (2e-3 ends at 40.60: each batch still descends, 71.78 -> 50.01 -> 40.60, but not below the other batch's start.)"""
    dev, tor = run_finetune("device"), run_finetune("torch")
    for out, name in ((dev, "device"), (tor, "torch")):
        assert out["loss"] == name and out["train"] == "heads" and out["images_per_step"] == 2 and len(out["losses"]) == 6
        assert np.isfinite(out["losses"]).all() and out["seconds"] > 0 and out["grad_norm_first"] > 0
        assert out["loss_first"] == out["losses"][0] and out["loss_last"] == out["losses"][-1]
        assert out["loss_last"] < out["loss_first"], (name, out["losses"])
    rel_loss = abs(dev["loss_first"] - tor["loss_first"]) / tor["loss_first"]
    rel_norm = abs(dev["grad_norm_first"] - tor["grad_norm_first"]) / tor["grad_norm_first"]
    print(f"finetune step 0, device against torch: loss {rel_loss:.3e}, gradient norm {rel_norm:.3e}; "
          f"losses device {dev['losses']}, torch {tor['losses']}")
    assert rel_loss <= FT_BOUND and rel_norm <= FT_BOUND
