"""CPU: the contract of the focal-L2 loss gradient.

* tests/lossgrad_reference.py (NumPy float64, unrounded) against the fixtures tests/golden/lossgrad_*.npz, which hold pred[t][s].grad of
  the reference's own MultiTaskLoss under autograd on the CPU in float32 (tests/golden/make_golden_lossgrad.py).  Bound: 1e-6 of each
  tensor's largest |gradient| -- about 6 x the reference's float32 rounding (measured 1.263e-07 and 3.041e-07 when the fixtures were
  written) and far below one wrong sign at a kink, which costs the whole (d d) term of that element.
* the restatement against central finite differences of loss_reference.focal_l2_terms in float64, bound derived below from the step.
* one-sided differences at the kink elements bracket the stored 0.
* the argument checks of pp_focal_l2_grad that come before the device is looked for, and of val_loss.focal_l2_grad before the library.
* finetune.py ends with a message, before the GPU is looked for, on the combinations it does not support.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import loss_reference as lr
import lossgrad_reference as lg
from conftest import GOLDEN

BOUND = 1e-6
CASES = ["16x16_binary", "12x20_soft"]
STEP = 2.0 ** -12            # exact in float64 on every binary16 value of the fixtures (|p| <= 1.1: multiples of 2^-24 at the most)
EPS = 2.0 ** -53


def load_case(name):
    return lg.load_case(GOLDEN, name)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in CASES:
        c = load_case(name)
        c["pooled"] = lr.pool_scales(c["target"], c["sizes"])
        c["tw"] = lg.combine_weights(2, 5, c["target"].shape[0], (1, 1))
        out[name] = c
    return out


def test_two_fixtures_are_present():
    for name in CASES:
        path = os.path.join(GOLDEN, f"lossgrad_{name}.npz")
        assert os.path.getsize(path) <= 600_000
    c = load_case("12x20_soft")
    assert c["sizes"] == [(12, 20), (6, 10), (3, 5), (2, 3), (1, 1)] and c["target"].shape == (2, 50, 12, 20)
    assert all(c["grads"][t][s].dtype == np.float32 and c["grads"][t][s].shape == c["preds"][t][s].shape for t in range(2) for s in range(5))


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference_gradients(cases, name):
    c = cases[name]
    assert lr.near_threshold_cells(c["target"], c["sizes"]) == 0 and lr.near_half_mask_values(c["mask"], c["sizes"]) == 0
    kinks = lg.kink_elements(c["preds"], c["target"], c["sizes"], c["pooled"])
    assert sum(int(k.sum()) for stack in kinks for k in stack) == c["kinks"] > 0
    got = lg.focal_l2_grad(c["preds"], c["target"], c["tw"], c["mask"], pooled=c["pooled"], rounded=False)
    worst = 0.0
    for t in range(2):
        for s in range(5):
            want = c["grads"][t][s].astype(np.float64)
            rel = float(np.abs(got[t][s] - want).max() / (np.abs(want).max() or 1.0))   # (a fully masked scale: 0 against 0)
            worst = max(worst, rel)
            assert rel < BOUND, (t, s, rel)
            assert (want[kinks[t][s]] == 0).all() and (got[t][s][kinks[t][s]] == 0).all()   # torch's abs backward: 0 at the kink
    print(f"lossgrad_{name}: largest difference / largest |gradient| of a tensor {worst:.3e}")
    # the rounded restatement is the unrounded one rounded to the predictions' dtype
    rounded = lg.focal_l2_grad(c["preds"], c["target"], c["tw"], c["mask"], pooled=c["pooled"])
    assert all(rounded[t][s].dtype == np.float16 and
               np.array_equal(rounded[t][s], got[t][s].astype(np.float32).astype(np.float16)) for t in range(2) for s in range(5))


def one_term(c, t, s, b, p, plain):
    """loss_reference.focal_l2_terms of image b's scale-s prediction p (C, h, w) alone: the one term the element belongs to"""
    return float(lr.focal_l2_terms([[p[None]]], c["target"][b:b + 1], c["mask"][b:b + 1], plain_l2=plain, pooled=[[c["pooled"][s][b]]])[0, 0, 0])


@pytest.mark.parametrize("plain", [False, True], ids=["focal", "plain"])
@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_central_differences(cases, name, plain):
    """d term / d p by (term(p + h) - term(p - h)) / 2h, h = 2^-12, on 240 seeded elements per case, none within h of its kink.
    An element's term is K (p - G)^2 |a +- p| with K = cw M: a cubic in p between kinks, so the central difference is off by exactly
    h^2 |phi'''| / 6 = h^2 K (plain: a parabola, 0).  The two evaluations are float64 sums of N non-negative terms, each within
    (N + 8) 2^-53 of its value (N additions and the few roundings of a term), so their difference adds at most
    2 (N + 8) 2^-53 term / 2h; the restatement's own four roundings stay below 8 2^-53 |g|.  The bound is the sum of the three."""
    c = cases[name]
    rng = np.random.default_rng(7)
    want = lg.focal_l2_grad(c["preds"], c["target"], np.ones((2, 5, 2)), c["mask"], plain_l2=plain, pooled=c["pooled"], rounded=False)
    cw = lr.channel_weights()
    checked, worst = 0, 0.0
    for t in range(2):
        for s, (h, w) in enumerate(c["sizes"]):
            for b in range(2):
                p = c["preds"][t][s][b].astype(np.float64)
                G = c["pooled"][s][b]
                M = lr.resample_mask(c["mask"][b], h, w)
                kink_at = np.where(G >= lr.FG, 1.0, 0.0)
                free = np.argwhere(np.abs(p - kink_at) > STEP)
                pick = free[rng.choice(len(free), size=min(12, len(free)), replace=False)]
                N = p.size
                for ch, y, x in pick:
                    hi, lo = p.copy(), p.copy()
                    hi[ch, y, x] += STEP
                    lo[ch, y, x] -= STEP
                    assert hi[ch, y, x] - lo[ch, y, x] == 2 * STEP
                    t_hi, t_lo = one_term(c, t, s, b, hi, plain), one_term(c, t, s, b, lo, plain)
                    fd = (t_hi - t_lo) / (2 * STEP)
                    g = want[t][s][b, ch, y, x]
                    bound = (0.0 if plain else STEP * STEP * cw[ch] * M[y, x]) + (N + 8) * EPS * max(t_hi, t_lo) / STEP + 8 * EPS * abs(g)
                    assert abs(fd - g) <= bound, (t, s, b, ch, y, x, fd, g, bound)
                    worst = max(worst, abs(fd - g) / bound if bound > 0 else 0.0)
                    checked += 1
    print(f"{name} {'plain' if plain else 'focal'}: {checked} elements, largest |difference| / bound {worst:.3f}")
    assert checked >= 200


@pytest.mark.parametrize("name", CASES)
def test_one_sided_differences_bracket_the_zero_at_a_kink(cases, name):
    """at a kink the element's term is 0 and non-negative on both sides: left difference <= 0 = stored gradient <= right difference,
    strictly where the mask keeps the pixel and p != G"""
    c = cases[name]
    kinks = lg.kink_elements(c["preds"], c["target"], c["sizes"], c["pooled"])
    got = lg.focal_l2_grad(c["preds"], c["target"], c["tw"], c["mask"], pooled=c["pooled"], rounded=False)
    seen = strict = 0
    for t in range(2):
        for s, (h, w) in enumerate(c["sizes"]):
            for b, ch, y, x in np.argwhere(kinks[t][s]):
                p = c["preds"][t][s][b].astype(np.float64)
                M = lr.resample_mask(c["mask"][b], h, w)
                hi, lo = p.copy(), p.copy()
                hi[ch, y, x] += STEP
                lo[ch, y, x] -= STEP
                here = one_term(c, t, s, b, p, False)
                right = (one_term(c, t, s, b, hi, False) - here) / STEP
                left = (here - one_term(c, t, s, b, lo, False)) / STEP
                noise = (p.size + 8) * EPS * here / STEP * 2
                assert got[t][s][b, ch, y, x] == 0.0
                assert left <= noise and right >= -noise, (t, s, b, ch, y, x, left, right)
                seen += 1
                if M[y, x] > 0 and abs(p[ch, y, x] - float(c["pooled"][s][b][ch, y, x])) > 0.05:
                    # K d^2 (1 -+ h ...) with K d^2 >= 0.1 * 0.5 * 0.05^2: far above the noise
                    assert left < -noise and right > noise, (t, s, b, ch, y, x, left, right)
                    strict += 1
    assert seen == c["kinks"] and strict > 0


def test_zero_weights_give_zero_gradients_and_plain_has_no_focal_factor(cases):
    c = cases["12x20_soft"]
    tw = c["tw"].copy()
    tw[:, :, 1] = 0.0
    got = lg.focal_l2_grad(c["preds"], c["target"], tw, c["mask"], pooled=c["pooled"])
    assert all((got[t][s][1] == 0).all() and (got[t][s][0] != 0).any() for t in range(2) for s in range(4))
    plain = lg.focal_l2_grad(c["preds"], c["target"], np.ones((2, 5, 2)), None, plain_l2=True, pooled=c["pooled"], rounded=False)
    cw = lr.channel_weights()
    d = c["preds"][1][2].astype(np.float64) - np.stack(c["pooled"][2]).astype(np.float64)
    assert np.array_equal(plain[1][2], 1.0 * (cw[None, :, None, None] * (1.0 * (2.0 * d))))


# ---------------------------------------------------------------------------------------------- the C entry's argument checks
def _call(L, **over):
    """pp_focal_l2_grad with plausible (never dereferenced) addresses; `over` replaces arguments"""
    k = dict(preds=[0x1000, 0x2000], dtype=1, stride=0, target=0x3000, tdtype=1, timg=50 * 8 * 8, mask=None, batch=1, H=8, W=8, T=1, K=2,
             hs=[8, 4], ws=[8, 4], tw=0x4000, grads=[0x7000, 0x8000])
    k.update(over)
    table = (C.c_void_p * len(k["preds"]))(*k["preds"]) if k["preds"] is not None else None
    gtable = (C.c_void_p * len(k["grads"]))(*k["grads"]) if k["grads"] is not None else None
    hs = (C.c_int * len(k["hs"]))(*k["hs"]) if k["hs"] is not None else None
    ws = (C.c_int * len(k["ws"]))(*k["ws"]) if k["ws"] is not None else None
    return L.pp_focal_l2_grad(table, k["dtype"], k["stride"], k["target"], k["tdtype"], k["timg"], k["mask"], k["batch"], k["H"], k["W"],
                              k["T"], k["K"], hs, ws, 0.1, 3.0, 0, k["tw"], gtable, None)


# what pp_focal_l2_terms refuses (tests/test_loss_reference_cpu.py), with the same codes, and the gradient entry's own refusals
REFUSED = [(dict(T=0), -2), (dict(T=9, preds=[0x1000] * 18, grads=[0x7000] * 18), -6), (dict(K=0), -2),
           (dict(K=6, hs=[8] * 6, ws=[8] * 6, preds=[0x1000] * 6, grads=[0x7000] * 6), -6),
           (dict(batch=0), -2), (dict(batch=65536), -3), (dict(hs=[8, 0]), -2), (dict(hs=[9, 4]), -2), (dict(ws=[8, 9]), -2),
           (dict(H=0), -2), (dict(preds=None), -2), (dict(preds=[0x1000, 0]), -2), (dict(preds=[0x1000, 0x2001]), -2),
           (dict(target=None), -2), (dict(target=0x3001), -2), (dict(mask=0x6002), -2), (dict(dtype=2), -2), (dict(tdtype=-1), -2),
           (dict(stride=1), -2), (dict(stride=49), -2), (dict(stride=-64), -2), (dict(timg=50 * 8 * 8 - 1), -2), (dict(hs=None), -2),
           (dict(tw=None), -2), (dict(tw=0x4004), -2), (dict(grads=None), -2), (dict(grads=[0x7000, 0]), -2), (dict(grads=[0x7001, 0x8000]), -2),
           (dict(grads=[0x7000, 0x2000]), -2), (dict(dtype=0, grads=[0x7002, 0x8000]), -2)]


def test_the_gradient_entry_refuses_bad_arguments_before_it_looks_for_a_device():
    from posepaf import _lib
    L = _lib.load()
    for over, want in REFUSED:
        assert _call(L, **over) == want, over
    if not torch.cuda.is_available():
        assert _call(L) == -1                                # PP_ERR_NO_DEVICE: the arguments were fine


def test_the_python_surface_refuses_before_the_library():
    from posepaf import val_loss
    from posepaf._lib import PosePafError
    preds = [[torch.zeros(1, 50, 8, 8, dtype=torch.float16), torch.zeros(1, 50, 4, 4, dtype=torch.float16)]]
    target = torch.zeros(1, 50, 8, 8)
    tw = torch.ones(1, 2, 1, dtype=torch.float64)
    with pytest.raises(PosePafError, match="HIP device"):
        val_loss.focal_l2_grad(preds, target, tw)
    with pytest.raises(PosePafError):
        val_loss.focal_l2_grad(preds, torch.zeros(1, 49, 8, 8), tw)
    # a host prediction that requires grad is refused like any host tensor, before the autograd node is built
    with pytest.raises(PosePafError, match="HIP device"):
        val_loss.focal_l2_terms([[p.float().requires_grad_(True) for p in preds[0]]], target)


# ---------------------------------------------------------------------------------------------- finetune.py's refusals
FINETUNE_REFUSED = [(["--steps", "2"], "--synthetic"), (["--synthetic", "4", "--sizes", "100x64"], "multiples of 64"),
                    (["--synthetic", "4", "--sizes", "64x64,128x128"], "one size"), (["--synthetic", "4", "--stages", "9"], "--stages"),
                    (["--synthetic", "4", "--stages", "0"], "--stages"), (["--synthetic", "4", "--batch", "0"], "--batch"),
                    (["--synthetic", "4", "--lr", "0"], "--lr"), (["--synthetic", "4", "-p", "no/such/weights.pth"], "no such file"),
                    (["--synthetic", "4", "--save", "no/such/dir/out.pth"], "--save")]


@pytest.mark.parametrize("argv,word", FINETUNE_REFUSED, ids=[" ".join(a) for a, _ in FINETUNE_REFUSED])
def test_finetune_refuses_before_the_gpu(argv, word, monkeypatch):
    import importlib.util
    from conftest import PKG
    spec = importlib.util.spec_from_file_location("finetune_under_test", os.path.join(PKG, "finetune.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the GPU was looked for before the refusal"))
    with pytest.raises(SystemExit) as e:
        ft.main(argv)
    assert isinstance(e.value.code, str) and e.value.code.startswith("finetune.py:") and word in e.value.code
