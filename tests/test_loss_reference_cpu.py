"""CPU: the validation loss' contract.

* tests/loss_reference.py (NumPy float64, loops) against the fixtures tests/golden/loss_*.npz, which hold what the reference's own
  MultiTaskLoss computed on the CPU in float32 (tests/golden/make_golden_loss.py).  Bound: a relative difference of 8 x the largest
  value measured over the fixtures when they were made.  Measured (per (stack, scale) sum / scalar):
      loss_16x16_binary   6.876e-08 / 1.347e-08
      loss_20x28_soft     1.169e-07 / 9.783e-09        (its 1 x 1 scale is fully masked: 0 against 0, compared as such)
      loss_20x28_ones     6.168e-08 / 4.112e-08
  largest 1.169e-07, so the bound is 9.4e-07.  The margin is there because the reference's side is float32 and torch's float32
  reduction order changes with build and thread count; the fixtures exclude the cells where that order, not the formula, decides
  (pooled values within 1e-6 of 0.01 in multi-cell windows, resampled mask values within 1e-6 of 0.5), asserted here again.
* the plateau definition: a window that holds nothing but 0.01f pools to exactly 0.01f and counts as foreground.
* evaluate.py --val_loss refuses the options it cannot be combined with, with a message and a non-zero exit, without a GPU.
* FusedIMHN / FusedIMHNFinal forward(all_preds=True) against net.posenet(x) for every [t][s], in float32 on the CPU.
* the argument checks of pp_focal_l2_terms / pp_focal_l2_workspace_bytes that come before the device is looked for.
"""
import ctypes as C
import glob
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import loss_reference as lr
from conftest import GOLDEN, PKG

BOUND = 8 * 1.169e-07
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "loss_*.npz")))


def load_fixture(path):
    g = np.load(path)
    sizes = [tuple(int(v) for v in hw) for hw in g["sizes"]]
    T = len([k for k in g.files if k.startswith("pred_") and k.endswith("_0")])
    preds = [[g[f"pred_{t}_{s}"] for s in range(len(sizes))] for t in range(T)]
    return g["target"], g["mask"], preds, sizes, g["per_stack_scale"], float(g["scalar"])


def test_three_fixtures_are_present():
    assert [os.path.basename(f) for f in FIXTURES] == ["loss_16x16_binary.npz", "loss_20x28_ones.npz", "loss_20x28_soft.npz"]
    assert all(os.path.getsize(f) <= 600_000 for f in FIXTURES)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_restatement_matches_the_reference_loss(path):
    target, mask, preds, sizes, want_sums, want_scalar = load_fixture(path)
    assert target.shape[0] == 2 and len(preds) == 2 and len(sizes) == 5 and preds[0][0].dtype == np.float16
    assert lr.near_threshold_cells(target, sizes) == 0 and lr.near_half_mask_values(mask, sizes) == 0
    terms = lr.focal_l2_terms(preds, target, mask)
    got_sums = terms.sum(axis=2)
    rel = np.abs(got_sums - want_sums) / np.where(want_sums > 0, want_sums, 1.0)
    got_scalar = lr.combine(terms, (1, 1))
    print(f"{os.path.basename(path)}: largest relative difference of a (stack, scale) sum {rel.max():.3e}, "
          f"of the scalar {abs(got_scalar - want_scalar) / want_scalar:.3e}")
    assert (np.abs(got_sums - want_sums) <= BOUND * want_sums).all(), rel
    assert abs(got_scalar - want_scalar) <= BOUND * want_scalar
    assert want_scalar > 1.0                    # the fixture is not degenerate


def test_a_plateau_of_the_floor_value_pools_to_itself_and_is_foreground():
    """The renderer floors limb responses to exactly 0.01f, so at scales >= 1 whole windows hold nothing but 0.01f.  The contract's G
    is the exact mean rounded once: 0.01f, foreground -- whatever the window size, aligned to the windows or not.  (A float32
    accumulation can land below: torch's CPU pooling of a 3 x 3 window of 0.01f gives 0.0099999988, of 8 x 8 0.0099999951, of
    16 x 16 0.0099999923 -- background -- and of 32 x 32 0.0100001357.)"""
    f = np.float32(0.01)
    g = np.zeros((1, 17, 23), np.float32)
    g[0, 2:14, 3:19] = f                                     # 17 x 23 -> 8 x 11: windows of 3 x 3 and 3 x 4 cells that overlap
    G = lr.pool_target(g, 8, 11)
    rows, cols = lr.windows(17, 8), lr.windows(23, 11)
    inside = np.array([[r0 >= 2 and r1 <= 14 and c0 >= 3 and c1 <= 19 for (c0, c1) in cols] for (r0, r1) in rows])
    assert inside.sum() >= 12 and max((r1 - r0) * (c1 - c0) for r0, r1 in rows for c0, c1 in cols) >= 6
    assert (G[0][inside] == f).all() and (G[0][inside] >= lr.FG).all()
    assert not (np.float64(f) >= 0.01)                       # the float64 comparison the contract rules out
    for k in (2, 3, 4, 7, 16):                               # aligned windows of k x k cells, up to 256 cells
        G = lr.pool_target(np.full((1, 2 * k, 2 * k), f, np.float32), 2, 2)
        assert (G == f).all()
    # the focal factor follows: on such a cell st = p, not 1 - p
    p = np.full((1, 1, 50, 2, 2), 0.25, np.float32)
    t = np.full((1, 50, 4, 4), f, np.float32)
    terms = lr.focal_l2_terms([[p[0]]], t)
    cw = lr.channel_weights()
    want = ((0.25 - float(f)) ** 2 * abs(1.0 - 0.25)) * cw.sum() * 4
    assert abs(terms[0, 0, 0] - want) <= 1e-12 * want


# ---------------------------------------------------------------------------------------------- evaluate.py --val_loss, refusals
def _evaluate_module():
    spec = importlib.util.spec_from_file_location("pp_evaluate_val_loss", os.path.join(PKG, "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    return ev


CONFLICTS = [(["--scales", "0.5", "1.0"], "--scales"), (["--rotation_search", "0", "15"], "--rotation_search"),
             (["--test_cfg", "thre2=0.05"], "--test_cfg"), (["--render_dir", "out"], "--render_dir"),
             (["--render_limbs_dir", "out"], "--render_limbs_dir"), (["--ap", "device"], "--ap"), (["--ap", "host"], "--ap"),
             (["--scenes", "bank"], "--scenes bank")]


@pytest.mark.parametrize("extra,name", CONFLICTS, ids=[" ".join(e) for e, _ in CONFLICTS])
def test_val_loss_refuses_conflicting_options_before_the_gpu(extra, name, monkeypatch):
    ev = _evaluate_module()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the GPU was looked for before the refusal"))
    with pytest.raises(SystemExit) as e:
        ev.main(["--val_loss", "--synthetic", "4"] + extra)
    assert isinstance(e.value.code, str) and "--val_loss" in e.value.code and name in e.value.code


def test_val_loss_refusal_is_a_message_and_a_non_zero_exit():
    r = subprocess.run([sys.executable, os.path.join(PKG, "evaluate.py"), "--val_loss", "--synthetic", "4", "--ap", "device", "--scales", "1.0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and r.stdout == ""
    assert "--val_loss" in r.stderr and "--ap" in r.stderr and "--scales" in r.stderr


def test_val_loss_flag_leaves_the_other_modes_alone():
    ev = _evaluate_module()
    a = ev.parse(["--synthetic", "4"])
    assert a.val_loss is False and a.scenes == "bank"
    assert ev.parse(["--synthetic", "4", "--scenes", "device"]).scenes == "device"
    assert ev.val_loss_conflicts(ev.parse(["--val_loss", "--synthetic", "4", "--batch", "2", "--sizes", "128x192", "--arch", "final"])) == []
    assert ev.val_loss_conflicts(ev.parse(["--val_loss", "--synthetic", "4", "--scenes", "device"])) == []


# ---------------------------------------------------------------------------------------------- all_preds on the CPU, float32
def _small(arch):
    from posepaf.model_init import deterministic_init
    if arch == "final":
        from models.posenet_final import PoseNet
        body = lambda: PoseNet(3, 32, 50, bn=True, increase=16, init_weights=False)
    else:   # (the backbone of models/posenet.py is 256 wide)
        from models.posenet import PoseNet
        body = lambda: PoseNet(2, 256, 50, bn=True, increase=32, init_weights=False)

    class Wrap(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.posenet = body()

        def forward(self, x):
            return self.posenet(x)

    net = Wrap().eval()
    deterministic_init(net, seed=11)
    return net


@pytest.mark.parametrize("arch", ["posenet", "final"])
def test_all_preds_is_every_prediction_of_the_module_in_float32(arch):
    """pred[t][s] of forward(all_preds=True) == net.posenet(x)[t][s] for every stage and all five scales, the last stage's coarse
    heads included, while the folded merges drive the chain.  Bound: the one tests/test_model_final_cpu.py uses for stage_preds,
    1e-5 of the output's scale.  fused(x) and stage_preds are what they were."""
    from posepaf import fused_model as fm
    net = _small(arch)
    fused = fm.FusedIMHN.from_network(net).eval()
    assert isinstance(fused, fm.FusedIMHNFinal) == (arch == "final") and fused.folded_merge
    x = torch.rand(2, 64, 128, 3, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        want = net.posenet(x)
        before = fused(x)
        got = fused(x, all_preds=True)
        stages = fused(x, stage_preds=True)
        after = fused(x)
    S = len(want)
    assert len(got) == S and all(len(g) == 5 for g in got)
    worst = 0.0
    for t in range(S):
        for s in range(5):
            assert got[t][s].shape == want[t][s].shape == (2, 50, 16 >> s, 32 >> s)
            scale = want[t][s].abs().max().item()
            assert scale > 1e-3
            err = (got[t][s] - want[t][s]).abs().max().item() / scale
            worst = max(worst, err)
            assert err <= 1e-5, (t, s, err)
    print(f"{arch}: largest error of the {S * 5} predictions, relative to each one's scale: {worst:.3e}")
    assert torch.equal(before, after) and torch.equal(before, got[-1][0])
    assert len(stages) == S and all(torch.equal(stages[t], got[t][0]) for t in range(S))


# ---------------------------------------------------------------------------------------------- the C entry's argument checks
def _call(L, **over):
    """pp_focal_l2_terms with plausible (never dereferenced) addresses; `over` replaces arguments"""
    k = dict(preds=[0x1000, 0x2000], dtype=1, stride=0, target=0x3000, tdtype=1, timg=50 * 8 * 8, mask=None, batch=1, H=8, W=8, T=1, K=2,
             hs=[8, 4], ws=[8, 4], ws_ptr=0x4000, terms=0x5000)
    k.update(over)
    table = (C.c_void_p * len(k["preds"]))(*k["preds"]) if k["preds"] is not None else None
    hs = (C.c_int * len(k["hs"]))(*k["hs"]) if k["hs"] is not None else None
    ws = (C.c_int * len(k["ws"]))(*k["ws"]) if k["ws"] is not None else None
    return L.pp_focal_l2_terms(table, k["dtype"], k["stride"], k["target"], k["tdtype"], k["timg"], k["mask"], k["batch"], k["H"], k["W"],
                               k["T"], k["K"], hs, ws, 0.1, 3.0, 0, k["ws_ptr"], k["terms"], None)


REFUSED = [(dict(T=0), -2), (dict(T=9, preds=[0x1000] * 18), -6), (dict(K=0), -2), (dict(K=6, hs=[8] * 6, ws=[8] * 6, preds=[0x1000] * 6), -6),
           (dict(batch=0), -2), (dict(batch=65536), -3), (dict(hs=[8, 0]), -2), (dict(hs=[9, 4]), -2), (dict(ws=[8, 9]), -2),
           (dict(H=0), -2), (dict(preds=None), -2), (dict(preds=[0x1000, 0]), -2), (dict(preds=[0x1000, 0x2001]), -2),
           (dict(target=None), -2), (dict(target=0x3001), -2), (dict(mask=0x6002), -2), (dict(ws_ptr=None), -2), (dict(ws_ptr=0x4004), -2),
           (dict(terms=None), -2), (dict(terms=0x5004), -2), (dict(dtype=2), -2), (dict(tdtype=-1), -2), (dict(stride=1), -2),
           (dict(stride=49), -2), (dict(stride=-64), -2), (dict(timg=50 * 8 * 8 - 1), -2), (dict(hs=None), -2)]


def test_the_entry_refuses_bad_arguments_before_it_looks_for_a_device():
    from posepaf import _lib
    L = _lib.load()
    for over, want in REFUSED:
        assert _call(L, **over) == want, over
    if not torch.cuda.is_available():
        assert _call(L) == -1                                # PP_ERR_NO_DEVICE: the arguments were fine
    hs, ws = (C.c_int * 5)(128, 64, 32, 16, 8), (C.c_int * 5)(128, 64, 32, 16, 8)
    # 128 + 32 + 8 + 2 + 1 tiles of 128 pixels per image, one float64 per stack
    assert L.pp_focal_l2_workspace_bytes(3, 4, 5, hs, ws) == 3 * 171 * 4 * 8
    assert L.pp_focal_l2_workspace_bytes(0, 4, 5, hs, ws) == -2 and L.pp_focal_l2_workspace_bytes(3, 9, 5, hs, ws) == -6
    assert L.pp_focal_l2_workspace_bytes(65536, 4, 5, hs, ws) == -3 and L.pp_focal_l2_workspace_bytes(3, 4, 6, hs, ws) == -6


def test_the_python_surface_refuses_host_tensors_before_the_library():
    from posepaf import val_loss
    from posepaf._lib import PosePafError
    preds = [[torch.zeros(1, 50, 8, 8, dtype=torch.float16), torch.zeros(1, 50, 4, 4, dtype=torch.float16)]]
    target = torch.zeros(1, 50, 8, 8)
    with pytest.raises(PosePafError, match="HIP device"):
        val_loss.focal_l2_terms(preds, target)
    with pytest.raises(PosePafError):
        val_loss.focal_l2_terms(preds, torch.zeros(1, 49, 8, 8))
    with pytest.raises(PosePafError):
        val_loss.focal_l2_terms([[preds[0][0], torch.zeros(1, 50, 9, 4, dtype=torch.float16)]], target)
    with pytest.raises(PosePafError):
        val_loss.combine(torch.zeros(4, 5, 2))               # float32 terms
    terms = torch.arange(40, dtype=torch.float64).reshape(4, 5, 2)
    assert abs(val_loss.combine(terms).item() - lr.combine(terms.numpy())) <= 1e-12 * lr.combine(terms.numpy())
