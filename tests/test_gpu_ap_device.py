"""GPU: the device half of the keypoint evaluation (csrc/posepaf_eval.hip, posepaf/ap_device.py) against its host specification:
pp_coco_rows_f32 against coco.humans_from_record + coco.coco_results, pp_oks_match against stage A of
oks_eval.evaluate_keypoints_ranges, the OKS matrix against compute_oks, the twelve summary values, and evaluate.py --ap.
Records are fabricated on the host and uploaded: no forward pass, no other kernel involved (except in the script tests)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ap_cases
from conftest import PKG

pytestmark = pytest.mark.gpu

TWELVE = ("AP", "AP50", "AP75", "APm", "APl", "AR", "AR50", "AR75", "ARm", "ARl", "n_gt", "n_dt")
OKS_BOUND = 1e-13     # exp within an ulp of a value <= 1, <= 17 terms summed in another order, one division: < 4e-15; factor 25


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _upload(torch, recs):
    return torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1).copy()).cuda()


def _same(a, b):
    return a == b or (a != a and b != b)


# ------------------------------------------------------------------------------------------------ rows
def _row_pool():
    """one record per rule of pp_coco_rows_f32"""
    rng = np.random.default_rng(5)
    full, none = np.ones(17, bool), np.zeros(17, bool)
    one = none.copy()
    one[9] = True

    def det(present, score):
        return (rng.integers(0, 700, (17, 2)), present, score)

    all18 = ap_cases.make_record([det(full, 0.625)])
    all18["humans"]["peak_id"][0][1], all18["humans"]["x"][0][1], all18["humans"]["y"][0][1] = 17, 333, 444     # the neck: no COCO keypoint
    crowd = [det(none if h % 9 == 4 else rng.uniform(size=17) < 0.6, rng.uniform()) for h in range(128)]
    halves = np.stack([np.array([10.5, 11.5, 2.5, 3.5, -0.5, -1.5, 7.49, 7.51, 0.5, 1.5, 100.5, 101.5, 6.0, 8.25, 9.75, 254.5, 255.5]),
                       np.array([0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5, 8.5, 9.5, 10.5, 11.5, 12.5, 13.5, 14.5, 15.5, 16.5])], axis=1)
    pool = [ap_cases.make_record([]),                                                       # nobody
            ap_cases.make_record([det(full, 0.9), det(none, 0.8), det(one, 0.7), det(none, 0.6), det(full, 0.5)]),   # partless humans are
            ap_cases.make_record([det(one, 0.25)]),                                         # skipped, later ones move up; one part
            all18,
            ap_cases.make_record(crowd),                                                    # 128 humans, some of them partless
            ap_cases.make_record(crowd, n_humans=300),                                      # n_humans beyond the capacity
            ap_cases.make_record([det(full, 0.5)], n_humans=-3),                            # ... and below zero
            ap_cases.make_record([(halves, full, 0.375), (halves[::-1], one, 0.5)], float_coords=True)]   # .5 coordinates, both parities
    return np.stack(pool)


_ROWS = {}


def _rows_case(batch):
    if batch not in _ROWS:
        pool = _row_pool()
        recs = pool[np.arange(batch) % len(pool)] if batch > 1 else pool
        _ROWS[batch] = (recs, [ap_cases.host_rows(r) for r in recs])
    return _ROWS[batch]


@pytest.mark.parametrize("batch", [1, 3, 130])
def test_rows_equal_humans_from_record_and_coco_results(torch_cuda, batch):
    """every word of the output: the rows exactly, zeros behind them, the counts.  batch 1: every record of the pool alone."""
    torch = torch_cuda
    from posepaf import _lib
    recs, want = _rows_case(batch)
    L = _lib.load()
    groups = [recs[i:i + 1] for i in range(len(recs))] if batch == 1 else [recs]
    at = 0
    for grp in groups:
        n = len(grp)
        dev = _upload(torch, grp)
        rows = torch.full((n + 1, 128, 52), float("nan"), dtype=torch.float32, device="cuda")      # one slot more: must stay untouched
        counts = torch.full((n + 1,), -77, dtype=torch.int32, device="cuda")
        _lib.check(L.pp_coco_rows_f32(C.c_void_p(dev.data_ptr()), n, C.c_void_p(rows.data_ptr()), C.c_void_p(counts.data_ptr()), None))
        torch.cuda.synchronize()
        rows, counts = rows.cpu().numpy().astype(np.float64), counts.cpu().numpy()
        assert counts[n] == -77 and np.isnan(rows[n]).all()
        for j in range(n):
            w = want[at + j]
            assert counts[j] == len(w)
            assert np.array_equal(rows[j, :len(w)], w), (batch, at + j)
            assert not rows[j, len(w):].any()
        at += n
    if batch == 1:   # the pool shows what it is for
        assert [len(w) for w in want[:4]] == [0, 3, 1, 1] and len(want[5]) == len(want[4]) < 128 and len(want[6]) == 0
        assert want[7][0, :6].tolist() == [10.0, 0.0, 1.0, 12.0, 2.0, 1.0]       # 10.5 -> 10, 0.5 -> 0; 11.5 -> 12, 1.5 -> 2


def test_rows_through_the_class(torch_cuda):
    from posepaf.ap_device import DeviceKeypointEval
    recs, want = _rows_case(3)
    ev = DeviceKeypointEval("cuda", [0, 1, 2], {})
    rows, counts = ev.rows(_upload(torch_cuda, recs))
    assert counts.cpu().tolist() == [len(w) for w in want]
    assert np.array_equal(rows[1, :3].cpu().numpy().astype(np.float64), want[1])


# ------------------------------------------------------------------------------------------------ matching
_DEVICE = {}


def _device_outputs(torch, which):
    """the device outputs of the seeded / hand cases (one call each, shared by the tests below)"""
    if which not in _DEVICE:
        from posepaf.ap_device import DeviceKeypointEval
        recs, gts, dts = ap_cases.seeded_cases() if which == "seeded" else ap_cases.hand_cases()
        ev = DeviceKeypointEval("cuda", list(range(len(recs))), gts)
        out = ev.match(_upload(torch, recs), want_oks=True)
        torch.cuda.synchronize()
        _DEVICE[which] = (ev, out, {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()})
    return _DEVICE[which]


def _check_against_stage_a(host, want, label):
    worst = 0.0
    for i, w in enumerate(want):
        n, g = len(w["order"]), w["oks"].shape[1]
        assert host["n_det"][i] == n, (label, i)
        assert host["order"][i].tolist() == w["order"].tolist() + [-1] * (20 - n), (label, i)
        assert np.array_equal(host["scores"][i, :n].astype(np.float64), w["scores"]) and not host["scores"][i, n:].any(), (label, i)
        assert host["n_gt"][i].tolist() == w["n_gt"].tolist(), (label, i)
        assert np.array_equal(host["match"][i, :, :, :n], w["match"]), (label, i, host["match"][i, :, :, :n], w["match"])
        assert not host["match"][i, :, :, n:].any(), (label, i)
        oks = host["oks"][i]
        if n and g:
            worst = max(worst, float(np.abs(oks[:n, :g] - w["oks"]).max()))
        assert not oks[n:].any() and not oks[:, g:].any(), (label, i)
    return worst


@pytest.mark.parametrize("which", ["seeded", "hand"])
def test_match_equals_stage_a_of_the_host_function(torch_cuda, which):
    """detection order, scores, all 3 x 10 x 20 flags and the counted ground truths exactly; the OKS matrix within 1e-13"""
    _, _, host = _device_outputs(torch_cuda, which)
    worst = _check_against_stage_a(host, ap_cases.stage_a(which), which)
    print(f"\n[{which}] max |OKS device - compute_oks| = {worst:.3e}")
    assert worst <= OKS_BOUND


def test_match_with_image_slots(torch_cuda):
    """records in another order than the ground truth's slots: image_slots names each record's image"""
    torch = torch_cuda
    ev, _, host = _device_outputs(torch, "hand")
    recs, _, _ = ap_cases.hand_cases()
    perm = np.array([3, 0, 6, 1, 1, 5, 2, 4])
    out = ev.match(_upload(torch, recs[perm]), image_slots=perm)
    torch.cuda.synchronize()
    for k in ("order", "scores", "match", "n_det", "n_gt"):
        assert np.array_equal(out[k].cpu().numpy(), host[k][perm]), k


def test_too_many_ground_truths_is_refused_before_any_launch(torch_cuda):
    torch = torch_cuda
    from posepaf import _lib, oks_eval as oe
    from posepaf.ap_device import DeviceKeypointEval
    g = ap_cases.gt_ann(ap_cases.grid_pose(10, 10), np.full(17, 2), 5000.0, (10, 10, 96, 48))
    with pytest.raises(_lib.PosePafError, match="'img-b'.*129"):
        DeviceKeypointEval("cuda", ["img-a", "img-b"], {"img-a": [g] * 128, "img-b": [g] * 129})
    # the C entry itself: PP_ERR_TOO_LARGE, and not one output word written
    L = _lib.load()
    recs, _, _ = ap_cases.hand_cases()
    ev = DeviceKeypointEval("cuda", [0], {})
    rows, counts = ev.rows(_upload(torch, recs[:1]))
    offs = np.array([0, 129], np.int32)
    offs_dev = torch.from_numpy(offs).cuda()
    gt = torch.zeros(129 * _lib.GT_ANN_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    outs = [torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda") for n in (80, 80, 600, 4, 12)]
    thr, rng = np.ascontiguousarray(oe.OKS_THRESHOLDS), np.ascontiguousarray(oe.AREA_RANGES)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    rc = L.pp_oks_match(C.c_void_p(rows.data_ptr()), C.c_void_p(counts.data_ptr()), 1, C.c_void_p(gt.data_ptr()),
                        C.c_void_p(offs_dev.data_ptr()), offs.ctypes.data_as(ip), 1, None, None, thr.ctypes.data_as(dp),
                        rng.ctypes.data_as(dp), *[C.c_void_p(o.data_ptr()) for o in outs], None, None)
    torch.cuda.synchronize()
    assert rc == -3
    assert all(bool((o == 0x5A).all()) for o in outs)


def test_summary_equals_the_host_function(torch_cuda):
    from posepaf import oks_eval as oe
    ev, out, _ = _device_outputs(torch_cuda, "seeded")
    _, gts, dts = ap_cases.seeded_cases()
    want, got = oe.evaluate_keypoints_ranges(gts, dts), ev.summary(out)
    assert tuple(got) == TWELVE
    for k in TWELVE:
        assert _same(got[k], want[k]), (k, got[k], want[k])
    assert 0.0 < got["AP"] < 1.0 and 0.0 < got["APm"] < 1.0 and 0.0 < got["APl"] < 1.0


# ------------------------------------------------------------------------------------------------ evaluate.py --ap
_RUNS = {}


def _evaluate(tmp, name, extra, timeout, env_extra=None):
    """one evaluate.py child under its own time limit -> (summary, bytes of results.json); a finished run is reused"""
    if name not in _RUNS:
        dump = os.path.join(tmp, name + ".json")
        env = dict(os.environ, **(env_extra or {}))
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
            env.pop(k, None)
        r = subprocess.run([sys.executable, os.path.join(PKG, "evaluate.py"), "--run_refactor", "--run_cpp", "--synthetic", "24",
                            "--batch", "8", "--sizes", "256x256", "--dump_name", dump] + extra,
                           capture_output=True, text=True, timeout=timeout, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        summary = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        _RUNS[name] = (summary, open(dump, "rb").read())
    return _RUNS[name]


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("ap_runs"))


def _twelve(summary):
    return [summary["synthetic_oks"][k] for k in TWELVE]


def test_evaluate_ap_host_and_device_agree_and_leave_results_json_as_it_was(torch_cuda, run_dir):
    host, host_json = _evaluate(run_dir, "host", ["--ap", "host"], 900)
    dev, dev_json = _evaluate(run_dir, "device", ["--ap", "device"], 600)
    assert host["ap"]["path"] == "host" and dev["ap"]["path"] == "device"
    for s in (host, dev):
        assert tuple(s["synthetic_oks"]) == TWELVE and s["status_or"] == 0 and s["images"] == 24
        assert all(s["ap"][k] >= 0.0 for k in ("seconds_rows_and_match", "seconds_accumulate", "seconds_json"))
    assert len(host_json) > 1000 and dev_json == host_json
    assert all(_same(a, b) for a, b in zip(_twelve(host), _twelve(dev))), (_twelve(host), _twelve(dev))
    assert host["people_found"] == dev["people_found"] == len(json.loads(dev_json)) > 0
    assert host["synthetic_oks"]["n_gt"] > 0 and host["synthetic_oks"]["AP"] > 0.0
    # the default run: its file is the same, its report evaluate_keypoints' (range `all` of the twelve)
    plain, plain_json = _evaluate(run_dir, "plain", [], 600)
    assert plain_json == dev_json and "ap" not in plain
    assert tuple(plain["synthetic_oks"]) == ("AP", "AP50", "AP75", "AR", "n_gt", "n_dt")
    assert all(_same(plain["synthetic_oks"][k], dev["synthetic_oks"][k]) for k in plain["synthetic_oks"])


def test_evaluate_ap_device_two_ranks_on_one_gpu_gloo_rehearsal(torch_cuda, run_dir):
    """every rank matches its own shard against its own shard's ground truth; rank 0 re-interleaves and accumulates"""
    one, one_json = _evaluate(run_dir, "device", ["--ap", "device"], 900)
    two, two_json = _evaluate(run_dir, "device2", ["--ap", "device", "--gpus", "2"], 900, {"POSEPAF_DIST_BACKEND": "gloo"})
    assert two["world"] == 2 and one["world"] == 1 and two["ap"]["path"] == "device"
    assert two_json == one_json
    assert all(_same(a, b) for a, b in zip(_twelve(one), _twelve(two))), (_twelve(one), _twelve(two))
