"""GPU: the C++-rule post-processing on feature maps kept in device memory (k_flip_average_maps + k_heat_peaks_hbm +
k_limb_connect_hbm) -- the same bits as the LDS-resident kernels wherever both run, the oracle's answer at sizes that only the
new path takes, the residency decision, hipGraph replay, and the evaluate.py script."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG
from large_map_cases import LARGE_CASES, MAX_PEAKS, case_nets, oracle_wants

pytestmark = pytest.mark.gpu


# torch_cuda and post are fixtures of tests/test_gpu_parity.py's module, not of conftest.py; this file has its own, and its `post` is
# created for 128 x 131 so that the ragged 125 x 131 case fits its capacity.
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def post(torch_cuda):
    from posepaf.api import PosePostProcessor
    p = PosePostProcessor(max_batch=8, max_h=128, max_w=131, max_peaks_per_part=MAX_PEAKS)
    yield p
    p.close()


def _records_vs_oracle(rec, want, ctx=""):
    nh = int(rec["n_humans"])
    assert nh == len(want["ids"]), f"{ctx}: humans {nh} vs {len(want['ids'])}"
    got_ids = rec["humans"]["peak_id"][:nh]
    assert np.array_equal(got_ids, want["ids"]), ctx
    assert np.array_equal(rec["humans"]["score"][:nh], want["scores"]), f"{ctx}: scores differ"
    for h in range(nh):
        for p in range(18):
            pid = got_ids[h, p]
            if pid >= 0:
                assert rec["humans"]["x"][h, p] == want["peaks"][pid, 0]
                assert rec["humans"]["y"][h, p] == want["peaks"][pid, 1]
                assert rec["humans"]["part_score"][h, p] == want["peaks"][pid, 2]


def _record_bytes(rec):
    """everything a record defines (slots beyond n_humans are never written)"""
    n = int(rec["n_humans"])
    return (n, int(rec["n_peaks"]), int(rec["n_connections"]), int(rec["status"]), rec["humans"][:n].tobytes())


def _snapshot(post, recs, batch):
    """records + every intermediate the context lets a caller read, as bytes"""
    out = [[_record_bytes(r) for r in recs]]
    for i in range(batch):
        out.append((post.read_peaks(i).tobytes(), post.read_part_counts(i).tobytes(), post.read_connection_counts(i).tobytes(),
                    [post.read_connections(i, limb).tobytes() for limb in range(30)], post.debug_read_flags(i).tobytes()))
    return out


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("shape", [(16, 24), (33, 47), (125, 131), (128, 128)])
def test_hbm_path_gives_the_bits_of_the_lds_path(torch_cuda, post, shape, dtype, flip):
    """PP_MAPS_AUTO (the map staged in LDS) against PP_MAPS_HBM (pre-pass + _hbm kernels) on shapes both take: a tiny map, an odd
    plane (33 x 47: the caller's planes are not 16-byte aligned), a ragged last mask vector (125 x 131) and the bench shape; empty,
    sparse and crowded images in one batch.  Records, peaks, counts, connections of every limb and the raw flag words are equal
    byte for byte; so are the peaks of pp_nms_batch_ex in both NMS modes and all four refine modes."""
    from posepaf import synth
    torch = torch_cuda
    h, w = shape
    nets = np.stack([synth.make_net_output(p, 300 + p, h=h, w=w, dtype=dtype, flip=flip) for p in (0, 2, 9)])
    dev = torch.from_numpy(nets).cuda()
    got = {}
    try:
        for mode in ("auto", "hbm"):
            post.set_map_residency(mode)
            assert post.map_residency(dtype, h, w) == ("lds" if mode == "auto" else "hbm")
            full = _snapshot(post, post.process(dev, 4 * h, flip=flip), 3)
            nms = []
            for nms_mode in (0, 1):
                for refine_mode in (0, 1, 2, 3):
                    lists = post.nms_ex(dev, flip=flip, nms_mode=nms_mode, threshold=0.1, refine_mode=refine_mode)
                    nms.append(([a.tobytes() for a in lists], [post.read_part_counts(i).tobytes() for i in range(3)],
                                [post.debug_read_flags(i)[:18].tobytes() for i in range(3)]))
            got[mode] = (full, nms)
    finally:
        post.set_map_residency("auto")
    assert sum(r[0] for r in got["auto"][0][0]) > 0              # the comparison is not between two empty results
    assert got["hbm"][0] == got["auto"][0]
    for k, (a, b) in enumerate(zip(got["auto"][1], got["hbm"][1])):
        assert a == b, f"nms_mode {k // 4} refine_mode {k % 4}"


@pytest.mark.parametrize("case", LARGE_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_maps_beyond_lds_match_the_oracle(torch_cuda, oracle, case):
    """Sizes the LDS kernels cannot take (a padded Full-HD frame in fp16; fp32 just past its bound), flip on: peaks including the
    refined score, connections, person ids and scores equal the oracle's, status 0.  No image is skipped: the scenes are free of
    sort_oob and of parts beyond 64 peaks (test_large_map_seeds_cpu.py).  Before the large-map kernels these shapes raised
    PosePafError (PP_ERR_TOO_LARGE)."""
    from posepaf.api import PosePostProcessor
    torch = torch_cuda
    name, h, w, scenes = case
    nets = case_nets(case)
    wants = oracle_wants(oracle, case)
    post = PosePostProcessor(max_batch=len(nets), max_h=h, max_w=w, max_peaks_per_part=MAX_PEAKS)
    try:
        assert post.map_residency(nets[0].dtype, h, w) == "hbm"
        recs = post.process(torch.from_numpy(np.stack(nets)).cuda(), 4 * h)
        for i, want in enumerate(wants):
            assert recs[i]["status"] == 0
            assert np.array_equal(post.read_peaks(i), want["joint_list"])
            for limb in range(30):
                exp = np.array([(c[0], c[1], c[2], c[5]) for c in want["connections"][limb]], np.float32).reshape(-1, 4)
                assert np.array_equal(post.read_connections(i, limb), exp), f"image {i} limb {limb}"
            _records_vs_oracle(recs[i], want, f"{name} {h}x{w} image {i}")
    finally:
        post.close()


def test_residency_decision_and_capacity(torch_cuda):
    from posepaf.api import PosePafError, PosePostProcessor
    small = PosePostProcessor(max_batch=2, max_h=128, max_w=128, max_peaks_per_part=MAX_PEAKS)
    big = PosePostProcessor(max_batch=2, max_h=272, max_w=480, max_peaks_per_part=MAX_PEAKS)
    try:
        assert small.map_workspace_bytes == 0                    # today's shapes allocate nothing new
        assert small.map_residency(np.float16, 128, 128) == "lds"
        assert big.map_residency(np.float16, 128, 128) == "lds" and big.map_residency(np.float32, 160, 160) == "lds"
        assert big.map_residency(np.float16, 272, 480) == "hbm" and big.map_residency(np.float32, 192, 200) == "hbm"
        assert big.map_workspace_bytes == 2 * 48 * 272 * 480 * 4 + 16
        with pytest.raises(PosePafError):                        # area beyond max_h * max_w: still PP_ERR_TOO_LARGE
            small.map_residency(np.float16, 272, 480)
        with pytest.raises(PosePafError):
            small.process(torch_cuda.zeros((1, 2, 50, 272, 480), dtype=torch_cuda.float16, device="cuda"), 1088)
        with pytest.raises(PosePafError):
            big.map_residency(np.float16, 273, 480)
        with pytest.raises(PosePafError):                        # the Python rules have no large-map kernels
            big.process_py(torch_cuda.zeros((1, 2, 50, 272, 480), dtype=torch_cuda.float16, device="cuda"), 1088)
        # the documented cap, 650 x 950 (the reference's 2600 x 3800 / 4): K_A's LDS then holds 77 KB of mask bytes
        cap = PosePostProcessor(max_batch=1, max_h=651, max_w=950, max_peaks_per_part=MAX_PEAKS)
        try:
            assert cap.map_residency(np.float16, 650, 950) == "hbm" and cap.map_residency(np.float32, 650, 950) == "hbm"
            with pytest.raises(PosePafError):
                cap.map_residency(np.float16, 651, 950)
        finally:
            cap.close()
        small.set_map_residency("hbm")                           # allocates on first use
        assert small.map_workspace_bytes == 2 * 48 * 128 * 128 * 4 + 16
        assert small.map_residency(np.float16, 128, 128) == "hbm"
        small.set_map_residency("auto")
        assert small.map_residency(np.float16, 128, 128) == "lds"
    finally:
        small.close()
        big.close()


def test_timing_entries_take_the_residency_decision(torch_cuda, post):
    """pp_time_kernels and pp_time_map_prepass with PP_MAPS_HBM at a tiny shape: both succeed, the pre-pass has a duration, and
    the records the timed chain leaves behind are those of process(); staged in LDS there is no pre-pass (0 ms)."""
    from posepaf import synth
    import ctypes as C
    from posepaf import _lib
    torch = torch_cuda
    h, w = 33, 47
    dev = torch.from_numpy(np.stack([synth.make_net_output(p, 300 + p, h=h, w=w, dtype=np.float16) for p in (2, 9)])).cuda()
    try:
        want = [_record_bytes(r) for r in post.process(dev, 4 * h)]
        assert post.time_map_prepass(dev, True, iters=2) == 0.0
        post.set_map_residency("hbm")
        ms = post.time_kernels(dev, 4 * h, True, iters=2)
        assert all(ms[k] > 0 for k in ("k_heat_peaks", "k_limb_connect", "k_assemble_wave", "chain"))
        assert post.time_map_prepass(dev, True, iters=2) > 0.0
        got = np.empty(2, _lib.RECORD_DTYPE)     # the context's own record buffer: what the chain's last timed pass wrote
        _lib.check(post.L.pp_read_records(post.ctx, None, got.ctypes.data_as(C.c_void_p), 2, None), post.ctx)
        assert [_record_bytes(r) for r in got] == want
    finally:
        post.set_map_residency("auto")


def test_hbm_path_graph_replay(torch_cuda):
    """PP_MAPS_HBM, 8 images of 33 x 47 fp16: pp_process_batch (three launches) captured into a graph and replayed five times
    over two batches gives the eager records, and every raw flag word carries defined bits only (each producing workgroup
    stores its word on every launch; nothing is zeroed in between)."""
    from posepaf import synth
    from posepaf.api import PosePostProcessor, records_to_numpy
    torch = torch_cuda
    B, h, w = 8, 33, 47
    post = PosePostProcessor(max_batch=B, max_h=h, max_w=w, max_peaks_per_part=MAX_PEAKS)
    try:
        post.set_map_residency("hbm")
        sets = [np.stack([synth.make_net_output((i + 3 * k) % 7, 500 + 10 * k + i, h=h, w=w, dtype=np.float16) for i in range(B)])
                for k in range(2)]
        eager = [post.process(torch.from_numpy(s).cuda(), 4 * h).copy() for s in sets]
        static_in = torch.from_numpy(sets[0]).cuda()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            post.process_async(static_in, 4 * h, True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = post.process_async(static_in, 4 * h, True)
        for rep in range(5):
            k = rep % 2
            static_in.copy_(torch.from_numpy(sets[k]).cuda(), non_blocking=True)
            g.replay()
            got = records_to_numpy(out)
            for i in range(B):
                assert _record_bytes(got[i]) == _record_bytes(eager[k][i]), (rep, i)
                assert (post.debug_read_flags(i) & ~np.uint32(0xFF) == 0).all(), (rep, i)
    finally:
        post.close()


def test_evaluate_script_on_the_hbm_path(tmp_path):
    """evaluate.py --run_refactor --run_cpp as a child process, plain and with POSEPAF_MAPS=hbm, both on one saved kernel-choice
    table (so the forward is the same): equal result dumps, and the summary names the residency."""
    cache = tmp_path / "cache"
    cache.mkdir()
    dumps, summaries = [], []
    for name, extra in (("plain", {}), ("hbm", {"POSEPAF_MAPS": "hbm"})):
        dump = tmp_path / f"{name}.json"
        env = {k: v for k, v in os.environ.items() if k != "POSEPAF_MAPS"}
        env.update(extra, POSEPAF_CACHE_DIR=str(cache))
        r = subprocess.run([sys.executable, os.path.join(PKG, "evaluate.py"), "--run_refactor", "--run_cpp", "--synthetic", "4",
                            "--batch", "2", "--sizes", "256x256", "--dump_name", str(dump)],
                           capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        summaries.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
        dumps.append(json.load(open(dump)))
    assert summaries[0]["map_residency"] == "lds" and summaries[1]["map_residency"] == "hbm"
    assert summaries[0]["status_or"] == 0 and summaries[1]["status_or"] == 0
    assert len(dumps[0]) > 0 and dumps[0] == dumps[1]
