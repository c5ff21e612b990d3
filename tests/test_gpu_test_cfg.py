"""GPU: the run-time test configuration of the batched Python-rule paths against the REFERENCE's own Python under the same
configuration (golden G7, tests/golden/make_golden_cfg.py).  Every test here fails on a library without pp_set_test_cfg."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_scene, scene_keys

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-4            # tests/test_gpu_parity.py: the record's float32 score field
INDEX = json.load(open(os.path.join(GOLDEN, "g7_cfg_index.json")))
ORIGINAL_ONLY = {"thre1", "offset_radius"}
PY_CONFIGS = sorted(n for n, c in INDEX["configs"].items() if not set(c["moved"]) <= ORIGINAL_ONLY)
ALL_CONFIGS = sorted(INDEX["configs"])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture()
def post(torch_cuda):
    from posepaf.api import PosePostProcessor
    p = PosePostProcessor(max_batch=8, max_h=192, max_w=192, max_peaks_per_part=64)
    yield p
    p.close()


def g7(name):
    return np.load(os.path.join(GOLDEN, f"g7_cfg_{name}.npz"))


def g7_scene(key):
    """input of a G7 refactored-path scene, regenerated and SHA-checked (the scenes of scenes.json plus any extra ones)"""
    from posepaf import synth
    m = INDEX["scenes"][key]
    net = synth.make_net_output(m["P"], m["seed"], noise=m["noise"], dtype=np.float16 if m["dtype"] == "f16" else np.float32)
    assert hashlib.sha256(net.tobytes()).hexdigest() == m["net_sha256"], \
        f"synthetic scene {key} no longer reproduces the input G7 was made from; re-run tests/golden/make_golden_cfg.py"
    return net


def check_py_record(rec, want, ncn, counts):
    """the assertions of test_python_twins_mode_against_reference_python"""
    n = int(rec["n_humans"])
    assert n == len(want)
    assert np.array_equal(rec["humans"]["peak_id"][:n], want[:, :18, 0].astype(np.int32))
    assert np.array_equal(rec["humans"]["n_parts"][:n], want[:, 19, 0].astype(np.int32))
    assert np.allclose(rec["humans"]["score"][:n], want[:, 18, 0] / want[:, 19, 0], rtol=0, atol=SCORE_TOL)
    assert np.array_equal(counts, ncn)                       # per limb, the reference's own Python
    assert rec["n_connections"] == int(ncn.sum())


@pytest.mark.parametrize("name", PY_CONFIGS)
def test_process_py_with_configuration_against_reference_python(torch_cuda, post, name):
    """pp_process_batch_py under every stored configuration, every stored scene: person ids, part counts and per-limb
    connection counts identical to the reference's find_connections + find_humans with that test_cfg; totals within 1e-4."""
    torch = torch_cuda
    g = g7(name)
    moved = INDEX["configs"][name]["moved"]
    post.set_test_cfg(moved)
    for k, v in moved.items():
        assert post.test_cfg[k] == v
    for key in sorted(INDEX["scenes"]):
        rec = post.process_py(torch.from_numpy(g7_scene(key)).cuda()[None], 512)[0]
        assert rec["status"] == 0, (name, key)
        check_py_record(rec, g[f"{key}__py_persons"], g[f"{key}__py_n_connections"], post.read_connection_counts(0))


def original_scene(torch, key, batch=2):
    from posepaf import synth
    from posepaf.api import PosePostProcessor
    from posepaf.original_path import OriginalPathProcessor
    m = INDEX["original_scenes"][key]
    sizes = [tuple(s) for s in m["sizes"]]
    outs, _ = synth.make_scene_at_scales(m["people"], m["seed"], sizes, dtype=np.float16 if m["dtype"] == "f16" else np.float32,
                                         img=m["img"])
    sha = hashlib.sha256(b"".join(np.ascontiguousarray(o).tobytes() for o in outs)).hexdigest()
    assert sha == m["outs_sha256"], f"{key} no longer reproduces the input G7 was made from"
    post = PosePostProcessor(max_batch=batch, max_h=96, max_w=96, max_peaks_per_part=64)
    proc = OriginalPathProcessor(post, m["img"], m["img"], batch)
    proc.reset()
    for o in outs:   # bit-equal to the oracle's accumulators the generator used (test_original_multiscale_path_against_oracle)
        proc.accumulate(torch.from_numpy(np.stack([o] * batch)).cuda(), 0, 0, len(sizes))
    return post, proc


def peak_rows(post, proc, image):
    """(N, 4) float64 [x, y, score, part] of k_fullres_peaks' output in joint-list order"""
    counts = post.read_part_counts(image)
    pk = proc.peaks64[image].cpu().numpy()
    return np.concatenate([np.column_stack([pk[p, :c, :3], np.full(c, float(p))]) for p, c in enumerate(counts)]).reshape(-1, 4)


@pytest.mark.parametrize("name", ALL_CONFIGS)
@pytest.mark.parametrize("key", sorted(INDEX["original_scenes"]))
def test_original_path_with_configuration_against_reference_python(torch_cuda, key, name):
    """OriginalPathProcessor.finish(test_cfg=...) against the reference's find_peaks (keypoint_heatmap_nms +
    refine_centroid(offset_radius)) + find_connections + find_humans on the same float64 maps: the assertions of
    test_original_multiscale_path_against_oracle (ids and counts exact, fractional coordinates and scores within 1e-4), the
    centroids at the rtol 1e-5 / atol 1e-6 of test_original_path_nms_and_centroid_modes."""
    from posepaf.api import records_to_numpy
    from posepaf.original_path import record_float_coords
    torch = torch_cuda
    g = g7(name)
    rows, persons, ncn = g[f"{key}__o_rows"], g[f"{key}__o_persons"], g[f"{key}__o_n_connections"]
    post, proc = original_scene(torch, key)
    recs = records_to_numpy(proc.finish(2, test_cfg=INDEX["configs"][name]["moved"]))
    for b, rec in enumerate(recs):
        assert rec["status"] == 32                          # PP_ST_FLOAT_COORDS and nothing else
        assert rec["n_peaks"] == len(rows)
        got_rows = peak_rows(post, proc, b)
        assert np.array_equal(got_rows[:, 3], rows[:, 4])
        print(name, key, "centroid max abs diff", np.abs(got_rows[:, :3] - rows[:, :3]).max(initial=0.0))
        assert np.allclose(got_rows[:, :3], rows[:, :3], rtol=1e-5, atol=1e-6)
        assert np.array_equal(post.read_connection_counts(b), ncn)
        n = int(rec["n_humans"])
        assert n == len(persons)
        assert np.array_equal(rec["humans"]["peak_id"][:n], persons[:, :18, 0].astype(np.int32))
        assert np.array_equal(rec["humans"]["n_parts"][:n], persons[:, 19, 0].astype(np.int32))
        assert np.allclose(rec["humans"]["score"][:n], persons[:, 18, 0] / persons[:, 19, 0], rtol=0, atol=SCORE_TOL)
        fx, fy = record_float_coords(rec)
        for h_ in range(n):
            for p in range(18):
                pid = rec["humans"]["peak_id"][h_, p]
                if pid >= 0:
                    assert abs(fx[h_, p] - rows[pid, 0]) < 1e-4 and abs(fy[h_, p] - rows[pid, 1]) < 1e-4
                    assert abs(rec["humans"]["part_score"][h_, p] - rows[pid, 2]) < 1e-4
    post.close()


def test_remove_recon_deletion_scene(torch_cuda, post):
    """the scenes on which the reference takes the deletion (:559-564): remove_recon = 1 equals the reference and differs from
    remove_recon = 0 on the same scene"""
    torch = torch_cuda
    g = g7("remove_recon")
    assert INDEX["recon_scenes"]
    for key in INDEX["recon_scenes"]:
        dev = torch.from_numpy(g7_scene(key)).cuda()[None]
        post.set_test_cfg({})
        off = post.process_py(dev, 512)[0]
        post.set_test_cfg({"remove_recon": 1})
        on = post.process_py(dev, 512)[0]
        assert on["status"] == 0
        check_py_record(on, g[f"{key}__py_persons"], g[f"{key}__py_n_connections"], post.read_connection_counts(0))
        assert defined_bytes([on]) != defined_bytes([off])


def recon_undefined_table():
    """Joint list and connections on which the reference's remove_recon branch RAISES: peak id 5 is held by person A both as
    neck and as nose (the host form takes ids as given), so for the nose -> Reye connection (5 -> 7), which A claims through
    its nose and B through its Reye while both have a neck, `int(np.where(person1_peak_ids == 5)[0])` sees two matches
    (utils/parse_skeletons.py:530).  Checked against the reference when this test was written: TypeError with remove_recon = 1,
    two people with remove_recon = 0."""
    rows = [(10.0, 10.0, 0.9, 0, 2), (20.0, 10.0, 0.9, 1, 3), (30.0, 10.0, 0.9, 2, 4), (40.0, 10.0, 0.9, 3, 5),
            (50.0, 10.0, 0.9, 4, 6), (60.0, 60.0, 0.9, 5, 0), (60.0, 80.0, 0.9, 5, 1), (90.0, 80.0, 0.9, 6, 1),
            (95.0, 55.0, 0.9, 7, 14)]
    all_peaks = [[r[:4] for r in rows if r[4] == k] for k in range(18)]
    conns = {0: [[5.0, 5.0, 0.8, 0, 0, 20.0]],        # neck 5 -> nose 5: person A
             1: [[6.0, 7.0, 0.8, 1, 0, 25.0]],        # neck 6 -> Reye 7: person B
             5: [[5.0, 7.0, 0.9, 0, 0, 35.0]]}        # nose 5 -> Reye 7: A by its nose, B by its Reye, both have a neck
    return all_peaks, conns


def host_find_humans(post, all_peaks, conns):
    from posepaf import _lib
    jl = np.asarray([tuple(float(v) for v in pk[:4]) + (float(part),) for part, pks in enumerate(all_peaks) for pk in pks],
                    np.float32).reshape(-1, 5)
    c = np.zeros((30, post.maxp, 6), np.float64)
    counts = np.zeros(30, np.int32)
    for k, rows in conns.items():
        counts[k] = len(rows)
        c[k, :len(rows)] = rows
    persons = np.zeros((128, 20, 2), np.float64)
    n = C.c_int(0)
    L = _lib.load()
    _lib.check(L.pp_py_find_humans_host(post.ctx, c.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(C.POINTER(C.c_int)),
                                        jl.ctypes.data_as(C.POINTER(C.c_float)), len(jl),
                                        persons.ctypes.data_as(C.POINTER(C.c_double)), 128, C.byref(n)), post.ctx)
    rec = np.zeros(1, _lib.RECORD_DTYPE)
    _lib.check(L.pp_read_records(post.ctx, None, rec.ctypes.data_as(C.c_void_p), 1, None), post.ctx)
    return persons[:n.value].copy(), int(rec[0]["status"])


def test_recon_undefined_is_flagged_and_changes_nothing(torch_cuda, post):
    all_peaks, conns = recon_undefined_table()
    post.set_test_cfg({})
    off, st_off = host_find_humans(post, all_peaks, conns)
    assert st_off & 128 == 0 and len(off) == 2
    post.set_test_cfg({"remove_recon": 1})
    on, st_on = host_find_humans(post, all_peaks, conns)
    assert st_on & 128                                       # PP_ST_RECON_UNDEFINED
    assert st_on & ~128 == st_off
    assert np.array_equal(on, off)
    # a table on which the branch is defined deletes the joint and raises no flag: B's neck is 6, A's nose becomes id 8
    all_peaks[0] = [(60.0, 60.0, 0.9, 8)]
    conns[0] = [[5.0, 8.0, 0.8, 0, 0, 20.0]]
    conns[5] = [[8.0, 7.0, 0.9, 0, 0, 35.0]]
    on, st_on = host_find_humans(post, all_peaks, conns)
    post.set_test_cfg({})
    off, st_off = host_find_humans(post, all_peaks, conns)
    assert st_on & 128 == 0 and st_off & 128 == 0
    assert not np.array_equal(on, off)
    assert sorted(on[:, 19, 0]) == [1.0, 2.0] or len(on) < len(off)      # one person lost a joint (and may then be pruned)


def defined_bytes(recs):
    """the bytes of a batch of records that the kernels define: the header and humans[:n_humans] (the slots beyond are never
    written and keep whatever the record buffer held)"""
    return b"".join(np.array([r["n_humans"], r["n_peaks"], r["status"], r["n_connections"]], np.int64).tobytes() +
                    r["humans"][:int(r["n_humans"])].tobytes() for r in recs)


def test_default_configuration_is_byte_equal_and_restorable(torch_cuda, post):
    """defaults set explicitly == a context that never called pp_set_test_cfg; a configuration, then the defaults again,
    restores byte-equal records -- on the refactored and on the original path"""
    from posepaf.api import PosePostProcessor, records_to_numpy
    torch = torch_cuda
    nets = np.stack([load_scene(k)[0].astype(np.float32) for k in scene_keys()[:8]])
    dev = torch.from_numpy(nets).cuda()
    fresh = PosePostProcessor(max_batch=8, max_h=192, max_w=192, max_peaks_per_part=64)
    base = defined_bytes(fresh.process_py(dev, 512))
    fresh.close()
    post.set_test_cfg({})
    assert defined_bytes(post.process_py(dev, 512)) == base
    post.set_test_cfg(INDEX["configs"]["all_moved"]["moved"])
    assert defined_bytes(post.process_py(dev, 512)) != base
    post.set_test_cfg(None)
    assert defined_bytes(post.process_py(dev, 512)) == base
    cpp = defined_bytes(post.process(dev, 512))                             # the C++ rules never look at the configuration
    post.set_test_cfg(INDEX["configs"]["all_moved"]["moved"])
    assert defined_bytes(post.process(dev, 512)) == cpp

    key = sorted(INDEX["original_scenes"])[-1]
    p2, proc = original_scene(torch, key)
    base_o = defined_bytes(records_to_numpy(proc.finish(2)))
    assert defined_bytes(records_to_numpy(proc.finish(2, test_cfg={}))) == base_o
    assert defined_bytes(records_to_numpy(proc.finish(2, test_cfg=INDEX["configs"]["all_moved"]["moved"]))) != base_o
    assert defined_bytes(records_to_numpy(proc.finish(2))) != base_o          # None = what the context holds
    assert defined_bytes(records_to_numpy(proc.finish(2, test_cfg={}))) == base_o
    p2.close()


def test_out_of_range_is_refused_and_previous_configuration_stays(torch_cuda, post):
    from posepaf import _lib
    torch = torch_cuda
    dev = torch.from_numpy(g7_scene(sorted(INDEX["scenes"])[0])).cuda()[None]
    post.set_test_cfg({"mid_num": 40, "thre2": 0.05})
    before = defined_bytes(post.process_py(dev, 512))
    held = post.test_cfg
    L = _lib.load()
    for field, val in (("mid_num", 0), ("mid_num", 129), ("offset_radius", 8), ("offset_radius", -1), ("remove_recon", 2),
                       ("thre2", float("nan")), ("connect_ration", -0.5), ("len_rate", float("inf")), ("connection_tole", -1.0)):
        c = _lib.TestCfg()
        assert L.pp_default_test_cfg(C.byref(c)) == 0
        setattr(c, field, val)
        assert L.pp_set_test_cfg(post.ctx, C.byref(c)) == -6, (field, val)      # PP_ERR_UNSUPPORTED
        assert post.test_cfg == held
    with pytest.raises(ValueError):
        post.set_test_cfg({"mid_num": 500})
    assert post.test_cfg == held
    assert defined_bytes(post.process_py(dev, 512)) == before


def test_shims_keep_the_defaults_after_another_processor_was_configured(torch_cuda, post, oracle):
    """utils.parse_skeletons.find_connections / find_humans still refuse a moved key and still match G3 (the reference's
    Python under the INI defaults) while a configured processor is alive"""
    from posepaf import skeleton as sk
    from utils import parse_skeletons as ps
    torch = torch_cuda
    post.set_test_cfg(INDEX["configs"]["all_moved"]["moved"])
    key = "P6_s2_f32"
    net, g = load_scene(key)
    post.process_py(torch.from_numpy(net).cuda()[None], 512)
    jl = g["joint_list"]
    all_peaks = [[tuple(float(v) for v in row[:4]) for row in jl[jl[:, 4] == k]] for k in range(18)]
    _, paf = oracle.flip_average(net)
    up = oracle.upsample4_hwc(paf)
    cfg = sk.default_test_cfg()
    connected, special = ps.find_connections(all_peaks, up, 512, cfg, np.array(sk.LIMB_PAIRS))
    assert np.array_equal(np.array([len(c) for c in connected], np.int32), g["py_n_connections"])
    persons, _ = ps.find_humans(connected, special, all_peaks, cfg, np.array(sk.LIMB_PAIRS))
    assert np.array_equal(persons[:, :, 0], g["py_persons"][:, :, 0])
    with pytest.raises(NotImplementedError):
        ps.find_connections(all_peaks, up, 512, dict(cfg, thre2=0.05), np.array(sk.LIMB_PAIRS))
    with pytest.raises(NotImplementedError):
        ps.find_humans(connected, special, all_peaks, dict(cfg, remove_recon=1), np.array(sk.LIMB_PAIRS))
