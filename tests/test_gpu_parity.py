"""GPU: the HIP path (through the C ABI of libposepaf.so) against the oracle, the compiled reference and the
golden vectors.  Bar: peak coordinates/ids, limb connections and person assignments bit-exact; scores within
1e-4 as BASELINE.json's north_star states -- in practice the kernels reproduce the reference's rounding order,
so scores are asserted EQUAL and the 1e-4 bound is only the documented contract.
"""
import numpy as np
import pytest

from conftest import load_scene, scene_keys

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def post(torch_cuda):
    from posepaf.api import PosePostProcessor
    return PosePostProcessor(max_batch=8, max_h=192, max_w=192, max_peaks_per_part=64)


def _records_vs_oracle(rec, want, ctx=""):
    nh = int(rec["n_humans"])
    assert nh == len(want["ids"]), f"{ctx}: humans {nh} vs {len(want['ids'])}"
    got_ids = rec["humans"]["peak_id"][:nh]
    assert np.array_equal(got_ids, want["ids"]), ctx
    got_scores = rec["humans"]["score"][:nh]
    assert np.allclose(got_scores, want["scores"], rtol=0, atol=SCORE_TOL), ctx
    assert np.array_equal(got_scores, want["scores"]), f"{ctx}: scores differ in the last bits"
    # x / y / part score of every assigned part == the oracle's peak table (getters of evaluate.py:119-126)
    for h in range(nh):
        for p in range(18):
            pid = got_ids[h, p]
            if pid >= 0:
                assert rec["humans"]["x"][h, p] == want["peaks"][pid, 0]
                assert rec["humans"]["y"][h, p] == want["peaks"][pid, 1]
                assert rec["humans"]["part_score"][h, p] == want["peaks"][pid, 2]


@pytest.mark.parametrize("key", scene_keys())
def test_full_path_golden_scene(torch_cuda, post, oracle, key):
    """net output -> records, against the reference C++'s stored outputs and the oracle's whole path."""
    torch = torch_cuda
    net, g = load_scene(key)
    dev = torch.from_numpy(net).cuda()[None]                    # (1,2,50,128,128)
    rec = post.process(dev, 512)[0]
    assert rec["status"] == 0          # make_golden.py asserts these scenes are free of the sort's undefined behaviour
    # stage 1: peaks (bit-exact incl. refined score)
    jl = post.read_peaks(0)
    assert np.array_equal(jl, g["joint_list"])
    # stage 2: connections per limb
    want = oracle.pipeline(net, 512)
    for limb in range(30):
        got = post.read_connections(0, limb)
        exp = np.array([(c[0], c[1], c[2], c[5]) for c in want["connections"][limb]], np.float32).reshape(-1, 4)
        assert np.array_equal(got, exp), f"limb {limb}"
    # stage 3: persons
    _records_vs_oracle(rec, want, key)
    assert np.array_equal(rec["humans"]["peak_id"][: rec["n_humans"]], g["cpp_ids"])
    assert np.array_equal(rec["humans"]["score"][: rec["n_humans"]], g["cpp_scores"])
    assert rec["n_peaks"] == len(g["joint_list"])


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("refine", [True, False])
def test_nms_only_matches_oracle(torch_cuda, post, oracle, dtype, refine):
    """config 2: flip-average + NMS (+ refinement) of the keypoint channels."""
    from posepaf import synth
    torch = torch_cuda
    nets = [synth.make_net_output(p, 40 + p, dtype=dtype) for p in (0, 1, 4, 12)]
    dev = torch.from_numpy(np.stack(nets)).cuda()
    lists = post.nms(dev, flip=True, refine=refine)
    for net, got in zip(nets, lists):
        heat, _ = oracle.flip_average(net)
        want, _ = oracle.heatmap_nms(heat, 4, refine=refine)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("shape", [(16, 24), (40, 56), (96, 160), (128, 128), (160, 160)])
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_other_map_sizes_and_batching(torch_cuda, post, oracle, shape, dtype):
    """ragged COCO sizes (padded to /64 -> feature maps that are multiples of 16) and a tiny scalar-path map."""
    from posepaf import synth
    torch = torch_cuda
    h, w = shape
    nets = [synth.make_net_output(p, 7 * p + 1, h=h, w=w, dtype=dtype) for p in (2, 5, 3)]
    dev = torch.from_numpy(np.stack(nets)).cuda()
    recs = post.process(dev, 4 * h)
    for i, net in enumerate(nets):
        want = oracle.pipeline(net, 4 * h)
        if want["sort_oob"]:
            continue
        assert np.array_equal(post.read_peaks(i), want["joint_list"])
        _records_vs_oracle(recs[i], want, f"{shape} img {i}")


def test_no_flip_and_empty_and_single_peak(torch_cuda, post, oracle):
    from posepaf import synth
    torch = torch_cuda
    # flip off: sample 0 only
    net = synth.make_net_output(5, 3, dtype=np.float16, flip=False)
    rec = post.process(torch.from_numpy(net).cuda()[None], 512, flip=False)[0]
    _records_vs_oracle(rec, oracle.pipeline(net, 512, flip=False), "noflip")
    # empty image: nothing above threshold
    z = np.zeros((1, 2, 50, 128, 128), np.float16)
    rec = post.process(torch.from_numpy(z).cuda(), 512)[0]
    assert rec["n_humans"] == 0 and rec["n_peaks"] == 0 and rec["n_connections"] == 0
    # one isolated keypoint (and its mirror image in the flipped sample): peaks but no limbs
    z[0, 0, 30, 60, 60] = 0.9
    z[0, 1, 30, 60, 127 - 60] = 0.9
    rec = post.process(torch.from_numpy(z).cuda(), 512)[0]
    assert rec["n_peaks"] == 1 and rec["n_humans"] == 0
    jl = post.read_peaks(0)
    want, _ = oracle.heatmap_nms(oracle.flip_average(z[0])[0])
    assert np.array_equal(jl, want)


def test_assembly_merge_that_sums_two_peak_ids(torch_cuda, post, oracle):
    """K_C applies independent connections of a limb from lookup tables; a merge that ADDS two ids (pafprocess.cpp:222-226
    with the `id > 0` membership test) creates an id the tables cannot know, and the kernel must fall back to the
    reference's scan for the rest of that limb.  The hand-built scene yields one person with nose id 2."""
    from posepaf import synth
    torch = torch_cuda
    net = synth.make_id_sum_merge_scene()
    rec = post.process(torch.from_numpy(net).cuda()[None], 512, flip=False)[0]
    want = oracle.pipeline(net, 512, flip=False)
    _records_vs_oracle(rec, want, "id-sum merge")
    assert rec["n_humans"] == 1 and rec["humans"]["peak_id"][0, 0] == 2
    # batched next to ordinary scenes (the fall-back is per image and per limb)
    other = synth.make_net_output(9, 77, dtype=np.float32, flip=False)
    both = np.stack([other, net, other])
    recs = post.process(torch.from_numpy(both).cuda(), 512, flip=False)
    _records_vs_oracle(recs[1], want, "id-sum merge, batched")
    _records_vs_oracle(recs[0], oracle.pipeline(other, 512, flip=False), "neighbour 0")
    _records_vs_oracle(recs[2], oracle.pipeline(other, 512, flip=False), "neighbour 2")


@pytest.mark.parametrize("people,noise", [(12, 0.04), (22, 0.03), (33, 0.04), (45, 0.02)])
def test_assembly_stress_crowded_and_noisy_scenes(torch_cuda, post, oracle, people, noise):
    """K_C's run batching / merge / erase paths on fresh crowded scenes (more spurious peaks and skeleton merges than the
    golden set): every image's persons, ids and scores equal the oracle's; images batched 8 at a time."""
    from posepaf import synth
    torch = torch_cuda
    nets = np.stack([synth.make_net_output(people, 7000 + 13 * people + i, noise=noise, dtype=np.float16 if i % 2 else np.float32)
                     .astype(np.float32) for i in range(8)])
    recs = post.process(torch.from_numpy(nets).cuda(), 512)
    checked = 0
    for i in range(8):
        want = oracle.pipeline(nets[i], 512)
        assert recs[i]["status"] & ~np.uint32(1 | 8) == 0
        assert bool(recs[i]["status"] & 8) == bool(want["sort_oob"])       # PP_ST_SORT_UNDEFINED exactly where the oracle sees it
        if want["sort_oob"] or recs[i]["status"] & 1:   # undefined reference behaviour / more than 64 peaks of one part
            continue
        _records_vs_oracle(recs[i], want, f"P={people} noise={noise} img {i}")
        checked += 1
    assert checked >= 4


def _same_record(a, b):
    """equal in everything the record defines (slots beyond n_humans are never written)"""
    n = int(a["n_humans"])
    return (n == int(b["n_humans"]) and a["n_peaks"] == b["n_peaks"] and a["n_connections"] == b["n_connections"]
            and a["status"] == b["status"] and a["humans"][:n].tobytes() == b["humans"][:n].tobytes())


def test_limb_scoring_many_survivors_full_batch(torch_cuda, oracle):
    """K_B parks the pairs that survive their first samples and finishes them in packed rounds; with more than 256 live
    survivors the packed rounds start INSIDE the pair loop.  A limb map that is high everywhere keeps every pair alive
    (64 x 64 pairs per limb), on a batch large enough that workgroups queue behind each other.  Checked against the oracle."""
    from posepaf import synth
    from posepaf.api import PosePostProcessor
    torch = torch_cuda
    rng = np.random.default_rng(11)
    net = np.zeros((1, 50, 128, 128), np.float32)
    net[0, :30] = 0.6 + 0.3 * rng.random((30, 128, 128), dtype=np.float32)      # every sample of every pair counts
    ys, xs = np.meshgrid(np.arange(8, 128, 16), np.arange(8, 128, 16), indexing="ij")
    for part in range(18):                                                          # 64 isolated peaks per part
        net[0, 30 + part, ys + (part % 4), xs + (part // 4)] = 0.5 + 0.4 * rng.random(ys.shape, dtype=np.float32)
    want = oracle.pipeline(net, 512, flip=False)
    assert min(want["n_candidates"]) > 512 and not want["sort_oob"]                 # beyond the candidate capacity: flagged below
    B = 48
    post = PosePostProcessor(max_batch=B, max_h=128, max_w=128, max_peaks_per_part=64)
    recs = post.process(torch.from_numpy(np.repeat(net[None], B, 0)).cuda(), 512, flip=False)
    assert all(r["status"] & 16 for r in recs)                                       # PP_ST_CAND_OVERFLOW, loud
    assert all(_same_record(recs[i], recs[0]) for i in range(B))
    jl = post.read_peaks(0)
    assert np.array_equal(jl, want["joint_list"])
    # 28 peaks per part -> 784 pairs per limb, ALL alive after their first samples (3 packed rounds start inside the pair loop),
    # but with min_img_size = 110 the long pairs fail `criterion2 > 0` in the end (pafprocess.cpp:92-95), so the accepted
    # candidates (275-358 per limb) fit the capacity and everything must equal the oracle
    r2 = np.random.default_rng(5)
    net2 = net.copy()
    net2[0, 30:48] = 0
    for part in range(18):
        sel = r2.permutation(64)[:28]
        net2[0, 30 + part, (ys.ravel() + (part % 4))[sel], (xs.ravel() + (part // 4))[sel]] = 0.5 + 0.4 * r2.random(28, dtype=np.float32)
    want2 = oracle.pipeline(net2, 110, flip=False)
    assert 256 < min(want2["n_candidates"]) and max(want2["n_candidates"]) <= 512 and not want2["sort_oob"]
    recs2 = post.process(torch.from_numpy(np.repeat(net2[None], B, 0)).cuda(), 110, flip=False)
    for i in (0, 17, B - 1):
        assert recs2[i]["status"] == 0
        _records_vs_oracle(recs2[i], want2, f"all-alive pairs, image {i}")
    assert all(_same_record(recs2[i], recs2[0]) for i in range(B))
    post.close()


@pytest.mark.parametrize("npk,size", [(8, 512), (20, 512), (28, 110)])
def test_massive_ties_terminate_and_are_flagged(torch_cuda, post, oracle, npk, size):
    """Constant limb maps and equal peak scores: hundreds of exactly tied candidates per limb, the case in which the reference's
    `>=` comparator drives std::sort's unguarded scans off the array (undefined behaviour there).  The kernel must finish,
    raise PP_ST_SORT_UNDEFINED where the oracle's restatement sees the out-of-bounds scan, and leave neighbours untouched."""
    from posepaf import synth
    torch = torch_cuda
    rng = np.random.default_rng(3)
    net = np.zeros((1, 50, 128, 128), np.float32)
    net[0, :30] = 0.8
    ys, xs = np.meshgrid(np.arange(8, 128, 16), np.arange(8, 128, 16), indexing="ij")
    for part in range(18):
        sel = rng.permutation(64)[:npk]
        net[0, 30 + part, (ys.ravel() + (part % 4))[sel], (xs.ravel() + (part // 4))[sel]] = 0.9
    want = oracle.pipeline(net, size, flip=False)
    assert want["sort_oob"]
    other = synth.make_net_output(7, 99, dtype=np.float32, flip=False)
    recs = post.process(torch.from_numpy(np.stack([other, net, net, other])).cuda(), size, flip=False)
    for i in (1, 2):
        assert recs[i]["status"] & 8, "PP_ST_SORT_UNDEFINED expected"
        assert recs[i]["status"] & ~np.uint32(8) == 0
        assert recs[i]["n_peaks"] == len(want["joint_list"]) and recs[i]["n_humans"] > 0
    w_other = oracle.pipeline(other, size, flip=False)
    if not w_other["sort_oob"]:
        _records_vs_oracle(recs[0], w_other, "neighbour 0")
        _records_vs_oracle(recs[3], w_other, "neighbour 3")


def test_border_peaks_and_plateaus(torch_cuda, post, oracle):
    """peaks on every border/corner (clipped 3x5 / 3x3 patches) and equal-valued neighbours (plateaus)."""
    torch = torch_cuda
    rng = np.random.default_rng(5)
    net = (rng.random((1, 50, 128, 128), dtype=np.float32) * 0.08).astype(np.float32)
    for c in range(30, 48):
        for (y, x) in [(0, 0), (0, 127), (127, 0), (127, 127), (0, 64), (64, 0), (127, 64), (64, 127), (1, 1), (126, 126)]:
            net[0, c, y, x] = 0.5 + 0.01 * c
        net[0, c, 50, 50] = net[0, c, 50, 51] = 0.7          # horizontal plateau: both are peaks
        net[0, c, 80, 80] = net[0, c, 81, 81] = 0.6          # diagonal neighbours: both are peaks (plus footprint)
    for dt in (np.float32, np.float16):
        n = net.astype(dt)
        got = post.nms(torch.from_numpy(n).cuda()[None], flip=False)[0]
        want, _ = oracle.heatmap_nms(oracle.flip_average(n, flip=False)[0])
        assert len(want) >= 18 * 13
        assert np.array_equal(got, want)


@pytest.mark.parametrize("people", [2, 9, 25])
def test_dropin_process_paf_against_compiled_reference(torch_cuda, oracle, reference_cpp, people):
    """utils.pafprocess drop-in (host arrays in, getters out) vs the reference's own C++ on the same arrays."""
    from posepaf import synth
    from utils.pafprocess import pafprocess
    for seed, dt in ((200, np.float16), (201, np.float32)):
        net = synth.make_net_output(people, seed, dtype=dt)
        heat, paf = oracle.flip_average(net)
        jl, _ = oracle.heatmap_nms(heat)
        up = oracle.upsample4_hwc(paf)
        o = oracle.process_paf(jl[None], up, 512)
        if o["sort_oob"]:
            continue
        want = reference_cpp.process_paf(jl[None], up, 512)
        assert pafprocess.process_paf(jl[None], up, 512) == 0
        nh = pafprocess.get_num_humans()
        assert nh == len(want["ids"])
        ids = np.array([[pafprocess.get_part_peak_id(h, p) for p in range(18)] for h in range(nh)]).reshape(nh, 18)
        assert np.array_equal(ids, want["ids"])
        sc = np.array([pafprocess.get_score(h) for h in range(nh)], np.float32)
        assert np.array_equal(sc, want["scores"])
        for cid in range(len(jl)):
            assert pafprocess.get_part_x(cid) == want["peaks"][cid, 0]
            assert pafprocess.get_part_y(cid) == want["peaks"][cid, 1]
            assert np.float32(pafprocess.get_part_score(cid)) == want["peaks"][cid, 2]


def _dropin_equals(jl, up, want, ctx):
    """utils.pafprocess.process_paf on (jl, up): ids, scores and the part getters equal `want`'s; -> the ids"""
    from utils.pafprocess import pafprocess
    assert pafprocess.process_paf(jl[None], up, 512) == 0, ctx
    nh = pafprocess.get_num_humans()
    assert nh == len(want["ids"]), ctx
    ids = np.array([[pafprocess.get_part_peak_id(h, p) for p in range(18)] for h in range(nh)]).reshape(nh, 18)
    assert np.array_equal(ids, want["ids"]), ctx
    sc = np.array([pafprocess.get_score(h) for h in range(nh)], np.float32)
    assert np.array_equal(sc, want["scores"]), ctx
    assert len(want["peaks"]) == len(jl), ctx
    for cid in range(len(jl)):
        assert pafprocess.get_part_x(cid) == want["peaks"][cid, 0], ctx
        assert pafprocess.get_part_y(cid) == want["peaks"][cid, 1], ctx
        assert np.float32(pafprocess.get_part_score(cid)) == want["peaks"][cid, 2], ctx
    return ids


def test_dropin_id_summing_merge(torch_cuda, oracle, reference_cpp):
    """The drop-in assembly on the hand-built scene whose merge ADDS two peak ids (pafprocess.cpp:200-228, 1 + 0 + 1 = 2) and
    whose later connection of the same limb meets the made-up id: one human, nose id 2, as the reference's own C++ gives."""
    from posepaf import synth
    heat, paf = oracle.flip_average(synth.make_id_sum_merge_scene(), flip=False)
    jl, _ = oracle.heatmap_nms(heat)
    up = oracle.upsample4_hwc(paf)
    ids = _dropin_equals(jl, up, reference_cpp.process_paf(jl[None], up, 512), "id-sum merge")
    assert ids.shape == (1, 18) and ids[0, 0] == 2


def test_dropin_rows_out_of_part_order(torch_cuda, oracle, reference_cpp):
    """The joint list regrouped part 17 first ... part 0 last (order inside a part kept).  process_paf numbers peaks by input
    row (pafprocess.cpp:34) and indexes the part-bucketed line BY that id (:162), so here a peak's id differs from its position
    in the line for almost every peak -- the case the .w ids exist for.  Seed 11: the oracle reports no sort_oob for these rows."""
    from posepaf import synth
    heat, paf = oracle.flip_average(synth.make_net_output(6, 11, dtype=np.float32))
    jl, _ = oracle.heatmap_nms(heat)
    up = oracle.upsample4_hwc(paf)
    rows = np.ascontiguousarray(jl[np.argsort(-jl[:, 4], kind="stable")])
    line_pos = np.argsort(np.argsort(rows[:, 4], kind="stable"), kind="stable")   # position of input row i in the bucketed line
    assert np.count_nonzero(line_pos != np.arange(len(rows))) >= 0.9 * len(rows)
    want = oracle.process_paf(rows[None], up, 512)
    assert not want["sort_oob"] and len(want["ids"]) > 0
    _dropin_equals(rows, up, want, "rows out of part order, oracle")
    _dropin_equals(rows, up, reference_cpp.process_paf(rows[None], up, 512), "rows out of part order, compiled reference")


def test_dropin_argument_errors(torch_cuda):
    from posepaf import _lib
    from utils.pafprocess import pafprocess
    with pytest.raises(TypeError):
        pafprocess.process_paf(np.zeros((3, 5), np.float32), np.zeros((8, 8, 30), np.float32), 8)
    bad_part = np.array([[[1, 1, 0.5, 0, 18]]], np.float32)
    with pytest.raises(_lib.PosePafError):
        pafprocess.process_paf(bad_part, np.zeros((8, 8, 30), np.float32), 8)
    # float64 / non-contiguous inputs are converted like the SWIG typemap does
    pk = np.array([[[2, 2, 0.9, 0, 1], [6, 2, 0.8, 1, 0]]], np.float64)
    paf = np.ones((8, 8, 30), np.float64)
    assert pafprocess.process_paf(pk, paf[:, :, :], 8) == 0
    assert pafprocess.get_num_humans() == 1


def test_full_size_properties(torch_cuda, oracle):
    """BASELINE-sized batch (64 images): size-independent properties instead of a per-image oracle run.
    (1) batching invariance: image i of a batch == the same image processed alone (every defined field);
    (2) determinism: two runs give identical records (every defined field, status included);
    (3) mirror covariance: swapping the roles of the two samples (the mirrored scene becomes sample 0) yields the same
        people with x -> 511 - x ... up to the refinement's arg-max tie-break, so only the person COUNT and the per-person
        part counts are compared."""
    from posepaf import synth
    from posepaf.api import PosePostProcessor
    torch = torch_cuda
    B = 64
    post = PosePostProcessor(max_batch=B, max_h=128, max_w=128, max_peaks_per_part=64)
    nets = np.stack([synth.make_net_output(2 + (i % 9), 1000 + i, dtype=np.float16) for i in range(B)])
    dev = torch.from_numpy(nets).cuda()
    r1 = post.process(dev, 512)
    r2 = post.process(dev, 512)
    assert all(int(r["status"]) & ~8 == 0 for r in r1)
    assert all(_same_record(r1[i], r2[i]) for i in range(B))
    for i in (0, 17, 63):
        alone = post.process(dev[i:i + 1].contiguous(), 512)[0]
        assert _same_record(alone, r1[i]), i
    # (3) sample 1 of make_net_output is the network's view of the MIRRORED scene with left/right channels exchanged, i.e.
    # exactly what sample 0 would be for the mirrored image: swapping the samples processes the mirrored image
    sw = post.process(dev[:16].flip(1).contiguous(), 512)
    for i in range(16):
        if (int(sw[i]["status"]) | int(r1[i]["status"])) & 8:
            continue
        assert sw[i]["n_peaks"] == r1[i]["n_peaks"], i
    # spot-check three images against the oracle
    for i in (5, 31, 48):
        want = oracle.pipeline(nets[i], 512)
        if not want["sort_oob"]:
            _records_vs_oracle(r1[i], want, f"batch image {i}")
    post.close()


def test_reference_shaped_parse_skeletons_surface(torch_cuda, oracle):
    """utils.parse_skeletons.{heatmap_nms, find_peaks_refactor, predict_refactor} (reference signatures, GPU inside)."""
    import os
    from conftest import GOLDEN
    from posepaf import synth
    from utils import parse_skeletons as ps
    net = synth.make_net_output(7, 77, dtype=np.float32)
    heat, paf = oracle.flip_average(net)
    hwc = np.ascontiguousarray(heat.transpose(1, 2, 0))
    got = ps.heatmap_nms(hwc, 4)
    want, _ = oracle.heatmap_nms(heat, 4, refine=True)
    assert len(got) == 18
    assert np.array_equal(np.concatenate(got), want[:, :4])
    got0 = ps.heatmap_nms(hwc, 4, bool_refine_center=False)
    want0, _ = oracle.heatmap_nms(heat, 4, refine=False)
    assert np.array_equal(np.concatenate(got0), want0[:, :4])
    g = np.load(os.path.join(GOLDEN, "g2_find_peaks.npz"))          # scipy-based reference outputs
    for i in (0, 3, 4, 5, 7):
        assert np.array_equal(ps.find_peaks_refactor(0.1, g[f"map{i}"]), g[f"peaks{i}"].reshape(-1, 2)), i
    from posepaf._lib import PosePafError
    with pytest.raises(PosePafError):      # 4430 peaks in one channel: refused loudly, not silently truncated
        ps.find_peaks_refactor(0.1, g["map1"])
    # predict_refactor: model -> flip-averaged HWC maps == numpy expression of :82-103 on the model's own output
    from posepaf.fused_model import build_inference_model
    from posepaf.pipeline import preprocess_batch
    model = build_inference_model(torch_cuda.device("cuda", 0))
    img = np.random.default_rng(2).integers(0, 256, (100, 150, 3), dtype=np.uint8)
    h_, p_ = ps.predict_refactor(img, model, {"rotation_search": [0.0]}, {}, "x.jpg", flip_avg=True)
    assert h_.shape == (32, 48, 20) and p_.shape == (32, 48, 30) and h_.dtype == np.float32
    with torch_cuda.no_grad():
        out = model(preprocess_batch(torch_cuda.from_numpy(img).cuda()[None], True, torch_cuda.float16)).cpu().numpy()
    hh, pp = oracle.flip_average(out)
    assert np.allclose(h_, hh.transpose(1, 2, 0), atol=2e-2) and np.allclose(p_, pp.transpose(1, 2, 0), atol=2e-2)


@pytest.mark.parametrize("key", ["P2_s1_f16", "P6_s2_f32", "P15_s0_f16", "P30_s2_f32"])
def test_find_connections_find_humans_host_surface(torch_cuda, oracle, key):
    """utils.parse_skeletons.find_connections / find_humans (reference signatures, kernels inside) against the
    reference's own Python output (golden G3), in float64."""
    from posepaf import skeleton as sk
    from utils import parse_skeletons as ps
    net, g = load_scene(key)
    _, paf = oracle.flip_average(net)
    up = oracle.upsample4_hwc(paf)
    jl = g["joint_list"]
    all_peaks = [[tuple(float(v) for v in row[:4]) for row in jl[jl[:, 4] == k]] for k in range(18)]
    cfg = sk.default_test_cfg()
    connected, special = ps.find_connections(all_peaks, up, 512, cfg, np.array(sk.LIMB_PAIRS))
    assert np.array_equal(np.array([len(c) for c in connected], np.int32), g["py_n_connections"])
    persons, cand = ps.find_humans(connected, special, all_peaks, cfg, np.array(sk.LIMB_PAIRS))
    want = g["py_persons"]
    assert persons.shape == want.shape and cand.shape == (len(jl), 4)
    assert np.array_equal(persons[:, :, 0], want[:, :, 0])              # ids, totals, counts: exact
    assert np.allclose(persons[:, :, 1], want[:, :, 1], rtol=0, atol=1e-9)
    with pytest.raises(NotImplementedError):
        ps.find_connections(all_peaks, up, 512, dict(cfg, thre2=0.05), np.array(sk.LIMB_PAIRS))


def test_original_path_nms_and_centroid_modes(torch_cuda, oracle):
    """A10 pieces: 3x3 / >= NMS (util.keypoint_heatmap_nms) and refine_centroid, against the reference's own outputs
    (tests/golden/g4_util.npz) and the oracle."""
    import os
    from conftest import GOLDEN
    from posepaf.api import PosePostProcessor
    torch = torch_cuda
    g = np.load(os.path.join(GOLDEN, "g4_util.npz"))
    hm, kept = g["hm"], g["kept"]                       # (1,18,24,40) and the reference's masked output
    post = PosePostProcessor(max_batch=1, max_h=64, max_w=64, max_peaks_per_part=128)
    net = torch.zeros((1, 1, 50, 24, 40), dtype=torch.float32, device="cuda")
    net[0, 0, 30:48] = torch.from_numpy(hm[0]).cuda()
    jl = post.nms_ex(net, flip=False, nms_mode=1, threshold=0.1, refine_mode=3)[0]
    for ch in range(18):
        rows = jl[jl[:, 4] == ch]
        want_yx = np.argwhere(kept[0, ch] != 0)          # row-major, like np.nonzero
        assert np.array_equal(rows[:, :2].astype(int), want_yx[:, ::-1]), ch
        assert np.array_equal(rows[:, 2], hm[0, ch][want_yx[:, 0], want_yx[:, 1]])
    # refine_centroid: single-peak maps built around the golden anchors
    big = g["big"]
    for (x, y), want in zip(g["anchors"], g["refined"]):
        m = np.zeros((1, 1, 50, 30, 30), np.float32)
        m[0, 0, 30] = big * 1e-3                          # keep the box values' RATIOS; below threshold everywhere ...
        m[0, 0, 30, y, x] = 1.0                           # ... except the anchor, which becomes the only peak
        src = m[0, 0, 30].copy()
        got = post.nms_ex(torch.from_numpy(m).cuda(), flip=False, nms_mode=1, threshold=0.5, refine_mode=2)[0]
        assert len(got) == 1
        exp = oracle.refine_centroid(src, int(x), int(y), 2)
        assert np.allclose(got[0, :3], exp, rtol=1e-5, atol=1e-6), (x, y)
        # the reference's own refine_centroid on the same array (imported in make_golden.py for `big`; here via the
        # package's numpy restatement, which test_util_golden pins against the golden values)
        from utils.util import refine_centroid
        ref = refine_centroid(src, (int(x), int(y)), 2)
        assert np.allclose(got[0, :3], np.array(ref, np.float64), rtol=1e-5, atol=1e-6)
    post.close()


@pytest.mark.parametrize("key", scene_keys())
def test_python_twins_mode_against_reference_python(torch_cuda, post, oracle, key):
    """A8 on the GPU (pp_process_batch_py): person ids / counts identical to the reference's own Python
    find_connections + find_humans (golden G3) and to the oracle; totals within 1e-4 (float32 record field)."""
    torch = torch_cuda
    net, g = load_scene(key)
    rec = post.process_py(torch.from_numpy(net).cuda()[None], 512)[0]
    want = g["py_persons"]                                   # (P, 20, 2) float64 from the reference
    n = int(rec["n_humans"])
    assert n == len(want)
    assert np.array_equal(rec["humans"]["peak_id"][:n], want[:, :18, 0].astype(np.int32))
    assert np.array_equal(rec["humans"]["n_parts"][:n], want[:, 19, 0].astype(np.int32))
    assert np.allclose(rec["humans"]["score"][:n], want[:, 18, 0] / want[:, 19, 0], rtol=0, atol=SCORE_TOL)
    assert rec["status"] == 0
    assert np.array_equal(post.read_connection_counts(0), g["py_n_connections"])      # per limb, the reference's own Python
    assert rec["n_connections"] == int(g["py_n_connections"].sum())
    jl = g["joint_list"]
    for h_ in range(n):
        for p in range(18):
            pid = rec["humans"]["peak_id"][h_, p]
            if pid >= 0:
                assert rec["humans"]["x"][h_, p] == jl[pid, 0] and rec["humans"]["y"][h_, p] == jl[pid, 1]
                assert rec["humans"]["part_score"][h_, p] == jl[pid, 2]


@pytest.mark.parametrize("people,dtype", [(3, np.float16), (8, np.float32)])
def test_original_multiscale_path_against_oracle(torch_cuda, oracle, people, dtype):
    """A10 / config 5: three scales accumulated at image resolution (predict), find_peaks, Python twins on float64 maps.
    GPU vs the oracle's restatement: accumulators within 1e-6 (identical operation order: expected equal), peaks and
    persons identical in ids; fractional coordinates / scores within 1e-4."""
    from posepaf import synth
    from posepaf.api import PosePostProcessor
    from posepaf.original_path import OriginalPathProcessor, record_float_coords
    torch = torch_cuda
    IMG = 256                                             # image 256x256; scales 0.5, 1.0, 1.5 -> 128, 256, 384
    # scale 0.5: image 128 -> pad to 128 (32x32 map, no pad); 1.0: 256 (64x64); 1.5: 384 (96x96)
    sizes = [(32, 32, 0.5), (64, 64, 1.0), (96, 96, 1.5)]
    outs, _ = synth.make_scene_at_scales(people, 321 + people, sizes, dtype=dtype, img=IMG)
    post = PosePostProcessor(max_batch=2, max_h=96, max_w=96, max_peaks_per_part=64)
    proc = OriginalPathProcessor(post, IMG, IMG, 2)
    heat = np.zeros((20, IMG, IMG)); paf = np.zeros((30, IMG, IMG))
    proc.reset()
    for o, (h, w, sc) in zip(outs, sizes):
        both = np.stack([o, o])                           # batch of two identical images
        proc.accumulate(torch.from_numpy(both).cuda(), 0, 0, len(sizes))
        oracle.predict_accumulate(o, 0, 0, IMG, IMG, len(sizes), heat, paf)
    got_heat = proc.heat_acc.cpu().numpy()
    got_paf = proc.paf_acc.cpu().numpy()
    assert np.array_equal(got_heat[0], got_heat[1])
    assert np.allclose(got_heat[0], heat, rtol=0, atol=1e-6) and np.allclose(got_paf[0], paf, rtol=0, atol=1e-6)
    assert np.array_equal(got_heat[0], heat) and np.array_equal(got_paf[0], paf)
    from posepaf.api import records_to_numpy
    recs = records_to_numpy(proc.finish(2))
    rows = oracle.find_peaks_original(heat, 0.1)
    persons, ncn = oracle.py_find_humans_f64(rows, paf, IMG)
    for rec in recs:
        assert rec["status"] & 32                          # PP_ST_FLOAT_COORDS
        assert rec["n_peaks"] == len(rows)
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
    post.close()


def test_original_path_padding_crop_and_image_resize(torch_cuda, oracle):
    """scale whose padded size differs from the scaled size (crop :272-273) and the uint8 image resize kernel."""
    from posepaf import synth
    from posepaf.api import PosePostProcessor
    from posepaf.original_path import OriginalPathProcessor, resize_images_u8
    torch = torch_cuda
    img = np.random.default_rng(9).integers(0, 256, (2, 200, 264, 3), dtype=np.uint8)
    for scale in (0.5, 1.5):
        got = resize_images_u8(torch.from_numpy(img).cuda(), scale).cpu().numpy()
        for b in range(2):
            assert np.array_equal(got[b], oracle.resize_u8(img[b], scale, scale))
    # image 200x264 at scale 1: padded to 256x320 -> feature map 64x80, crop 56 rows / 56 cols of the x4 upsample
    net = synth.make_net_output(4, 55, h=64, w=80, dtype=np.float16)
    post = PosePostProcessor(max_batch=1, max_h=80, max_w=80, max_peaks_per_part=64)
    proc = OriginalPathProcessor(post, 200, 264, 1)
    proc.reset()
    proc.accumulate(torch.from_numpy(net).cuda()[None], 56, 56, 1)
    heat = np.zeros((20, 200, 264)); paf = np.zeros((30, 200, 264))
    oracle.predict_accumulate(net, 56, 56, 200, 264, 1, heat, paf)
    assert np.array_equal(proc.heat_acc.cpu().numpy()[0], heat) and np.array_equal(proc.paf_acc.cpu().numpy()[0], paf)
    post.close()


def test_capacity_flags_per_image_sizes_and_graph_capture(torch_cuda, oracle):
    """Edge cases of the native path: peak-capacity overflow is flagged (not silent), per-image min_img_size from a
    device array, a 128-peaks-per-part context, and hipGraph capture/replay of pp_process_batch."""
    from posepaf import synth
    from posepaf.api import PosePostProcessor, records_to_numpy
    torch = torch_cuda
    # (1) overflow: a tiny capacity on a 12-people scene
    net = synth.make_net_output(12, 3, dtype=np.float16)
    small = PosePostProcessor(max_batch=1, max_h=128, max_w=128, max_peaks_per_part=4)
    rec = small.process(torch.from_numpy(net).cuda()[None], 512)[0]
    assert rec["status"] & 1                     # PP_ST_PEAK_OVERFLOW
    with pytest.raises(Exception):
        small.read_peaks(0)                      # truncated joint list is refused loudly
    small.close()
    # (2) per-image min_img_size (device array) == separate runs with scalar sizes
    post = PosePostProcessor(max_batch=4, max_h=128, max_w=128, max_peaks_per_part=128)
    nets = np.stack([synth.make_net_output(6, 60 + i, dtype=np.float16) for i in range(4)])
    dev = torch.from_numpy(nets).cuda()
    sizes = [512, 256, 128, 64]
    mis = torch.tensor(sizes, dtype=torch.int32, device="cuda")
    recs = records_to_numpy(post.process_async(dev, 999, True, min_img_size_dev=mis))
    for i, s in enumerate(sizes):
        want = oracle.pipeline(nets[i], s)
        n = int(recs[i]["n_humans"])
        assert n == len(want["ids"]) and np.array_equal(recs[i]["humans"]["peak_id"][:n], want["ids"])
        assert np.array_equal(recs[i]["humans"]["score"][:n], want["scores"])
    # (3) capture into a HIP graph and replay on new data
    static_in = dev.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        post.process_async(static_in, 512, True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = post.process_async(static_in, 512, True)
    other = np.stack([synth.make_net_output(5, 90 + i, dtype=np.float16) for i in range(4)])
    static_in.copy_(torch.from_numpy(other).cuda())
    g.replay()
    got = records_to_numpy(out)
    for i in range(4):
        want = oracle.pipeline(other[i], 512)
        n = int(got[i]["n_humans"])
        assert n == len(want["ids"]) and np.array_equal(got[i]["humans"]["peak_id"][:n], want["ids"])
    post.close()


def test_python_twin_mode_batched_and_fp32(torch_cuda, oracle):
    from posepaf import synth
    from posepaf.api import PosePostProcessor
    torch = torch_cuda
    post = PosePostProcessor(max_batch=3, max_h=128, max_w=128, max_peaks_per_part=64)
    nets = [synth.make_net_output(p, 700 + p, dtype=np.float32) for p in (2, 9, 17)]
    recs = post.process_py(torch.from_numpy(np.stack(nets)).cuda(), 512)
    for net, rec in zip(nets, recs):
        heat, paf = oracle.flip_average(net)
        jl, _ = oracle.heatmap_nms(heat)
        persons, ncn = oracle.py_find_humans(jl, oracle.upsample4_hwc(paf), 512)
        n = int(rec["n_humans"])
        assert n == len(persons) and rec["n_connections"] == int(ncn.sum())
        assert np.array_equal(rec["humans"]["peak_id"][:n], persons[:, :18, 0].astype(np.int32))
        assert np.allclose(rec["humans"]["score"][:n], persons[:, 18, 0] / persons[:, 19, 0], rtol=0, atol=SCORE_TOL)
    post.close()


def test_status_words_after_graph_replay_at_bench_batch(torch_cuda, oracle):
    """Round-1 defect: pp_record.status carried garbage (bits outside include/posepaf.h:53-59) on the HIP-graph replay path
    at 64 images per batch.  The status protocol no longer has a memset node or atomics (every workgroup plainly stores its
    own flag word on every launch, the assembly ORs them).  Capture pp_process_batch at B = 64, replay it repeatedly on
    fresh inputs with other work in flight, and require every record -- header fields and people -- to equal the eager run,
    every status word to be 0 or PP_ST_SORT_UNDEFINED exactly where the oracle sees it, and every raw flag word to be clean."""
    from posepaf import synth
    from posepaf.api import PosePostProcessor, records_to_numpy, check_status
    torch = torch_cuda
    B = 64
    people = (1, 2, 3, 4, 5, 6, 8, 10, 12, 15, 20, 30, 2, 4, 6, 3)                  # bench.py's mix
    post = PosePostProcessor(max_batch=B, max_h=128, max_w=128, max_peaks_per_part=64)
    sets = [np.stack([synth.make_net_output(people[(i + k) % 16], 9000 + (i + 5 * k) % 16, dtype=np.float16) for i in range(B)])
            for k in range(3)]
    eager = [post.process(torch.from_numpy(s).cuda(), 512).copy() for s in sets]
    for r in eager:
        check_status(r, allow=8, what="eager run")
    static_in = torch.from_numpy(sets[0]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        post.process_async(static_in, 512, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = post.process_async(static_in, 512, True)
    filler = torch.randn(4096, 4096, device="cuda", dtype=torch.float16)
    for rep in range(12):
        k = rep % 3
        static_in.copy_(torch.from_numpy(sets[k]).cuda(), non_blocking=True)
        _ = filler @ filler                          # unrelated kernels queued around the replay
        g.replay()
        _ = filler @ filler
        got = records_to_numpy(out)
        check_status(got, allow=8, what=f"graph replay {rep}")
        for i in range(B):
            assert _same_record(got[i], eager[k][i]), (rep, i, hex(int(got[i]["status"])), hex(int(eager[k][i]["status"])))
        for i in (0, 11, 63):
            assert (post.debug_read_flags(i) & ~np.uint32(0x3F) == 0).all()
    for i in (3, 11, 40):                                     # and the eager run itself is the oracle's answer
        want = oracle.pipeline(sets[0][i], 512)
        assert bool(eager[0][i]["status"] & 8) == bool(want["sort_oob"])
        if not want["sort_oob"]:
            _records_vs_oracle(eager[0][i], want, f"bench-mix image {i}")
    post.close()


def test_fused_scale_accumulation_equals_the_per_scale_chain(torch_cuda):
    """pp_original_accumulate_all (one launch, accumulators written once) against n calls of pp_original_accumulate (x4 map in
    HBM, read-modify-write per scale): bit-identical float64 accumulators -- ragged image size (tiles cut at the border),
    padded inputs (crop), a down-scaling, an identity and an up-scaling resize, fp16 and fp32 maps, flip on and off."""
    from posepaf import synth
    from posepaf.api import PosePostProcessor
    from posepaf.original_path import OriginalPathProcessor
    torch = torch_cuda
    H, W = 200, 264                                       # image; scales 0.5 / 1.0 / 1.5 -> 100x132, 200x264, 300x396
    sizes = [(32, 48, 0.5), (64, 80, 1.0), (80, 112, 1.5)]   # maps of the inputs padded to /64: 128x192, 256x320, 320x448
    pads = [(128 - 100, 192 - 132), (256 - 200, 320 - 264), (320 - 300, 448 - 396)]
    post = PosePostProcessor(max_batch=2, max_h=80, max_w=112, max_peaks_per_part=64)
    for dtype in (np.float16, np.float32):
        for flip in (True, False):
            g = np.random.default_rng(7)
            maps = [torch.from_numpy((g.random((2, 2 if flip else 1, 50, h, w)) * 0.8).astype(dtype)).cuda() for h, w, _ in sizes]
            res = []
            for fused in (True, False):
                proc = OriginalPathProcessor(post, H, W, 2)
                proc.fused = fused
                proc.reset()
                for m, (pd, pr) in zip(maps, pads):
                    proc.accumulate(m, pd, pr, len(sizes), flip=flip)
                res.append((proc.heat_acc.clone(), proc.paf_acc.clone()))
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), (dtype, flip)
            assert float(res[0][1].abs().max()) > 0.1
    post.close()


def test_launch_structures_give_identical_records(torch_cuda):
    """include/posepaf.h pp_debug_set_mode: "results are identical in every mode" -- 0 = assembly fused into the limb kernel's
    last workgroup per image with load-ordered dispatch (the hand-rolled publish protocol: write-through stores, ticket,
    acquire), 1 = assembly as its own launch (plain kernel boundary), 2 = fused without the ordering.  Eager and HIP-graph
    replay, bench mix at B = 64: every record byte must agree across the three."""
    from posepaf import synth
    from posepaf.api import PosePostProcessor
    torch = torch_cuda
    B = 64
    people = (1, 2, 3, 4, 5, 6, 8, 10, 12, 15, 20, 30, 2, 4, 6, 3)
    post = PosePostProcessor(max_batch=B, max_h=128, max_w=128, max_peaks_per_part=64)
    nets = torch.from_numpy(np.stack([synth.make_net_output(people[i % 16], 9000 + i % 16, dtype=np.float16) for i in range(B)])).cuda()
    ref = None
    for mode in (1, 0, 2):
        post.set_mode(mode)
        eager = post.process_async(nets, 512, True).cpu().numpy().copy()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            post.process_async(nets, 512, True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = post.process_async(nets, 512, True)
        for _ in range(3):
            g.replay()
        replay = out.cpu().numpy().copy()
        assert np.array_equal(eager, replay), f"mode {mode}: eager != graph replay"
        if ref is None:
            ref = eager
        assert np.array_equal(ref, eager), f"mode {mode} differs from the separate-launch structure"
    post.set_mode(0)
    post.close()


@pytest.mark.parametrize("shape", [(125, 131), (127, 129), (33, 47)])
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_odd_map_sizes_with_ragged_mask_tail(torch_cuda, oracle, shape, dtype):
    """Map sizes whose pixel count is not a multiple of 8 (and rows that are not multiples of 8): the peak kernel's mask bytes
    then end in a partial group.  125 x 131 gives 2047 mask bytes = 8 per thread with a ragged last thread, the case the
    one-word fast path of round 1 silently dropped.  Peaks are planted in the very last pixels."""
    from posepaf import synth
    from posepaf.api import PosePostProcessor
    torch = torch_cuda
    h, w = shape
    post = PosePostProcessor(max_batch=2, max_h=h, max_w=w, max_peaks_per_part=64)
    nets = np.stack([synth.make_net_output(p, 500 + p, h=h, w=w, dtype=dtype, flip=False) for p in (3, 6)]).astype(np.float32)
    for c in range(30, 48):
        nets[:, 0, c, h - 1, w - 1] = 0.9             # last pixel of the map
        nets[:, 0, c, h - 1, w - 4] = 0.8             # inside the last partial 8-pixel group
        nets[:, 0, c, h - 3, w - 2] = 0.7
    nets = nets.astype(dtype)
    lists = post.nms(torch.from_numpy(nets).cuda(), flip=False, refine=True)
    for i in range(2):
        heat, _ = oracle.flip_average(nets[i], flip=False)
        want, _ = oracle.heatmap_nms(heat, 4, refine=True)
        assert np.array_equal(lists[i], want), (shape, i)
        last = want[(want[:, 0] >= 4 * (w - 1)) & (want[:, 1] >= 4 * (h - 1))]
        assert len(last) >= 18                        # the corner peaks are in the expected list, so they were checked
    recs = post.process(torch.from_numpy(nets).cuda(), 4 * h, flip=False)
    for i in range(2):
        want = oracle.pipeline(nets[i], 4 * h, flip=False)
        if not want["sort_oob"]:
            _records_vs_oracle(recs[i], want, f"{shape} image {i}")
    post.close()


def test_config5_multiscale_full_size_properties(torch_cuda):
    """BASELINE configs[4] at its real size (512 x 512 image, scales 0.5 / 1.0 / 1.5 -> 64 / 128 / 192 maps, flip on): too
    slow for the per-image oracle, so size-independent properties: determinism (two passes give bit-identical float64
    accumulators and records) and batching invariance (image i of a batch of two == the same image alone)."""
    from posepaf import synth
    from posepaf.api import PosePostProcessor, records_to_numpy, check_status
    from posepaf.original_path import OriginalPathProcessor
    torch = torch_cuda
    IMG = 512
    sizes = [(64, 64, 0.5), (128, 128, 1.0), (192, 192, 1.5)]
    scenes = [synth.make_scene_at_scales(p, 4000 + p, sizes, dtype=np.float16, img=IMG)[0] for p in (4, 11)]
    post = PosePostProcessor(max_batch=2, max_h=192, max_w=192, max_peaks_per_part=64)
    proc = OriginalPathProcessor(post, IMG, IMG, 2)

    def run(idx):
        proc.reset()
        for k in range(len(sizes)):
            maps = torch.from_numpy(np.stack([scenes[i][k] for i in idx])).cuda()
            proc.accumulate(maps, 0, 0, len(sizes))
        rec = records_to_numpy(proc.finish(len(idx))).copy()
        return rec, proc.heat_acc[: len(idx)].clone(), proc.paf_acc[: len(idx)].clone()

    r1, h1, p1 = run([0, 1])
    r2, h2, p2 = run([0, 1])
    assert torch.equal(h1, h2) and torch.equal(p1, p2)
    check_status(r1, allow=32, what="multi-scale records")              # PP_ST_FLOAT_COORDS only
    assert all(int(r["status"]) == 32 for r in r1)
    assert all(_same_record(r1[i], r2[i]) for i in range(2))
    assert r1[0]["n_humans"] >= 3 and r1[1]["n_humans"] >= 8            # the injected people are found
    for i in range(2):
        ra, ha, pa = run([i])
        assert torch.equal(ha[0], h1[i]) and torch.equal(pa[0], p1[i])
        assert _same_record(ra[0], r1[i]), i
    post.close()


def test_config2_forward_plus_nms_batch1_at_512(torch_cuda, oracle):
    """BASELINE configs[1]: one 512 x 512 image, IMHN forward on the GPU, HIP flip-average + NMS + refinement of the 18
    keypoint channels.  The peak list must be exactly what the oracle extracts from the SAME network output (a random
    network emits no peaks, so a synthetic scene is added to its output, as bench.py does)."""
    from posepaf import synth
    from posepaf.api import PosePostProcessor
    from posepaf.fused_model import build_inference_model
    from posepaf.pipeline import PosePipeline
    torch = torch_cuda
    post = PosePostProcessor(max_batch=1, max_h=128, max_w=128, max_peaks_per_part=64)
    model = build_inference_model(torch.device("cuda", 0))
    pipe = PosePipeline(model, post)
    img = torch.from_numpy(np.random.default_rng(12).integers(0, 256, (1, 512, 512, 3), dtype=np.uint8)).cuda()
    maps = pipe.forward_maps(img)
    assert maps.shape == (1, 2, 50, 128, 128) and torch.isfinite(maps).all()
    inject = torch.from_numpy(synth.make_net_output(7, 321, dtype=np.float16)).cuda()[None]
    amp = maps.float().abs().max().item()           # random weights: O(1) ripple, no structure
    maps = torch.addcmul(inject, maps, torch.tensor(0.02 / amp, dtype=torch.float16, device="cuda")).contiguous()   # ripple <= 0.02
    for refine in (True, False):
        got = post.nms(maps, flip=True, refine=refine)[0]
        heat, _ = oracle.flip_average(maps[0].cpu().numpy())
        want, _ = oracle.heatmap_nms(heat, 4, refine=refine)
        assert len(want) > 50
        assert np.array_equal(got, want)
    post.close()


def test_fp16_fused_forward_and_fp32_module_find_the_same_people(torch_cuda):
    """Scene-level check of the fp16 forward: the SAME image through the fused fp16 model and through the checkpoint-
    compatible fp32 nn.Module, each output scaled to an amplitude of 0.05 (below the peak threshold) and added to the same clean synthetic scene, then the
    full HIP post-processing.  The two runs must find the same people: equal counts, equal part sets per person, joint
    coordinates within one feature-map cell (4 px; the x4 refinement arg-max may move by a pixel under fp16 noise)."""
    from config.config import GetConfig, TrainingOpt
    from models.posenet import NetworkEval
    from posepaf import synth
    from posepaf.api import PosePostProcessor
    from posepaf.fused_model import FusedIMHN
    from posepaf.model_init import deterministic_init
    from posepaf.pipeline import preprocess_batch
    torch = torch_cuda
    net = NetworkEval(TrainingOpt(), GetConfig("Canonical"), bn=True).eval()
    deterministic_init(net, 7)
    img = torch.from_numpy(np.random.default_rng(21).integers(0, 256, (1, 256, 256, 3), dtype=np.uint8)).cuda()
    with torch.no_grad():
        x32 = preprocess_batch(img, True, torch.float32)
        out32 = net.cuda()(x32)[-1][0].float()
        fused = FusedIMHN.from_network(net).eval().cuda().half().to(memory_format=torch.channels_last)
        out16 = fused(preprocess_batch(img, True, torch.float16)).float()
    amp = out32.abs().max().item()
    assert amp > 0.0
    k = 0.05 / amp                    # the network's own ripple scaled to 0.05: below the 0.1 peak threshold, no spurious peaks
    out32, out16 = out32 * k, out16 * k
    post = PosePostProcessor(max_batch=1, max_h=64, max_w=64, max_peaks_per_part=64)
    people = 0
    for seed in (1, 2, 3):
        scene = torch.from_numpy(synth.make_net_output(5, 800 + seed, h=64, w=64, noise=0.0, dtype=np.float32)).cuda()
        recs = []
        for out in (out32, out16):
            maps = (scene + out.view(2, 50, 64, 64)).half().contiguous()[None]
            recs.append(post.process(maps, 256)[0])
        a, b = recs
        assert a["status"] == 0 and b["status"] == 0
        n = int(a["n_humans"])
        assert n == int(b["n_humans"]) and n >= 3
        ha, hb = a["humans"][:n], b["humans"][:n]
        assert np.array_equal(ha["peak_id"] >= 0, hb["peak_id"] >= 0)
        m = ha["peak_id"] >= 0
        assert (np.abs(ha["x"][m] - hb["x"][m]) <= 4).all() and (np.abs(ha["y"][m] - hb["y"][m]) <= 4).all()
        assert np.allclose(ha["score"], hb["score"], rtol=0, atol=0.02)
        people += n
    assert people >= 10
    post.close()


def test_reference_named_original_path_functions(torch_cuda, oracle):
    """utils.parse_skeletons.predict / find_peaks (reference :180-283, :286-321) as an evaluate.py:81-84-style caller uses
    them: predict's float64 image-resolution maps equal the oracle's accumulation of the SAME network output; find_peaks'
    (x, y, score, id) rows equal the oracle's find_peaks restatement (itself pinned to the reference's keypoint_heatmap_nms /
    refine_centroid outputs, golden G4) on a synthetic scene; ids run across parts."""
    from posepaf import skeleton as sk, synth
    from posepaf.fused_model import build_inference_model
    from posepaf.pipeline import preprocess_batch
    from utils import parse_skeletons as ps
    torch = torch_cuda
    cfg = sk.default_test_cfg()
    model = build_inference_model(torch.device("cuda", 0))
    img = np.random.default_rng(4).integers(0, 256, (120, 200, 3), dtype=np.uint8)      # padded to 128 x 256 -> maps 32 x 64
    heat, paf = ps.predict(img, model, cfg, sk.default_model_cfg(), "x.jpg", flip_avg=True)
    assert heat.shape == (120, 200, 20) and paf.shape == (120, 200, 30) and heat.dtype == np.float64
    with torch.no_grad():
        out = model(preprocess_batch(torch.from_numpy(img).cuda()[None], True, torch.float16)).cpu().numpy()
    h0 = np.zeros((20, 120, 200)); p0 = np.zeros((30, 120, 200))
    oracle.predict_accumulate(out, 8, 56, 120, 200, 1, h0, p0)
    assert np.allclose(heat, h0.transpose(1, 2, 0), rtol=0, atol=2e-2) and np.allclose(paf, p0.transpose(1, 2, 0), rtol=0, atol=2e-2)
    # find_peaks on an image-resolution scene
    net = synth.make_net_output(6, 31, h=64, w=64, dtype=np.float32)
    hs = np.zeros((20, 256, 256)); pfs = np.zeros((30, 256, 256))
    oracle.predict_accumulate(net, 0, 0, 256, 256, 1, hs, pfs)
    got = ps.find_peaks(np.ascontiguousarray(hs.transpose(1, 2, 0)), cfg)
    rows = oracle.find_peaks_original(hs, 0.1)
    assert len(got) == 18 and sum(len(g) for g in got) == len(rows) > 30
    flat = np.array([r for part in got for r in part], np.float64).reshape(-1, 4)
    assert np.allclose(flat[:, :2], rows[:, :2], rtol=0, atol=1e-9)
    # score = box.mean() of a float32 box: a float32 reduction in NumPy; the kernel rounds the float64 mean to float32, the
    # oracle keeps the float64 mean (oracle/posepaf_oracle.c:843-845): equal to float32 rounding, tolerance 1e-6
    assert np.allclose(flat[:, 2], rows[:, 2], rtol=0, atol=1e-6)
    assert np.array_equal(flat[:, 3], np.arange(len(rows)))
    parts = np.concatenate([[k] * len(g) for k, g in enumerate(got)])
    assert np.array_equal(parts, rows[:, 4].astype(int))
    # the whole evaluate.py:81-89 chain on the reference-named functions
    all_peaks = ps.find_peaks(np.ascontiguousarray(hs.transpose(1, 2, 0)), cfg)
    connected, special = ps.find_connections(all_peaks, np.ascontiguousarray(pfs.transpose(1, 2, 0)).astype(np.float32), 256, cfg,
                                             np.array(sk.LIMB_PAIRS))
    persons, cand = ps.find_humans(connected, special, all_peaks, cfg, np.array(sk.LIMB_PAIRS))
    assert persons.shape[1:] == (20, 2) and len(persons) >= 4 and cand.shape == (len(rows), 4)
