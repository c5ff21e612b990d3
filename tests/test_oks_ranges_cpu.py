"""CPU: oks_eval.evaluate_keypoints_ranges -- the host specification of the device evaluation -- against evaluate_keypoints
(range `all`, exact) and against hand-computed range cases.  pycocotools is absent: parity with it stays unpinned."""
import numpy as np

import ap_cases

ALL_KEYS = ("AP", "AP50", "AP75", "AR", "n_gt", "n_dt")
TWELVE = ("AP", "AP50", "AP75", "APm", "APl", "AR", "AR50", "AR75", "ARm", "ARl", "n_gt", "n_dt")


def same(a, b):
    return a == b or (a != a and b != b)


def assert_all_range_equal(gts, dts):
    from posepaf import oks_eval as oe
    want, got = oe.evaluate_keypoints(gts, dts), oe.evaluate_keypoints_ranges(gts, dts)
    assert tuple(got) == TWELVE
    for k in ALL_KEYS:
        assert same(got[k], want[k]), (k, got[k], want[k])
    return got


def test_range_all_equals_evaluate_keypoints_on_seeded_and_hand_cases():
    for cases in (ap_cases.seeded_cases(), ap_cases.hand_cases()):
        _, gts, dts = cases
        got = assert_all_range_equal(gts, dts)
        assert got["n_dt"] > 0 and got["n_gt"] > 0
    # the seeded cases exercise what they are for: the cut at 20, every range, crowd and unlabelled ground truth
    recs, gts, dts = ap_cases.seeded_cases()
    assert max(len(d) for d in dts.values()) > 20 and min(len(d) for d in dts.values()) == 0
    assert any(len(g) == 0 for g in gts.values()) and max(len(g) for g in gts.values()) == 8
    flat = [x for g in gts.values() for x in g]
    assert any(x["iscrowd"] for x in flat) and any(x["num_keypoints"] == 0 for x in flat)
    assert any(x["area"] < 32 ** 2 for x in flat) and any(32 ** 2 < x["area"] < 96 ** 2 for x in flat) and any(x["area"] > 96 ** 2 for x in flat)
    got = [ap_cases.stage_a("seeded")[i]["match"] for i in range(len(recs))]
    flags = np.concatenate(got, axis=2)
    assert all((flags[r] == v).any() for r in range(3) for v in (1, 0, -1))


def test_range_all_equals_evaluate_keypoints_on_the_inputs_of_test_oks_eval():
    from test_oks_eval import _gt
    gts = {1: [_gt(), _gt(300, 200)], 2: [_gt(50, 50)]}
    perfect = {k: [{"keypoints": g["keypoints"], "score": 0.9 - 0.1 * i} for i, g in enumerate(v)] for k, v in gts.items()}
    r = assert_all_range_equal(gts, perfect)
    assert abs(r["AP"] - 1.0) < 1e-9 and r["AR50"] == 1.0 and r["AR75"] == 1.0
    assert_all_range_equal(gts, {1: perfect[1], 2: []})
    assert_all_range_equal(gts, {1: perfect[1] + [{"keypoints": _gt(400, 400)["keypoints"], "score": 0.99}], 2: perfect[2]})
    assert_all_range_equal(gts, {})
    assert_all_range_equal({}, perfect)
    real, crowd = _gt(), dict(_gt(300, 300), iscrowd=1)
    dts = {1: [{"keypoints": real["keypoints"], "score": 0.9},
               {"keypoints": crowd["keypoints"], "score": 0.8}, {"keypoints": crowd["keypoints"], "score": 0.7}]}
    assert_all_range_equal({1: [crowd, real]}, dts)
    far = _gt(600, 600)["keypoints"]
    assert_all_range_equal({1: [real]}, {1: [dts[1][0], {"keypoints": far, "score": 0.8}]})
    assert_all_range_equal({1: [real]}, {1: [{"keypoints": real["keypoints"], "score": 0.5}, {"keypoints": far, "score": 0.8}]})
    blank = dict(_gt(300, 300), num_keypoints=0)
    kp = np.asarray(blank["keypoints"]).reshape(17, 3).copy()
    kp[:, 2] = 0
    blank["keypoints"] = kp.reshape(-1).tolist()
    d_in = np.asarray(_gt(300, 300)["keypoints"]).reshape(17, 3)
    assert_all_range_equal({1: [real, blank]}, {1: [dts[1][0], {"keypoints": d_in.reshape(-1).tolist(), "score": 0.99}]})
    many = {1: [{"keypoints": far, "score": 0.9 - 0.01 * i} for i in range(20)] + [{"keypoints": real["keypoints"], "score": 0.1}]}
    assert_all_range_equal({1: [real]}, many)
    d = np.asarray(real["keypoints"]).reshape(17, 3).copy()
    d[:, 0] += 10
    for area in (200.0, 1e6):
        assert_all_range_equal({1: [dict(real, area=area)]}, {1: [{"keypoints": d.reshape(-1).tolist(), "score": 1.0}]})


def test_hand_computed_range_cases():
    from posepaf import oks_eval as oe
    recs, gts, dts = ap_cases.hand_cases()
    A = ap_cases.stage_a("hand")
    # image 6: ground truths of area exactly 32^2 and exactly 96^2 -- both ends belong to a range
    m = A[6]
    assert m["n_gt"].tolist() == [2, 2, 1]                          # 32^2: all + medium;  96^2: all + medium + large
    assert m["order"].tolist() == [0, 1, 2]
    assert oe.detection_area(dts[6][2]["keypoints"]) == 32.0 * 16.0 and oe.detection_area(dts[6][0]["keypoints"]) == 96.0 * 48.0
    # detection 0 -> the 32^2 person: counted in all / medium, that person is ignored in large
    # detection 1 (area 4608, outside large) -> the 96^2 person, who counts in large: a matched detection outside the range counts
    # detection 2 (area 512) matches nobody: false positive in `all`, outside medium and large -> ignored there
    for ti in range(10):
        assert m["match"][:, ti, :].tolist() == [[1, 1, 0], [1, 1, -1], [-1, 1, -1]]
    r = oe.evaluate_keypoints_ranges({6: gts[6]}, {6: dts[6]})
    assert r["n_gt"] == 2 and r["n_dt"] == 3 and r["ARl"] == 1.0 and r["ARm"] == 1.0
    assert all(abs(r[k] - 1.0) < 1e-9 for k in ("AP", "APm", "APl"))
    # image 4: detections and no ground truth: everything is a false positive in `all`; the 32 x 16 one is outside medium / large,
    # the 96 x 48 one is outside large only
    m = A[4]
    assert m["n_gt"].tolist() == [0, 0, 0] and m["oks"].shape == (2, 0)
    assert m["match"][:, 0, :].tolist() == [[0, 0], [0, -1], [-1, -1]]
    r = oe.evaluate_keypoints_ranges({}, {4: dts[4]})
    assert r["AP"] != r["AP"] and r["APm"] != r["APm"] and r["AP50"] == 0.0 and r["AR"] == 0.0 and r["n_dt"] == 2 and r["n_gt"] == 0
    # image 5: ground truth and no detection
    m = A[5]
    assert m["n_gt"].tolist() == [1, 1, 0] and m["match"].shape == (3, 10, 0) and len(m["scores"]) == 0
    r = oe.evaluate_keypoints_ranges({5: gts[5]}, {})
    assert r["AP"] == 0.0 and r["APm"] == 0.0 and r["APl"] != r["APl"] and r["AR"] == 0.0 and r["n_gt"] == 1 and r["n_dt"] == 0
    # image 0: equal scores keep record order
    assert A[0]["order"].tolist() == [3, 0, 1, 2] and A[0]["match"][0, 0].tolist() == [1, 0, 0, 0]
    # image 1: the crowd region absorbs three detections (ignored), the real person is found
    assert A[1]["match"][0, 0].tolist() == [-1, -1, -1, 1] and A[1]["n_gt"].tolist() == [1, 1, 0]
    # image 2: inside the doubled box OKS is 1 (ignored match), far outside 0 (false positive); without a box OKS is 0
    assert A[2]["oks"][0, :2].tolist() == [1.0, 0.0] and A[2]["oks"][0, 2] < 1e-6 and A[2]["oks"][1, 0] < 1e-6
    assert A[2]["match"][0, 0].tolist() == [-1, 0, 1]
    # image 3: 26 detections on 128 ground truths: the 20 best are kept, every one finds its own person
    assert A[3]["order"].tolist() == list(range(20)) and (A[3]["match"][0] == 1).all() and A[3]["n_gt"][0] == 128


def test_seeded_cases_keep_a_margin_to_every_decision():
    """The condition under which the device flags must equal the host's EXACTLY although the device's exp and summation order
    may differ in the last bits: every OKS value is further than 1e-9 from every threshold and from 1 - 1e-10, and two ground
    truths that compete for a detection are further than 1e-9 apart.  Two ground truths compete when both can be taken at
    some threshold, i.e. both reach the lowest start value 0.5 (a value below 0.5 - 1e-9 is never taken, whatever its rival)."""
    from posepaf import oks_eval as oe
    recs, gts, dts = ap_cases.seeded_cases()
    marks = np.concatenate([oe.OKS_THRESHOLDS, [1 - 1e-10]])
    n_values = n_pairs = 0
    for i, m in enumerate(ap_cases.stage_a("seeded")):
        oks = m["oks"]
        assert oks.shape == (min(len(dts[i]), 20), len(gts[i]))
        if oks.size == 0:
            continue
        n_values += oks.size
        assert np.abs(oks[:, :, None] - marks[None, None, :]).min() > ap_cases.MARGIN, i
        for row in oks:
            live = np.sort(row[row >= 0.5 - ap_cases.MARGIN])
            n_pairs += max(len(live) - 1, 0)
            assert len(live) < 2 or np.diff(live).min() > ap_cases.MARGIN, (i, live)
    assert n_values > 1000 and n_pairs > 20


def test_vectorised_stage_b_takes_images_in_image_id_order():
    """scores tie across images: the stable sort keeps image-id order, as evaluate_keypoints' loop over sorted ids does"""
    from posepaf import oks_eval as oe
    from test_oks_eval import _gt
    real = _gt()
    far = _gt(600, 600)["keypoints"]
    gts = {7: [real], 3: [real]}
    dts = {7: [{"keypoints": real["keypoints"], "score": 0.5}], 3: [{"keypoints": far, "score": 0.5}]}
    r = assert_all_range_equal(gts, dts)
    assert abs(r["AP50"] - 0.5 * 51 / 101) < 1e-12      # the false positive of image 3 comes first: precision 1/2 up to recall 1/2
