"""CPU: the restatement of the COCO person-mask contract (tests/coco_mask_reference.py) against properties
that follow from the statement, the packer's refusals, make_mask's combination and the choice of training instances against the
reference's own (tests/golden/coco_instances.*, made by tests/golden/make_golden_coco.py), and finetune.py's new refusals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import coco_mask_cases as cases
import coco_mask_reference as cr
from conftest import GOLDEN, PKG
from posepaf import coco_masks
from posepaf import skeleton as sk
from posepaf._lib import PosePafError


def test_an_integer_rectangle_fills_its_half_open_box():
    assert np.array_equal(np.argwhere(cr.ring_mask([1, 1, 4, 1, 4, 4, 1, 4], 6, 7)), [[y, x] for y in (1, 2, 3) for x in (1, 2, 3)])
    for (x0, y0, x1, y1) in ((0, 0, 9, 5), (2, 3, 7, 4), (3, 0, 4, 5)):
        want = np.zeros((5, 9), np.uint8)
        want[y0:y1, x0:x1] = 1
        for ring in ([x0, y0, x1, y0, x1, y1, x0, y1], [x0, y0, x0, y1, x1, y1, x1, y0]):          # both directions of travel
            assert np.array_equal(cr.ring_mask(ring, 5, 9), want)


def test_a_ring_around_the_frame_fills_it():
    assert cr.ring_mask([-3, -2, 20, -2, 20, 15, -3, 15], 11, 13).sum() == 11 * 13
    assert cr.ring_mask([-30.5, -20.25, 200, -2, 180.5, 150, -3, 15], 11, 13).sum() == 11 * 13


def random_ring(rng, it, h, w):
    k = int(rng.integers(3, 12))
    if it % 4 == 0:
        return rng.uniform(-0.3, 1.3, (k, 2)) * (w, h)
    if it % 4 == 1:
        return np.round(rng.uniform(-0.3, 1.3, (k, 2)) * (w, h))                                   # integer vertices, repeated ones
    if it % 4 == 2:
        return np.round(rng.uniform(-0.3, 1.3, (k, 2)) * (w, h) * 5) / 5                           # on rleFrPoly's own grid
    return rng.uniform(-2.0, 3.0, (k, 2)) * (w, h)                                                 # mostly out of frame


def test_linear_column_and_run_forms_agree_on_random_rings():
    rng = np.random.default_rng(1)
    filled = 0
    for it in range(1000):
        h, w = int(rng.integers(1, 60)), int(rng.integers(1, 90))
        ring = random_ring(rng, it, h, w)
        linear = cr.ring_mask(ring, h, w)
        columns, even = cr.ring_mask_columns(ring, h, w)
        assert even, (it, "a column with an odd number of events")
        assert np.array_equal(linear, columns), it
        assert np.array_equal(linear, cr.ring_mask_runs(ring, h, w)), it
        filled += int(linear.any())
    assert filled > 600


def test_zero_length_edges_and_a_repeated_closing_vertex_change_nothing():
    ring = [10.3, 5.7, 60.2, 12.9, 31.4, 50.1]
    want = cr.ring_mask(ring, 64, 70)
    assert want.sum() > 500
    assert np.array_equal(cr.ring_mask(ring + ring[:2], 64, 70), want)                             # closed explicitly
    assert np.array_equal(cr.ring_mask(ring[:2] + ring[:2] + ring[2:4] + ring[2:4] + ring[2:4] + ring[4:], 64, 70), want)
    assert cr.ring_mask([20, 60, 50, 60, 35, 60], 64, 70).sum() == 0 and cr.ring_mask([9.2, 3.2] * 3, 64, 70).sum() == 0


def test_the_rings_of_one_annotation_are_ored():
    a, b = [20, 30, 50, 30, 50, 55, 20, 55], [35.5, 40.5, 80.5, 40.5, 80.5, 68.5, 35.5, 68.5]
    both = cr.ann_mask(cases.person([a, b], 1), 70, 150)
    assert np.array_equal(both, cr.ring_mask(a, 70, 150) | cr.ring_mask(b, 70, 150))
    assert both.sum() < cr.ring_mask(a, 70, 150).sum() + cr.ring_mask(b, 70, 150).sum()            # they overlap: OR, not XOR or sum


def test_the_crowd_loses_only_what_earlier_persons_cover():
    h, w = 40, 50
    p, c = cases.person([[10, 10, 30, 10, 30, 30, 10, 30]], 5), cases.crowd(h, w, 20, 38, 20, 45)
    miss_after, all_after = cr.make_mask([p, c], h, w)           # the person first: the overlap leaves the crowd and comes back through all
    miss_before, all_before = cr.make_mask([c, p], h, w)
    assert np.array_equal(all_after, all_before)                 # mask_all is an OR either way ...
    assert not np.array_equal(miss_after, miss_before)           # ... mask_miss is not: the overlap is masked only with the crowd first
    assert (miss_after[20:30, 20:30] == 255).all() and (miss_before[20:30, 20:30] == 0).all()
    # a later person WITHOUT keypoints in front of the crowd: order changes mask_all's source, a crowd between two persons both ways
    q = cases.person([[25, 25, 48, 25, 48, 39, 25, 39]], 0)
    for order in ([p, c, q], [q, c, p], [p, q, c]):
        masks = [cr.ann_mask(a, h, w) for a in order]
        miss, all_ = cr.combine(order, masks, h, w)
        crowd_at = [i for i, a in enumerate(order) if a["iscrowd"]][0]
        before = np.zeros((h, w), np.uint8)
        for m in masks[:crowd_at]:
            before |= m
        eff = masks[crowd_at] & (1 - before)
        assert np.array_equal(all_, 255 * (masks[0] | masks[1] | masks[2]))
        assert np.array_equal(miss, 255 * (1 - (cr.ann_mask(q, h, w) | eff)))
    with pytest.raises(ValueError, match="crowd segments > 1"):
        cr.make_mask([c, p, c], h, w)


def test_crowd_runs_decode_column_major():
    m = np.zeros((3, 4), np.uint8)
    m[1:, 1] = m[0, 2] = 1
    assert cases.rle_counts(m) == [4, 3, 5] and np.array_equal(cr.rle_mask([4, 3, 5], 3, 4), m)
    m[0, 0] = 1
    assert cases.rle_counts(m)[0] == 0 and np.array_equal(cr.rle_mask(cases.rle_counts(m), 3, 4), m)


REFUSED = [
    ([dict(cases.crowd(8, 8, 0, 4, 0, 4), segmentation={"size": [8, 8], "counts": "04L4"})], "compressed"),
    ([{"segmentation": {"size": [8, 8], "counts": [64]}, "iscrowd": 0, "num_keypoints": 3}], "no crowd"),
    ([cases.person([[1, 1, 5, 5]], 3)], "fewer than 3"),
    ([cases.person([[1, 1, 5, 5, 3, 1, 2]], 3)], "odd number"),
    ([cases.person([[1, 1, 5, float("nan"), 3, 1]], 3)], "non-finite"),
    ([cases.person([[1, 1, 5, float("inf"), 3, 1]], 3)], "non-finite"),
    ([cases.person([[1, 1, 5, 2.0 ** 24 + 2, 3, 1]], 3)], "2\\^24"),
    ([cases.crowd(8, 9, 0, 4, 0, 4)], "size"),
    ([dict(cases.crowd(8, 8, 0, 4, 0, 4), segmentation={"size": [8, 8], "counts": [10, 4, 49]})], "sum to 63"),
    ([dict(cases.crowd(8, 8, 0, 4, 0, 4), segmentation={"size": [8, 8], "counts": [70, -6]})], "non-negative"),
    ([dict(cases.crowd(8, 8, 0, 4, 0, 4), segmentation=[[1, 1, 5, 1, 5, 5]])], "run-length code"),
]


@pytest.mark.parametrize("anns,word", REFUSED, ids=[w for _, w in REFUSED])
def test_the_packer_refuses_what_the_contract_does_not_cover(anns, word):
    with pytest.raises(PosePafError, match=word):
        coco_masks.pack_segmentations([anns], [(8, 8)])


def test_the_packer_names_an_image_with_two_crowds_and_packs_the_tables():
    c = cases.crowd(8, 8, 0, 4, 0, 4)
    with pytest.raises(coco_masks.MultiCrowdError, match="image 4711"):
        coco_masks.pack_segmentations([[], [c, cases.person([[1, 1, 5, 1, 5, 5]], 2), c]], [(8, 8), (8, 8)], names=[17, 4711])
    first, _ = cases.batches()
    p = coco_masks.pack_segmentations(first, cases.SIZES)
    assert p["verts"].dtype == np.float64 and p["rings"].dtype == np.int32 and p["images"].dtype == np.int64 and p["runs"].dtype == np.int64
    assert p["images"][:, :2].tolist() == [[0, 0], [0, 17], [17, 0]] and p["images"][1, 2:].tolist()[1:] == [len(first[1][3]["segmentation"]["counts"]), 3]
    assert p["rings"][:, 2].tolist() == sorted(p["rings"][:, 2].tolist()) and set(p["rings"][:, 3]) == {0, 1}
    assert p["rings"][:, 1].sum() == len(p["verts"]) and p["runs"][-1] == 64 * 64 and p["sizes"].tolist() == [[37, 70, 64], [53, 150, 64]]


def test_instances_and_combination_match_the_reference():
    doc = json.load(open(os.path.join(GOLDEN, "coco_instances.json")))
    planes = np.load(os.path.join(GOLDEN, "coco_instances.npz"))
    assert [len(x) for x in doc["instances"]] == [2, 1, 1]                      # the stale side admits one person and refuses another
    assert any(a["num_keypoints"] == 0 and not a["iscrowd"] for anns in doc["annotations"] for a in anns)
    assert sum(a["iscrowd"] for anns in doc["annotations"] for a in anns) == 1
    got, skipped = coco_masks.training_instances(doc["images"], doc["annotations"])
    want = [(i, w) for i, per_image in enumerate(doc["instances"]) for w in per_image]
    assert skipped == 0 and len(got) == len(want)
    for g, (i, w) in zip(got, want):
        assert g["image"] == i and g["image_id"] == doc["images"][i]["id"] and g["people_index"] == w["people_index"]
        assert len(g["joints"]) == 1 + w["numOtherPeople"]
        assert np.array_equal(np.array(g["objpos"]), np.array(w["objpos"])) and g["scale_provided"] == w["scale_provided"]
        for mine, ref in zip(g["joints"], np.array(w["joints"])):
            for coco_i, cmu_i in enumerate(sk.ORDER_COCO):
                assert (mine[cmu_i, 2] == 1) == (ref[coco_i, 2] < 2)
                if ref[coco_i, 2] < 2:
                    assert np.array_equal(mine[cmu_i, :2], ref[coco_i, :2])
    for i, (meta, anns) in enumerate(zip(doc["images"], doc["annotations"])):
        miss, all_ = cr.make_mask(anns, meta["height"], meta["width"])
        assert np.array_equal(miss, planes[f"m{i}_miss"]) and np.array_equal(all_, planes[f"m{i}_all"])
        assert 0 < (all_ == 255).sum() < all_.size and ((miss == 0).any() or i == 2)     # image 2 has nothing to mask
    # more people than the renderer takes: the instance is left out and counted, never truncated
    got, skipped = coco_masks.training_instances(doc["images"][:1], doc["annotations"][:1], max_people=1)
    assert got == [] and skipped == 2


def finetune(argv):
    return subprocess.run([sys.executable, os.path.join(PKG, "finetune.py")] + argv, capture_output=True, text=True, timeout=120)


def test_finetune_refuses_bad_sources_before_the_gpu(tmp_path):
    ann, img_dir, _ = cases.write_annotation_fixture(str(tmp_path))
    for argv, word in ((["--ann_file", ann, "--img_dir", img_dir, "--synthetic", "4"], "two data sources"),
                       (["--ann_file", str(tmp_path / "none.json"), "--img_dir", img_dir], "no such file"),
                       (["--ann_file", ann, "--img_dir", str(tmp_path / "none")], "no such directory"),
                       (["--ann_file", ann], "needs --img_dir"),
                       (["--ann_file", ann, "--img_dir", img_dir, "--src_sizes", "64x64"], "--src_sizes"),
                       (["--synthetic", "4", "--limit", "2"], "belong to --ann_file"),
                       (["--steps", "2"], "--synthetic")):
        r = finetune(argv)
        assert r.returncode != 0 and word in r.stderr and "MI355X" not in r.stderr, (argv, r.stderr[-500:])
