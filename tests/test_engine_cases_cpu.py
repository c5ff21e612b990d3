"""CPU: what tests/test_gpu_engine_pipeline.py takes for granted about its cases (tests/engine_cases.py) -- the plans its job
list runs on, people in every bank scene, no undefined sort in the oracle, a record that really depends on the image height in
the 16-row bucket, slot sizes -- so that the GPU test cannot pass for lack of anything to see."""
import numpy as np
import pytest

import engine_cases as ec


def test_job_list_has_the_plans_of_the_table():
    from evaluate import plan_batch
    assert plan_batch(5, 16) == plan_batch(8, 16) == 8
    labels = [ec.bucket(i) for i in range(ec.N_IMAGES)]
    assert {k: labels.count(k) for k in "ABC"} == ec.COUNTS and ec.N_IMAGES == 66
    jobs = ec.make_jobs(ec.shapes())
    assert len(jobs) == 6 and len({key for key, _ in jobs}) == 5
    for label in "ABC":
        mine = [(key, loc) for key, loc in jobs if key[:2] == ec.PADDED[label]]
        assert [key[2] for key, _ in mine] == ec.PLANS[label]
        assert all(ec.bucket(i) == label for _, loc in mine for i in loc)
        assert sorted(i for _, loc in mine for i in loc) == [i for i in range(66) if labels[i] == label]
    assert sorted(len(loc) for _, loc in jobs) == [5, 5, 8, 16, 16, 16]
    first, second = ec.passes()
    assert second == first[::-1] and sorted(map(repr, first)) == sorted(map(repr, jobs))
    assert [key[:2] for key, _ in first[:3]] == [ec.PADDED[k] for k in dict.fromkeys(labels)]      # three buckets in a row
    assert first != jobs and len(first) + len(second) == 12
    for key, loc in ec.single_bucket_jobs(8):
        assert key == (128, 128, 16) and len(loc) == 16 and all(ec.bucket(i) == "A" for i in loc)


def test_image_sizes_pad_to_their_bucket_and_mix():
    from posepaf.engine import padded_shape
    for i, (h, w) in enumerate(ec.shapes()):
        assert padded_shape(h, w) == ec.PADDED[ec.bucket(i)]
        assert ec.image(i).shape == (h, w, 3)
    for label in "ABC":
        mine = [hw for i, hw in enumerate(ec.shapes()) if ec.bucket(i) == label]
        hp, wp = ec.PADDED[label]
        assert (hp, wp) in mine and (9 if label == "C" else hp - 63, wp - 63) in mine      # a full-size and a minimal image
        assert sum(hw != (hp, wp) for hw in mine) >= len(mine) * 3 // 4     # most entries leave part of the slot unwritten
    heights = [h for i, (h, w) in enumerate(ec.shapes()) if ec.bucket(i) == "C"]
    assert set(heights) == {64, 40, 17, 9} and sum(h in (17, 9) for h in heights) * 2 >= len(heights)
    assert (ec.poison(1 << 16) != 128).all() and len(np.unique(ec.poison(1 << 16))) == ec.POISON_SPAN


def test_every_plan_fits_the_slots():
    from posepaf.engine import header_bytes, padded_shape, scene_bytes
    hp, wp = padded_shape(*ec.MAX_IMAGE_HW)
    for extra in (lambda b: 0, lambda b: scene_bytes(b, ec.DEVICE_MAX_PEOPLE)):       # scenes="bank", scenes="device"
        max_bytes = header_bytes(ec.B) + ec.B * hp * wp * 3 + extra(ec.B)
        for (php, pwp, b), _ in ec.make_jobs(ec.shapes()):
            assert b <= ec.B and header_bytes(b) + b * php * pwp * 3 + extra(b) <= max_bytes
    assert max(len(ec.people(i)) for i in range(ec.N_IMAGES)) <= ec.DEVICE_MAX_PEOPLE


@pytest.mark.parametrize("label", "ABC")
def test_oracle_finds_people_in_every_bank_scene(oracle, label):
    bank = ec.bank(label)
    hp, wp = ec.PADDED[label]
    assert bank.shape == (16, 2, 50, hp // 4, wp // 4) and bank.dtype == np.float16
    heights = sorted({h for i, (h, w) in enumerate(ec.shapes()) if ec.bucket(i) == label})
    for s in range(ec.N_SCENES):
        for h in heights if label == "C" else (heights[0], hp):
            want = oracle.pipeline(bank[s], h)
            assert len(want["ids"]) >= 1 and not want["sort_oob"], (label, s, h)


def test_bucket_c_records_depend_on_the_image_height(oracle):
    """the only bucket in which a height on the wrong image shows: at least 3/4 of its images of height 17 or 9 get another
    record at the padded height 64"""
    bank = ec.bank("C")
    low = [i for i, (h, w) in enumerate(ec.shapes()) if ec.bucket(i) == "C" and h in (17, 9)]
    assert len(low) >= 4
    moved = 0
    for i in low:
        own = oracle.pipeline(bank[ec.scene_index(i)], ec.shapes()[i][0])
        padded = oracle.pipeline(bank[ec.scene_index(i)], 64)
        same = (np.array_equal(own["ids"], padded["ids"]) and np.array_equal(own["scores"], padded["scores"])
                and own["connections"] == padded["connections"])
        moved += not same
    print(f"bucket C: {moved} of {len(low)} low images have a height-dependent record")
    assert 4 * moved >= 3 * len(low)


def test_model_restatement_and_sensitive_pixel():
    """model_numpy agrees with TinyModel run by torch on the CPU, at batch 1 and inside a batch; sensitive_pixel names a pixel
    inside the corner whose restated output changes"""
    import torch
    model = ec.TinyModel(torch, device="cpu")
    imgs = [ec.padded_image(i) for i in range(ec.N_IMAGES) if ec.bucket(i) == "C"][:3]
    x = torch.from_numpy(np.stack(imgs).astype(np.float32) / np.float32(255)).half()
    both = model(x).numpy()
    for j, im in enumerate(imgs):
        want = ec.model_numpy(im)
        assert np.array_equal(both[j].view(np.uint16), want.view(np.uint16))
        assert np.array_equal(model(x[j:j + 1]).numpy()[0].view(np.uint16), want.view(np.uint16))
    i = 0
    maps = np.zeros((2, 50) + tuple(v // 4 for v in ec.PADDED[ec.bucket(i)]), np.float16)
    y, x_, col, new = ec.sensitive_pixel(i, maps)
    h, w = ec.shapes()[i]
    assert y < h // 4 * 4 and x_ < w // 4 * 4 and abs(new - int(ec.image(i)[y, x_, col])) == 1
