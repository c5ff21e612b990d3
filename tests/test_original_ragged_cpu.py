"""CPU: the bucket rule of the ragged original path (posepaf.original_path.bucket_key) and, in the manner of
test_large_map_seeds_cpu.py, that the scenes test_gpu_original_ragged.py compares are not vacuous."""
import numpy as np
import pytest

import ragged_cases as rc


def test_bucket_key_of_the_test_bucket():
    from posepaf.original_path import bucket_key, scaled_size
    assert [scaled_size(97, 115, s) for s in rc.SCALES] == [(48, 58), (97, 115), (146, 172)]      # half to even, both ways
    assert [scaled_size(86, 127, s) for s in rc.SCALES] == [(43, 64), (86, 127), (129, 190)]
    for hw in rc.SIZES:
        assert bucket_key(*hw, rc.SCALES) == rc.KEY
    assert bucket_key(128, 129, rc.SCALES) != rc.KEY
    assert bucket_key(128, 129, rc.SCALES) == ((64, 64), (128, 192), (192, 256))
    # one scale of the list is enough to part two images: 64 and 128 pad alike at 0.5 only
    assert bucket_key(64, 64, [0.5]) == bucket_key(128, 128, [0.5])
    assert bucket_key(64, 64, [0.5, 1.0]) != bucket_key(128, 128, [0.5, 1.0])
    assert len({tuple(rc.pads(hw)) for hw in rc.SIZES}) == 4                # the pads differ per image
    tiles = {(-(-h // 32)) * (-(-w // 32)) for h, w in rc.SIZES}
    assert tiles == {12, 16} and rc.SLOT in rc.SIZES


def test_grouping_of_mixed_sizes():
    from posepaf.original_path import group_by_bucket_key
    shapes = [(120, 100), (64, 64), (128, 128), (128, 129), (64, 64), (97, 115), (86, 127), (128, 129)]
    groups = group_by_bucket_key(shapes, rc.SCALES)
    assert [(members, ragged) for _, members, ragged in groups] == [([0, 2, 5, 6], True), ([1, 4], False), ([3, 7], False)]
    assert groups[0][0] == rc.KEY
    # a one-size group takes the equal-size path even where another size would share its key
    assert group_by_bucket_key([(128, 128)] * 3, rc.SCALES) == [(rc.KEY, [0, 1, 2], False)]
    exact = group_by_bucket_key(shapes, rc.SCALES, exact=True)
    assert [(key, members, ragged) for key, members, ragged in exact] == [
        ((120, 100), [0], False), ((64, 64), [1, 4], False), ((128, 128), [2], False), ((128, 129), [3, 7], False),
        ((97, 115), [5], False), ((86, 127), [6], False)]


@pytest.mark.parametrize("which", ["ragged", "equal"])
def test_ragged_scenes_show_people_and_fit_the_peak_tables(oracle, which):
    """every image of the GPU comparison shows the oracle at least one person, no part has more than 64 peaks, and the
    image with the corner peak has a peak on its own last row and last column"""
    cases = list(zip(rc.SIZES, rc.SCENES)) if which == "ragged" else [(rc.SLOT, s) for s in rc.EQUAL_SCENES]
    for b, (size, (people, seed)) in enumerate(cases):
        corner = which == "ragged" and b == rc.CORNER_IMAGE
        _, _, rows, persons = rc.oracle_image(oracle, size, people, seed, corner=corner)
        per_part = np.bincount(rows[:, 4].astype(int), minlength=18)
        assert 0 < per_part.max() <= 64, (size, people, seed, per_part)
        assert len(persons) > 0, (size, people, seed)
        if corner:
            assert ((rows[:, 0] == size[1] - 1) & (rows[:, 1] == size[0] - 1)).any(), rows
