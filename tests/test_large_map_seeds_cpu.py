"""CPU: the scenes test_gpu_large_maps.py compares against the oracle are free of the two conditions under which the other
GPU tests skip an image (the reference's sort reading out of bounds; more peaks of one part than the context holds)."""
import numpy as np
import pytest

from large_map_cases import LARGE_CASES, MAX_PEAKS, oracle_wants


@pytest.mark.parametrize("case", LARGE_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_large_map_scenes_need_no_skip(oracle, case):
    for (people, seed), want in zip(case[3], oracle_wants(oracle, case)):
        assert not want["sort_oob"], (people, seed)
        per_part = np.bincount(want["joint_list"][:, 4].astype(int), minlength=18)
        assert 0 < per_part.max() <= MAX_PEAKS, (people, seed, per_part)
        assert len(want["ids"]) > 0, (people, seed)
