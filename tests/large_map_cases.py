"""Scenes of the large-map tests (maps that do not fit LDS), shared by the GPU test and the CPU test that keeps it honest.

Each case: (dtype name, h, w, [(people, seed), ...]).  The seeds were chosen on the CPU so that the oracle reports no sort_oob
and no part has more than 64 peaks -- test_large_map_seeds_cpu.py asserts exactly that, so the GPU comparison has no reason to
skip an image."""
import numpy as np

LARGE_CASES = [
    ("float16", 272, 480, [(6, 6100)]),                # a 1920 x 1080 frame padded to 1088 x 1920
    ("float32", 192, 200, [(3, 6200), (5, 6201)]),     # just past the fp32 LDS bound
]
MAX_PEAKS = 64


def case_nets(case):
    from posepaf import synth
    name, h, w, scenes = case
    return [synth.make_net_output(p, seed, h=h, w=w, dtype=np.dtype(name).type) for p, seed in scenes]


_wants = {}


def oracle_wants(oracle, case):
    """oracle.pipeline of every image of the case, computed once per process and shared (never modified by the tests)"""
    key = (case[0], case[1], case[2])
    if key not in _wants:
        _wants[key] = [oracle.pipeline(net, 4 * case[1]) for net in case_nets(case)]
    return _wants[key]
