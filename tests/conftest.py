import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "improved-body-parts_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    from oracle.oracle import Oracle
    return Oracle()


def reference_key(joint_list, paf_hwc, min_img_size) -> str:
    """identifies one process_paf call by its inputs (as the compiled reference receives them)"""
    import hashlib

    import numpy as np
    h = hashlib.sha256()
    for a in (joint_list, paf_hwc):
        a = np.ascontiguousarray(a, np.float32)
        h.update(repr(a.shape).encode())
        h.update(a.tobytes())
    h.update(str(int(min_img_size)).encode())
    return h.hexdigest()[:24]


class StoredReference:
    """The reference's own C++ process_paf as recorded by tests/golden/make_reference_cpp.py (golden G6): the result of a
    call is looked up by its inputs.  Where the compiled reference is present (oracle/_ref, built from the reference's
    sources by oracle/Makefile) every call also runs it, and it must reproduce the record."""

    def __init__(self):
        import numpy as np
        from oracle.oracle import REF_SO, Reference
        self.store = np.load(os.path.join(GOLDEN, "g6_reference_process_paf.npz"))
        self.live = Reference() if os.path.exists(REF_SO) else None

    def process_paf(self, joint_list, paf_hwc, min_img_size):
        import numpy as np
        key = reference_key(joint_list, paf_hwc, min_img_size)
        assert f"{key}_ids" in self.store.files, \
            "no recorded reference result for these inputs: add the case to tests/golden/make_reference_cpp.py and re-run it"
        want = {f: self.store[f"{key}_{f}"] for f in ("ids", "scores", "peaks")}
        if self.live is not None:
            got = self.live.process_paf(joint_list, paf_hwc, min_img_size)
            assert all(np.array_equal(got[f], want[f]) for f in want), "the compiled reference no longer gives the recorded result"
        return want


@pytest.fixture(scope="session")
def reference_cpp():
    """The reference's own C++ pafprocess: its recorded results, checked against oracle/_ref where that is built."""
    return StoredReference()


def load_scene(key):
    """Regenerate a golden scene's input and verify it against the stored checksum."""
    import hashlib
    import json

    import numpy as np
    from posepaf import synth
    meta = json.load(open(os.path.join(GOLDEN, "scenes.json")))[key]
    g = np.load(os.path.join(GOLDEN, f"g1_scene_{key}.npz"))
    net = synth.make_net_output(meta["P"], meta["seed"], dtype=np.float16 if meta["dtype"] == "f16" else np.float32)
    sha = np.frombuffer(hashlib.sha256(net.tobytes()).digest(), np.uint8)
    assert (sha == g["net_sha256"]).all(), \
        f"synthetic scene {key} no longer reproduces the input the golden vector was made from; " \
        "re-run tests/golden/make_golden.py in the build container"
    return net, g


def scene_keys():
    import json
    return sorted(json.load(open(os.path.join(GOLDEN, "scenes.json"))).keys())
