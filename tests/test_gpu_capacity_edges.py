"""GPU: the post-processing exactly at, and one over, each of its fixed capacities (tests/capacity_cases.py builds the scenes,
tests/test_capacity_cases_cpu.py proves on the CPU that each one meets its condition).  An off-by-one in this code faults
nowhere: a store lands in the next part's rows, the next image's slots or the LDS carved behind a table, so every image under
test runs as the MIDDLE image of a batch of three whose outer images are ordinary scenes, and everything the record defines is
compared with the oracle -- people, ids, scores, coordinates, the peak list and the connections of all 30 limbs.

Paths, each with its own copy of a limit:
  lds     PosePostProcessor.process, maps staged in LDS (k_heat_peaks, k_limb_connect with the assembly fused in)
  hbm     the same with the maps kept in device memory (k_heat_peaks_hbm, k_limb_connect_hbm)
  wave    the same with the assembly as its own launch (k_assemble_wave, pp_debug_set_mode 1)
  py      the Python rules (process_py: k_limb_connect_py, k_assemble_py) against oracle.py_find_humans
  dropin  pp_process_paf_host on the joint list and the HWC maps (k_limb_connect_hwc, k_assemble): 0 at a limit with equal
          results, PP_ERR_OVERFLOW over it
Over a limit the inputs are the documented overflow contract of include/posepaf.h (status bits, extra dropped), every store
indexed by peak rank, candidate position, slot or human row being clamped or predicated; nothing here is expected to fault.
Within an overflowing record humans[n_humans:] is undefined and never read.
"""
import ctypes as C

import numpy as np
import pytest

import capacity_cases as cc
from test_gpu_parity import SCORE_TOL, _records_vs_oracle, _same_record

pytestmark = pytest.mark.gpu

PP_ERR_OVERFLOW = -5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


# ------------------------------------------------------------------------------------------------ expectations, computed once
_want, _up, _py = {}, {}, {}


def _key(net, size):
    return (net.shape, net.dtype.str, int(size), hash(net.tobytes()))


def want_of(oracle, net, size):
    k = _key(net, size)
    if k not in _want:
        _want[k] = oracle.pipeline(net, size, flip=False)
    return _want[k]


def up_of(oracle, net):
    k = _key(net, 0)
    if k not in _up:
        _up[k] = oracle.upsample4_hwc(oracle.flip_average(net, flip=False)[1])
    return _up[k]


def py_of(oracle, net, size, joint_list=None):
    k = _key(net, size) + (None if joint_list is None else len(joint_list),)
    if k not in _py:
        jl = want_of(oracle, net, size)["joint_list"] if joint_list is None else joint_list
        _py[k] = oracle.py_find_humans(jl, up_of(oracle, net), size) + (jl,)
    return _py[k]


# ------------------------------------------------------------------------------------------------ running one path
class Ctx:
    """a context created for one test with the capacity the case needs, and closed afterwards"""

    def __init__(self, torch, maxp, hw, path, dtype):
        from posepaf.api import PosePostProcessor
        self.torch, self.path = torch, path
        self.post = PosePostProcessor(max_batch=3, max_h=hw[0], max_w=hw[1], max_peaks_per_part=maxp)
        if path == "hbm":
            self.post.set_map_residency("hbm")
        if path == "wave":
            self.post.set_mode(1)
        if path != "dropin":
            assert self.post.map_residency(np.dtype(dtype), *hw) == ("hbm" if path == "hbm" else "lds")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.post.close()

    def run(self, nets, size):
        dev = self.torch.from_numpy(np.stack(nets)).cuda()
        if self.path == "py":
            return self.post.process_py(dev, size, flip=False)
        return self.post.process(dev, size, flip=False)


def check_image(ctx, oracle, rec, image, net, size, what):
    """image `image` of the last batch equals the oracle in every field the record and the read-back calls define"""
    assert rec["status"] == 0, f"{what}: status {int(rec['status']):#x}"
    if ctx.path == "py":
        persons, ncn, jl = py_of(oracle, net, size)
        n = int(rec["n_humans"])
        assert n == len(persons) and rec["n_peaks"] == len(jl) and rec["n_connections"] == int(ncn.sum()), what
        assert np.array_equal(ctx.post.read_peaks(image), jl), what
        assert np.array_equal(ctx.post.read_connection_counts(image), ncn), what
        check_py_people(rec, persons, jl, what)
        return
    want = want_of(oracle, net, size)
    _records_vs_oracle(rec, want, what)
    assert rec["n_peaks"] == len(want["joint_list"]) and rec["n_connections"] == sum(len(c) for c in want["connections"]), what
    assert np.array_equal(ctx.post.read_peaks(image), want["joint_list"]), what
    for limb in range(30):
        exp = np.array([(c[0], c[1], c[2], c[5]) for c in want["connections"][limb]], np.float32).reshape(-1, 4)
        assert np.array_equal(ctx.post.read_connections(image, limb), exp), f"{what}: limb {limb}"


def check_py_people(rec, persons, jl, what):
    n = len(persons)
    assert np.array_equal(rec["humans"]["peak_id"][:n], persons[:, :18, 0].astype(np.int32)), what
    assert np.array_equal(rec["humans"]["n_parts"][:n], persons[:, 19, 0].astype(np.int32)), what
    assert np.allclose(rec["humans"]["score"][:n], persons[:, 18, 0] / persons[:, 19, 0], rtol=0, atol=SCORE_TOL), what
    ids = rec["humans"]["peak_id"][:n]
    m = ids >= 0
    assert np.array_equal(rec["humans"]["x"][:n][m], jl[ids[m], 0].astype(np.int32)), what
    assert np.array_equal(rec["humans"]["y"][:n][m], jl[ids[m], 1].astype(np.int32)), what
    assert np.array_equal(rec["humans"]["part_score"][:n][m], jl[ids[m], 2]), what


def dropin(ctx, oracle, net, size, joint_list=None):
    """pp_process_paf_host on the oracle's joint list and HWC maps -> the status code"""
    jl = np.ascontiguousarray(want_of(oracle, net, size)["joint_list"] if joint_list is None else joint_list, np.float32)
    up = up_of(oracle, net)
    fp = C.POINTER(C.c_float)
    return ctx.post.L.pp_process_paf_host(ctx.post.ctx, 1, len(jl), 5, jl.ctypes.data_as(fp), up.shape[0], up.shape[1], up.shape[2],
                                          up.ctypes.data_as(fp), int(size))


def check_dropin(ctx, oracle, net, size, what):
    L, c = ctx.post.L, ctx.post.ctx
    want = want_of(oracle, net, size)
    assert dropin(ctx, oracle, net, size) == 0, what
    assert L.pp_get_status(c) == 0, what
    nh = L.pp_get_num_humans(c)
    assert nh == len(want["ids"]), what
    ids = np.array([[L.pp_get_part_peak_id(c, h, p) for p in range(18)] for h in range(nh)], np.int32).reshape(nh, 18)
    assert np.array_equal(ids, want["ids"]), what
    assert np.array_equal(np.array([L.pp_get_score(c, h) for h in range(nh)], np.float32), want["scores"]), what
    got = np.array([(L.pp_get_part_x(c, i), L.pp_get_part_y(c, i), L.pp_get_part_score(c, i)) for i in range(len(want["peaks"]))],
                   np.float32).reshape(-1, 3)
    assert np.array_equal(got, want["peaks"]), what


def exact_capacity(torch, oracle, case, path, nbrs, maxp=None):
    """the case as the middle image of a batch of three: no overflow bit on any image, everything equal to the oracle"""
    maxp = case.maxp if maxp is None else maxp
    with Ctx(torch, maxp, case.hw, path, case.net.dtype) as ctx:
        if path == "dropin":
            check_dropin(ctx, oracle, case.net, case.min_img_size, case.name)
            check_dropin(ctx, oracle, nbrs[0], case.min_img_size, case.name + ": an ordinary scene afterwards")
            return
        nets = [nbrs[0], case.net, nbrs[1]]
        recs = ctx.run(nets, case.min_img_size)
        assert all(int(r["status"]) & cc.OVERFLOW_BITS == 0 for r in recs), case.name
        for i, net in enumerate(nets):
            check_image(ctx, oracle, recs[i], i, net, case.min_img_size, f"{case.name} [{path}] image {i}")


def over_capacity(torch, oracle, case, path, nbrs, maxp, bits, also_allowed=0):
    """the case one over a limit, as the middle image of a batch of three -> (its record, the context's results are checked):
    exactly `bits` of the overflow bits on it and none on the neighbours; the neighbours byte-equal to a batch of their own
    and equal to the oracle; an ordinary batch on the same context afterwards equal to both."""
    with Ctx(torch, maxp, case.hw, path, case.net.dtype) as ctx:
        size = case.min_img_size
        alone = ctx.run(nbrs, size)
        for i, net in enumerate(nbrs):
            check_image(ctx, oracle, alone[i], i, net, size, f"{case.name} [{path}] neighbour {i} alone")
        recs = ctx.run([nbrs[0], case.net, nbrs[1]], size)
        st = int(recs[1]["status"])
        assert st & cc.OVERFLOW_BITS == bits and st & ~(cc.OVERFLOW_BITS | also_allowed) == 0, f"{case.name} [{path}]: status {st:#x}"
        assert 0 <= int(recs[1]["n_humans"]) <= cc.MAX_HUMANS
        for k, i in enumerate((0, 2)):
            assert _same_record(recs[i], alone[k]), f"{case.name} [{path}]: neighbour {i} differs from its own batch"
            check_image(ctx, oracle, recs[i], i, nbrs[k], size, f"{case.name} [{path}] neighbour {i}")
        over = recs[1].copy()
        after = ctx.run(nbrs, size)       # nothing stale in counts, flags or workspace
        for i, net in enumerate(nbrs):
            assert _same_record(after[i], alone[i]), f"{case.name} [{path}]: run after the overflow, image {i}"
            check_image(ctx, oracle, after[i], i, net, size, f"{case.name} [{path}] after the overflow, image {i}")
        return over


def raw_records(ctx):
    """the three pp_record of the context's own buffer, as bytes"""
    from posepaf._lib import RECORD_BYTES, check
    buf = np.zeros((3, RECORD_BYTES), np.uint8)
    check(ctx.post.L.pp_read_records(ctx.post.ctx, None, buf.ctypes.data_as(C.c_void_p), 3, None), ctx.post.ctx)
    return buf


def dropin_over(torch, oracle, case, nbr, maxp, joint_list=None):
    """over a limit the drop-in answers PP_ERR_OVERFLOW and keeps no result; an ordinary scene afterwards is right"""
    with Ctx(torch, maxp, case.hw, "dropin", case.net.dtype) as ctx:
        before = raw_records(ctx)
        assert dropin(ctx, oracle, case.net, case.min_img_size, joint_list) == PP_ERR_OVERFLOW, case.name
        assert ctx.post.L.pp_get_num_humans(ctx.post.ctx) == 0
        # the drop-in owns record 0 of the context: a human row past PP_MAX_HUMANS would land in record 1
        assert np.array_equal(raw_records(ctx)[1:], before[1:]), case.name + ": a store behind the drop-in's record"
        check_dropin(ctx, oracle, nbr, case.min_img_size, case.name + ": an ordinary scene after the refusal")


# ------------------------------------------------------------------------------------------------ 1. peaks per part
@pytest.mark.parametrize("path", ["lds", "hbm", "py", "dropin"])
@pytest.mark.parametrize("h,w,P,dtype", cc.PEAK_CASES)
def test_peaks_exactly_full_and_one_over(torch_cuda, oracle, h, w, P, dtype, path):
    """Branch `total == maxp` (kept = min(total, maxp), s_pk / the peak rows / cb1, cb2 / usedA, usedB exactly full): the nose
    channel has P peaks (10 on the 33 x 47 map, whose width takes mask8's ragged branch; 20 on 64 x 64), the other parts fewer.
    maxp = P: status 0 and everything equals the oracle.  maxp = P - 1: PP_ST_PEAK_OVERFLOW alone, and the record equals the
    oracle's process_paf on the truncated table -- per part the first maxp peaks in row-major order, ids renumbered over the
    kept peaks (off[] is formed from min(count, maxp)); read_peaks refuses the truncated list."""
    case = cc.get_case(cc.peaks_case, h, w, P, dtype=dtype)
    nbrs = cc.peaks_neighbours(h, w, dtype)
    exact_capacity(torch_cuda, oracle, case, path, nbrs)
    size = case.min_img_size
    cut = cc.truncate_joint_list(want_of(oracle, case.net, size)["joint_list"], P - 1)
    if path == "dropin":     # the drop-in refuses a list with more peaks of a part than the context holds
        dropin_over(torch_cuda, oracle, case, nbrs[0], P - 1)
        return
    rec = over_capacity(torch_cuda, oracle, case, path, nbrs, P - 1, cc.ST_PEAK)
    assert rec["n_peaks"] == len(cut)
    if path == "py":
        persons, ncn, _ = py_of(oracle, case.net, size, cut)
        assert int(rec["n_humans"]) == len(persons) and rec["n_connections"] == int(ncn.sum())
        check_py_people(rec, persons, cut, case.name + " truncated")
    else:
        want_cut = oracle.process_paf(cut[None], up_of(oracle, case.net), size)
        _records_vs_oracle(rec, want_cut, case.name + " truncated")
        assert rec["n_connections"] == sum(len(c) for c in want_cut["connections"])


def test_truncated_peak_list_is_refused(torch_cuda, oracle):
    from posepaf._lib import PosePafError
    case = cc.get_case(cc.peaks_case, 33, 47, 10, dtype="float32")
    with Ctx(torch_cuda, 9, case.hw, "lds", case.net.dtype) as ctx:
        rec = ctx.run([case.net], case.min_img_size)[0]
        assert int(rec["status"]) == cc.ST_PEAK
        with pytest.raises(PosePafError):
            ctx.post.read_peaks(0)
        assert ctx.post.read_part_counts(0)[0] == 10          # the true count, beyond the capacity


# ------------------------------------------------------------------------------------------------ 2. limb candidates
@pytest.mark.parametrize("path", ["lds", "hbm", "dropin"])
@pytest.mark.parametrize("nA,nB,maxp,dtype", cc.CAND_EXACT_CASES)
def test_candidates_exactly_cap(torch_cuda, oracle, nA, nB, maxp, dtype, path):
    """Branch `ncand == cap`: limb 0 of a map that is high everywhere accepts every one of its nA x nB pairs.  The oracle
    counted 512 candidates for 16 x 32 at maxp = 32 (cap 512; float32 and binary16) and 256 for 16 x 16 at maxp = 16 (cap 256),
    0 for every other limb.  The survivor buffers are flushed on nsv + NT > cap and the last candidate sits in position
    cap - 1: status 0 and everything equals the oracle.  (The Python rules accept by their own criteria and their oracle does
    not report a candidate count, so that path has no proven boundary here and is left out.)"""
    case = cc.get_case(cc.candidates_case, nA, nB, maxp, dtype=dtype)
    exact_capacity(torch_cuda, oracle, case, path, cc.neighbours(*case.hw, dtype))


@pytest.mark.parametrize("path", ["lds", "hbm", "dropin"])
def test_candidates_one_row_over_cap(torch_cuda, oracle, path):
    """17 x 32 pairs at maxp = 32: the oracle counted 544 candidates for limb 0 against cap = 512.  PP_ST_CAND_OVERFLOW on
    that image and only on it; the candidates kept after the truncation are not the oracle's, so the flag is the whole
    expectation (PP_ST_SORT_UNDEFINED may accompany it: the kept set is sorted, not the oracle's)."""
    nA, nB, maxp, dtype = cc.CAND_OVER_CASE
    case = cc.get_case(cc.candidates_case, nA, nB, maxp, dtype=dtype)
    nbrs = cc.neighbours(*case.hw, dtype)
    if path == "dropin":
        dropin_over(torch_cuda, oracle, case, nbrs[0], maxp)
        return
    rec = over_capacity(torch_cuda, oracle, case, path, nbrs, maxp, cc.ST_CAND, also_allowed=cc.ST_SORT)
    assert rec["n_peaks"] == nA + nB


# ------------------------------------------------------------------------------------------------ 3. / 4. assembly table
@pytest.mark.parametrize("path", ["lds", "hbm", "wave", "dropin"])
@pytest.mark.parametrize("kind,dtype", cc.ASM_EXACT_CASES)
def test_assembly_table_branches(torch_cuda, oracle, kind, dtype, path):
    """The branches of assemble_image_wave that no ordinary scene reaches (counts by count_assembly on the oracle's connections):
      a  96 births, no merge: limb 14 is dispatched with S.nb = 96 -> assemble_pass<2>.
      b  168 births (64 + 64 + 40), 104 humans after 64 merges at limb 27: limbs 9 and 13 run with S.nb = 128 exactly
         (assemble_pass<2>, the last value it takes), limbs 14 and 27 with S.nb = 168 -> assemble_pass<kBanks>; limb 7 with
         S.nb = 64 exactly (assemble_pass<1>).
      c  289 births, at most 193 live, 97 humans: S.nb = 193 before limbs 9, 27 and 29, whose first 64 connections need
         193 + 64 = 257 = kSlots + 1 slots -> assemble_compact (nothing to drop at limbs 9 and 27, 96 erased slots at limb 29,
         after which S.nb = 97); limbs 0, 7, 9, 27 and 29 have 96 or 97 connections -> the `m > 64` second pass.  Status 0.
    Everything equals the oracle on every launch structure, and on the drop-in's k_assemble, which erases physically."""
    case = cc.get_case(cc.assembly_case, kind, dtype=dtype)
    exact_capacity(torch_cuda, oracle, case, path, cc.neighbours(*case.hw, dtype))


@pytest.mark.parametrize("path", ["lds", "hbm", "wave", "dropin"])
def test_assembly_more_live_skeletons_than_slots(torch_cuda, oracle, path):
    """Scene d: 264 births and no merge, so 264 live skeletons against kSlots = kMaxSkel = 256 (176 of them are pruned in the
    end: 88 humans, no other capacity is touched).  PP_ST_SKEL_OVERFLOW alone, every born slot below kSlots, neighbours intact."""
    case = cc.get_case(cc.assembly_case, "d", dtype="float32")
    nbrs = cc.neighbours(*case.hw)
    if path == "dropin":
        dropin_over(torch_cuda, oracle, case, nbrs[0], case.maxp)
        return
    over_capacity(torch_cuda, oracle, case, path, nbrs, case.maxp, cc.ST_SKEL)


# ------------------------------------------------------------------------------------------------ 5. humans per record
# the Python-rule path takes at most 64 peaks per part: the split scenes are its 128-human cases
HUMANS_RUNS = [(n, split, dtype, path) for (n, split, dtype) in cc.HUMANS_EXACT_CASES
               for path in ("lds", "hbm", "wave", "py", "dropin") if split or path != "py"]


@pytest.mark.parametrize("n,split,dtype,path", HUMANS_RUNS)
def test_exactly_128_humans(torch_cuda, oracle, n, split, dtype, path):
    """128 two-joint people, all kept by the prune: row PP_MAX_HUMANS - 1 of the record is written and no bit is set.  Unsplit
    (all on limb 0, maxp = 128): 128 peaks per part (`total == maxp` at the largest capacity) and 128 connections of one limb,
    so connections 64 .. 127 take the `m > 64` second pass.  Split over three limbs (maxp = 64): also the Python rules, whose
    k_assemble_py holds kMaxSkelPy = 128 live persons -- exactly full here (128 connections, each a birth)."""
    case = cc.get_case(cc.humans_case, n, split, dtype=dtype)
    exact_capacity(torch_cuda, oracle, case, path, cc.neighbours(*case.hw, dtype))


@pytest.mark.parametrize("path", ["lds", "hbm", "wave", "py", "dropin"])
def test_129_humans_keep_the_first_128(torch_cuda, oracle, path):
    """129 two-joint people: the `n_out > PP_MAX_HUMANS` clamp.  PP_ST_HUMAN_OVERFLOW alone, n_humans == 128 and the 128 records
    are the oracle's first 128 in birth order (ids, scores, x / y / part_score).  The Python rules hold 128 LIVE persons
    (kMaxSkelPy), so there the 129th birth raises PP_ST_SKEL_OVERFLOW instead and PP_ST_HUMAN_OVERFLOW cannot arise."""
    case = cc.get_case(cc.humans_case, 129, True, dtype="float32")
    nbrs = cc.neighbours(*case.hw)
    if path == "dropin":
        dropin_over(torch_cuda, oracle, case, nbrs[0], case.maxp)
        return
    rec = over_capacity(torch_cuda, oracle, case, path, nbrs, case.maxp, cc.ST_SKEL if path == "py" else cc.ST_HUMAN)
    if path == "py":
        return
    want = want_of(oracle, case.net, case.min_img_size)
    assert len(want["ids"]) == 129 and int(rec["n_humans"]) == 128
    _records_vs_oracle(rec, dict(want, ids=want["ids"][:128], scores=want["scores"][:128]), case.name)
    assert rec["n_peaks"] == len(want["joint_list"]) and rec["n_connections"] == 129
