"""CPU: every scene of tests/capacity_cases.py really sits where test_gpu_capacity_edges.py says it does -- exactly at a
capacity, or one over -- shown through the oracle and the counting restatement (count_assembly), never through the code under
test.  Each test prints the measured quantity next to its limit (pytest -s) and fails when a scene stops meeting its condition.
"""
import numpy as np
import pytest

import capacity_cases as cc


def _common(want, case):
    """no sort UB in the scene; -> (peaks per part, candidates per limb)"""
    ppp = cc.peaks_per_part(want["joint_list"])
    assert not want["sort_oob"], case.name
    return ppp, want["n_candidates"]


def _neighbour_ok(oracle, net, size, maxp):
    want = oracle.pipeline(net, size, flip=False)
    ppp = cc.peaks_per_part(want["joint_list"])
    assert not want["sort_oob"] and ppp.max() <= maxp and want["n_candidates"].max() <= cc.candidate_cap(maxp)
    assert 0 < len(want["ids"]) <= cc.MAX_HUMANS
    return want


@pytest.mark.parametrize("h,w,P,dtype", cc.PEAK_CASES)
def test_peak_scenes_fill_one_part_exactly(oracle, h, w, P, dtype):
    """`total == maxp` at maxp = P; at maxp = P - 1 exactly one peak -- the last nose in row-major order -- is dropped."""
    case = cc.get_case(cc.peaks_case, h, w, P, dtype=dtype)
    want = cc.oracle_pipeline(oracle, case)
    ppp, ncand = _common(want, case)
    print(f"{case.name}: peaks per part {ppp.tolist()} (limit {P} / {P - 1}), candidates max {ncand.max()} (cap {cc.candidate_cap(P - 1)}), "
          f"humans {len(want['ids'])}")
    assert 8 <= P <= 24
    assert ppp[0] == P and (ppp[1:] < P).all()
    assert ncand.max() <= cc.candidate_cap(P - 1) and len(want["ids"]) <= cc.MAX_HUMANS
    jl = want["joint_list"]
    assert np.array_equal(jl[:, 3], np.arange(len(jl))) and (np.diff(jl[:, 4]) >= 0).all()   # ids = rows, grouped by part
    nose = jl[jl[:, 4] == 0]
    cell = (nose[:, 1].astype(int) // 4) * w + nose[:, 0].astype(int) // 4
    assert (np.diff(cell) > 0).all(), "the oracle's rows of a part are in row-major order of the map"
    cut = cc.truncate_joint_list(jl, P - 1)
    assert len(cut) == len(jl) - 1 and cc.peaks_per_part(cut)[0] == P - 1
    assert np.array_equal(cut[:P - 1, :3], nose[:P - 1, :3]) and np.array_equal(cut[P - 1:, :3], jl[P:, :3])
    _, paf = oracle.flip_average(case.net, flip=False)
    want_cut = oracle.process_paf(cut[None], oracle.upsample4_hwc(paf), case.min_img_size)
    assert not want_cut["sort_oob"]
    assert not np.array_equal(want_cut["ids"], want["ids"])      # the truncation is visible in the result
    for net in cc.peaks_neighbours(h, w, dtype):
        _neighbour_ok(oracle, net, case.min_img_size, P - 1)


@pytest.mark.parametrize("nA,nB,maxp,dtype", cc.CAND_EXACT_CASES + [cc.CAND_OVER_CASE])
def test_candidate_scenes_fill_one_limb_exactly(oracle, nA, nB, maxp, dtype):
    """`ncand == cap`: limb 0 has exactly cap = clamp(maxp^2, 256, 512) accepted candidates (every pair), or 32 more."""
    case = cc.get_case(cc.candidates_case, nA, nB, maxp, dtype=dtype)
    want = cc.oracle_pipeline(oracle, case)
    ppp, ncand = _common(want, case)
    cap = cc.candidate_cap(maxp)
    print(f"{case.name}: candidates per limb {ncand.tolist()} (cap {cap}), peaks per part max {ppp.max()} (limit {maxp})")
    assert ppp.max() <= maxp and ppp[1] == nA and ppp[0] == nB
    assert ncand[0] == nA * nB and (ncand[1:] <= cap).all()
    if (nA, nB, maxp, dtype) == cc.CAND_OVER_CASE:
        assert ncand[0] == cap + 32
    else:
        assert ncand[0] == cap
    assert len(want["ids"]) <= cc.MAX_HUMANS


def _print_count(case, c, ppp, ncand):
    print(f"{case.name}: births {c['births']} (slots {cc.K_SLOTS}), max live {c['max_live']} (limit {cc.K_SLOTS}), max births in one "
          f"limb {c['max_births_in_limb']}, humans {c['humans']} (limit {cc.MAX_HUMANS}), compactions {c['compactions']}, "
          f"max connections of a limb {c['max_connections']}, peaks per part max {ppp.max()} (limit {case.maxp}), candidates max "
          f"{ncand.max()} (cap {cc.candidate_cap(case.maxp)})\n    S.nb before each limb {c['nb_before']}\n    passes (limb, pass, "
          f"nb in, nb, connections, NB) {[p for p in c['passes'] if p[5] != 1 or p[1]]}")


@pytest.mark.parametrize("kind,dtype", cc.ASM_EXACT_CASES + [("d", "float32")])
def test_assembly_scenes_enter_their_branch(oracle, kind, dtype):
    case = cc.get_case(cc.assembly_case, kind, dtype=dtype)
    want = cc.oracle_pipeline(oracle, case)
    ppp, ncand = _common(want, case)
    c = cc.count_assembly(want)
    _print_count(case, c, ppp, ncand)
    assert np.array_equal(c["ids"], want["ids"]), "the counting restatement replays the oracle's assembly"
    assert ppp.max() <= case.maxp and ncand.max() <= cc.candidate_cap(case.maxp) and c["humans"] <= cc.MAX_HUMANS
    first = [p for p in c["passes"] if p[1] == 0]
    if kind == "a":      # assemble_pass<2>: a limb's first pass dispatched with 64 < S.nb <= 128
        assert 65 <= c["births"] <= 128 and not c["overflow"] and c["compactions"] == 0
        assert any(p[5] == 2 and 64 < p[3] <= 128 for p in first) and not any(p[5] == 4 for p in c["passes"])
    elif kind == "b":    # assemble_pass<kBanks>: a first pass dispatched with S.nb > 128, no compaction yet
        assert 128 < c["births"] <= cc.K_SLOTS and not c["overflow"] and c["compactions"] == 0
        assert any(p[5] == 4 and p[3] > 128 for p in first)
        assert c["humans"] < c["births"]                      # fragments merged
    elif kind == "c":    # assemble_compact, then the m > 64 pass
        assert c["births"] > cc.K_SLOTS and c["max_live"] <= cc.K_SLOTS and not c["overflow"]
        assert any(p[2] + p[4] == cc.K_SLOTS + 1 and p[3] < p[2] for p in c["passes"]), \
            "a pass that needs exactly one slot more than the table has, with erased slots to drop"
        assert c["max_connections"] > 64 and any(p[1] == 1 for p in c["passes"])
    else:                # PP_ST_SKEL_OVERFLOW: more live skeletons than slots; pruned down so that no other bit is raised
        assert c["max_live"] > cc.K_SLOTS and c["overflow"]
    for net in cc.neighbours(*case.hw):
        _neighbour_ok(oracle, net, case.min_img_size, case.maxp)


@pytest.mark.parametrize("n,split,dtype", cc.HUMANS_EXACT_CASES + [(129, True, "float32")])
def test_human_scenes_fill_the_record_exactly(oracle, n, split, dtype):
    """the `n_out > PP_MAX_HUMANS` clamp: exactly 128 humans after the prune, or 129; the Python rules give the same people"""
    case = cc.get_case(cc.humans_case, n, split, dtype=dtype)
    want = cc.oracle_pipeline(oracle, case)
    ppp, ncand = _common(want, case)
    c = cc.count_assembly(want)
    _print_count(case, c, ppp, ncand)
    assert np.array_equal(c["ids"], want["ids"])
    assert len(want["ids"]) == n == c["humans"] == c["births"] and not c["overflow"]
    assert ppp.max() <= case.maxp and ncand.max() <= cc.candidate_cap(case.maxp)
    if not split:        # the m > 64 pass: limb 0 has 128 connections
        assert c["max_connections"] == n > 64 and any(p[1] == 1 for p in c["passes"])
    else:                # k_assemble_py holds kMaxSkelPy = 128 live persons; every birth consumes a connection
        _, paf = oracle.flip_average(case.net, flip=False)
        persons, ncn = oracle.py_find_humans(want["joint_list"], oracle.upsample4_hwc(paf), case.min_img_size)
        print(f"    Python rules: persons {len(persons)}, connections {int(ncn.sum())} (live limit {cc.K_SLOTS_PY})")
        assert len(persons) == n == int(ncn.sum()) and ppp.max() <= 64
    for net in cc.neighbours(*case.hw):
        _neighbour_ok(oracle, net, case.min_img_size, case.maxp)


def test_counter_flags_a_table_that_is_too_small(oracle):
    """the restatement itself: with fewer slots than live skeletons it reports the overflow, with enough it does not"""
    want = cc.oracle_pipeline(oracle, cc.get_case(cc.assembly_case, "a", dtype="float32"))
    assert cc.count_assembly(want, slots=95)["overflow"] and not cc.count_assembly(want, slots=96)["overflow"]
