"""Scenes that sit exactly at, and one over, each fixed capacity of the post-processing kernels, and a counting restatement
of the assembly that proves on the CPU which branch of assemble_image_wave a scene enters.  Helper module: no tests.

Every scene is synth.render_maps on hand-placed joints followed by channel edits (limb planes zeroed, heat / limb planes
scaled), so that one "person" can be born as several fragments that merge at a later limb, or be pruned in the end.  Joints sit
on map-cell centres (4 i + 1.5 px), people on a grid wide enough that neither their Gaussians nor their limb boxes touch, and a
small seeded perturbation is added last so that no two candidate keys of a limb tie (test_capacity_cases_cpu.py asserts
sort_oob is false for every case).

The limits (csrc/posepaf_kernels.hip, csrc/posepaf_map_kernels.inc, csrc/posepaf_py_rules.inc, include/posepaf.h):
  peaks per part      max_peaks_per_part (maxp)           kept = min(total, maxp), row-major; PP_ST_PEAK_OVERFLOW
  limb candidates     cap = clamp(maxp^2, 256, 512)       PP_ST_CAND_OVERFLOW
  assembly slots      kSlots = 256 (wave form), kMaxSkel = 256 live (k_assemble), kMaxSkelPy = 128 live (k_assemble_py)
  humans per record   PP_MAX_HUMANS = 128                 PP_ST_HUMAN_OVERFLOW
"""
from dataclasses import dataclass, field

import numpy as np

from test_assembly_batching_equivalence import LIMBS, NUM_PART, scan_and_apply

K_SLOTS = 256          # kSlots / kMaxSkel
K_SLOTS_PY = 128       # kMaxSkelPy
MAX_HUMANS = 128       # PP_MAX_HUMANS
ST_PEAK, ST_HUMAN, ST_SKEL, ST_SORT, ST_CAND = 1, 2, 4, 8, 16
OVERFLOW_BITS = ST_PEAK | ST_HUMAN | ST_SKEL | ST_CAND
PERTURB = 0.004        # far below the 0.1 peak / sample thresholds and below every step between neighbouring Gaussian cells


def candidate_cap(maxp):
    """cap = clamp(maxp^2, 256, 512), the accepted candidates one limb holds"""
    return min(max(maxp * maxp, 256), 512)


@dataclass
class Case:
    name: str
    net: np.ndarray            # (1, 50, h, w), flip off
    maxp: int
    min_img_size: int
    extra: dict = field(default_factory=dict)

    @property
    def hw(self):
        return self.net.shape[2], self.net.shape[3]


# ------------------------------------------------------------------------------------------------ scene construction
def _grid(h, w, step, first):
    """cell centres (cx, cy) in row-major order"""
    return [(cx, cy) for cy in range(first, h - first + 1, step) for cx in range(first, w - first + 1, step)]


def _render(h, w, people, keep_limbs, heat_scale=None, limb_scale=None, dtype=np.float32, seed=1):
    """people: list of ((cx, cy) map cell of the centre, {part: (dx, dy) px offset, a multiple of 4}).  Limb planes outside
    keep_limbs are zeroed; heat_scale / limb_scale: {channel index within its group: factor}."""
    from posepaf import synth
    joints = np.zeros((len(people), NUM_PART, 3))
    joints[:, :, 2] = 2
    for i, ((cx, cy), parts) in enumerate(people):
        for p, (dx, dy) in parts.items():
            assert dx % 4 == 0 and dy % 4 == 0
            joints[i, p] = (4 * cx + 1.5 + dx, 4 * cy + 1.5 + dy, 1)
            assert 0 <= joints[i, p, 0] < 4 * w and 0 <= joints[i, p, 1] < 4 * h
    maps = synth.render_maps(joints, h, w)
    for limb in range(30):
        if limb not in keep_limbs:
            maps[limb] = 0
    for limb, f in (limb_scale or {}).items():
        maps[limb] *= np.float32(f)
    for part, f in (heat_scale or {}).items():
        maps[30 + part] *= np.float32(f)
    maps[:48] += np.float32(PERTURB) * np.random.default_rng(seed).random((48, h, w), dtype=np.float32)
    return np.ascontiguousarray(maps[None].astype(dtype))


def _limb(a, b):
    return LIMBS.index((a, b))


# limb indices used below (config/config.py order, pafprocess.cpp walks them 0..29)
L_NECK_NOSE, L_REYE_REAR, L_NECK_RSHO = _limb(1, 0), _limb(14, 16), _limb(1, 2)
L_LSHO_LELB, L_LELB_LWRI = _limb(5, 6), _limb(6, 7)
L_RHIP_RKNE, L_RKNE_RANK = _limb(8, 9), _limb(9, 10)
L_NOSE_RSHO, L_REAR_RSHO, L_RHIP_LHIP = _limb(0, 2), _limb(16, 2), _limb(8, 11)

# fragments of one person, px offsets from the person's centre
FRAG_A = {1: (0, 4), 0: (0, -12), 2: (-12, 8)}       # neck, nose, right shoulder: born at limb 0, extended at limb 9
FRAG_B = {14: (-4, -16), 16: (-16, -8)}              # right eye, right ear: born at limb 7, joined to A at limb 27 (16, 2)
FRAG_C = {8: (-8, 16), 11: (8, 16)}                  # hips: born at limb 29
TWO = {1: (0, 8), 0: (0, -8)}                        # a two-joint "person": neck and nose, 16 px apart


def ordinary_scene(seed=77, h=128, w=128, people=7, dtype=np.float32):
    """a neighbour image: synth's random people, flip off"""
    from posepaf import synth
    return synth.make_net_output(people, seed, h=h, w=w, dtype=dtype, flip=False)


# ---- 1. peaks per part
def peaks_case(h, w, P, dtype=np.float32):
    """The fullest part (nose) has exactly P peaks, neck P - 1, the shoulders P - 2; `total == maxp` at maxp = P, one over at
    maxp = P - 1 (the last nose in row-major order is dropped)."""
    cells = _grid(h, w, 10, 5)
    assert len(cells) >= P
    people = []
    for i in range(P):
        parts = {0: (0, -12)}
        if i != 1:
            parts[1] = (0, 4)
        if i not in (1, 2):
            parts[2] = (-12, 8)
            parts[5] = (12, 8)
        people.append((cells[i], parts))
    keep = {L_NECK_NOSE, L_NECK_RSHO, _limb(1, 5), L_NOSE_RSHO, _limb(0, 5)}
    return Case(f"peaks_{h}x{w}_P{P}_{np.dtype(dtype).name}", _render(h, w, people, keep, dtype=dtype, seed=3), P, 4 * min(h, w),
                extra={"P": P, "full_part": 0})


def truncate_joint_list(joint_list, maxp):
    """What the peak kernel keeps at capacity maxp: per part the first maxp rows in row-major (np.nonzero) order -- the order
    of the oracle's joint list -- and ids renumbered over the KEPT rows (the kernels form off[] from min(count, maxp))."""
    rows = []
    for part in range(NUM_PART):
        rows.append(joint_list[joint_list[:, 4] == part][:maxp])
    out = np.concatenate(rows).astype(np.float32)
    out[:, 3] = np.arange(len(out), dtype=np.float32)
    return np.ascontiguousarray(out)


# ---- 2. limb candidates
def candidates_case(nA, nB, maxp, dtype=np.float32):
    """Limb maps high everywhere (0.6 .. 0.9), nA isolated neck peaks and nB isolated nose peaks and nothing else: limb 0 has
    nA * nB pairs and every one is accepted."""
    rng = np.random.default_rng(11)
    net = np.zeros((1, 50, 128, 128), np.float32)
    net[0, :30] = 0.6 + 0.3 * rng.random((30, 128, 128), dtype=np.float32)
    # a 64-cell window: no pair is longer than 360 px, so the length prior min(0.5 * 512 / length - 1, 0) stays above -0.3
    # and criterion2 = mean sample (0.6 .. 0.9) + prior is positive for every pair
    ys, xs = np.meshgrid(np.arange(36, 100, 10), np.arange(36, 100, 10), indexing="ij")      # 7 x 7 = 49 cells
    ys, xs = ys.ravel(), xs.ravel()
    assert nA <= 49 and nB <= 49
    net[0, 30 + 1, ys[:nA], xs[:nA]] = 0.5 + 0.4 * rng.random(nA, dtype=np.float32)
    net[0, 30 + 0, ys[:nB] + 3, xs[:nB] + 2] = 0.5 + 0.4 * rng.random(nB, dtype=np.float32)
    return Case(f"cand_{nA}x{nB}_maxp{maxp}_{np.dtype(dtype).name}", np.ascontiguousarray(net.astype(dtype)), maxp, 512,
                extra={"limb": L_NECK_NOSE, "pairs": nA * nB})


# ---- 3. assembly table
def assembly_case(kind, dtype=np.float32):
    """a: 65..128 slots born (assemble_pass<2>); b: more than 128 born, at most 256 births (assemble_pass<kBanks>);
    c: more than 256 births, never more than 256 live, at most 128 humans (assemble_compact, status 0), and a limb with more
    than 64 connections (the m > 64 pass); d: more than 256 live (PP_ST_SKEL_OVERFLOW)."""
    keep = {L_NECK_NOSE, L_REYE_REAR, L_NECK_RSHO, L_REAR_RSHO, L_LSHO_LELB, L_LELB_LWRI, L_RHIP_RKNE, L_RKNE_RANK,
            L_RHIP_LHIP}
    arm = {5: (8, -8), 6: (8, 4), 7: (8, 16)}               # left shoulder, elbow, wrist: born at limb 13, extended at limb 14
    leg = {8: (-8, -8), 9: (-8, 4), 10: (-8, 16)}           # right hip, knee, ankle: born at limb 16, extended at limb 17
    if kind == "a":      # 48 A at limb 0 + 48 arms at limb 13 = 96 births; limb 14 then runs against 96 slots
        cells = _grid(128, 128, 12, 6)
        people = [(cells[i], FRAG_A) for i in range(48)] + [(cells[48 + i], arm) for i in range(48)]
        return Case("asm_a_" + np.dtype(dtype).name, _render(128, 128, people, keep, dtype=dtype, seed=5), 64, 512)
    if kind == "b":      # 64 A (limb 0) + 64 B (limb 7) + 40 arms (limb 13) = 168 births; A and B merge at limb 27: 104 humans
        cells = _grid(128, 128, 11, 6)
        people = [(cells[i], {**FRAG_A, **FRAG_B}) for i in range(64)] + [(cells[64 + i], arm) for i in range(40)]
        return Case("asm_b_" + np.dtype(dtype).name, _render(128, 128, people, keep, dtype=dtype, seed=6), 64, 512)
    if kind == "c":
        # 96 people of three fragments (A at limb 0, B at limb 7, merged at limb 27, C at limb 29 from heat planes scaled so low
        # that `total / count < 0.45` prunes it) and one person of fragment A alone: 289 births.  Before limb 29 the table
        # holds 193 slots of which 97 are live; its first 64 connections make 193 + 64 = 257 > kSlots: the table is compacted.
        cells = _grid(128, 128, 12, 6)
        people = [(cells[i], {**FRAG_A, **FRAG_B, **FRAG_C}) for i in range(96)] + [(cells[96], FRAG_A)]
        return Case("asm_c_" + np.dtype(dtype).name,
                    _render(128, 128, people, keep, heat_scale={8: 0.2, 11: 0.2}, limb_scale={L_RHIP_LHIP: 0.4}, dtype=dtype,
                            seed=7), 128, 512)
    if kind == "d":      # 3 x 88 two- or three-joint people that never merge: 264 live.  Arms and legs are pruned (88 humans).
        cells = _grid(160, 160, 9, 5)
        assert len(cells) >= 264
        people = ([(cells[i], TWO) for i in range(88)] + [(cells[88 + i], arm) for i in range(88)]
                  + [(cells[176 + i], leg) for i in range(88)])
        return Case("asm_d_" + np.dtype(dtype).name,
                    _render(160, 160, people, keep, heat_scale={5: 0.2, 6: 0.2, 7: 0.2, 8: 0.2, 9: 0.2, 10: 0.2},
                            limb_scale={L_LSHO_LELB: 0.3, L_LELB_LWRI: 0.3, L_RHIP_RKNE: 0.3, L_RKNE_RANK: 0.3}, dtype=dtype,
                            seed=8), 128, 640)
    raise ValueError(kind)


# ---- 4. / 5. humans per record; more than 64 connections of one limb
def humans_case(n, split=False, dtype=np.float32):
    """n two-joint people.  split = False: all of them neck + nose, so limb 0 has n connections (more than 64: the second
    pass of the wave form) and the scene needs maxp = 128.  split = True: a third each on limbs (1, 0), (5, 6) and (8, 9), at
    most 43 peaks per part, for the paths that take at most 64 peaks per part."""
    cells = _grid(160, 160, 13, 8)
    assert len(cells) >= n
    kinds = [TWO, {5: (0, -8), 6: (0, 8)}, {8: (0, -8), 9: (0, 8)}]
    people = [(cells[i], kinds[i % 3] if split else TWO) for i in range(n)]
    keep = {L_NECK_NOSE, L_LSHO_LELB, L_RHIP_RKNE}
    return Case(f"humans_{n}{'_split' if split else ''}_{np.dtype(dtype).name}",
                _render(160, 160, people, keep, dtype=dtype, seed=9), 64 if split else 128, 640, extra={"n": n})


# ------------------------------------------------------------------------------------------------ the counting restatement
def connections_of(want):
    """the oracle's connections and peak scores in the form test_assembly_batching_equivalence's functions take"""
    conns = [[{"id1": c[3], "id2": c[4], "score": np.float32(c[2]), "len": np.float32(c[5])} for c in want["connections"][l]]
             for l in range(30)]
    ps = [np.float32(s) for s in want["peaks"][:, 2]]
    return conns, ps


def count_assembly(want, slots=K_SLOTS):
    """Replays the oracle's connections through the reference loop (scan_and_apply, one connection at a time) and counts what
    decides the branches of assemble_image_wave:
      births, max_live, max_births_in_limb, humans (after the prune), nb_before[limb] = S.nb when limb `limb` starts, and
      passes = [(limb, pass index, S.nb before the pass, S.nb at dispatch (after a compaction), connections in the pass,
                 NB template argument)]; a pass was compacted when S.nb before + connections > slots.
    S.nb follows the kernel: connections go in passes of 64; before a pass the table is compacted to the live count when
    S.nb + mc > slots; births of a pass take the next slots; `overflow` when a birth finds no slot."""
    conns, ps = connections_of(want)
    skel = []
    births = max_live = max_births_in_limb = 0
    nb, overflow, compactions = 0, False, 0
    nb_before, passes = [], []
    for limb, (part1, part2) in enumerate(LIMBS):
        nb_before.append(nb)
        born_in_limb = 0
        cs = conns[limb]
        for p0 in range(0, len(cs), 64):
            mc = min(64, len(cs) - p0)
            nb_in = nb
            if nb + mc > slots:
                nb = min(len(skel), slots)     # after an overflow the kernel's table no longer follows the reference
                compactions += 1
            template = (1 if nb <= 64 else 2 if nb <= 128 else 4) if p0 == 0 else 4
            passes.append((limb, p0 // 64, nb_in, nb, mc, template))
            for c in cs[p0:p0 + mc]:
                before = len(skel)
                erased, _ = scan_and_apply(skel, part1, part2, c, ps)
                if erased is None and len(skel) == before + 1:
                    births += 1
                    born_in_limb += 1
                    if nb < slots:
                        nb += 1
                    else:
                        overflow = True
                max_live = max(max_live, len(skel))
        max_births_in_limb = max(max_births_in_limb, born_in_limb)
    kept = [row for row in skel if not (row[0][19] < 2 or row[1][18] / np.float32(row[0][19]) < np.float32(0.45))]
    return {"births": births, "max_live": max_live, "max_births_in_limb": max_births_in_limb, "nb_before": nb_before,
            "passes": passes, "compactions": compactions, "overflow": overflow, "humans": len(kept),
            "ids": np.array([row[0][:NUM_PART] for row in kept], np.int32).reshape(-1, NUM_PART),
            "max_connections": max(len(c) for c in conns)}


def peaks_per_part(joint_list):
    return np.bincount(joint_list[:, 4].astype(int), minlength=NUM_PART)[:NUM_PART]


# ------------------------------------------------------------------------------------------------ shared oracle results
_cache = {}


def oracle_pipeline(oracle, case):
    """oracle.pipeline of a case, computed once per session and never modified"""
    if case.name not in _cache:
        _cache[case.name] = oracle.pipeline(case.net, case.min_img_size, flip=False)
    return _cache[case.name]


_cases = {}


def get_case(maker, *args, **kw):
    key = (maker.__name__, args, tuple(sorted((k, np.dtype(v).name if k == "dtype" else v) for k, v in kw.items())))
    if key not in _cases:
        _cases[key] = maker(*args, **kw)
    return _cases[key]


# ------------------------------------------------------------------------------------------------ the case lists both files use
PEAK_CASES = [(33, 47, 10, "float32"), (64, 64, 20, "float32"), (64, 64, 20, "float16")]   # w = 47: mask8's ragged branch
CAND_EXACT_CASES = [(16, 32, 32, "float32"), (16, 16, 16, "float32"), (16, 32, 32, "float16")]
CAND_OVER_CASE = (17, 32, 32, "float32")
ASM_EXACT_CASES = [("a", "float32"), ("b", "float32"), ("c", "float32"), ("c", "float16")]
HUMANS_EXACT_CASES = [(128, False, "float32"), (128, True, "float32"), (128, True, "float16")]


def peaks_neighbours(h, w, dtype):
    """two ordinary images for the batch around a peak-overflow image: few people, so that they stay under its capacity"""
    return [ordinary_scene(31, h, w, 3, dtype), ordinary_scene(32, h, w, 4, dtype)]


def neighbours(h, w, dtype=np.float32):
    return [ordinary_scene(77, h, w, 7, dtype), ordinary_scene(78, h, w, 5, dtype)]
