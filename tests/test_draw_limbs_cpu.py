"""CPU: the ground the device renderer of the original branch's style (pp_draw_limbs_u8, csrc/posepaf_limbs.hip) stands on.

1. rint(c 0.4 + c 0.6) == c for every byte: draw.py's whole-canvas blend leaves a pixel nothing hits as it was.
2. So utils.draw.draw_limbs_original equals a per-pixel ordered fold with no bounding box (tests/limb_draw_reference.py:fold).
3. pp_limb_angle_deg -- the host instance of the kernel's libm-free angle -- equals int(math.degrees(math.atan2(dy, dx))).
4. pp_limb_angle_table holds the bits of math.cos / math.sin of math.radians(k).
5. On every coordinate set the GPU tests use, sqrt + pp_limb_angle_deg give the per-instance parameters draw.py forms with
   `** 0.5` and atan2: a disagreement would show here and not as a pixel difference on the GPU.
6. posepaf.render.record_to_persons builds what draw_limbs_original takes.
7. evaluate.py --render_limbs_dir is an original-path option and says so before anything touches the GPU."""
import math

import numpy as np
import pytest

from draw_reference import make_record, random_parts
from limb_draw_reference import fold, fractional, instances_device, instances_drawpy


@pytest.fixture(scope="module")
def lib():
    from posepaf import _lib
    return _lib.load()


def test_an_untouched_pixel_survives_the_blend():
    c = np.arange(256, dtype=np.uint8)
    assert np.array_equal(np.clip(np.rint(c.astype(np.float64) * 0.4 + c.astype(np.float64) * 0.6), 0, 255).astype(np.uint8), c)


def _check(canvas, people, float_coords=False):
    from posepaf import skeleton as sk
    from posepaf.render import draw_limbs_record_numpy, record_to_persons
    from utils import draw
    rec = make_record(people, float_coords)                 # the people as the renderers meet them: through a record
    persons, cand = record_to_persons(rec)
    assert len(persons) == sum(1 for p in people if p)
    want = draw.draw_limbs_original(canvas.copy(), persons, cand, sk.LIMB_PAIRS, sk.DRAW_LIST)
    assert np.array_equal(draw_limbs_record_numpy(canvas, rec), want)
    got = fold(canvas, instances_drawpy(persons, cand))
    assert np.array_equal(got, want), f"{(got != want).any(axis=2).sum()} pixels differ"
    return int((want != canvas).any(axis=2).sum())


def _aligned_person(rng, h, w):
    """limbs along the axes and the diagonals, and one between coincident joints (a = 0.5, angle 0)"""
    x, y, d = int(rng.integers(-4, w + 4)), int(rng.integers(-4, h + 4)), int(rng.integers(1, 14))
    return {1: (x, y), 0: (x, y), 2: (x + d, y), 3: (x + d, y - d), 4: (x + 2 * d, y - d), 5: (x - d, y), 6: (x - d, y + d),
            7: (x - 2 * d, y + 2 * d), 8: (x, y + d), 9: (x + d, y + 2 * d), 10: (x + d, y + 2 * d + 3), 11: (x - d, y - d)}


def test_the_per_pixel_fold_equals_draw_limbs_original_on_random_scenes():
    """320 scenes of 8 people on canvases from 1 x 1 to 40 x 56: absent parts, coincident joints, joints up to 12 px outside on
    every side, integer and fractional coordinates, axis-aligned and diagonal limbs"""
    rng = np.random.default_rng(2025)
    shapes = [(1, 1), (1, 7), (5, 1), (3, 3), (8, 13), (16, 16), (23, 31), (40, 56)]
    painted = 0
    for scene in range(320):
        h, w = shapes[scene % len(shapes)]
        canvas = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        people = [random_parts(rng, -12, w + 11, -12, h + 11, p_absent=float(rng.choice([0.0, 0.3, 0.8]))) for _ in range(6)]
        people += [_aligned_person(rng, h, w) for _ in range(2)]
        float_coords = scene % 2 == 1
        if float_coords:
            fx, fy = float(rng.choice([0.25, 0.5, 0.75])), float(rng.choice([0.125, 0.5, 0.875]))
            people = fractional(people[:4], fx, fy) + people[4:]
        painted += _check(canvas, people, float_coords)
    assert painted > 20_000            # the comparison is not between untouched canvases


def test_fold_edge_cases():
    canvas = np.random.default_rng(1).integers(0, 256, (24, 24, 3), dtype=np.uint8)
    for c in (-7, -6, -5, -1, 0, 23, 24, 28, 29, 30):
        _check(canvas, [{1: (c, 12), 2: (12, c)}])
        _check(canvas, [{1: (c, c), 2: (c, c), 3: (23 - c, c)}])
    assert _check(canvas, [{1: (5, 5), 2: (5, 5)}]) > 0                       # a = 0.5, angle 0: a dot inside two rings
    assert _check(canvas, [{1: (-10, 3), 2: (40, 20)}]) > 0                   # both ends outside, the limb crosses
    assert _check(canvas, [{1: (-300, -300), 2: (-200, 500)}, {5: (30, 40)}]) == 0
    assert _check(canvas, [{2: (5, 5), 4: (9, 9)}]) == 0                      # joints, but no limb of the draw list between them


def _py_angle(dy, dx):
    return int(math.degrees(math.atan2(dy, dx)))


def test_angle_exact_directions(lib):
    got = []
    for dy in (0.0, -0.0, 1.0, -1.0, 7.5, -7.5):
        for dx in (0.0, -0.0, 1.0, -1.0, 7.5, -7.5):
            if abs(dy) in (0.0, abs(dx)) or dx == 0.0:
                got.append(lib.pp_limb_angle_deg(dy, dx))
                assert got[-1] == _py_angle(dy, dx), (dy, dx)
    # the sixteen: 4 axis directions x the other coordinate's two zeros, 4 diagonals x 2 lengths; then the four (0, 0)
    assert lib.pp_limb_angle_deg(0.0, 0.0) == 0 and lib.pp_limb_angle_deg(-0.0, -1.0) == -180
    assert [lib.pp_limb_angle_deg(dy, dx) for dy, dx in ((0.0, -0.0), (-0.0, -0.0), (-0.0, 0.0))] == [180, -180, 0]
    assert sorted(set(got)) == [-180, -135, -90, -45, 0, 45, 90, 135, 180]


def test_angle_random_float32_differences(lib):
    rng = np.random.default_rng(7)
    a = rng.uniform(-300, 300, (200_000, 4)).astype(np.float32).astype(np.float64)
    a[::5] = np.rint(a[::5])                                      # a fifth of them integer coordinates
    dys, dxs = a[:, 0] - a[:, 1], a[:, 2] - a[:, 3]
    bad = [(dy, dx) for dy, dx in zip(dys.tolist(), dxs.tolist()) if lib.pp_limb_angle_deg(dy, dx) != _py_angle(dy, dx)]
    assert not bad, bad[:5]


def test_angle_beside_every_integer_degree(lib):
    """the float32 roundings of (R sin j, R cos j), each coordinate also moved by one float32 ulp either way: the directions
    float32 coordinates can put closest to an integer degree, the slivers beside the axes included"""
    n = 0
    for j in range(-180, 181):
        for radius in (1.0, 37.0, 600.0):
            y0, x0 = np.float32(radius * math.sin(math.radians(j))), np.float32(radius * math.cos(math.radians(j)))
            for y in (np.nextafter(y0, np.float32(-np.inf)), y0, np.nextafter(y0, np.float32(np.inf))):
                for x in (np.nextafter(x0, np.float32(-np.inf)), x0, np.nextafter(x0, np.float32(np.inf))):
                    dy, dx = float(y), float(x)
                    assert lib.pp_limb_angle_deg(dy, dx) == _py_angle(dy, dx), (j, radius, dy, dx)
                    n += 1
    assert n == 361 * 3 * 9
    # exact zeros moved by one (subnormal) ulp: atan2 rounds to pi and pi / 2 there
    tiny = float(np.nextafter(np.float32(0), np.float32(1)))
    for dy, dx in ((tiny, -1.0), (-tiny, -1.0), (1.0, tiny), (-1.0, tiny), (1.0, -tiny), (tiny, 1.0), (-tiny, 600.0)):
        assert lib.pp_limb_angle_deg(dy, dx) == _py_angle(dy, dx), (dy, dx)


def test_angle_table_holds_pythons_bits():
    from posepaf.render import limb_angle_table
    tab = limb_angle_table()
    assert tab.shape == (361, 2) and tab.dtype == np.float64
    want = np.array([[math.cos(math.radians(k)), math.sin(math.radians(k))] for k in range(-180, 181)])
    assert tab.tobytes() == want.tobytes()


def test_the_gpu_cases_have_draw_pys_parameters(lib):
    """(ring centres, ellipse centre, a, k, colour) of every instance of every record tests/test_gpu_draw_limbs.py draws,
    through sqrt and pp_limb_angle_deg, against draw.py's `** 0.5` and atan2; and the ragged bucket's kind of record
    (float32 coordinates) is covered by the float records there"""
    from posepaf.render import record_to_persons
    from test_gpu_draw_limbs import all_records
    n = 0
    for rec in all_records():
        want = instances_drawpy(*record_to_persons(rec))
        got = instances_device(rec, lib)
        assert got == want
        n += len(want)
    assert n > 18 * 128 + 500


@pytest.mark.parametrize("float_coords", [False, True])
def test_record_to_persons(float_coords):
    from posepaf.render import persons_to_record, record_to_persons
    rng = np.random.default_rng(5)
    people = [random_parts(rng, -8, 70, -8, 50) for _ in range(3)] + [{}] + [random_parts(rng, -8, 70, -8, 50)]   # one without parts
    if float_coords:
        people = fractional(people, 0.75, 0.5)
    rec = make_record(people, float_coords)
    persons, cand = record_to_persons(rec)
    kept = [p for p in people if p]
    assert persons.shape == (4, 20, 2) and persons.dtype == np.float64 and cand.dtype == np.float64
    assert cand.shape == (sum(len(p) for p in kept), 4) and np.array_equal(cand[:, 3], np.arange(len(cand)))
    row = 0
    for person, parts in zip(persons, kept):
        for part in range(18):
            if part in parts:
                assert person[part, 0] == row and tuple(cand[row, :2]) == tuple(float(np.float32(v)) for v in parts[part])
                assert cand[row, 2] == np.float32(0.25 + part / 32)
                row += 1
            else:
                assert person[part, 0] == -1
        assert person[19, 0] == len(parts)
    assert row == len(cand)
    back = persons_to_record(persons, cand, float_coords)                   # the demo's packer inverts it
    again = record_to_persons(back)
    assert np.array_equal(again[0][:, :18], persons[:, :18]) and np.array_equal(again[1], cand)
    assert int(back["status"]) == (32 if float_coords else 0) and int(back["n_humans"]) == 4


def test_record_to_persons_clamps_the_human_count():
    from posepaf.render import record_to_persons
    rec = make_record([{0: (1, 2)}])
    rec["n_humans"] = -3
    persons, cand = record_to_persons(rec)
    assert persons.shape == (0, 20, 2) and cand.shape == (0, 4)
    rec["n_humans"] = 100000
    assert len(record_to_persons(rec)[0]) == 128


def test_evaluate_refuses_render_limbs_dir_on_the_refactored_path(tmp_path):
    import torch

    import evaluate
    a = evaluate.parse(["--synthetic", "4", "--render_limbs_dir", str(tmp_path / "r")])
    assert a.render_limbs_dir == str(tmp_path / "r") and a.render_format == "npy"
    assert evaluate.parse(["--synthetic", "4"]).render_limbs_dir is None
    was_initialised = torch.cuda.is_initialized()
    with pytest.raises(SystemExit, match="original path only"):
        evaluate.main(["--run_refactor", "--synthetic", "4", "--render_limbs_dir", str(tmp_path / "r")])
    assert torch.cuda.is_initialized() == was_initialised and not (tmp_path / "r").exists()
