"""CPU: the ground the device renderer (pp_draw_humans_u8, csrc/posepaf_draw.hip) stands on.

1. The argument that lets it run one thread per pixel: utils.draw.draw_humans -- primitive after primitive inside bounding
   boxes, later over earlier -- equals "every pixel takes the last primitive in draw order whose test holds", with no box at all
   (tests/draw_reference.py:render_last_hit), on a few thousand random people.
2. posepaf.render.record_to_humans builds from a record what demo_image.process builds (demo_image.py:83-92).
3. evaluate.py --render_dir is a refactored-path option and says so before anything touches the GPU."""
import numpy as np
import pytest

from draw_reference import make_record, random_parts, render_last_hit


def _check(canvas, people):
    from posepaf.render import record_to_humans
    from utils import draw
    humans = record_to_humans(make_record(people))          # the people as the renderers meet them: through a record
    assert len(humans) == sum(1 for p in people if p)
    want = draw.draw_humans(canvas.copy(), humans)
    got = render_last_hit(canvas, humans)
    assert np.array_equal(got, want)
    return int((want != canvas).any(axis=2).sum())


def test_last_hit_per_pixel_equals_draw_humans_on_random_people():
    """2400 random people in 300 scenes on canvases from 1 x 1 to 40 x 56: absent parts, coincident joints, joints up to 12 px
    outside the canvas on every side (negative coordinates included), crowded so that draw order decides most pixels."""
    rng = np.random.default_rng(2024)
    shapes = [(1, 1), (1, 7), (5, 1), (3, 3), (8, 13), (16, 16), (23, 31), (40, 56)]
    painted = 0
    for scene in range(300):
        h, w = shapes[scene % len(shapes)]
        canvas = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        people = [random_parts(rng, -12, w + 11, -12, h + 11, p_absent=float(rng.choice([0.0, 0.3, 0.8])))
                  for _ in range(8)]
        painted += _check(canvas, people)
    assert painted > 10_000            # the comparison is not between untouched canvases


def test_last_hit_edge_cases():
    """joints exactly on and just past every border, a limb between two coincident joints (den == 0), a limb whose joints are
    both outside with the segment crossing the canvas, far-away people that must leave the canvas alone"""
    canvas = np.random.default_rng(1).integers(0, 256, (24, 24, 3), dtype=np.uint8)
    for c in (-6, -5, -4, -1, 0, 23, 24, 27, 28, 29):
        assert _check(canvas, [{1: (c, 12), 2: (12, c)}]) >= 0
        _check(canvas, [{1: (c, c), 2: (c, c), 3: (23 - c, c)}])
    assert _check(canvas, [{1: (5, 5), 2: (5, 5)}]) > 0                      # den == 0: u = 0, a dot of radius 1.5
    assert _check(canvas, [{1: (-10, 3), 2: (40, 20)}]) > 0                  # both ends outside, the limb crosses
    assert _check(canvas, [{1: (-300, -300), 2: (-200, 500)}, {5: (30, 30)}]) == 0
    assert _check(np.zeros((1, 1, 3), np.uint8), [{0: (2, 3)}]) == 1          # 2^2 + 3^2 = 13 <= 20.25
    assert _check(np.zeros((1, 1, 3), np.uint8), [{0: (4, 3)}]) == 0          # 25 > 20.25


def _demo_humans(rec):
    """demo_image.py:83-92 as demo_image.process runs it (its record loop, verbatim), coordinates as that path holds them"""
    from posepaf.api import record_humans
    from utils.common import BodyPart, Human
    is_float = bool(int(rec["status"]) & 32)
    humans = []
    for hid, hm in enumerate(record_humans(rec)):
        human = Human([])
        xs, ys = (hm["x"].view(np.float32), hm["y"].view(np.float32)) if is_float else (hm["x"], hm["y"])
        for part in range(18):
            if hm["ids"][part] >= 0:
                x, y = (float(xs[part]), float(ys[part])) if is_float else (int(xs[part]), int(ys[part]))
                human.body_parts[part] = BodyPart("%d-%d" % (hid, part), part, x, y, float(hm["part_score"][part]))
        if human.body_parts:
            human.score = hm["score"]
            humans.append(human)
    return humans


@pytest.mark.parametrize("float_coords", [False, True])
def test_record_to_humans_builds_what_the_demo_builds(float_coords):
    from posepaf.render import draw_record_numpy, record_to_humans
    from utils import draw
    rng = np.random.default_rng(5)
    people = [random_parts(rng, -8, 70, -8, 50) for _ in range(5)] + [{}]            # the last person has no part: dropped
    if float_coords:
        people = [{p: (x + 0.75, y - 0.5) for p, (x, y) in parts.items()} for parts in people]
    rec = make_record(people, float_coords)
    got, want = record_to_humans(rec), _demo_humans(rec)
    assert len(got) == len(want) == 5
    for g, w in zip(got, want):
        assert sorted(g.body_parts) == sorted(w.body_parts) and g.score == w.score
        for p in g.body_parts:
            a, b = g.body_parts[p], w.body_parts[p]
            assert (a.uidx, a.part_idx, a.x, a.y, a.score) == (b.uidx, b.part_idx, b.x, b.y, b.score)
            assert type(a.x) is type(b.x) and a.x == people[int(a.uidx.split("-")[0])][p][0]
    canvas = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    keep = canvas.copy()
    out = draw_record_numpy(canvas, rec)
    assert np.array_equal(canvas, keep)                                                # the input is left alone
    assert np.array_equal(out, draw.draw_humans(canvas.copy(), want)) and (out != canvas).any()
    # a float record is drawn at the truncated coordinates (int(bp.x): towards zero, also below zero)
    if float_coords:
        trunc = make_record([{p: (int(x), int(y)) for p, (x, y) in parts.items()} for parts in people])
        assert np.array_equal(out, draw_record_numpy(canvas, trunc))


def test_record_to_humans_clamps_the_human_count():
    from posepaf.render import record_to_humans
    rec = make_record([{0: (1, 2)}])
    rec["n_humans"] = -3
    assert record_to_humans(rec) == []
    rec["n_humans"] = 100000
    assert len(record_to_humans(rec)) == 128


def test_evaluate_refuses_render_dir_on_the_original_path(tmp_path):
    import torch

    import evaluate
    a = evaluate.parse(["--run_refactor", "--synthetic", "4", "--render_dir", str(tmp_path / "r")])
    assert a.render_dir == str(tmp_path / "r") and a.render_format == "npy"
    assert evaluate.parse(["--synthetic", "4"]).render_dir is None
    was_initialised = torch.cuda.is_initialized()
    with pytest.raises(SystemExit, match="refactored path only"):
        evaluate.main(["--synthetic", "4", "--render_dir", str(tmp_path / "r")])
    assert torch.cuda.is_initialized() == was_initialised and not (tmp_path / "r").exists()


def test_engine_takes_the_render_keyword_last():
    """render is a new TRAILING keyword of InferenceEngine, default off: every existing caller is untouched"""
    import inspect

    from posepaf.engine import InferenceEngine
    params = list(inspect.signature(InferenceEngine.__init__).parameters.values())
    assert params[-1].name == "render" and params[-1].default is False
