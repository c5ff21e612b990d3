"""GPU: pp_draw_limbs_u8 (csrc/posepaf_limbs.hip) -- the ellipse / alpha-blend style of the demo's original branch, a whole
bucket drawn in one launch straight from device-side records -- against the NumPy renderer utils.draw.draw_limbs_original, byte
for byte: hand-made records, ragged sizes, two-buffer and in-place forms, a crowd whose 2304 instances cross the LDS chunks,
float-coordinate records, hipGraph replay, bad arguments, the original path's ragged bucket end to end, evaluate.py.

The case builders at the top are imported by tests/test_draw_limbs_cpu.py, which checks on the CPU that the per-instance
parameters of every coordinate set used here come out of sqrt + pp_limb_angle_deg as draw.py forms them."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ragged_cases as rc
from conftest import PKG
from draw_reference import make_record, random_parts
from limb_draw_reference import fold, fractional, instances_drawpy

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SLOTS = [(64, 64), (61, 77), (128, 192)]       # one tile row; an odd row pitch (the byte path); several tiles both ways


def slot_records(hp, wp):
    """the four images of a slot: nobody; two people with absent parts, one touching pixel (0, 0); nine random people with
    joints from -8 to wp + 8; one person with a limb across the whole slot (an ellipse over several tiles: 1 -> 2), a
    zero-length limb (2 -> 3) and limbs at 0 (8 -> 9), 90 (9 -> 10), 45 (11 -> 12) and -135 degrees (12 -> 13)"""
    rng = np.random.default_rng(hp * 1000 + wp + 1)
    two = [{0: (0, 0), 1: (10, 14), 2: (wp - 9, 20), 5: (wp // 2, hp - 3), 14: (6, 2)},
           {1: (wp // 2, hp // 2), 8: (wp // 2 + 9, hp - 1), 9: (5, hp + 4), 11: (wp // 2 - 7, hp - 8)}]
    nine = [random_parts(rng, -8, wp + 8, -8, hp + 8, p_absent=0.25, p_coincident=0.2) for _ in range(9)]
    special = [{1: (2, 3), 2: (wp - 3, hp - 2), 3: (wp - 3, hp - 2), 8: (40, 30), 9: (20, 30), 10: (20, 10), 11: (30, 40),
                12: (18, 28), 13: (27, 37)}]
    return np.stack([make_record([]), make_record(two), make_record(nine), make_record(special)])


def slot_sizes(hp, wp, ragged):
    if not ragged:
        return None
    return np.array([[hp, 1, hp - 13, hp - 1], [wp - 3, 1, wp - 5, wp]], np.int32)


def crowd_record():
    """128 humans with all 18 parts inside one 24 x 24 region of a 64 x 64 image: 2304 instances over the same pixels"""
    rng = np.random.default_rng(77)
    return make_record([random_parts(rng, 20, 43, 18, 41, p_absent=0.0, p_coincident=0.1) for _ in range(128)])


def float_records(hp=48, wp=80):
    """[fractional and negative float32 coordinates, the truncated integers]: the rings of both sit on the same pixels"""
    rng = np.random.default_rng(3)
    ints = [random_parts(rng, -6, wp + 6, -6, hp + 6, p_absent=0.3) for _ in range(6)]
    frac = fractional(ints)
    frac[0][0], ints[0][0] = (-0.9, 0.99), (0, 0)                             # truncates to (0, 0), not to (-1, 0)
    frac[0][1], ints[0][1] = (12.25, 9.5), (12, 9)
    return np.stack([make_record(frac, float_coords=True), make_record(ints)])


def graph_record_sets(hp=61, wp=128):
    rng = np.random.default_rng(11)
    return [np.stack([make_record([random_parts(rng, -8, wp + 8, -8, hp + 8) for _ in range(n)]) for n in counts])
            for counts in ((3, 0, 12), (1, 40, 2))]


def all_records():
    """every hand-made record of this file (the CPU test walks their instances)"""
    out = [crowd_record()]
    for hp, wp in SLOTS:
        out.extend(slot_records(hp, wp))
    out.extend(float_records())
    for s in graph_record_sets():
        out.extend(s)
    return out


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_CASES = {}


def _case(hp, wp, ragged):
    """(src, records, sizes or None, [(h, w)], [NumPy drawing of each image's corner]) -- computed once, shared, never modified"""
    key = (hp, wp, ragged)
    if key not in _CASES:
        from posepaf.render import draw_limbs_record_numpy
        src = np.random.default_rng(hp + wp).integers(0, 256, (4, hp, wp, 3), dtype=np.uint8)
        recs, sizes = slot_records(hp, wp), slot_sizes(hp, wp, ragged)
        hw = [(hp, wp)] * 4 if sizes is None else [(int(sizes[0, b]), int(sizes[1, b])) for b in range(4)]
        want = [draw_limbs_record_numpy(src[b, :h, :w], recs[b]) for b, (h, w) in enumerate(hw)]
        for a in (src, recs):
            a.setflags(write=False)
        _CASES[key] = (src, recs, sizes, hw, want)
    return _CASES[key]


def _to_dev(torch, recs):
    return torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1).copy()).cuda()


@pytest.mark.parametrize("in_place", [False, True], ids=["two_buffers", "in_place"])
@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("slot", SLOTS, ids=lambda s: "%dx%d" % s)
def test_equals_the_numpy_renderer(torch_cuda, slot, ragged, in_place):
    from posepaf.render import draw_limbs_records
    torch = torch_cuda
    hp, wp = slot
    src, recs, sizes, hw, want = _case(hp, wp, ragged)
    src_dev = torch.from_numpy(src.copy()).cuda()
    sizes_dev = None if sizes is None else torch.from_numpy(sizes).cuda()
    dst_dev = src_dev if in_place else torch.full((4, hp, wp, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    out = draw_limbs_records(src_dev, _to_dev(torch, recs), sizes_dev, out=dst_dev)
    assert out is dst_dev
    got = out.cpu().numpy()
    if not in_place:
        assert np.array_equal(src_dev.cpu().numpy(), src)                   # the source is only read
    outside = src if in_place else np.full_like(src, SENTINEL)
    for b, (h, w) in enumerate(hw):
        assert np.array_equal(got[b, :h, :w], want[b]), f"image {b}: {(got[b, :h, :w] != want[b]).any(axis=2).sum()} pixels differ"
        rest = np.ones((hp, wp), bool)
        rest[:h, :w] = False
        assert np.array_equal(got[b][rest], outside[b][rest]), f"image {b}: written outside its {h} x {w} corner"
    for b in (2, 3):
        assert (want[b] != src[b, :hw[b][0], :hw[b][1]]).any(), b            # pixels changed
    assert np.array_equal(want[0], src[0, :hw[0][0], :hw[0][1]])


def test_a_crowd_folds_in_draw_order_across_the_chunks(torch_cuda):
    """2304 instances (nine LDS chunks) over the same 24 x 24 region: every channel there is the fold of hundreds of blends, so
    one instance out of order shows.  Held to the helper's per-pixel fold, which test_draw_limbs_cpu.py holds to draw.py."""
    from posepaf.render import draw_limbs_records, record_to_persons
    torch = torch_cuda
    rec = crowd_record()
    insts = instances_drawpy(*record_to_persons(rec))
    assert len(insts) == 18 * 128
    src = np.random.default_rng(5).integers(0, 256, (1, 64, 64, 3), dtype=np.uint8)
    want = fold(src[0], insts)
    got = draw_limbs_records(torch.from_numpy(src).cuda(), _to_dev(torch, np.stack([rec]))).cpu().numpy()[0]
    assert np.array_equal(got, want), f"{(got != want).any(axis=2).sum()} pixels differ"
    assert (want != src[0]).any(axis=2).sum() > 24 * 24


def test_float_coordinate_records(torch_cuda):
    """rings at the truncated centres, the ellipse from the un-truncated differences"""
    from posepaf.render import draw_limbs_record_numpy, draw_limbs_records
    torch = torch_cuda
    recs = float_records()
    src = np.repeat(np.random.default_rng(3).integers(0, 256, (1, 48, 80, 3), dtype=np.uint8), 2, axis=0)
    got = draw_limbs_records(torch.from_numpy(src).cuda(), _to_dev(torch, recs)).cpu().numpy()
    for b in range(2):
        want = draw_limbs_record_numpy(src[b], recs[b])
        assert np.array_equal(got[b], want) and (want != src[b]).any(), b
    # joint (-0.9, 0.99) rings pixel (0, 0), not (-1, 0): (x, y) = (3, 0) is on that ring (9 <= 9) in both records
    assert (got[:, 0, 3] != src[:, 0, 3]).any(axis=1).all()


def test_graph_replay_over_two_record_sets(torch_cuda):
    from posepaf.render import draw_limbs_record_numpy, draw_limbs_records, limb_angle_table_dev
    torch = torch_cuda
    hp, wp = 61, 128
    sets = graph_record_sets(hp, wp)
    rng = np.random.default_rng(12)
    srcs = [rng.integers(0, 256, (3, hp, wp, 3), dtype=np.uint8) for _ in range(2)]
    sizes = torch.tensor([[hp, hp - 7, 33], [wp, wp - 2, 100]], dtype=torch.int32, device="cuda")
    hw = [(hp, wp), (hp - 7, wp - 2), (33, 100)]
    limb_angle_table_dev("cuda")                                             # built outside the capture
    static_src, static_rec = torch.from_numpy(srcs[0]).cuda(), _to_dev(torch, sets[0])
    static_out = torch.zeros_like(static_src)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        draw_limbs_records(static_src, static_rec, sizes, out=static_out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        draw_limbs_records(static_src, static_rec, sizes, out=static_out)
    want = [[draw_limbs_record_numpy(srcs[k][b, :h, :w], sets[k][b]) for b, (h, w) in enumerate(hw)] for k in range(2)]
    for rep in range(4):
        k = rep % 2
        static_src.copy_(torch.from_numpy(srcs[k]).cuda())
        static_rec.copy_(_to_dev(torch, sets[k]))
        g.replay()
        got = static_out.cpu().numpy()
        for b, (h, w) in enumerate(hw):
            assert np.array_equal(got[b, :h, :w], want[k][b]), (rep, b)
    assert (want[1][1] != srcs[1][1, :hw[1][0], :hw[1][1]]).any()


def test_bad_arguments_write_nothing(torch_cuda):
    from posepaf import _lib
    from posepaf.render import limb_angle_table_dev
    torch = torch_cuda
    L = _lib.load()
    src = torch.full((1, 16, 16, 3), 200, dtype=torch.uint8, device="cuda")
    dst = torch.full((1, 16, 16, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    rec = _to_dev(torch, np.stack([make_record([{1: (8, 8), 0: (8, 8)}])]))
    tab = limb_angle_table_dev("cuda")
    r, s, d, t = (C.c_void_p(v.data_ptr()) for v in (rec, src, dst, tab))
    for args in ((r, s, d, None, 1, 16, 16, None), (None, s, d, None, 1, 16, 16, t), (r, s, d, None, 0, 16, 16, t),
                 (r, s, d, None, -1, 16, 16, t), (r, None, d, None, 1, 16, 16, t), (r, s, None, None, 1, 16, 16, t),
                 (r, s, d, None, 1, 0, 16, t), (r, s, d, None, 1, 16, -2, t)):
        assert L.pp_draw_limbs_u8(*args, None) == -2          # PP_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == SENTINEL).all()
    assert L.pp_draw_limbs_u8(r, s, d, None, 1, 16, 16, t, None) == 0
    got = dst.cpu().numpy()[0]
    assert tuple(got[8, 8]) == (157, 148, 230)                 # rint(200 * 0.4 + (128, 114, 250) * 0.6): the dot of a = 0.5
    assert tuple(got[8, 11]) == (80, 80, 80) and tuple(got[0, 0]) == (200, 200, 200)    # the ring; an untouched pixel is copied


def test_the_original_path_draws_its_ragged_bucket_from_device_records(torch_cuda):
    """tests/ragged_cases.py's bucket through OriginalPathProcessor to finish, then drawn from the records where they are with
    the bucket's own size rows: each corner equals the NumPy drawing of the host copy of its record, the rest of each slot is
    left as it was"""
    from posepaf.api import PosePostProcessor, records_to_numpy
    from posepaf.original_path import OriginalPathProcessor, RaggedBucket
    from posepaf.render import draw_limbs_record_numpy, draw_limbs_records
    torch = torch_cuda
    post = PosePostProcessor(max_batch=4, max_h=48, max_w=48, max_peaks_per_part=64)
    try:
        per_image = [rc.scene_maps(size, people, seed, np.float16) for size, (people, seed) in zip(rc.SIZES, rc.SCENES)]
        maps = [torch.from_numpy(np.stack([m[i] for m in per_image])).cuda() for i in range(len(rc.SCALES))]
        rg = RaggedBucket(rc.SIZES, rc.SCALES, torch.device("cuda", post.device))
        proc = OriginalPathProcessor(post, None, None, 4, slot_area=rg.slot_area)
        proc.reset(rg)
        for i, m in enumerate(maps):
            proc.accumulate(m, *rg.pads(i), len(maps), flip=True)
        rec_dev = proc.finish(4)
        images = np.random.default_rng(8).integers(0, 256, (4,) + rc.SLOT + (3,), dtype=np.uint8)
        canvas = torch.full((4,) + rc.SLOT + (3,), SENTINEL, dtype=torch.uint8, device="cuda")
        out = draw_limbs_records(torch.from_numpy(images).cuda(), rec_dev, rg.dev[0], out=canvas)
        got, recs = out.cpu().numpy(), records_to_numpy(rec_dev)
    finally:
        post.close()
    changed = 0
    for b, (h, w) in enumerate(rc.SIZES):
        assert int(recs[b]["status"]) == 32 and int(recs[b]["n_humans"]) > 0, b
        want = draw_limbs_record_numpy(images[b, :h, :w], recs[b])
        assert np.array_equal(got[b, :h, :w], want), b
        rest = np.ones(rc.SLOT, bool)
        rest[:h, :w] = False
        assert (got[b][rest] == SENTINEL).all(), b
        changed += int((want != images[b, :h, :w]).any(axis=2).sum())
    assert changed > 100


def test_evaluate_renders_the_original_path(tmp_path):
    d = tmp_path / "limbs"
    r = subprocess.run([sys.executable, os.path.join(PKG, "evaluate.py"), "--synthetic", "8", "--sizes", "120x100,128x128",
                        "--batch", "4", "--scales", "1.0", "--people", "2", "3", "--render_limbs_dir", str(d),
                        "--dump_name", str(tmp_path / "res.json")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    summary = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps(summary))
    assert summary["images"] == 8 and summary["rendered_files"] == 8
    import evaluate
    src = evaluate.SyntheticSource(8, [(120, 100), (128, 128)], [2, 3])
    differ = 0
    for i in range(8):
        got = np.load(d / ("%06d.npy" % i))
        assert got.shape == src.shape(i) + (3,) and got.dtype == np.uint8, i
        differ += int(not np.array_equal(got, src.load(i)))
    assert differ >= 1
