"""GPU: pp_draw_humans_u8 (csrc/posepaf_draw.hip) -- a whole bucket of images drawn in one launch straight from device-side
records -- against the NumPy renderer utils.draw.draw_humans, byte for byte: hand-made records (no other kernel involved),
ragged sizes, two-buffer and in-place forms, float-coordinate records, hipGraph replay, the engine's render=True, bad arguments."""
import ctypes as C

import numpy as np
import pytest

from draw_reference import make_record, random_parts

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SLOTS = [(64, 64), (61, 77), (128, 192)]       # one tile row; an odd row pitch (the byte path); several tiles both ways


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _spanning(hp, wp, k):
    """a person whose limbs cross the whole slot (and leave it)"""
    return [{1: (-6, -4), 2: (wp + 5, hp + 3), 3: (wp // 2, -7), 4: (3, hp + 6), 5: (wp + 7, 2), 8: (wp // 3, hp // 2)},
            {0: (wp - 1, 0), 1: (0, hp - 1), 14: (wp // 2, hp // 2), 15: (wp - 2, hp - 2), 16: (2, 2), 11: (wp + 8, hp // 2)},
            {1: (wp // 2, hp // 2), 2: (0, 0), 5: (wp - 1, hp - 1), 8: (0, hp - 1), 11: (wp - 1, 0)}][k]


def _records(hp, wp):
    """the four images of a slot: nobody; two people with absent parts (one touching pixel (0, 0)); nine random people with
    joints from -8 to wp + 8, coincident joints and crossing limbs, so that draw order shows; all 128 people -- 125 packed into
    one 16 x 16 region (the LDS list is consumed in chunks) and three spanning the image, first, in the middle and last"""
    rng = np.random.default_rng(hp * 1000 + wp)
    two = [{0: (2, 1), 1: (10, 14), 2: (wp - 9, 20), 5: (wp // 2, hp - 3)}, {1: (wp // 2, hp // 2), 8: (wp // 2 + 9, hp - 1), 9: (5, hp + 4)}]
    nine = [random_parts(rng, -8, wp + 8, -8, hp + 8, p_absent=0.25, p_coincident=0.2) for _ in range(9)]
    x0, y0 = wp // 2 - 3, hp // 2 - 5
    packed = [random_parts(rng, x0, x0 + 15, y0, y0 + 15, p_absent=0.4) for _ in range(125)]
    crowd = [_spanning(hp, wp, 0)] + packed[:60] + [_spanning(hp, wp, 1)] + packed[60:] + [_spanning(hp, wp, 2)]
    assert len(crowd) == 128
    return np.stack([make_record([]), make_record(two), make_record(nine), make_record(crowd)])


def _sizes(hp, wp, ragged):
    if not ragged:
        return None
    return np.array([[hp, 1, hp - 13, hp - 1], [wp - 3, 1, wp - 5, wp]], np.int32)


_CASES = {}


def _case(hp, wp, ragged):
    """(src, records, sizes or None, [NumPy drawing of each image's corner]) -- computed once, shared, never modified"""
    key = (hp, wp, ragged)
    if key not in _CASES:
        from posepaf.render import draw_record_numpy
        src = np.random.default_rng(hp + wp).integers(0, 256, (4, hp, wp, 3), dtype=np.uint8)
        recs, sizes = _records(hp, wp), _sizes(hp, wp, ragged)
        hw = [(hp, wp)] * 4 if sizes is None else [(int(sizes[0, b]), int(sizes[1, b])) for b in range(4)]
        want = [draw_record_numpy(src[b, :h, :w], recs[b]) for b, (h, w) in enumerate(hw)]
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
    from posepaf.render import draw_records
    torch = torch_cuda
    hp, wp = slot
    src, recs, sizes, hw, want = _case(hp, wp, ragged)
    src_dev = torch.from_numpy(src.copy()).cuda()
    sizes_dev = None if sizes is None else torch.from_numpy(sizes).cuda()
    dst_dev = src_dev if in_place else torch.full((4, hp, wp, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    out = draw_records(src_dev, _to_dev(torch, recs), sizes_dev, out=dst_dev)
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
    assert (want[3] != src[3, :hw[3][0], :hw[3][1]]).any() and np.array_equal(want[0], src[0, :hw[0][0], :hw[0][1]])


def test_float_coordinate_records_draw_at_the_truncated_pixels(torch_cuda):
    from posepaf.render import draw_record_numpy, draw_records
    torch = torch_cuda
    hp, wp = 48, 80
    rng = np.random.default_rng(3)
    ints = [random_parts(rng, -6, wp + 6, -6, hp + 6, p_absent=0.3) for _ in range(6)]
    frac = [{p: (x + (0.75 if x >= 0 else -0.75), y + (0.5 if y >= 0 else -0.5)) for p, (x, y) in parts.items()} for parts in ints]
    frac[0][0] = (-0.9, 0.99)                                                # truncates to (0, 0), not to (-1, 0)
    ints[0][0] = (0, 0)
    src = np.repeat(rng.integers(0, 256, (1, hp, wp, 3), dtype=np.uint8), 2, axis=0)      # the same picture twice
    recs = np.stack([make_record(frac, float_coords=True), make_record(ints)])
    got = draw_records(torch.from_numpy(src).cuda(), _to_dev(torch, recs)).cpu().numpy()
    want = draw_record_numpy(src[0], recs[0])
    assert np.array_equal(got[0], want) and (want != src[0]).any()
    assert np.array_equal(got[1], got[0]) and np.array_equal(got[1], draw_record_numpy(src[1], recs[1]))


def test_graph_replay_over_two_record_sets(torch_cuda):
    from posepaf.render import draw_record_numpy, draw_records
    torch = torch_cuda
    hp, wp = 61, 128
    rng = np.random.default_rng(11)
    sets = [np.stack([make_record([random_parts(rng, -8, wp + 8, -8, hp + 8) for _ in range(n)]) for n in counts])
            for counts in ((3, 0, 12), (1, 40, 2))]
    srcs = [rng.integers(0, 256, (3, hp, wp, 3), dtype=np.uint8) for _ in range(2)]
    sizes = torch.tensor([[hp, hp - 7, 33], [wp, wp - 2, 100]], dtype=torch.int32, device="cuda")
    hw = [(hp, wp), (hp - 7, wp - 2), (33, 100)]
    eager = [draw_records(torch.from_numpy(s).cuda(), _to_dev(torch, r), sizes).cpu().numpy() for s, r in zip(srcs, sets)]
    static_src, static_rec = torch.from_numpy(srcs[0]).cuda(), _to_dev(torch, sets[0])
    static_out = torch.zeros_like(static_src)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        draw_records(static_src, static_rec, sizes, out=static_out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        draw_records(static_src, static_rec, sizes, out=static_out)
    for rep in range(4):
        k = rep % 2
        static_src.copy_(torch.from_numpy(srcs[k]).cuda())
        static_rec.copy_(_to_dev(torch, sets[k]))
        g.replay()
        got = static_out.cpu().numpy()
        for b, (h, w) in enumerate(hw):
            assert np.array_equal(got[b, :h, :w], eager[k][b, :h, :w]), (rep, b)
            assert np.array_equal(got[b, :h, :w], draw_record_numpy(srcs[k][b, :h, :w], sets[k][b])), (rep, b)


def test_engine_render_canvas(torch_cuda):
    """InferenceEngine(render=True) on the post-processing alone: after submit, plan.canvas holds the NumPy drawing of
    plan.records on the slot's images, corner by corner, under graph replay and eagerly; the records are those of render=False."""
    from posepaf import synth
    from posepaf.api import PosePostProcessor, records_to_numpy
    from posepaf.engine import InferenceEngine
    from posepaf.render import draw_record_numpy
    torch = torch_cuda
    bank = np.stack([synth.make_net_output(p, 900 + p, h=64, w=64, dtype=np.float16) for p in (0, 1, 3, 5, 2)])
    rng = np.random.default_rng(21)
    batches = []
    for k in range(2):
        hw = [(256, 256), (200, 251), (193, 256), (256, 197)] if k == 0 else [(255, 255), (256, 256), (222, 203), (199, 256)]
        batches.append((hw, [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in hw], [(k + j + 1) % 5 for j in range(4)]))
    post = PosePostProcessor(max_batch=4, max_h=64, max_w=64, max_peaks_per_part=64)
    try:
        results = {}
        for render in (True, False):
            for use_graph in (True, False):
                eng = InferenceEngine(None, post, 4, 0, rules="cpp", use_graph=use_graph, postproc_only=True,
                                      max_image_hw=(256, 256), render=render)
                plan = eng.plan(256, 256)
                assert (plan.canvas is not None) == render
                eng.set_bank(plan, bank)
                eng.prepare(plan)
                assert (plan.graph is not None) == use_graph
                out = []
                for hw, imgs, idx in batches:
                    slot = eng.acquire()
                    sizes, bank_idx, slot_imgs = slot.views(4, 256, 256)
                    for j, ((h, w), im) in enumerate(zip(hw, imgs)):
                        slot_imgs[j, :h, :w] = im
                        sizes[0, j], sizes[1, j], bank_idx[j] = h, w, idx[j]
                    rec_dev = eng.submit(slot, plan)
                    eng.sync()
                    recs = records_to_numpy(rec_dev)
                    out.append(rec_dev.cpu().numpy().tobytes())
                    if render:
                        assert tuple(plan.canvas.shape) == (4, 256, 256, 3)
                        canvas = plan.canvas.cpu().numpy()
                        for j, ((h, w), im) in enumerate(zip(hw, imgs)):
                            want = draw_record_numpy(im, recs[j])
                            assert np.array_equal(canvas[j, :h, :w], want), (use_graph, j)
                        assert sum(int(r["n_humans"]) for r in recs) > 0
                results[(render, use_graph)] = out
        assert results[(True, True)] == results[(False, True)] == results[(True, False)] == results[(False, False)]
    finally:
        post.close()


def test_bad_arguments_write_nothing(torch_cuda):
    from posepaf import _lib
    torch = torch_cuda
    L = _lib.load()
    src = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    dst = torch.full((1, 8, 8, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    rec = _to_dev(torch, np.stack([make_record([{0: (4, 4)}])]))
    r, s, d = C.c_void_p(rec.data_ptr()), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())
    for args in ((None, s, d, None, 1, 8, 8), (r, None, d, None, 1, 8, 8), (r, s, None, None, 1, 8, 8), (r, s, d, None, 0, 8, 8),
                 (r, s, d, None, -1, 8, 8), (r, s, d, None, 1, 0, 8), (r, s, d, None, 1, 8, -2)):
        assert L.pp_draw_humans_u8(*args, None) == -2          # PP_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == SENTINEL).all()
    assert L.pp_draw_humans_u8(r, s, d, None, 1, 8, 8, None) == 0
    assert tuple(dst.cpu().numpy()[0, 4, 4]) == (255, 0, 0)    # CocoColors[0]
