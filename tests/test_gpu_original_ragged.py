"""GPU: the ragged form of the original path.  Images of different sizes that share bucket_key run in one batch and every
one of them comes out BIT FOR BIT as it does alone through the equal-size entries: every comparison here is for equality.
The bucket is tests/ragged_cases.py; test_original_ragged_cpu.py shows that its scenes are not vacuous."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ragged_cases as rc
from conftest import PKG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture()
def post(torch_cuda):
    from posepaf.api import PosePostProcessor
    p = PosePostProcessor(max_batch=4, max_h=48, max_w=48, max_peaks_per_part=64)
    yield p
    p.close()


def _record_bytes(rec):
    """everything a record defines (slots beyond n_humans are never written)"""
    n = int(rec["n_humans"])
    return (n, int(rec["n_peaks"]), int(rec["n_connections"]), int(rec["status"]), rec["humans"][:n].tobytes())


def _bucket_maps(torch, sizes, scenes, dtype, flip):
    """per scale the (B, 2|1, 50, h, w) maps of the bucket, image b showing its own scene"""
    per_image = [rc.scene_maps(size, people, seed, dtype) for size, (people, seed) in zip(sizes, scenes)]
    ns = 2 if flip else 1
    return [torch.from_numpy(np.stack([m[i][:ns] for m in per_image])).cuda() for i in range(len(rc.SCALES))]


def _accumulate_ragged(torch, post, sizes, maps, flip, fill):
    """the bucket through the ragged launch, the accumulators pre-filled with `fill`"""
    from posepaf.original_path import OriginalPathProcessor, RaggedBucket
    rg = RaggedBucket(sizes, rc.SCALES, torch.device("cuda", post.device))
    proc = OriginalPathProcessor(post, None, None, len(sizes), slot_area=rg.slot_area)
    proc.reset(rg)
    proc._heat.fill_(fill)      # the buffers themselves: reading .heat_acc would run the launch
    proc._paf.fill_(fill)
    for i, m in enumerate(maps):
        proc.accumulate(m, *rg.pads(i), len(maps), flip=flip)
    for i in range(len(maps)):
        assert rg.pads(i) == ([rc.pads(s)[i][0] for s in sizes], [rc.pads(s)[i][1] for s in sizes])
    return proc, rg


def _accumulate_alone(post, size, maps, b, flip):
    """image b alone through the equal-size entries"""
    from posepaf.original_path import OriginalPathProcessor
    proc = OriginalPathProcessor(post, size[0], size[1], 1)
    proc.reset()
    for m, (pd, pr) in zip(maps, rc.pads(size)):
        proc.accumulate(m[b:b + 1].contiguous(), pd, pr, len(maps), flip=flip)
    return proc


def test_ragged_resize_equals_the_resize_of_each_image_alone(torch_cuda):
    from posepaf.original_path import RaggedBucket, resize_images_u8
    torch = torch_cuda
    rng = np.random.default_rng(41)
    scales = [0.5, 1.5]
    slots = np.full((4,) + rc.SLOT + (3,), 0xA5, np.uint8)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in rc.SIZES]
    for b, im in enumerate(images):
        slots[b, :im.shape[0], :im.shape[1]] = im
    dev = torch.from_numpy(slots).cuda()
    rg = RaggedBucket(rc.SIZES, scales, dev.device)
    for i, scale in enumerate(scales):
        ph, pw = rg.key[i]
        out = torch.full((4, ph, pw, 3), 0x3C, dtype=torch.uint8, device=dev.device)
        got = resize_images_u8(dev, scale, ragged=rg, out=out).cpu().numpy()
        outside = np.ones(got.shape[:3], bool)
        for b, im in enumerate(images):
            want = resize_images_u8(torch.from_numpy(im[None]).cuda(), scale).cpu().numpy()[0]
            dh, dw = want.shape[:2]
            assert (dh, dw) == (int(round(im.shape[0] * scale)), int(round(im.shape[1] * scale)))
            assert np.array_equal(got[b, :dh, :dw], want), (scale, b)
            outside[b, :dh, :dw] = False
        assert outside.any() and (got[outside] == 0x3C).all(), scale


@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("flip", [True, False], ids=["flip", "noflip"])
def test_ragged_accumulation_equals_the_per_image_run(torch_cuda, post, dtype, flip):
    torch = torch_cuda
    maps = _bucket_maps(torch, rc.SIZES, rc.SCENES, dtype, flip)
    proc, rg = _accumulate_ragged(torch, post, rc.SIZES, maps, flip, float("nan"))
    heat, paf = proc.heat_acc.cpu().numpy(), proc.paf_acc.cpu().numpy()
    assert heat.shape == (4, 20, rg.slot_area) and paf.shape == (4, 30, rg.slot_area) and rg.slot_area == 128 * 128
    for b, (h, w) in enumerate(rc.SIZES):
        alone = _accumulate_alone(post, (h, w), maps, b, flip)
        assert np.array_equal(proc.heat_view(b).cpu().numpy(), alone.heat_acc.cpu().numpy()[0]), b
        assert np.array_equal(proc.paf_view(b).cpu().numpy(), alone.paf_acc.cpu().numpy()[0]), b
        assert not np.isnan(heat[b, :, :h * w]).any() and not np.isnan(paf[b, :, :h * w]).any()
        assert np.isnan(heat[b, :, h * w:]).all() and np.isnan(paf[b, :, h * w:]).all(), b   # the slot tails are untouched


@pytest.mark.parametrize("cfg", [None, rc.CFG], ids=["default", "cfg"])
def test_ragged_finish_equals_the_per_image_finish(torch_cuda, post, cfg):
    """Slot tails poisoned with 1e9: a read past an image's own extent would change the NMS, the centroid or a limb sample."""
    from posepaf.api import records_to_numpy
    torch = torch_cuda
    if cfg is not None:
        post.set_test_cfg(cfg)
    maps = _bucket_maps(torch, rc.SIZES, rc.SCENES, np.float16, True)
    proc, rg = _accumulate_ragged(torch, post, rc.SIZES, maps, True, 1e9)
    rc.add_corner_peak(proc.heat_view(rc.CORNER_IMAGE), rc.SIZES[rc.CORNER_IMAGE])
    for b, (h, w) in enumerate(rc.SIZES):
        assert bool((proc.heat_acc[b, :, h * w:] == 1e9).all()) and bool((proc.paf_acc[b, :, h * w:] == 1e9).all())
    got = records_to_numpy(proc.finish(4)).copy()
    for b, size in enumerate(rc.SIZES):
        alone = _accumulate_alone(post, size, maps, b, True)
        if b == rc.CORNER_IMAGE:
            rc.add_corner_peak(alone.heat_acc[0], size)
        want = records_to_numpy(alone.finish(1))[0]
        assert _record_bytes(got[b]) == _record_bytes(want), b
        assert int(got[b]["status"]) == 32 and int(got[b]["n_humans"]) > 0, b
    assert int(got["n_humans"].sum()) > 0


def test_an_all_equal_bucket_through_the_ragged_entries(torch_cuda, post):
    from posepaf.api import records_to_numpy
    from posepaf.original_path import OriginalPathProcessor
    torch = torch_cuda
    sizes = [rc.SLOT] * 4
    maps = _bucket_maps(torch, sizes, rc.EQUAL_SCENES, np.float16, True)
    proc, rg = _accumulate_ragged(torch, post, sizes, maps, True, float("nan"))
    scalar = OriginalPathProcessor(post, rc.SLOT[0], rc.SLOT[1], 4)
    scalar.reset()
    for m, (pd, pr) in zip(maps, rc.pads(rc.SLOT)):
        scalar.accumulate(m, pd, pr, len(maps))
    assert np.array_equal(proc.heat_acc.cpu().numpy().reshape(4, 20, 128, 128), scalar.heat_acc.cpu().numpy())
    assert np.array_equal(proc.paf_acc.cpu().numpy().reshape(4, 30, 128, 128), scalar.paf_acc.cpu().numpy())
    got = records_to_numpy(proc.finish(4)).copy()
    want = records_to_numpy(scalar.finish(4))
    assert [_record_bytes(r) for r in got] == [_record_bytes(r) for r in want]
    assert int(got["n_humans"].sum()) > 0


def test_a_ragged_run_refuses_a_rotation_search(torch_cuda, post):
    from posepaf._lib import PosePafError
    from posepaf.original_path import OriginalPathProcessor
    torch = torch_cuda

    def model(x):
        raise AssertionError("the refusal comes before any launch")

    proc = OriginalPathProcessor(post, None, None, 4, slot_area=128 * 128)
    proc._heat.fill_(7.0)
    images = torch.zeros((4,) + rc.SLOT + (3,), dtype=torch.uint8, device="cuda")
    with pytest.raises(PosePafError):
        proc.run(model, images, rc.SCALES, angles=(0.0, 15.0), sizes=rc.SIZES)
    assert bool((proc._heat == 7.0).all())
    with pytest.raises(PosePafError):      # and a rotated entry handed to accumulate() directly
        from posepaf.original_path import RaggedBucket
        proc.reset(RaggedBucket(rc.SIZES, rc.SCALES, images.device))
        proc.accumulate(torch.zeros((4, 2, 50, 16, 16), dtype=torch.float16, device="cuda"), [0] * 4, [0] * 4, 3,
                        m_inv=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0])


@pytest.mark.parametrize("buckets,groups,ragged", [("", 1, 1), ("exact", 4, 0)], ids=["bucket_key", "exact"])
def test_evaluate_runs_mixed_sizes_in_one_ragged_bucket(tmp_path, buckets, groups, ragged):
    """evaluate.py on the original path with four sizes of one key: one ragged bucket; POSEPAF_ORIGINAL_BUCKETS=exact forms
    the four exact-size groups instead.  (The dumps are not compared: the forward's kernel choice depends on the batch.)"""
    dump = tmp_path / "res.json"
    env = dict(os.environ)
    env.pop("POSEPAF_ORIGINAL_BUCKETS", None)
    if buckets:
        env["POSEPAF_ORIGINAL_BUCKETS"] = buckets
    r = subprocess.run([sys.executable, os.path.join(PKG, "evaluate.py"), "--synthetic", "8", "--sizes",
                        "120x100,128x128,97x115,86x127", "--batch", "4", "--scales", "0.5", "1.0", "1.5", "--people", "2", "3",
                        "--dump_name", str(dump)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    summary = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps(summary))
    assert summary["images"] == 8 and summary["status_or"] == 32
    assert summary["original_buckets"] == {"groups": groups, "ragged": ragged}
    if not buckets:
        assert summary["synthetic_oks"]["AP"] > 0.5, summary
