"""CPU: the yardstick of the scene renderers.  tests/scene_reference.py (a float64 restatement of the reference's training-target
recipe) is pinned to the reference's own Heatmapper through tests/golden/scene_*.npz, and posepaf.synth.render_maps (the host
renderer) to the restatement; plus the COCO -> 18-part mapping shared by the bank and the device path, and render_scenes'
argument checks.  The device renderer itself is compared with the same restatement in tests/test_gpu_scenes.py."""
import os

import numpy as np
import pytest

import scene_cases
import scene_reference as ref
from conftest import GOLDEN

FIXTURES = ("heatmap_test_128x128", "edge_16x24", "edge_33x47")


@pytest.fixture(scope="module")
def restated():
    """restatement of every fixture's joints, computed once"""
    out = {}
    for name in FIXTURES:
        d = np.load(os.path.join(GOLDEN, f"scene_{name}.npz"))
        maps, mask = ref.render(d["joints"], int(d["h"]), int(d["w"]))
        out[name] = (d["joints"], int(d["h"]), int(d["w"]), d["maps"], maps, mask)
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_the_reference(restated, name):
    joints, h, w, stored, maps, mask = restated[name]
    assert stored.dtype == np.float32 and stored.shape == (48, h, w) and joints.dtype == np.float32
    share = ref.masked_share(mask)
    err = ref.max_err_outside(stored, maps[:48], ref.full_mask(mask)[:48])
    print(f"{name}: reference vs restatement max {err:.3e} outside the mask, masked share {share:.2e}")
    assert share <= ref.MASK_CAP
    assert err <= ref.TOL
    assert np.count_nonzero(stored) > 1000         # not an empty agreement


@pytest.mark.parametrize("name", FIXTURES)
def test_host_renderer_matches_the_restatement(restated, name):
    from posepaf import synth
    joints, h, w, _, maps, mask = restated[name]
    got = synth.render_maps(joints, h, w)
    err = ref.max_err_outside(got, maps, ref.full_mask(mask))
    print(f"{name}: synth.render_maps vs restatement max {err:.3e}")
    assert err <= ref.TOL
    assert np.array_equal(got[48:], np.zeros_like(got[48:]))


def test_host_renderer_on_the_batch_scenes():
    """the scenes the GPU tests use (0, 1, 9 and 12 people at the two small shapes): host renderer vs restatement"""
    from posepaf import synth
    for h, w in scene_cases.SHAPES[:2]:
        for people in scene_cases.batch_people(h, w):
            maps, mask = ref.render(people, h, w)
            assert ref.masked_share(mask) <= ref.MASK_CAP
            assert ref.max_err_outside(synth.render_maps(people, h, w), maps, ref.full_mask(mask)) <= ref.TOL


def test_edge_scene_reaches_the_branches():
    """the edge scene does what its docstring says: skipped and empty windows, ties, a zero-length limb, a count-2 average"""
    h, w = 16, 24
    people = scene_cases.edge_people(h, w)
    assert people.dtype == np.float32 and people.shape == (9, 18, 3)
    assert (people[2, :, :2] < -32).all() and (people[3, :, 0] > 4 * w + 32).all()
    assert (people[4, :, :2].min(axis=0) < 0).all() and (people[5, :, 0].max() > 4 * w) and (people[5, :, 1].max() > 4 * h)
    assert np.all((people[6, :, 0] / 4) % 1 == 0.5) and np.array_equal(people[6, 0, :2], people[6, 1, :2])
    one, _ = ref.render(people[:1], h, w)
    two, _ = ref.render(people[:2], h, w)
    assert np.allclose(one, two, atol=1e-15)        # the same person twice: max and mean both leave the maps as they are
    none, _ = ref.render(people[2:4], h, w)
    assert not none.any()                            # both off-frame people draw nothing
    # the joint flag: 0, 1 and 2 all occur; 0 is drawn like 1 ("< 2 means annotated"), so a renderer that asked for == 1 differs
    assert set(np.unique(people[:, :, 2]).tolist()) == {0.0, 1.0, 2.0}
    for scene in (people, scene_cases.batch_people(h, w)[3]):
        assert (scene[:, :, 2] == 0).sum() >= 6
        as_one, only_one = scene.copy(), scene.copy()
        as_one[:, :, 2] = np.where(scene[:, :, 2] == 0, 1, scene[:, :, 2])
        only_one[:, :, 2] = np.where(scene[:, :, 2] == 0, 2, scene[:, :, 2])
        full, _ = ref.render(scene, h, w)
        assert np.array_equal(full, ref.render(as_one, h, w)[0])
        assert np.abs(full - ref.render(only_one, h, w)[0]).max() > 0.5


def test_mirror_is_the_host_mirror():
    from posepaf import synth
    maps = np.random.default_rng(0).random((50, 5, 7))
    assert np.array_equal(ref.mirror(maps), synth.mirror_sample(maps))
    assert np.array_equal(ref.mirror(ref.mirror(maps)), maps)


def test_reverse_kp_channel():
    people = scene_cases.edge_people(16, 24)
    maps, _ = ref.render(people, 16, 24, reverse_kp=True)
    assert np.array_equal(maps[49], maps[30:48].max(axis=0)) and maps[49].max() > 0.9 and not maps[48].any()


# ------------------------------------------------------------------------------------------------ coco_to_joints
def _inline_bank_people(gts):
    """the code CocoSource.bank_for_bucket held inline before posepaf.synth_device.coco_to_joints"""
    from posepaf import skeleton as sk
    people = []
    for g in gts:
        kp = np.asarray(g["keypoints"], np.float64).reshape(17, 3)
        j = np.zeros((sk.NUM_PART, 3))
        j[:, 2] = 2
        for coco_i, cmu_i in enumerate(sk.ORDER_COCO):
            if kp[coco_i, 2] > 0:
                j[cmu_i] = (kp[coco_i, 0], kp[coco_i, 1], 1)
        if kp[5, 2] > 0 and kp[6, 2] > 0:
            j[1] = ((kp[5, 0] + kp[6, 0]) / 2, (kp[5, 1] + kp[6, 1]) / 2, 1)
        if (j[:, 2] < 2).any():
            people.append(j)
    return np.stack(people) if people else np.zeros((0, sk.NUM_PART, 3))


def test_coco_to_joints_is_the_inline_mapping():
    from posepaf import synth_device
    from posepaf._lib import PosePafError
    rng = np.random.default_rng(3)
    gts = []
    for k in range(6):
        kp = np.zeros((17, 3))
        kp[:, :2] = rng.uniform(0, 300, (17, 2))
        kp[:, 2] = rng.integers(0, 3, 17)
        if k == 2:
            kp[:, 2] = 0                      # nothing labelled: dropped
        if k == 3:
            kp[5, 2] = 0                      # one shoulder missing: no neck
        gts.append({"keypoints": kp.reshape(-1).tolist(), "area": 1.0})
    want = _inline_bank_people(gts)
    got = synth_device.coco_to_joints(gts)
    assert got.dtype == np.float64 and np.array_equal(got, want) and got.shape[0] == 5
    assert synth_device.coco_to_joints([]).shape == (0, 18, 3)
    assert np.array_equal(synth_device.coco_to_joints(gts, max_people=5), want)
    with pytest.raises(PosePafError):
        synth_device.coco_to_joints(gts, max_people=4)       # refused, never truncated
    joints, n = synth_device.pack_joints([want, want[:0]], 8)
    assert joints.dtype == np.float32 and joints.shape == (2, 8, 18, 3) and n.tolist() == [5, 0]
    assert np.array_equal(joints[0, :5], want.astype(np.float32)) and (joints[0, 5:, :, 2] == 2).all() and (joints[1, :, :, 2] == 2).all()
    with pytest.raises(PosePafError):
        synth_device.pack_joints([want], 4)


# ------------------------------------------------------------------------------------------------ argument checks
def test_render_scenes_refuses_bad_arguments_and_has_no_cpu_path():
    import torch

    from posepaf import synth_device
    from posepaf._lib import PosePafError
    j = torch.zeros((2, 4, 18, 3), dtype=torch.float32)
    n = torch.zeros(2, dtype=torch.int32)
    # every case names the check that must refuse it: the tensors are host tensors, so without `match` the last check of all
    # ("must live on the HIP device") would hide a missing one
    bad = [(dict(joints=j.double()), "joints must be float32"), (dict(joints=j[:, :, :17]), "joints must be float32"),
           (dict(joints=torch.zeros((0, 4, 18, 3))), "at least one image"), (dict(joints=torch.zeros((2, 0, 18, 3))), "at least one image"),
           (dict(n_people=n.long()), "n_people must be int32"), (dict(n_people=n[:1]), "n_people must be int32"),
           (dict(h=0), "h and w must be positive"), (dict(w=-3), "h and w must be positive"),
           (dict(dtype=torch.bfloat16), "dtype must be torch.float16 or torch.float32"),
           (dict(noise=-1.0), "noise must be >= 0"), (dict(noise=float("nan")), "noise must be >= 0"),
           (dict(scene_ids=torch.zeros(2, dtype=torch.int32)), "scene_ids must be an int64"),
           (dict(scene_ids=torch.zeros(3, dtype=torch.int64)), "scene_ids must be an int64"),
           (dict(joints=torch.zeros((2, 65, 18, 3))), "beyond the 64 the kernel stages"), (dict(joints=j.numpy()), "takes device tensors"),
           (dict(out=torch.zeros((2, 2, 50, 8, 9))), "out must be a contiguous"),
           (dict(out=torch.zeros((2, 2, 50, 8, 8), dtype=torch.float32)), "out must be a contiguous"),
           (dict(out=torch.zeros((2, 2, 50, 8, 16), dtype=torch.float16)[..., ::2]), "out must be a contiguous"),
           (dict(flip=False, out=torch.zeros((2, 2, 50, 8, 8), dtype=torch.float16)), "out must be a contiguous")]
    for kw, message in bad:
        args = dict(joints=j, n_people=n, h=8, w=8, dtype=torch.float16)
        args.update(kw)
        with pytest.raises(PosePafError, match=message):
            synth_device.render_scenes(**args)
    if not torch.cuda.is_available():
        with pytest.raises(PosePafError, match="no CPU path"):      # host tensors, valid otherwise: loud, not computed
            synth_device.render_scenes(j, n, 8, 8)


def test_c_entry_refuses_before_touching_memory():
    """pp_render_scenes' own checks, with pointers it must never follow (no launch happens on a bad argument or without a device)"""
    import ctypes as C

    import torch

    from posepaf import _lib
    L = _lib.load()
    p = C.c_void_p(4096)

    def call(joints=p, n=p, ids=None, batch=2, people=4, h=8, w=8, ns=2, dtype=_lib.PP_F16, flags=0, sigma=0.0, out=p):
        return L.pp_render_scenes(joints, n, ids, batch, people, h, w, ns, dtype, flags, sigma, 7, out, None)
    BAD_ARG, UNSUPPORTED, NO_DEVICE = -2, -6, -1
    for kw in (dict(joints=None), dict(n=None), dict(out=None), dict(ns=0), dict(ns=3), dict(dtype=2), dict(batch=0), dict(people=0),
               dict(h=0), dict(w=-1), dict(sigma=-0.5)):
        assert call(**kw) == BAD_ARG, kw
    assert call(people=_lib.SCENE_MAX_PEOPLE + 1) == UNSUPPORTED
    if not torch.cuda.is_available():
        assert call() == NO_DEVICE
        assert call(people=_lib.SCENE_MAX_PEOPLE) == NO_DEVICE     # 64 people pass the capacity check


# ------------------------------------------------------------------------------------------------ evaluate.py --scenes
def _evaluate_module():
    import importlib.util

    from conftest import PKG
    spec = importlib.util.spec_from_file_location("pp_evaluate_scenes", os.path.join(PKG, "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    return ev


def test_scenes_device_is_refused_on_the_original_path_before_the_gpu():
    import torch
    ev = _evaluate_module()
    was_initialised = torch.cuda.is_initialized()
    with pytest.raises(SystemExit, match="refactored path only"):
        ev.main(["--synthetic", "4", "--scenes", "device"])
    with pytest.raises(SystemExit, match="needs scenes to render"):
        ev.main(["--run_refactor", "--run_cpp", "--images", "somewhere", "--scenes", "device"])
    assert torch.cuda.is_initialized() == was_initialised
    a = ev.parse(["--synthetic", "4"])
    assert a.scenes == "bank" and a.scene_noise == 0.02          # the defaults are today's behaviour


def test_synthetic_source_gives_every_image_its_own_scene():
    """per_image (--scenes device): scene i, seed 20_000 + i, people[i mod len]; below 64 these are the bank's people, and the
    ground-truth joints are the ones make_scene renders -- without rendering them"""
    from posepaf import synth
    ev = _evaluate_module()
    people = [1, 2, 3, 4, 6, 8, 10, 5]
    bank = ev.SyntheticSource(200, [(512, 512)], people)
    dev = ev.SyntheticSource(200, [(512, 512)], people, noise=0.0, per_image=True)
    assert [bank.scene_slot(i) for i in (0, 63, 64, 150)] == [0, 63, 0, 22] and [dev.scene_slot(i) for i in (0, 63, 64, 150)] == [0, 63, 64, 150]
    assert bank.distinct_scenes(False) == 64 and dev.distinct_scenes(True) == 200 and bank.scene_noise == 0.02
    assert ev.SyntheticSource(40, [(512, 512), (256, 512)], people).distinct_scenes(False) == 40
    for i in (0, 5, 63):
        assert np.array_equal(dev.scene_joints(i, 512, 512), bank.scene_joints(i, 512, 512))
    for i in (5, 70):
        want = synth.make_scene(people[i % 8], 20_000 + i, h=16, w=24, noise=0.0)[1]
        got = dev.scene_joints(i, 64, 96)
        assert got.shape == (people[i % 8], 18, 3) and np.array_equal(got, want)
    assert not np.array_equal(dev.scene_joints(6, 512, 512), dev.scene_joints(70, 512, 512))    # the bank would repeat here
    assert np.array_equal(bank.scene(3, 64, 96)[1], bank.joints(3, 64, 96))
    assert dev.max_people(range(200)) == 10


def test_slot_layout_of_device_scenes():
    from posepaf.engine import header_bytes, scene_bytes
    assert scene_bytes(4, 12) == 4 * 4 + 4 * 12 * 18 * 3 * 4 and scene_bytes(4, 12) % 4 == 0
    assert (header_bytes(4) + 4 * 64 * 64 * 3) % 4 == 0          # the joints behind the images stay float32-aligned
