"""CPU: the NumPy restatement of the data transformer's contract (tests/augment_reference.py) pinned to cases
with known answers, and the host half (posepaf/augment.py: the draws, the matrix, the refusals) against what the reference's own
AugmentSelection / Transformer gave (tests/golden/augment_reference.npz, made by tests/golden/make_golden_augment.py).

Bounds: draws equal; M within 1e-12 relative, element by element (the same float64 products in the same order: the measured
difference is 0); joints against the reference's np.matmul within 1 float32 ulp (BLAS may order or fuse the two products
differently; both sides are rounded from float64, whose error is far below half a float32 ulp, so only the last rounding can differ)
and bit-equal to the restatement; the left / right exchange exact."""
import os
import random

import numpy as np
import pytest

import augment_reference as ar
from conftest import GOLDEN
from posepaf import augment, rotation
from posepaf._lib import PosePafError

IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def rand_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- the restatement
def test_identity_gives_the_source():
    src = rand_u8((12, 20, 3), 1)
    assert np.array_equal(ar.warp_u8(src, IDENTITY, 12, 20, ar.BORDER), src)
    plane = rand_u8((12, 20), 2)
    assert np.array_equal(ar.warp_u8(plane, IDENTITY, 12, 20, 255), plane)


def test_integer_translation_is_an_exact_shift_with_border_elsewhere():
    src = rand_u8((12, 20, 3), 3)
    m = np.array([[1.0, 0.0, 3.0], [0.0, 1.0, -2.0]])           # forward: x + 3, y - 2
    out = ar.warp_u8(src, rotation.invert_affine(m), 16, 24, ar.BORDER)
    want = np.empty((16, 24, 3), np.uint8)
    want[:] = np.array(ar.BORDER, np.uint8)
    want[0:10, 3:23] = src[2:12, 0:20]
    assert np.array_equal(out, want)


def test_half_pixel_translation_averages_with_the_half_rounded_up():
    row = np.array([[10, 13, 13, 200, 0, 255, 254, 1]], np.uint8)
    m_inv = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.0]])        # destination x reads source x + 0.5
    out = ar.warp_u8(row, m_inv, 1, 8, 77)
    a, b = row[0].astype(int), np.append(row[0, 1:], 77).astype(int)   # the last tap pair reaches the border value
    assert np.array_equal(out[0], (a + b + 1) >> 1)


def test_source_wholly_outside_gives_the_border():
    src = rand_u8((9, 9, 3), 4)
    m_inv = np.array([[1.0, 0.0, 1000.0], [0.0, 1.0, -500.0]])
    out = ar.warp_u8(src, m_inv, 8, 12, ar.BORDER)
    assert (out == np.array(ar.BORDER, np.uint8)).all()
    img, miss, fg, _ = ar.transform(src, rand_u8((9, 9), 5), rand_u8((9, 9), 6), m_inv, IDENTITY, False, np.zeros((1, 18, 3)), 0, 8, 12)
    assert np.array_equal(img, np.broadcast_to(np.array(ar.BORDER, np.float32) / np.float32(255), (8, 12, 3)))
    assert (miss == 1.0).all() and (fg == 0.0).all()


def test_area_rounding_goes_to_even():
    plane = np.zeros((4, 12), np.uint8)
    plane[0, 0] = 8                      # sum 8: 0.5 -> 0
    plane[0, 4:7] = 8                    # sum 24: 1.5 -> 2
    plane[0, 8:12] = 10                  # sum 40: 2.5 -> 2
    assert ar.area4(plane).tolist() == [[0, 2, 2]]
    plane[:] = 255
    assert ar.area4(plane).tolist() == [[255, 255, 255]]
    assert ar.unit(np.uint8(255)) == np.float32(1.0)


def test_erode_ignores_what_lies_outside_the_frame():
    plane = np.ones((4, 5), np.float32)
    assert np.array_equal(ar.erode3(plane), plane)              # a frame corner keeps its value: no zero padding
    plane[1, 1] = 0.25
    out = ar.erode3(plane)
    want = np.ones((4, 5), np.float32)
    want[0:3, 0:3] = 0.25
    assert np.array_equal(out, want)
    corner = np.ones((3, 3), np.float32)
    corner[2, 2] = 0.5
    assert ar.erode3(corner).tolist() == [[1, 1, 1], [1, 0.5, 0.5], [1, 0.5, 0.5]]


def test_partially_outside_block_reads_the_border_for_the_outside_taps_only():
    src = np.full((2, 2), 100, np.uint8)
    m_inv = np.array([[1.0, 0.0, 1.5], [0.0, 1.0, 0.0]])        # x = 0 reads columns 1 and 2 (outside) at a = 16
    out = ar.warp_u8(src, m_inv, 1, 1, 0)
    assert out[0, 0] == (100 * 16 * 32 + 0 + 512) >> 10


# ---------------------------------------------------------------------------------------------- the host half against the reference
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "augment_reference.npz"))


def test_random_draws_are_the_references(golden):
    assert golden["draws"][:, 1].any() and (golden["draws"][:, 5] == 1.0).any()     # a tint draw and an unscaled draw are among them
    for seed, want in zip(golden["seeds"], golden["draws"]):
        a = augment.AugmentSelection.random(augment.TransformParams(), random.Random(int(seed)))
        got = [float(a.flip), float(a.tint), a.degree, a.crop[0], a.crop[1], a.scale]
        assert isinstance(a.crop[0], int) and isinstance(a.crop[1], int)
        assert got == want.tolist(), (seed, got, want)
    u = augment.AugmentSelection.unrandom()
    assert (u.flip, u.tint, u.degree, u.crop, u.scale) == (False, False, 0.0, (0, 0), 1.0)


def cases(golden):
    for c in range(int(golden["n_cases"])):
        g = {k: golden[f"c{c}_{k}"] for k in ("aug", "objpos", "scale_provided", "hw", "M", "scale_size", "joints_in", "joints_out")}
        a = g["aug"]
        g["sel"] = augment.AugmentSelection(bool(a[0]), bool(a[1]), float(a[2]), (int(a[3]), int(a[4])), float(a[5]))
        yield c, g


def test_affine_matrix_is_the_references(golden):
    worst = 0.0
    for c, g in cases(golden):
        M, scale_size = augment.affine_matrix(g["sel"], tuple(g["objpos"]), float(g["scale_provided"]), int(g["hw"][0]), int(g["hw"][1]))
        assert M.shape == (2, 3) and M.dtype == np.float64
        assert (g["M"] != 0).all()
        rel = np.abs(M - g["M"]) / np.abs(g["M"])
        worst = max(worst, float(rel.max()))
        assert (rel <= 1e-12).all(), (c, M, g["M"])
        assert abs(scale_size - float(g["scale_size"])) <= 1e-12 * float(g["scale_size"])
    print(f"affine_matrix against the reference: largest relative difference {worst:.3e}")


def test_joints_follow_the_reference_and_the_restatement(golden):
    worst, flips = 0, 0
    for c, g in cases(golden):
        jin, want = g["joints_in"], g["joints_out"]
        got = ar.map_joints(g["M"], jin, jin.shape[0], g["sel"].flip)
        assert got.dtype == np.float32 and got.shape == want.shape
        ref32 = want.astype(np.float32)
        # 1 float32 ulp: the neighbour of the reference's value on either side
        lo, hi = np.nextafter(ref32, np.float32(-np.inf)), np.nextafter(ref32, np.float32(np.inf))
        assert ((got >= lo) & (got <= hi)).all(), c
        worst = max(worst, int(np.abs(got.view(np.int32).astype(np.int64) - ref32.view(np.int32).astype(np.int64)).max()))
        assert np.array_equal(got[:, :, 2], ref32[:, :, 2])                  # the flags travel with their rows
        if g["sel"].flip:
            flips += 1
            plain = ar.map_joints(g["M"], jin, jin.shape[0], False)
            assert np.array_equal(got[:, ar.LEFT_PARTS], plain[:, ar.RIGHT_PARTS]) and np.array_equal(got[:, ar.RIGHT_PARTS], plain[:, ar.LEFT_PARTS])
            rest = [k for k in range(18) if k not in ar.LEFT_PARTS + ar.RIGHT_PARTS]
            assert np.array_equal(got[:, rest], plain[:, rest])
        # persons past n_people stay as they were
        part = ar.map_joints(g["M"], jin, 1, g["sel"].flip)
        assert np.array_equal(part[:1], got[:1]) and np.array_equal(part[1:], jin[1:].astype(np.float32))
    assert flips == int(golden["n_cases"]) // 2
    assert augment.LEFT_PARTS == ar.LEFT_PARTS and augment.RIGHT_PARTS == ar.RIGHT_PARTS
    print(f"joints against the reference's np.matmul: at most {worst} float32 ulp")


def test_pack_params_layout_and_inverse(golden):
    ms = [g["M"] for _, g in cases(golden)][:3]
    raw = augment.pack_params(ms, [True, False, True], 64, 64)
    assert raw.dtype == np.uint8 and raw.shape == (augment.params_bytes(3),)
    d = raw[:3 * 96].view(np.float64).reshape(2, 3, 6)
    for i, m in enumerate(ms):
        assert np.array_equal(d[0, i], rotation.invert_affine(m).reshape(6)) and np.array_equal(d[1, i], m.reshape(6))
    assert raw[3 * 96:].view(np.int32).tolist() == [1, 0, 1]


# ---------------------------------------------------------------------------------------------- refusals, before any library call
@pytest.fixture()
def no_library(monkeypatch):
    from posepaf import _lib

    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)


def host_batch(b=2, slot=(24, 32), p=2):
    import torch
    return dict(images=torch.zeros((b,) + slot + (3,), dtype=torch.uint8), mask_miss=None, mask_all=None, sizes=None,
                joints=torch.zeros((b, p, 18, 3), dtype=torch.float64), n_people=torch.zeros(b, dtype=torch.int32),
                augs=[augment.AugmentSelection.unrandom() for _ in range(b)], objpos=[(10.0, 12.0)] * b, scale_provided=[0.5] * b,
                out_hw=(16, 16))


def test_tint_is_refused_with_its_reason(no_library):
    kw = host_batch()
    kw["augs"][1] = augment.AugmentSelection(tint=True)
    with pytest.raises(PosePafError, match="colour"):
        augment.transform_batch(**kw)


def test_host_tensors_are_refused(no_library):
    with pytest.raises(PosePafError, match="no CPU path"):
        augment.transform_batch(**host_batch())
    kw = host_batch()
    kw["images"] = kw["images"].numpy()
    with pytest.raises(PosePafError, match="no CPU path"):
        augment.transform_batch(**kw)


@pytest.mark.parametrize("change, match", [
    (dict(out_hw=(18, 16)), "multiples of 4"),
    (dict(out_hw=(0, 16)), "multiples of 4"),
    (dict(augs=[augment.AugmentSelection.unrandom()]), "per image"),
    (dict(objpos=[(1.0, 2.0)]), "per image"),
    (dict(scale_provided=[0.5, 0.0]), "positive"),
    (dict(scale_provided=[0.5, 1e9]), "fixed-point range"),
    (dict(augs=["flip", "flop"]), "AugmentSelection"),
])
def test_bad_host_arguments_are_refused(no_library, change, match):
    kw = host_batch()
    kw.update(change)
    with pytest.raises(PosePafError, match=match):
        augment.transform_batch(**kw)


def test_bad_device_arguments_are_refused_by_the_shape_checks(no_library):
    """the tensor checks run before the device check, so host tensors reach them here"""
    import torch
    bad = [
        (dict(images=torch.zeros((2, 24, 32, 4), dtype=torch.uint8)), "images must be"),
        (dict(images=torch.zeros((2, 24, 32, 3), dtype=torch.float32)), "images must be"),
        (dict(mask_miss=torch.zeros((2, 24, 31), dtype=torch.uint8)), "mask_miss must be"),
        (dict(mask_all=torch.zeros((2, 24, 32), dtype=torch.float32)), "mask_all must be"),
        (dict(sizes=torch.zeros((2, 3), dtype=torch.int32)), "sizes must be"),
        (dict(joints=torch.zeros((2, 2, 18, 3), dtype=torch.float32)), "joints must be"),
        (dict(joints=torch.zeros((2, 65, 18, 3), dtype=torch.float64)), "max_people"),
        (dict(n_people=torch.zeros(2, dtype=torch.int64)), "n_people must be"),
        (dict(dtype=torch.float64), "dtype must be"),
        (dict(border=(1, 2)), "border"),
        (dict(border=(1, 2, 256)), "border"),
        (dict(target=torch.zeros((2, 1, 50, 4, 5), dtype=torch.float16)), "target must be"),
        (dict(out={"image": torch.zeros((2, 16, 16, 3), dtype=torch.float16)}), "out\\['image'\\]"),
        (dict(out={"fg": torch.zeros((2, 4, 4))}, target=torch.zeros((2, 1, 50, 4, 4), dtype=torch.float16)), "out takes"),
    ]
    for change, match in bad:
        kw = host_batch()
        kw.update(change)
        with pytest.raises(PosePafError, match=match):
            augment.transform_batch(**kw)
    with pytest.raises(PosePafError, match="fixed-point range"):
        augment.check_inverse(np.array([[3e4, 0.0, 0.0], [0.0, 1.0, 0.0]]), 64, 128)
    with pytest.raises(PosePafError, match="not finite"):
        augment.check_inverse(np.full((2, 3), np.nan), 8, 8)
