"""CPU: the host half of the test-time rotation search (posepaf.rotation) and the conventions of the NumPy restatement of
cv2.warpAffine the GPU tests hold the kernels to (tests/rotation_reference.py)."""
import math

import numpy as np
import pytest

from rotation_reference import warp_affine


def test_rotation_matrix_closed_form():
    from posepaf.rotation import rotation_matrix
    for (cx, cy), ang in [((256.0, 256.0), 15.0), ((224.0, 320.0), -30.0), ((32.5, 7.0), 90.0), ((100.0, 60.0), 0.0)]:
        a = math.radians(ang)
        al, be = math.cos(ang * (math.pi / 180)), math.sin(ang * (math.pi / 180))
        want = np.array([[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]])
        m = rotation_matrix((cx, cy), ang)
        assert m.dtype == np.float64 and m.shape == (2, 3)
        assert np.array_equal(m, want)
        assert abs(m[0, 0] - math.cos(a)) < 1e-15 and abs(m[0, 1] - math.sin(a)) < 1e-15


def test_center_is_swapped_and_float32():
    from posepaf.rotation import reference_center
    assert reference_center(256, 448) == (128.0, 224.0)      # (x, y) = (H / 2, W / 2)
    assert reference_center(65, 3) == (32.5, 1.5)


def test_inverse_of_inverse_gives_the_matrix_back():
    from posepaf.rotation import invert_affine, rotation_matrix
    for ang in (7.5, -30.0, 90.0, 180.0, 15.0):
        m = rotation_matrix((224.0, 320.0), ang)
        mi = invert_affine(m)
        back = invert_affine(mi)
        assert np.allclose(back, m, rtol=1e-12, atol=1e-12 * np.abs(m).max())
        # and M_inv really inverts: M(M_inv(p)) = p
        from posepaf.rotation import apply_affine
        p = np.array([[3.0, 4.0], [400.0, 12.0], [-5.0, 600.0]])
        assert np.allclose(apply_affine(m, apply_affine(mi, p)), p, rtol=0, atol=1e-9)


def test_angle_zero_is_an_exact_copy():
    from posepaf.rotation import invert_affine, reference_center, rotation_matrix
    src = np.random.default_rng(0).standard_normal((13, 21, 3)).astype(np.float32)
    out = warp_affine(src, invert_affine(rotation_matrix(reference_center(13, 21), 0.0)))
    assert np.array_equal(out, src)


def _rot(n_h, n_w, ang):
    from posepaf.rotation import invert_affine, reference_center, rotation_matrix
    return invert_affine(rotation_matrix(reference_center(n_h, n_w), ang))


def test_90_degrees_on_an_even_square_is_a_ccw_permutation():
    src = (np.arange(64, dtype=np.float32) + 1).reshape(8, 8)
    out = warp_affine(src, _rot(8, 8, 90.0))
    # dst (x, y) = src (8 - y, x): row 0 reads column 8 (outside) and is zero; input (0, 0) is lost
    assert np.array_equal(out[0], np.zeros(8, np.float32))
    want = np.zeros((8, 8), np.float32)
    for y in range(1, 8):
        for x in range(8):
            want[y, x] = src[x, 8 - y]
    assert np.array_equal(out, want)
    assert src[0, 0] not in out
    # counter-clockwise as displayed: the top-middle pixel lands at the left-middle
    assert out[4, 0] == src[0, 4]


def test_180_degrees_on_an_even_square():
    src = (np.arange(64, dtype=np.float32) + 1).reshape(8, 8)
    out = warp_affine(src, _rot(8, 8, 180.0))
    want = np.zeros((8, 8), np.float32)
    want[1:, 1:] = src[::-1, ::-1][:-1, :-1]          # dst (x, y) = src (8 - x, 8 - y)
    assert np.array_equal(out, want)


def test_non_square_inputs_use_the_swapped_center():
    from posepaf.rotation import invert_affine, rotation_matrix
    H, W = 8, 16
    src = np.random.default_rng(1).random((H, W)).astype(np.float32)
    swapped = warp_affine(src, _rot(H, W, 90.0))
    assert np.array_equal(swapped, warp_affine(src, invert_affine(rotation_matrix((4.0, 8.0), 90.0))))
    assert not np.array_equal(swapped, warp_affine(src, invert_affine(rotation_matrix((8.0, 4.0), 90.0))))
    # 90 deg about (x, y) = (4, 8): M = [[0, 1, -4], [-1, 0, 12]], so dst (x, y) = src (12 - y, x + 4)
    for y in range(H):
        for x in range(W):
            sx, sy = 12 - y, x + 4
            want = src[sy, sx] if (0 <= sx < W and 0 <= sy < H) else 0.0
            assert swapped[y, x] == np.float32(want), (y, x)


def test_subpixel_translation_pins_the_fixed_point_rounding():
    from posepaf.rotation import invert_affine
    v = np.random.default_rng(2).random((3, 10)).astype(np.float32)
    out = warp_affine(v, invert_affine(np.array([[1.0, 0.0, 0.3], [0.0, 1.0, 0.0]])))
    left = np.concatenate([np.zeros((3, 1), np.float32), v[:, :-1]], axis=1)
    want = (np.float32(10 / 32) * left + np.float32(22 / 32) * v).astype(np.float32)
    assert np.array_equal(out, want)


def test_rotated_scene_joints_come_back_under_the_inverse():
    from posepaf import synth
    from posepaf.rotation import apply_affine, invert_affine, reference_center, rotation_matrix
    hp = wp = 512
    (outs, joints) = synth.make_scene_at_scales(3, 5, [(hp // 4, wp // 4, 1.0, 15.0)], img=512, noise=0.0)
    m = rotation_matrix(reference_center(hp, wp), 15.0)
    rot = synth.rotate_joints(joints, m)
    back = apply_affine(invert_affine(m), rot[:, :, :2])
    assert np.allclose(back, joints[:, :, :2], rtol=0, atol=1e-9)
    # the scene was rendered at the rotated positions: its maps differ from the unrotated rendering
    plain = synth.make_scene_at_scales(3, 5, [(hp // 4, wp // 4, 1.0)], img=512, noise=0.0)[0][0]
    assert outs[0].shape == plain.shape and not np.array_equal(outs[0], plain)


def test_preprocess_batch_host_refuses_a_matrix():
    import torch
    from posepaf.pipeline import preprocess_batch
    img = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        preprocess_batch(img, True, torch.float32, m_inv=np.eye(2, 3))


def test_evaluate_refuses_rotation_on_the_refactored_path():
    import evaluate
    a = evaluate.parse(["--synthetic", "4", "--rotation_search", "0", "15"])
    assert a.rotation_search == [0.0, 15.0]
    assert evaluate.parse(["--synthetic", "4"]).rotation_search is None
    with pytest.raises(SystemExit, match="original path only"):
        evaluate.main(["--run_refactor", "--synthetic", "4", "--rotation_search", "0", "15"])
