"""CPU: every bicubic step of the oracle against an independent float64 statement of the published algorithm
(tests/cubic_reference.py), and that statement against torch's float64 bicubic.

OpenCV is absent, so cv2.resize(INTER_CUBIC) itself cannot be run.  What CAN be pinned is the algorithm it documents --
Keys' kernel with a = -0.75, half-pixel centres, replicated borders, float coordinates -- and that is what the oracle and
the kernels restate.  The chain is: torch float64 bicubic == reference (1e-12) ; reference ~ oracle (float32 rounding only,
DYADIC_TOL / GENERAL_TOL) ; four plausible wrong algorithms miss those tolerances by more than 1000x.  What stays
unverifiable here is OpenCV's own last bits (its SIMD / IPP code paths)."""
import numpy as np
import pytest

import cubic_reference as cr
from conftest import load_scene, scene_keys
from test_gpu_parity import SCORE_TOL

# (source shape, fy, fx) of cv2.resize(fx=, fy=) and (source shape, destination shape) of cv2.resize(dsize=)
FACTOR_CASES = [((16, 24), 4, 4), ((5, 5), 4, 4), ((3, 2), 4, 4), ((1, 7), 4, 4), ((64, 48), 0.5, 0.5),
                ((37, 50), 1.37, 1.37), ((33, 47), 3, 2)]
SIZE_CASES = [((40, 56), (43, 59)), ((224, 224), (200, 264)), ((384, 384), (256, 256))]
DYADIC = (4, 2, 0.5)


def _oracle_resize_to(oracle, src, dh, dw):
    """cv2.resize(src, (dw, dh)): scale = 1 / (dsize / ssize) in double, as orc_predict_accumulate calls it"""
    from oracle.oracle import _fp
    sh, sw = src.shape
    dst = np.empty((dh, dw), np.float32)
    oracle.L.orc_resize_cubic(_fp(src), sh, sw, sw, 1, _fp(dst), dh, dw, dw, 1, 1.0 / (dw / sw), 1.0 / (dh / sh))
    return dst


def _cases(oracle):
    """[(name, dyadic, oracle result, kwargs -> reference result)] on inputs uniform in [-0.5, 1.5]"""
    rng = np.random.default_rng(2024)
    out = []
    for shape, fy, fx in FACTOR_CASES:
        src = rng.uniform(-0.5, 1.5, shape).astype(np.float32)
        out.append((f"{shape} x({fy},{fx})", fy in DYADIC and fx in DYADIC, oracle.resize_cubic(src, fx, fy),
                    lambda src=src, fy=fy, fx=fx, **kw: cr.resize_by_factor(src, fy, fx, coord_dtype=np.float32, **kw)))
    for shape, (dh, dw) in SIZE_CASES:
        src = rng.uniform(-0.5, 1.5, shape).astype(np.float32)
        out.append((f"{shape} -> {(dh, dw)}", False, _oracle_resize_to(oracle, src, dh, dw),
                    lambda src=src, dh=dh, dw=dw, **kw: cr.resize(src, dh, dw, 1.0 / (dh / src.shape[0]), 1.0 / (dw / src.shape[1]),
                                                                  coord_dtype=np.float32, **kw)))
    return out


@pytest.fixture(scope="module")
def cases(oracle):
    return _cases(oracle)


def test_reference_equals_torch_float64_bicubic():
    """factors torch can express exactly (size = in * factor): 4, 2, 0.5 and 3 x 2; 1 x 7, 3 x 2 and 5 x 5 clamp every tap.
    Bound 1e-12: float64, 16 terms of magnitude <= 1.5 * 1.6 (measured 5e-15)."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(1)
    worst, n = 0.0, 0
    for h, w in [(1, 7), (3, 2), (5, 5), (33, 47)]:
        src = rng.uniform(-0.5, 1.5, (h, w))
        for fy, fx in [(4, 4), (2, 2), (0.5, 0.5), (3, 2)]:
            oh, ow = int(h * fy), int(w * fx)
            if oh < 1 or ow < 1:
                continue
            want = F.interpolate(torch.from_numpy(src)[None, None], size=(oh, ow), mode="bicubic", align_corners=False)[0, 0].numpy()
            got = cr.resize(src, oh, ow, coord_dtype=np.float64)
            assert got.shape == want.shape
            worst = max(worst, float(np.abs(got - want).max()))
            n += 1
    print(f"reference vs torch float64 over {n} cases: {worst:.3g}")
    assert n == 15 and worst <= 1e-12


def test_tolerances_are_four_times_the_measurement_and_under_the_cap(cases):
    """the two constants of cubic_reference.py against what this case list measures today"""
    worst = {True: 0.0, False: 0.0}
    for name, dyadic, got, ref in cases:
        worst[dyadic] = max(worst[dyadic], float(np.abs(got - ref()).max()))
    print(f"oracle vs reference: dyadic {worst[True]:.3g}, general {worst[False]:.3g}")
    assert cr.DYADIC_TOL <= cr.TOL_CAP and cr.GENERAL_TOL <= cr.TOL_CAP
    assert worst[True] <= cr.DYADIC_TOL / 4 * 1.05 and worst[False] <= cr.GENERAL_TOL / 4 * 1.05
    assert worst[True] >= cr.DYADIC_TOL / 8 and worst[False] >= cr.GENERAL_TOL / 8     # the comment beside each is current


def test_oracle_resize_cubic(cases):
    for name, dyadic, got, ref in cases:
        want = ref()
        assert got.shape == want.shape, name
        err = float(np.abs(got - want).max())
        print(f"{name}: {err:.3g}")
        assert err <= (cr.DYADIC_TOL if dyadic else cr.GENERAL_TOL), name


CONTROLS = {"a = -0.5": dict(a=-0.5), "align_corners centres": dict(centres="align_corners"),
            "taps floor(c) .. floor(c)+3": dict(first_tap=0), "x4 phase order reversed": dict(reverse_phase=True)}


@pytest.mark.parametrize("control", sorted(CONTROLS))
def test_negative_controls_fail_by_three_orders_of_magnitude(cases, control):
    """The same reference with one thing wrong must miss the oracle by >= 1000 x the tolerance of its case: the tolerances
    cannot hide a wrong constant, centre convention, tap window or phase table.  (Reversing the phases replaces the
    fraction f by 1 - f, which is what reading the x4 coefficient table backwards does; at f = 0.5 it changes nothing, so
    the scale-0.5 case is left to the other three controls.)"""
    checked = 0
    for name, dyadic, got, ref in cases:
        if control == "align_corners centres" and min(got.shape) < 2:
            continue                                    # a one-pixel axis has no corners to align
        if control == "x4 phase order reversed" and "x(0.5,0.5)" in name:
            continue
        miss = float(np.abs(got - ref(**CONTROLS[control])).max())
        tol = cr.DYADIC_TOL if dyadic else cr.GENERAL_TOL
        print(f"{control}, {name}: off by {miss:.3g} = {miss / tol:.3g} x tolerance")
        assert miss >= 1000 * tol, (control, name)
        checked += 1
    assert checked >= 8


def _scene_checks(oracle, heat, paf, what, min_img_size=512):
    jl0, _ = oracle.heatmap_nms(heat, 4, refine=False)
    jl, _ = oracle.heatmap_nms(heat, 4, refine=True)
    cr.assert_refined_peaks(jl, jl0, heat, what)
    up = oracle.upsample4_hwc(paf)
    ref = cr.upsample4(paf).transpose(1, 2, 0)
    err = float(np.abs(up - ref).max())
    print(f"{what}: x4 limb map {err:.3g}")
    assert err <= cr.DYADIC_TOL, what
    a = oracle.process_paf(jl[None], up, min_img_size)
    b = oracle.process_paf(jl[None], np.ascontiguousarray(ref, np.float32), min_img_size)
    assert np.array_equal(a["ids"], b["ids"]), what
    if len(a["scores"]):
        print(f"{what}: person scores {float(np.abs(a['scores'] - b['scores']).max()):.3g}")
    assert np.allclose(a["scores"], b["scores"], rtol=0, atol=SCORE_TOL), what
    return jl, a


@pytest.mark.parametrize("key", scene_keys())
def test_golden_scene_refinement_and_limb_maps(oracle, key):
    net, g = load_scene(key)
    heat, paf = oracle.flip_average(net)
    jl, res = _scene_checks(oracle, heat, paf, key)
    assert np.array_equal(jl, g["joint_list"]) and len(res["ids"]) == len(g["cpp_ids"])


def test_corner_and_edge_peaks(oracle):
    """no golden scene has a peak in a corner: patches clipped to 3 x 3 and 3 x 5, replication at the patch edge"""
    net = cr.corner_edge_map()
    h, w = net.shape[-2:]
    heat, paf = oracle.flip_average(net, flip=False)
    paf = paf + np.random.default_rng(6).uniform(-0.5, 1.5, paf.shape).astype(np.float32)
    jl, _ = _scene_checks(oracle, heat, paf, "corner / edge map", 4 * h)
    jl0, _ = oracle.heatmap_nms(heat, 4, refine=False)
    got = {tuple(p) for p in cr.integer_peaks(jl0[jl0[:, 4] == 0])}
    assert {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (0, h // 2)} <= got


@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("flip", [True, False], ids=["flip", "noflip"])
def test_oracle_predict_accumulate(oracle, dtype, flip):
    for name, img, entries in cr.PREDICT_CASES:
        heat, paf = np.zeros((20,) + img), np.zeros((30,) + img)
        want_h, want_p = np.zeros((20,) + img), np.zeros((30,) + img)
        for net, (pd, pr) in cr.predict_inputs(entries, dtype, flip):
            oracle.predict_accumulate(net, pd, pr, img[0], img[1], len(entries), heat, paf, flip=flip)
            h_, p_ = cr.predict_entry(net, pd, pr, img[0], img[1], len(entries), flip)
            want_h += h_
            want_p += p_
        err = max(float(np.abs(heat - want_h).max()), float(np.abs(paf - want_p).max()))
        print(f"{name}: {err:.3g}")
        assert err <= cr.GENERAL_TOL, name
        assert float(np.abs(want_p).max()) > 0.5


@pytest.mark.parametrize("scale", cr.U8_SCALES)
def test_oracle_resize_u8(oracle, scale):
    """OpenCV's 11-bit fixed-point coefficients against real arithmetic: never more than one count, and at most 15 % of the
    pixels differ at all (measured: 8.2 % on the noise image at 1.5, none at 2.0)"""
    for name, img in cr.u8_images().items():
        cr.assert_u8_close(oracle.resize_u8(img, scale, scale), img, scale, f"{name} x{scale}")
