"""Bicubic resampling written from its published definition, in float64 NumPy -- TEST DATA ONLY.

Keys' cubic convolution (R. Keys, "Cubic convolution interpolation for digital image processing", IEEE TASSP 29(6), 1981)
with a = -0.75, pixel centres at the half-integers and replicated borders: what cv2.resize(INTER_CUBIC) and
torch.nn.functional.interpolate(mode="bicubic", align_corners=False) both document.  Nothing here is taken from
oracle/posepaf_oracle.c or from the kernels: the weight is the two-branch polynomial evaluated at each tap's distance (no
weight is "one minus the others"), and a destination pixel is ONE sum over its 4 x 4 taps (no horizontal pass, no
intermediate rounding).  test_cubic_reference_cpu.py pins it to torch's float64 bicubic to 1e-12.

`coord_dtype`: OpenCV holds the source coordinate and its fractional part in `float`, and that rounding is part of the
operation (at x ~ 200 and a non-dyadic scale it moves a weight by ~1e-5).  np.float32 reproduces that; everything after
the coordinate is float64 either way.  For dyadic scales both give the same coordinates.

The remaining keyword arguments exist for the negative controls only: each one turns the definition into a plausible wrong
one (see test_negative_controls_fail_by_three_orders_of_magnitude)."""
import numpy as np

A_CUBIC = -0.75

# Tolerances of a float32 separable implementation (the oracle, the kernels) against this reference, for |src| <= 1.5:
# the largest difference over the case list of test_cubic_reference_cpu.py::test_oracle_resize_cubic (inputs uniform in
# [-0.5, 1.5], seed 2024), times 4 -- another seed moves the maximum by about 2x.  Cap for both: 1e-5 * max|src| = 1.5e-5.
DYADIC_TOL = 4 * 2.9e-7      # measured 2.87e-07: scales 4, 2, 0.5 -- the coefficients are exact in float32
GENERAL_TOL = 4 * 1.8e-6     # measured 1.77e-06: every other scale -- float32 coordinate -> float32 coefficients
TOL_CAP = 1e-5 * 1.5


def keys_weight(t, a=A_CUBIC):
    """W(t): (a+2)|t|^3 - (a+3)|t|^2 + 1 on |t| <= 1, a|t|^3 - 5a|t|^2 + 8a|t| - 4a on 1 < |t| < 2, else 0"""
    t = np.abs(np.asarray(t, np.float64))
    near = (a + 2.0) * t ** 3 - (a + 3.0) * t ** 2 + 1.0
    far = a * t ** 3 - 5.0 * a * t ** 2 + 8.0 * a * t - 4.0 * a
    return np.where(t <= 1.0, near, np.where(t < 2.0, far, 0.0))


def _taps(n_dst, n_src, scale, a, coord_dtype, centres, first_tap, reverse_phase):
    """source indices (n_dst, 4), clamped to the source, and their weights (n_dst, 4) float64"""
    d = np.arange(n_dst, dtype=np.float64)
    if centres == "half_pixel":
        c = (d + 0.5) * np.float64(scale) - 0.5
    elif centres == "align_corners":
        c = d * ((n_src - 1) / (n_dst - 1) if n_dst > 1 else 0.0)
    else:
        raise ValueError(centres)
    c = c.astype(coord_dtype)
    base = np.floor(c)
    frac = (c - base).astype(np.float64)          # the subtraction is exact in either type
    if reverse_phase:
        frac = 1.0 - frac
    offs = np.arange(first_tap, first_tap + 4)
    idx = np.clip(base.astype(np.int64)[:, None] + offs[None, :], 0, n_src - 1)
    wgt = keys_weight(frac[:, None] - offs[None, :].astype(np.float64), a)
    return idx, wgt


def resize(src, out_h, out_w, scale_y=None, scale_x=None, a=A_CUBIC, coord_dtype=np.float64, centres="half_pixel",
           first_tap=-1, reverse_phase=False):
    """src (..., H, W) -> (..., out_h, out_w) float64.  scale_*: source step per destination pixel (cv2: 1 / fx, or
    1 / (dsize / ssize) when the size is given); default in / out."""
    src = np.asarray(src, np.float64)
    sh, sw = src.shape[-2:]
    scale_y = sh / out_h if scale_y is None else scale_y
    scale_x = sw / out_w if scale_x is None else scale_x
    iy, wy = _taps(out_h, sh, scale_y, a, coord_dtype, centres, first_tap, reverse_phase)
    ix, wx = _taps(out_w, sw, scale_x, a, coord_dtype, centres, first_tap, reverse_phase)
    out = np.zeros(src.shape[:-2] + (out_h, out_w), np.float64)
    for i in range(4):
        for j in range(4):
            out += (wy[:, i, None] * wx[None, :, j]) * src[..., iy[:, i, None], ix[None, :, j]]
    return out


def cv_size(n, f):
    """cv2.resize(fx=f): dsize = cvRound(n * f), round-half-to-even like Python's round"""
    return int(round(n * f))


def resize_by_factor(src, fy, fx, **kw):
    """cv2.resize(src, None, fx=fx, fy=fy, INTER_CUBIC) on the last two axes"""
    sh, sw = np.shape(src)[-2:]
    return resize(src, cv_size(sh, fy), cv_size(sw, fx), 1.0 / fy, 1.0 / fx, **kw)


def upsample4(plane, **kw):
    """x4 on the last two axes"""
    return resize_by_factor(plane, 4.0, 4.0, **kw)


def resize_u8_real(img, scale, coord_dtype=np.float32):
    """cv2.resize(img, (0, 0), fx=scale, fy=scale, INTER_CUBIC) of a uint8 (H, W, C) image in real arithmetic: the UNROUNDED,
    unclipped float64 result (OpenCV rounds 11-bit fixed-point coefficients instead)"""
    planes = np.moveaxis(np.asarray(img, np.float64), -1, 0)
    return np.moveaxis(resize_by_factor(planes, scale, scale, coord_dtype=coord_dtype), 0, -1)


def flip_average(net_out, flip=True):
    """utils/parse_skeletons.py:82-103 with NumPy in the array's own dtype, as test_flip_average_matches_numpy_semantics
    writes it: net_out (2|1, 50, h, w) -> heat (20, h, w), paf (30, h, w) float32"""
    from posepaf import skeleton as sk
    o0 = net_out[0].transpose(1, 2, 0)
    if flip:
        o1 = net_out[1].transpose(1, 2, 0)
        paf = (o0[:, :, :30] + o1[:, :, :30][:, ::-1, :][:, :, sk.FLIP_PAF_ORD]) / 2
        heat = (o0[:, :, 30:50] + o1[:, :, 30:50][:, ::-1, :][:, :, sk.FLIP_HEAT_ORD]) / 2
        assert paf.dtype == net_out.dtype
    else:
        paf, heat = o0[:, :, :30], o0[:, :, 30:50]
    return (np.ascontiguousarray(heat.transpose(2, 0, 1)).astype(np.float32),
            np.ascontiguousarray(paf.transpose(2, 0, 1)).astype(np.float32))


def predict_entry(net_out, pad_down, pad_right, img_h, img_w, n_scales, flip=True):
    """One scale of predict (utils/parse_skeletons.py:252-281): flip-average, x4, crop the padding, resize to the image
    (cv2.resize with dsize: scale = 1 / (dsize / ssize); a copy when the size does not change), divide by the number of
    scales.  -> heat (20, img_h, img_w), paf (30, img_h, img_w) float64: what this scale adds to the accumulators."""
    out = []
    for planes in flip_average(net_out, flip):
        up = upsample4(planes)
        ch, cw = up.shape[-2] - pad_down, up.shape[-1] - pad_right
        up = up[:, :ch, :cw]
        if (ch, cw) != (img_h, img_w):
            up = resize(up, img_h, img_w, 1.0 / (img_h / ch), 1.0 / (img_w / cw), coord_dtype=np.float32)
        out.append(up / n_scales)
    return out[0], out[1]


def integer_peaks(joint_list_norefine, upsample=4):
    """(px, py) of heatmap_nms(refine=False) rows, whose coordinates are (p + 0.5) * upsample - 0.5"""
    xy = (np.asarray(joint_list_norefine, np.float64)[:, :2] + 0.5) / upsample - 0.5
    assert np.array_equal(xy, np.round(xy))
    return xy.astype(np.int64)


def refine_peaks(heat, peaks_xy, parts, win=2):
    """heatmap_nms's refinement (utils/parse_skeletons.py:143-163) on this reference: per peak the window clipped to the map,
    x4 with replication at the PATCH edge, first arg-max.  heat (>=18, h, w); -> x (N,), y (N,), score (N,) and the gap
    between the largest and the second-largest value of each up-sampled patch (how decisive the arg-max is)."""
    heat = np.asarray(heat, np.float64)
    h, w = heat.shape[-2:]
    xs, ys, sc, gap = [], [], [], []
    for (px, py), part in zip(peaks_xy, parts):
        x0, y0 = max(px - win, 0), max(py - win, 0)
        x1, y1 = min(px + win, w - 1), min(py + win, h - 1)
        up = upsample4(heat[int(part), y0:y1 + 1, x0:x1 + 1])
        k = int(np.argmax(up))
        row, col = divmod(k, up.shape[1])
        top = np.partition(up.ravel(), -2)[-2:]
        xs.append(4 * x0 + col)
        ys.append(4 * y0 + row)
        sc.append(up[row, col])
        gap.append(top[1] - top[0])
    return np.array(xs, np.float64), np.array(ys, np.float64), np.array(sc), np.array(gap)


def assert_refined_peaks(joint_list, joint_list_norefine, heat, what=""):
    """rows [x, y, score, id, part] of a refined joint list against this reference: every peak on the reference's arg-max
    pixel, its score within DYADIC_TOL; ids and parts those of the unrefined list.  Returns the smallest arg-max gap."""
    jl, jl0 = np.asarray(joint_list), np.asarray(joint_list_norefine)
    assert jl.shape == jl0.shape and np.array_equal(jl[:, 3:], jl0[:, 3:]), what
    x, y, score, gap = refine_peaks(heat, integer_peaks(jl0), jl0[:, 4])
    err = np.abs(jl[:, 2].astype(np.float64) - score)
    print(f"{what}: {len(jl)} peaks, score error max {err.max():.3g}, smallest arg-max gap {gap.min():.3g}")
    assert np.array_equal(jl[:, 0], x) and np.array_equal(jl[:, 1], y), what
    assert err.max() <= DYADIC_TOL, (what, err.max())
    return gap.min()


def corner_edge_map(h=24, w=32, dtype=np.float32):
    """Heat planes (1, 50, h, w) with one blob per keypoint channel group in each corner, on each edge and inside.  The blobs
    are centred off the pixel grid (by 0.3 / 0.2 px, signs differing) so that no two up-sampled values tie."""
    net = np.zeros((1, 50, h, w), np.float64)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    sites = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2 - 3), (h // 2, 0), (h // 2 - 3, w - 1),
             (1, 8), (h - 2, w - 8), (h // 2, w // 2)]
    for part in range(18):
        for k, (cy, cx) in enumerate(sites):
            # towards the inside of the map, so the maximum pixel is the site itself
            oy = 0.3 if cy < h // 2 else -0.3
            ox = 0.2 if cx < w // 2 else -0.2
            amp = 0.45 + 0.02 * part + 0.03 * k
            net[0, 30 + part] += amp * np.exp(-((yy - cy - oy) ** 2 + (xx - cx - ox) ** 2) / (2 * 1.3 ** 2))
    return net.astype(dtype)


# ---- the cases the CPU test (oracle) and the GPU test (kernels) share

# (name, image size, [(map size, (pad_down, pad_right))]): a crop and a down-scaling resize; a x4 up-scaling, an identity
# (cv2.resize returns a copy) and a cropped down-scaling accumulated into one image
PREDICT_CASES = [("one scale", (50, 66), [((16, 24), (8, 24))]),
                 ("three scales", (64, 96), [((8, 12), (0, 0)), ((16, 24), (0, 0)), ((24, 36), (8, 16))])]


def predict_inputs(entries, dtype, flip, seed=77):
    """[(network output (2|1, 50, h, w) uniform in [-0.5, 1.5], (pad_down, pad_right))]"""
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-0.5, 1.5, (2 if flip else 1, 50, h, w)).astype(dtype), pads) for (h, w), pads in entries]


U8_SCALES = [0.5, 0.7, 1.37, 1.5, 2.0]


def u8_images(h=50, w=66):
    """a random-noise image and a smooth one, uint8 (h, w, 3)"""
    noise = np.random.default_rng(9).integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    smooth = np.stack([127.5 + 127.5 * np.sin(0.11 * (k + 1) * xx + 0.5 * k) * np.cos(0.07 * (k + 2) * yy) for k in range(3)], -1)
    return {"noise": noise, "smooth": np.rint(smooth).astype(np.uint8)}


def assert_u8_close(got, img, scale, what=""):
    """a uint8 INTER_CUBIC resize against rint(clip(real arithmetic)): no pixel off by more than one count, at most 15 % of
    the pixels off at all"""
    want = np.rint(np.clip(resize_u8_real(img, scale), 0, 255))
    assert got.shape == want.shape and got.dtype == np.uint8, what
    diff = np.abs(got.astype(np.float64) - want)
    print(f"{what}: max {diff.max():.0f} count, {100 * (diff > 0).mean():.2f} % of the pixels differ")
    assert diff.max() <= 1, what
    assert (diff > 0).mean() <= 0.15, what
