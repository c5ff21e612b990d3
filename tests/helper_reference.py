"""A NumPy restatement, in float64 and written from the formulas of include/posepaf.h, of the forward's helper entries
(csrc/posepaf_epilogue.hip).  Every function returns the float64 value that the entry's output ROUNDS (once, to the output's type):

    pp_bias_act_f16            t = y + b[c] (+ res);  t = t if t > 0 else slope t  (has_act);  t (+ post);              y = half(t)
    pp_add3_f16                a + b (+ c)                                                                              y = half(t)
    pp_channel_scale_f16       x[n][p][c] * s[n][c]                                                                     y = half(t)
    pp_channel_mean(_finish)   fl32(sum_p x[n][p][c] * fl32(1 / hw))                                                    m = half(t)
    pp_se_gains_f16            m = half(mean);  h = half(W1 m + b1);  h = half(leaky(h));  z = half(W2 h + b2);         g = half(sigmoid(z))
    pp_maxpool2_f16 / the pooled output of pp_pw_pool_f16      pool_max: the maximum of the window's non-NaN elements (+0 above -0), NaN
                               only when all four are NaN
    pp_upsample2_f16, pp_nhwc64_to_planes_f16                  copies
    pp_preprocess_u8(_ragged)  fl32(u8) / fl32(255) inside the image, fl32(pad_value) / fl32(255) outside; the mirror is that of the
                               PADDED image
    pp_flip_average            binary16: half(half(a + b') * 0.5);  float32: fl32(a + b') / 2;  b' = the mirrored sample's partner channel
                               at the mirrored column (the reference's utils/parse_skeletons.py:92-93 with config.flip_paf_ord / flip_heat_ord)

with the operand recipes of tests/test_gpu_helper_kernels.py (`small`, `rounding`, `subnormal`: every fp32 partial sum exact in any
order, so bit equality may be asked of any kernel; `special`: NaN, +-inf, +-0, +-65504 at known indices), the rounding bound of the
real-operand runs and the shape lists with what each of them is there to reach.  Nothing here imports the package."""
import numpy as np

SLOPE = 0.125                       # the exact recipes' slope: a power of two, slope * t is exact
LEAK = np.float32(0.01)             # fused_model.LEAK as the entries receive it
SUB = 2.0 ** -24                    # the binary16 subnormal grid
RECIPES = ("small", "rounding", "subnormal", "special")
SPECIALS = np.array([0x7E00, 0x7C00, 0xFC00, 0x0000, 0x8000, 0x7BFF, 0xFBFF], np.uint16).view(np.float16)  # NaN +-inf +-0 +-65504
NUM_LIMB, NUM_HEAT, NUM_CH = 30, 20, 50
# the flip tables of the reference's configuration (data: config/config.py flip_heat_ord / flip_paf_ord), typed as lists
FLIP_HEAT = [0, 1, 5, 6, 7, 2, 3, 4, 11, 12, 13, 8, 9, 10, 15, 14, 17, 16, 18, 19]
FLIP_PAF = [0, 2, 1, 4, 3, 6, 5, 8, 7, 12, 13, 14, 9, 10, 11, 18, 19, 20, 15, 16, 17, 22, 21, 25, 26, 23, 24, 28, 27, 29]
FLIP_CH = FLIP_PAF + [NUM_LIMB + k for k in FLIP_HEAT]          # network channels: 30 limb channels, then 20 heat channels

WORK_ITEMS_FIRST_PASS = 8192 * 256  # grid-stride kernels: at most 8192 workgroups of 256; item 2,097,152 is the second pass's first


def to_half(t):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(t).astype(np.float16)


def f64(a):
    return np.asarray(a).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the restatements

def bias_act(y, bias, res, post, act, slope):
    """y, res, post: binary16 (..., c); bias: binary16 (c); slope as the float32 the entry receives -> float64 (..., c)"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = f64(y) + f64(bias)
        if res is not None:
            t = t + f64(res)
        if act:
            t = np.where(t > 0.0, t, t * float(np.float32(slope)))
        if post is not None:
            t = t + f64(post)
    return t


def bias_act_abs_terms(y, bias, res, post):
    s = np.abs(f64(y)) + np.abs(f64(bias))
    for a in (res, post):
        if a is not None:
            s = s + np.abs(f64(a))
    return s


def add3(a, b, c=None):
    with np.errstate(invalid="ignore", over="ignore"):
        t = f64(a) + f64(b)
        return t if c is None else t + f64(c)


def channel_scale(x, s):
    """x: binary16 (n, hw, c); s: binary16 (n, c)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return f64(x) * f64(s)[:, None, :]


def channel_sums(x):
    """x: binary16 (n, hw, c) -> float64 (n, c), the sums over the pixels"""
    return f64(x).sum(axis=1)


def mean_of_sums(sums, hw):
    """fl32(sum * fl32(1 / hw)) as float64; the sums must be float32 values (asserted): the exact recipes' are"""
    s32 = np.asarray(sums).astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), f64(sums)), "the channel sums are not float32 values"
    inv = np.float32(1.0) / np.float32(hw)
    return (s32 * inv).astype(np.float64)


def channel_mean_real(x):
    """the mean in real arithmetic, for the real-operand run: float64 (n, c)"""
    return f64(x).mean(axis=1)


def sigmoid(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-f64(z)))


def se_gains(mean, w1, b1, w2, b2, slope, round_hidden_sum=True):
    """mean: binary16 (n, c) -- half(mean_of_sums(..)) for the partial-sum source; w1 (hidden, c), b1 (hidden), w2 (c, hidden), b2 (c)
    binary16 -> dict of float64: `hidden_sum` (n, hidden) = W1 m + b1 before its rounding, `hidden` after both roundings, `z_sum` (n, c)
    = W2 h + b2 before its rounding, `z` after it, `gain` = sigmoid(z), the value the output rounds.  round_hidden_sum=False leaves out
    the hidden vector's first rounding: NOT the contract, for the CPU test that shows a case can tell the two apart"""
    m = f64(mean)
    hs = m @ f64(w1).T + f64(b1)
    h = f64(to_half(hs)) if round_hidden_sum else hs
    h = f64(to_half(np.where(h > 0.0, h, h * float(np.float32(slope)))))
    zs = h @ f64(w2).T + f64(b2)
    z = f64(to_half(zs))
    return dict(hidden_sum=hs, hidden=h, z_sum=zs, z=z, gain=sigmoid(z))


def half_boundary_distance(v):
    """relative distance of the float64 values v > 0 from the binary16 rounding boundary between the two neighbouring binary16 values
    that enclose v (their midpoint; 2^-25 below the smallest subnormal): every other boundary is at least 2^-13 away"""
    v = f64(v)
    lo = f64(to_half(v))
    lo = np.where(lo > v, np.nextafter(lo.astype(np.float16), np.float16(-np.inf)).astype(np.float64), lo)     # largest half <= v
    hi = np.nextafter(lo.astype(np.float16), np.float16(np.inf)).astype(np.float64)
    mid = 0.5 * (lo + hi)
    return np.abs(v - mid) / v


SE_Z_CLEARANCE = 2.0 ** -18


def se_z_is_clear(z):
    """sigmoid(z) in float64 is at least 2^-18 relative away from a binary16 rounding boundary: an fp32 evaluation of
    1 / (1 + expf(-z)), good to a few 2^-24, rounds to the same binary16 value"""
    return half_boundary_distance(sigmoid(z)) >= SE_Z_CLEARANCE


def pool_max(x):
    """x: binary16 (n, 2 ho, 2 wo, c) -> float64 (n, ho, wo, c): per 2x2 window the maximum of the non-NaN elements, +0 above -0
    (IEEE 754-2019 maximumNumber); NaN only when all four are NaN"""
    x = np.asarray(x)
    assert x.dtype == np.float16 and x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0
    v = np.stack([f64(x[:, i::2, j::2]) for i in (0, 1) for j in (0, 1)], axis=-1)
    nan = np.isnan(v)
    m = np.where(nan, -np.inf, v).max(axis=-1)
    pos_zero = ((v == 0.0) & ~np.signbit(v)).any(axis=-1)
    m = np.where(m == 0.0, np.where(pos_zero, 0.0, -0.0), m)
    return np.where(nan.all(axis=-1), np.nan, m)


def upsample2(x):
    """x: (n, h, w, c) -> (n, 2 h, 2 w, c), nearest"""
    return np.repeat(np.repeat(np.asarray(x), 2, axis=1), 2, axis=2)


def nhwc64_to_planes(x, c_out):
    """x: (n, hw, 64) -> (n, c_out, hw): y[i][c][p] = x[i][p][c]"""
    return np.ascontiguousarray(np.asarray(x).transpose(0, 2, 1)[:, :c_out])


def preprocess(images, sizes, pad_value, flip):
    """images: uint8 (b, hp, wp, 3) slots, image i in the top-left (sizes[0][i], sizes[1][i]) corner of its slot (for the entry with
    equal sizes: the image padded by anything); -> float64 (b * (2 if flip else 1), hp, wp, 3) of float32 values; bytes outside an
    image's corner do not enter the result"""
    images = np.asarray(images)
    assert images.dtype == np.uint8
    b, hp, wp, _ = images.shape
    v = (images.astype(np.float32) / np.float32(255)).astype(np.float64)
    pad = float(np.float32(pad_value) / np.float32(255))
    yy, xx = np.arange(hp)[None, :, None], np.arange(wp)[None, None, :]
    inside = (yy < np.asarray(sizes[0])[:, None, None]) & (xx < np.asarray(sizes[1])[:, None, None])
    v = np.where(inside[..., None], v, pad)
    if not flip:
        return v
    out = np.empty((b, 2, hp, wp, 3), np.float64)
    out[:, 0], out[:, 1] = v, v[:, :, ::-1]
    return out.reshape(2 * b, hp, wp, 3)


def flip_average(net, flip):
    """net: binary16 or float32 (b * (2 if flip else 1), 50, h, w) -> (heat float64 (b, h, w, 20), paf float64 (b, h, w, 30)), the
    float32 values the entry stores"""
    net = np.asarray(net)
    assert net.dtype in (np.float16, np.float32) and net.shape[1] == NUM_CH
    if not flip:
        avg = f64(net)
    else:
        a, b = net[0::2], net[1::2][:, FLIP_CH][:, :, :, ::-1]
        with np.errstate(over="ignore", invalid="ignore"):
            if net.dtype == np.float16:
                avg = f64(to_half(f64(to_half(f64(a) + f64(b))) * 0.5))
            else:
                avg = f64((a + b).astype(np.float32)) / 2.0
    hwc = avg.transpose(0, 2, 3, 1)
    return np.ascontiguousarray(hwc[..., NUM_LIMB:]), np.ascontiguousarray(hwc[..., :NUM_LIMB])


def rounding_bound(t, abs_terms, k):
    """|got - t| <= E + max(2^-11 (|t| + E), 2^-25),  E = 2^-24 k sum |terms|: k float32 operations, each within 2^-24 relative of a
    value no larger than the sum of the |terms|, then one binary16 rounding: relative 2^-11 of the rounded value, or half a subnormal step"""
    E = 2.0 ** -24 * k * f64(abs_terms)
    return E + np.maximum(2.0 ** -11 * (np.abs(f64(t)) + E), 2.0 ** -25)


# ------------------------------------------------------------------------------------------------ operand recipes

def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(np.float16)


def special_index(shape, operand):
    """the index into SPECIALS (7 = an ordinary value) that element (pixel, channel) of operand number `operand` holds under `special`:
    a tensor operand cycles with its pixel in base 7 (digit `operand`), so 7^k pixels hold every combination of k tensor operands"""
    pix = np.arange(shape[0])[:, None]
    return np.broadcast_to((pix // 7 ** operand) % 7, shape)


def tensor_operands(recipe, pixels, c, count, seed):
    """`count` binary16 tensors (pixels, c) and one per-channel vector (c):
    small      integers in [-4, 4]
    rounding   integers of magnitude up to 3000 (sums beyond 2048 need the store's rounding), a quarter of the elements +-60000
               (sums beyond 65520 overflow to infinity); the vector in [-255, 255]
    subnormal  integers in [-40, 40] times 2^-24
    special    `small`, with SPECIALS[special_index] in every tensor and SPECIALS[channel % 8] (channel % 8 == 7: ordinary) in the vector"""
    assert recipe in RECIPES
    rng = np.random.default_rng([seed, pixels, c, RECIPES.index(recipe)])
    shape = (pixels, c)
    if recipe == "rounding":
        ts = [_ints(rng, -3000, 3000, shape) for _ in range(count)]
        for t in ts:
            big = rng.random(shape) < 1 / 4
            t[big] = (rng.choice(np.array([-60000.0, 60000.0]), int(big.sum()))).astype(np.float16)
        vec = _ints(rng, -255, 255, (c,))
    else:
        ts = [_ints(rng, -4, 4, shape) for _ in range(count)]
        vec = _ints(rng, -4, 4, (c,))
    if recipe == "subnormal":
        ts = [(f64(_ints(rng, -40, 40, shape)) * SUB).astype(np.float16) for _ in range(count)]
        vec = (f64(_ints(rng, -40, 40, (c,))) * SUB).astype(np.float16)
    if recipe == "special":
        for k, t in enumerate(ts):
            idx = special_index(shape, k)
            t[idx < 7] = SPECIALS[idx[idx < 7]]
        ch = np.arange(c) % 8
        vec[ch < 7] = SPECIALS[ch[ch < 7]]
    return ts, vec


def scale_operands(recipe, n, hw, c, seed):
    """x (n, hw, c) and the gains s (n, c) of pp_channel_scale_f16:
    small      x integers in [-4, 4], s from {0.5, 1, 1.5, 2, -3}
    rounding   x integers up to +-3000, s integers up to +-3000 (products of 22 bits: exact in float32, rounded by the store) and, for a
               quarter of x, +-60000 (overflow)
    subnormal  x integers in [-40, 40] times 2^-24, s from {0.5, 0.25, 1, -1.5, 3}: products on the 2^-26 grid, ties included
    special    x as tensor_operands' first tensor (per image), s = SPECIALS[channel % 8]"""
    (x,), vec = tensor_operands(recipe, n * hw, c, 1, seed)
    rng = np.random.default_rng([seed, n, hw, c, 77])
    if recipe == "small":
        s = rng.choice(np.array([0.5, 1, 1.5, 2, -3], np.float16), (n, c))
    elif recipe == "rounding":
        s = _ints(rng, -3000, 3000, (n, c))
    elif recipe == "subnormal":
        s = rng.choice(np.array([0.5, 0.25, 1, -1.5, 3], np.float16), (n, c))
    else:
        s = np.broadcast_to(vec, (n, c)).copy()
    return x.reshape(n, hw, c), s


def mean_operands(case):
    """x binary16 (n, hw, c) of pp_channel_mean_f16: integers in [-4, 4], a function of the case alone"""
    n, hw, c, splits = case
    return _ints(np.random.default_rng([n, hw, c, splits, 3]), -4, 4, (n, hw, c))


def grid_units(abs_sum, grid):
    return float(np.max(f64(abs_sum))) / grid


def assert_exact(values, abs_sum, grid, what):
    """the condition under which ANY order of float32 additions is exact: every term an integer multiple of `grid` (a power of two)
    and the sum of the |terms| below 2^24 grid units"""
    for v in values:
        q = f64(v)[np.isfinite(f64(v))] / grid
        assert np.array_equal(q, np.round(q)), f"{what}: a term is off the {grid} grid"
    a = f64(abs_sum)
    units = grid_units(a[np.isfinite(a)], grid)
    assert units < 2.0 ** 24, f"{what}: sum |terms| = {units} grid units"
    return units


def recipe_grid(recipe):
    return SUB * SLOPE if recipe == "subnormal" else SLOPE        # slope * t is a term too


# ------------------------------------------------------------------------------------------------ pooled windows

def pool_windows(c, per_row=4):
    """binary16 (1, 2 * 32 / per_row, 2 * per_row, c): 32 windows -- NaN in each of the four positions, in every pair and triple of them, all NaN;
    +-inf against finite values, each other and NaN; +0 and -0 mixed in every arrangement of the four positions, all -0, -0 with NaN,
    -0 against negative values; +-65504.  Channel k of a window adds k to its ordinary values, so channels differ."""
    nan, inf = np.nan, np.inf
    base = [
        [nan, 1, 2, 3], [1, nan, 2, 3], [1, 2, nan, 3], [1, 2, 3, nan], [nan, nan, 2, 3], [nan, 1, nan, 3], [1, nan, 3, nan], [1, 2, nan, nan],
        [nan, nan, nan, 3], [nan, nan, 3, nan], [nan, 3, nan, nan], [3, nan, nan, nan], [nan, nan, nan, nan], [inf, 1, 2, 3], [1, -inf, 2, 3],
        [-inf, -inf, -inf, -inf], [inf, -inf, nan, 1], [-inf, nan, nan, nan], [nan, inf, nan, -inf], [65504, -65504, 1, 2],
        [0.0, -0.0, -0.0, -0.0], [-0.0, 0.0, -0.0, -0.0], [-0.0, -0.0, 0.0, -0.0], [-0.0, -0.0, -0.0, 0.0], [-0.0, -0.0, -0.0, -0.0],
        [-0.0, nan, nan, nan], [nan, -0.0, 0.0, nan], [-0.0, -1, -2, -3], [0.0, -0.0, -1, nan], [-0.0, 0.0, 0.0, -0.0], [-1, -2, -3, -4],
        [-65504, -inf, nan, -65504],
    ]
    x = np.zeros((1, 2 * (32 // per_row), 2 * per_row, c), np.float16)
    for i, wv in enumerate(base):
        r, q = 2 * (i // per_row), 2 * (i % per_row)
        for j, v in enumerate(wv):
            ordinary = np.isfinite(v) and v != 0.0 and abs(v) < 100
            x[0, r + j // 2, q + j % 2, :] = (v + np.arange(c) % 5 * np.sign(v)) if ordinary else v
    return x


# ------------------------------------------------------------------------------------------------ the SE excitation's integer recipe

SE_CASES = [(1, 8, 1, 1), (2, 256, 16, 40), (3, 768, 48, 7), (1, 4096, 1024, 2)]      # (n, c, hidden, splits)
SE_HW = {1: 4096, 40: 1000, 7: 4096, 2: 36}                                            # per splits: a power of two and not
# 0.125 as everywhere; and 0.375 = 3 * 2^-3, still exact in float32 (a binary16 value times 3 has 13 bits) but no power of two: under
# a power of two half(slope * half(t)) == half(slope * t), and a kernel that forgot the hidden vector's first rounding would go unseen
SE_SLOPES = (SLOPE, 0.375)


def se_operands(case, slope=SLOPE):
    """dict for pp_se_gains_f16 on grids: means integers in [-2, 2]; w1 integers in [-2, 2] times 2^-9; b1 = +-4 + {-1, 0, 1} (so
    W1 m + b1 carries more bits than binary16 keeps: the hidden vector's rounding shows); w2 from {-1, 0, 1} times 2^-k, k such that z
    stays of order one; b2 integers in [-2, 2], moved by eighths where a sample's z would leave sigmoid(z) near a binary16 rounding
    boundary (se_z_is_clear): the gain's bits then do not depend on the last bits of expf.  `partial` (n, splits, c) float32 integers
    with sum = mean * hw.  grid1 / grid2: the grids of the two products' terms (the hidden vector is below 8: a negative one times
    the slope sits on 2^-12).  A function of the case alone."""
    n, c, hidden, splits = case
    hw = SE_HW[splits]
    rng = np.random.default_rng([n, c, hidden, splits, 5])
    mean = _ints(rng, -2, 2, (n, c))
    w1 = (rng.integers(-2, 3, (hidden, c)) * 2.0 ** -9).astype(np.float16)
    b1 = (rng.choice(np.array([-4.0, 4.0]), hidden) + rng.integers(-1, 2, hidden)).astype(np.float16)
    k2 = int(np.ceil(np.log2(np.sqrt(hidden) * 2)))
    w2 = (rng.integers(-1, 2, (c, hidden)) * 2.0 ** -k2).astype(np.float16)
    b2 = f64(_ints(rng, -2, 2, (c,)))
    zs0 = se_gains(mean, w1, b1, w2, np.zeros(c, np.float16), slope)["z_sum"]          # W2 h: b2 is added below
    todo, chosen = np.ones(c, bool), b2.copy()
    for step in (0, 1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6):
        cand = b2 + step * 0.125
        ok = se_z_is_clear(f64(to_half(zs0 + cand))).all(axis=0)
        chosen[todo & ok] = cand[todo & ok]
        todo &= ~ok
        if not todo.any():
            break
    assert not todo.any(), "no b2 within six eighths clears every sample's z"
    b2 = chosen
    b2 = b2.astype(np.float16)
    parts = rng.integers(-50, 51, (n, splits, c)).astype(np.float64)
    parts[:, -1] += f64(mean) * hw - parts.sum(axis=1)
    return dict(n=n, c=c, hidden=hidden, splits=splits, hw=hw, slope=slope, mean=mean, w1=w1, b1=b1, w2=w2, b2=b2, partial=parts.astype(np.float32),
                grid1=2.0 ** -9, grid2=2.0 ** -12 * 2.0 ** -k2)


def se_z_values(case, slope=SLOPE):
    """the sorted list of the z values the case's samples reach"""
    o = se_operands(case, slope)
    return np.unique(se_gains(o["mean"], o["w1"], o["b1"], o["w2"], o["b2"], slope)["z"])


# ------------------------------------------------------------------------------------------------ shapes and what they reach

SECOND_PASS_VECTORS = WORK_ITEMS_FIRST_PASS + 3                 # bias_act / add3: 16-byte vectors, c = 8
POOL_SHAPES = [(1, 1, 1, 8), (2, 3, 5, 24), (1, 2, 7, 8)]       # (n, h_out, w_out, c): one output, odd w_out, both channel counts
POOL_SECOND_PASS = (1, 1449, 1449, 8)                           # 2,099,601 output vectors (one per pixel at c = 8)
UPSAMPLE_SECOND_PASS = (1, 1449, 1449, 8)                       # the same count of INPUT vectors
MEAN_CASES = [(1, 5, 8, 4), (2, 1000, 192, 7), (1, 300, 2048, 3), (3, 4096, 64, 8), (1, 64, 8, 64)]   # (n, hw, c, splits)
SCALE_CHANNELS = [8, 24, 192]
SCALE_CAPPED = (1, 8 * 32 * 4096 + 5, 64)                       # (n, hw, c): 32 pixel lanes, 4097 pixel blocks for a grid capped at 4096
PLANES_HW, PLANES_C_OUT = [72, 8, 64, 63 + 64], [1, 50, 64]
PREPROCESS_LARGE = dict(batch=9, h=481, w=483, pad_to=5)        # padded to 485 x 485: 2,117,025 pixels
RAGGED_LARGE = dict(batch=9, hp=485, wp=485, sizes=[(481, 483), (300, 485)])
FLIP_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 205, 205)]             # (batch, h, w); the last: 2,101,250 elements
