"""GPU: the helper entries of csrc/posepaf_epilogue.hip against the float64 restatement of tests/helper_reference.py, bit for bit:
on the exact recipes that tests/test_helper_reference_cpu.py proves exact (`small`, `rounding`, `subnormal`) and on `special` (NaN,
+-inf, +-0, +-65504 at known indices; any NaN equals any NaN), at the shapes where the kernels take another path -- the second pass of
the grid-stride loops, every split shape of the channel sums, idle threads and one pixel lane, the capped grid of the scale kernel, the
partial tile with 16-byte rows of the layout change -- and inside the derived rounding bound on real operands with subnormals.
Every operand is framed by 0xFF bytes (NaN in binary16 and float32), every output is filled with them and followed by a 64-byte guard
that must stay intact; an output element that still holds the fill was not written."""
import ctypes as C

import numpy as np
import pytest
import torch

import helper_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL, FRAME, GUARD = 0xFF, 128, 64
PP_F32, PP_F16 = 0, 1
NP_OF = {PP_F16: np.float16, PP_F32: np.float32}


@pytest.fixture(scope="module")
def lib():
    from posepaf import _lib
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync():
    torch.cuda.synchronize()


class In:
    """a device copy of `a` with FRAME bytes of 0xFF in front of it and behind it, 16-byte aligned"""

    def __init__(self, a):
        a = np.ascontiguousarray(a)
        raw = torch.from_numpy(a.reshape(-1).view(np.uint8).copy())
        self.buf = torch.full((raw.numel() + 2 * FRAME,), FILL, dtype=torch.uint8, device=DEV)
        self.buf[FRAME:FRAME + raw.numel()].copy_(raw)
        self.ptr = self.buf.data_ptr() + FRAME
        assert self.ptr % 16 == 0


class Out:
    """a device buffer of `shape` elements filled with 0xFF (or holding `init`, for an entry that works in place) and a guard behind it"""

    def __init__(self, shape, dtype, init=None):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.buf = torch.full((self.nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        if init is not None:
            init = np.ascontiguousarray(init)
            assert init.dtype == self.dtype and init.shape == self.shape
            self.buf[:self.nbytes].copy_(torch.from_numpy(init.reshape(-1).view(np.uint8).copy()))
        self.ptr = self.buf.data_ptr()
        assert self.ptr % 16 == 0

    def read(self):
        sync()
        host = self.buf.cpu().numpy()
        assert (host[self.nbytes:] == FILL).all(), "the guard behind the output was written"
        return host[:self.nbytes].view(self.dtype).reshape(self.shape)


def vp(x):
    return None if x is None else C.c_void_p(x.ptr)


def round_to(want64, dtype):
    return ref.to_half(want64) if dtype == np.float16 else np.asarray(want64).astype(np.float32)


def assert_bits(got, want64, what):
    """got: binary16 or float32 from the device; want64: the float64 value it rounds.  Bit patterns; any NaN equals any NaN but the fill"""
    want = round_to(want64, got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    U = np.uint16 if got.dtype == np.float16 else np.uint32
    gb, wb = got.view(U), want.view(U)
    ok = np.where(np.isnan(want), np.isnan(got) & (gb != np.iinfo(U).max), gb == wb)
    if not ok.all():
        first = tuple(np.argwhere(~ok)[0].tolist())
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements differ, first at {first}: {gb[first]:#x} ({got[first]!r}) "
                             f"for {wb[first]:#x} ({want[first]!r})")


def assert_bits_chunked(got, want_of, rows, what):
    """the same over the leading axis in pieces of `rows`: want_of(lo, hi) -> the float64 expectation of got[lo:hi]"""
    for lo in range(0, got.shape[0], rows):
        hi = min(lo + rows, got.shape[0])
        assert_bits(got[lo:hi], want_of(lo, hi), f"{what}, rows {lo}..{hi}")


def real16(rng, shape):
    """N(0, 1) binary16 with a tenth of subnormals of either sign"""
    v = rng.standard_normal(shape).astype(np.float16)
    sub = rng.integers(1, 0x400, shape).astype(np.uint16).view(np.float16) * rng.choice(np.array([-1, 1], np.float16), shape)
    out = np.where(rng.random(shape) < 0.1, sub, v).astype(np.float16)
    assert ((np.abs(out) < 2.0 ** -14) & (out != 0)).mean() > 0.05
    return out


def report_bound(got, want64, bound, what):
    err = np.abs(got.astype(np.float64) - want64)
    print(f"{what}: largest err / bound = {(err / bound).max():.4f}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), what


# ------------------------------------------------------------------------------------------------ pp_bias_act_f16

def run_bias_act(lib, y, bias, res, post, act, slope):
    out = Out(y.shape, np.float16, init=y)
    ops = [In(bias), In(res) if res is not None else None, In(post) if post is not None else None]
    assert lib.pp_bias_act_f16(vp(out), vp(ops[0]), vp(ops[1]), vp(ops[2]), y.size, y.shape[-1], float(slope), int(act), stream()) == 0
    return out.read()


@pytest.mark.parametrize("recipe", ref.RECIPES)
@pytest.mark.parametrize("res,act,post", [(r, a, p) for r in (0, 1) for a in (0, 1) for p in (0, 1)])
def test_bias_act_exact(lib, res, act, post, recipe):
    for c in (8, 24, 192):
        (y, r, p), b = ref.tensor_operands(recipe, 343, c, 3, 11)
        r, p = (r if res else None), (p if post else None)
        got = run_bias_act(lib, y, b, r, p, act, ref.SLOPE)
        assert_bits(got, ref.bias_act(y, b, r, p, act, ref.SLOPE), f"c = {c}")


def test_bias_act_second_pass(lib):
    (y, r, p), b = ref.tensor_operands("small", ref.SECOND_PASS_VECTORS, 8, 3, 12)
    got = run_bias_act(lib, y, b, r, p, 1, ref.SLOPE)
    assert_bits_chunked(got, lambda lo, hi: ref.bias_act(y[lo:hi], b, r[lo:hi], p[lo:hi], 1, ref.SLOPE), 1 << 18, "second pass")


def test_bias_act_real_operands(lib):
    rng = np.random.default_rng(13)
    y, r, p, b = real16(rng, (1000, 24)), real16(rng, (1000, 24)), real16(rng, (1000, 24)), real16(rng, (24,))
    got = run_bias_act(lib, y, b, r, p, 1, ref.LEAK)
    want = ref.bias_act(y, b, r, p, 1, ref.LEAK)
    report_bound(got, want, ref.rounding_bound(want, ref.bias_act_abs_terms(y, b, r, p), 4), "bias_act (res, act, post)")   # 3 sums, 1 product


# ------------------------------------------------------------------------------------------------ pp_add3_f16

def run_add3(lib, a, b, c):
    out = Out(a.shape, np.float16)
    ops = [In(a), In(b), In(c) if c is not None else None]
    assert lib.pp_add3_f16(vp(ops[0]), vp(ops[1]), vp(ops[2]), vp(out), a.size, stream()) == 0
    return out.read()


@pytest.mark.parametrize("recipe", ref.RECIPES)
@pytest.mark.parametrize("with_c", [0, 1])
def test_add3_exact(lib, with_c, recipe):
    (a, b, c), _ = ref.tensor_operands(recipe, 343, 24, 3, 21)
    c = c if with_c else None
    assert_bits(run_add3(lib, a, b, c), ref.add3(a, b, c), recipe)


def test_add3_second_pass(lib):
    (a, b, c), _ = ref.tensor_operands("small", ref.SECOND_PASS_VECTORS, 8, 3, 22)
    assert_bits_chunked(run_add3(lib, a, b, c), lambda lo, hi: ref.add3(a[lo:hi], b[lo:hi], c[lo:hi]), 1 << 18, "second pass")


def test_add3_real_operands(lib):
    rng = np.random.default_rng(23)
    a, b, c = real16(rng, (1000, 24)), real16(rng, (1000, 24)), real16(rng, (1000, 24))
    want = ref.add3(a, b, c)
    report_bound(run_add3(lib, a, b, c), want, ref.rounding_bound(want, np.abs(ref.f64(a)) + np.abs(ref.f64(b)) + np.abs(ref.f64(c)), 2), "add3")


# ------------------------------------------------------------------------------------------------ the pools and the upsampling

def run_maxpool(lib, x, x_ptr=None):
    n, h, w, c = x.shape if x_ptr is None else x
    out = Out((n, h // 2, w // 2, c), np.float16)
    src = In(x) if x_ptr is None else None
    assert lib.pp_maxpool2_f16(vp(src) if src else C.c_void_p(x_ptr), vp(out), n, h // 2, w // 2, c, stream()) == 0
    return out.read()


@pytest.mark.parametrize("shape", ref.POOL_SHAPES, ids=str)
def test_maxpool_and_upsample_shapes(lib, shape):
    n, ho, wo, c = shape
    rng = np.random.default_rng([31, *shape])
    x = real16(rng, (n, 2 * ho, 2 * wo, c)) if ho * wo > 1 else rng.standard_normal((n, 2, 2, c)).astype(np.float16)
    assert_bits(run_maxpool(lib, x), ref.pool_max(x), "maxpool2")
    small = x[:, :ho, :wo].copy()
    out = Out((n, 2 * ho, 2 * wo, c), np.float16)
    src = In(small)
    assert lib.pp_upsample2_f16(vp(src), vp(out), n, ho, wo, c, stream()) == 0
    assert np.array_equal(out.read().view(np.uint16), ref.upsample2(small).view(np.uint16))


@pytest.mark.parametrize("c", [8, 24])
def test_maxpool_windows_of_nan_infinities_and_signed_zeros(lib, c):
    """the rule of include/posepaf.h: the maximum of the non-NaN elements, NaN only when all four are NaN, +0 above -0"""
    x = ref.pool_windows(c)
    assert_bits(run_maxpool(lib, x), ref.pool_max(x), "maxpool2")


def test_the_two_pools_agree_on_nan_infinities_and_signed_zeros(lib):
    """The same windows through the pooled output of pp_pw_pool_f16 and, on the tensor that call wrote, through pp_maxpool2_f16: the
    tuner may take either for one layer, so both must give the same bits, those of pool_max.  The 1x1 convolution is exact: w = 2^-14 I,
    x = -2^-14 where the tensor shall hold -0 (the product -2^-28 rounds to -0 at the store) and 0 elsewhere, zero bias, slope 1, and every
    other value arrives through `extra` (mode 1: added before the activation) -- NaN and infinities must not pass through the matrix
    product, where they would reach every channel of their pixel."""
    c, width = 128, 32
    target = ref.pool_windows(c, per_row=width // 2)                 # (1, 4, 32, c)
    _, h, _, _ = target.shape
    m = h * width
    neg_zero = target.view(np.uint16) == 0x8000
    x = np.where(neg_zero, np.float16(-2.0 ** -14), np.float16(0)).astype(np.float16).reshape(m, c)
    extra = np.where(neg_zero, np.float16(0), target).astype(np.float16).reshape(m, c)
    w = (np.eye(c) * 2.0 ** -14).astype(np.float16)
    bias = np.zeros(c, np.float16)
    ops = [In(x), In(w), In(bias), In(extra)]
    y, pooled = Out((1, h, width, c), np.float16), Out((1, h // 2, width // 2, c), np.float16)
    assert lib.pp_pw_supported(c, c)
    assert lib.pp_pw_pool_f16(vp(ops[0]), None, vp(ops[1]), vp(ops[2]), vp(ops[3]), None, vp(y), None, vp(pooled), m, m, width, c, c, c, 1, 1.0,
                              stream()) == 0
    assert_bits(y.read(), ref.f64(target), "the tensor that is pooled")
    want = ref.pool_max(target)
    fused = pooled.read()
    assert_bits(fused, want, "the pooled output of pp_pw_pool_f16")
    alone = run_maxpool(lib, (1, h, width, c), x_ptr=y.ptr)
    assert_bits(alone, want, "pp_maxpool2_f16 on the same tensor")
    assert_bits(alone, ref.f64(fused), "pp_maxpool2_f16 against the pooled output of pp_pw_pool_f16")


def test_maxpool_second_pass(lib):
    n, ho, wo, c = ref.POOL_SECOND_PASS
    x = np.random.default_rng(33).integers(-100, 101, (n, 2 * ho, 2 * wo, c), dtype=np.int8).astype(np.float16)
    got = run_maxpool(lib, x)
    assert_bits_chunked(got[0], lambda lo, hi: ref.pool_max(x[:, 2 * lo:2 * hi])[0], 128, "second pass")


def test_upsample_second_pass(lib):
    n, hi, wi, c = ref.UPSAMPLE_SECOND_PASS
    x = np.random.default_rng(34).integers(1, 0x7C00, (n, hi, wi, c), dtype=np.uint16).view(np.float16)
    out, src = Out((n, 2 * hi, 2 * wi, c), np.float16), In(x)
    assert lib.pp_upsample2_f16(vp(src), vp(out), n, hi, wi, c, stream()) == 0
    got = out.read().view(np.uint16)
    for i in (0, 1):
        for j in (0, 1):
            assert np.array_equal(got[:, i::2, j::2], x.view(np.uint16)), (i, j)


# ------------------------------------------------------------------------------------------------ the SE squeeze

def run_mean(lib, x, splits):
    n, hw, c = x.shape
    ws, out, src = Out((n, splits, c), np.float32), Out((n, c), np.float16), In(x)
    assert lib.pp_channel_mean_f16(vp(src), vp(ws), vp(out), n, hw, c, splits, stream()) == 0
    return ws, out.read()


@pytest.mark.parametrize("case", ref.MEAN_CASES, ids=str)
def test_channel_mean_exact(lib, case):
    n, hw, c, splits = case
    x = ref.mean_operands(case)
    ws, got = run_mean(lib, x, splits)
    partial = ws.read()
    unwritten = partial.view(np.uint32) == 0xFFFFFFFF
    assert not unwritten.any(), f"(n, split, c) {np.argwhere(unwritten)[0].tolist()} of the workspace was not written"
    sums = ref.channel_sums(x)
    assert np.array_equal(partial.astype(np.float64).sum(axis=1), sums), "the partial sums do not add up to the channel sums"
    want = ref.mean_of_sums(sums, hw)
    assert_bits(got, want, "the mean")
    alone = Out((n, c), np.float16)                                 # the second half alone, on the workspace the call left
    assert lib.pp_channel_mean_finish_f16(vp(ws), vp(alone), n, hw, c, splits, stream()) == 0
    assert_bits(alone.read(), want, "pp_channel_mean_finish_f16")


def test_channel_mean_real_operands(lib):
    rng = np.random.default_rng(43)
    n, hw, c, splits = ref.MEAN_CASES[1]
    x = real16(rng, (n, hw, c))
    _, got = run_mean(lib, x, splits)
    want = ref.channel_mean_real(x)
    bound = ref.rounding_bound(want, np.abs(ref.f64(x)).sum(axis=1) / hw, hw + 1)     # hw additions in any order, one product
    report_bound(got, want, bound, "channel_mean")


# ------------------------------------------------------------------------------------------------ pp_channel_scale_f16

def run_scale(lib, x, s, in_place):
    n, hw, c = x.shape
    out = Out(x.shape, np.float16, init=x if in_place else None)
    src, gains = (None if in_place else In(x)), In(s)
    assert lib.pp_channel_scale_f16(vp(out if in_place else src), vp(gains), vp(out), n, hw, c, stream()) == 0
    return out.read()


@pytest.mark.parametrize("in_place", [0, 1])
@pytest.mark.parametrize("recipe", ref.RECIPES)
def test_channel_scale_exact(lib, recipe, in_place):
    for c in ref.SCALE_CHANNELS:
        for n, hw in ((2, 37), (3, 1)) if recipe != "special" else ((1, 7), (2, 37)):
            x, s = ref.scale_operands(recipe, n, hw, c, 51)
            assert_bits(run_scale(lib, x, s, in_place), ref.channel_scale(x, s), f"(n, hw, c) = {(n, hw, c)}")


def test_channel_scale_capped_grid(lib):
    n, hw, c = ref.SCALE_CAPPED
    x, s = ref.scale_operands("small", n, hw, c, 52)
    got = run_scale(lib, x, s, 0)
    assert_bits_chunked(got[0], lambda lo, hi: ref.channel_scale(x[:, lo:hi], s)[0], 1 << 15, "capped grid")


def test_channel_scale_real_operands(lib):
    rng = np.random.default_rng(53)
    x, s = real16(rng, (2, 500, 24)), real16(rng, (2, 24))
    want = ref.channel_scale(x, s)
    report_bound(run_scale(lib, x, s, 0), want, ref.rounding_bound(want, np.abs(want), 1), "channel_scale")


# ------------------------------------------------------------------------------------------------ pp_se_gains_f16

@pytest.mark.parametrize("slope", ref.SE_SLOPES)
@pytest.mark.parametrize("case", ref.SE_CASES, ids=str)
def test_se_gains_exact(lib, case, slope):
    o = ref.se_operands(case, slope)
    n, c, hidden, splits, hw = (o[k] for k in ("n", "c", "hidden", "splits", "hw"))
    want = ref.se_gains(o["mean"], o["w1"], o["b1"], o["w2"], o["b2"], slope)["gain"]
    weights = [In(o[k]) for k in ("w1", "b1", "w2", "b2")]
    partial, mean = In(o["partial"]), In(o["mean"])
    from_sums, from_mean = Out((n, c), np.float16), Out((n, c), np.float16)
    assert lib.pp_se_gains_f16(vp(partial), None, *map(vp, weights), vp(from_sums), n, hw, c, hidden, splits, slope, stream()) == 0
    assert lib.pp_se_gains_f16(None, vp(mean), *map(vp, weights), vp(from_mean), n, 0, c, hidden, 0, slope, stream()) == 0
    assert_bits(from_sums.read(), want, "from the partial sums")
    assert_bits(from_mean.read(), want, "from the mean")


# ------------------------------------------------------------------------------------------------ pp_nhwc64_to_planes_f16

@pytest.mark.parametrize("c_out", ref.PLANES_C_OUT)
@pytest.mark.parametrize("hw", ref.PLANES_HW)
def test_nhwc64_to_planes(lib, hw, c_out):
    n = 2
    rng = np.random.default_rng([61, hw, c_out])
    x = (rng.integers(0, 0x7C00, (n, hw, 64)) | rng.integers(0, 2, (n, hw, 64)) << 15).astype(np.uint16).view(np.float16)   # any finite value
    x[:, :, c_out:] = np.nan                                         # what lies at and behind c_out must not appear
    out, src = Out((n, c_out, hw), np.float16), In(x)
    assert lib.pp_nhwc64_to_planes_f16(vp(src), vp(out), n, hw, c_out, stream()) == 0
    got = out.read()
    assert not np.isnan(got).any()
    assert_bits(got, ref.f64(ref.nhwc64_to_planes(x, c_out)), f"hw = {hw}, c_out = {c_out}")


# ------------------------------------------------------------------------------------------------ the pre-processing

def bytes_with_every_value(rng, shape):
    """random bytes; the first 256 (the start of image 0's first row, or rows) hold every value"""
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    a.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    return a


def check_preprocess(got, slots, sizes, pad_value, flip, what):
    """image by image, so that no float64 copy of the batch is held"""
    ns = 2 if flip else 1
    for b in range(slots.shape[0]):
        want = ref.preprocess(slots[b:b + 1], ([sizes[0][b]], [sizes[1][b]]), pad_value, flip)
        assert_bits(got[b * ns:(b + 1) * ns], want, f"{what}, image {b}")


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("dtype", [PP_F16, PP_F32])
@pytest.mark.parametrize("shape", [dict(batch=2, h=9, w=11, pad_to=4), ref.PREPROCESS_LARGE], ids=["small", "second pass"])
def test_preprocess(lib, shape, dtype, flip):
    batch, h, w, pad_to = (shape[k] for k in ("batch", "h", "w", "pad_to"))
    hp, wp = -(-h // pad_to) * pad_to, -(-w // pad_to) * pad_to
    img = bytes_with_every_value(np.random.default_rng([71, h, w]), (batch, h, w, 3))
    assert np.unique(img).size == 256
    out, src = Out((batch * (2 if flip else 1), hp, wp, 3), NP_OF[dtype]), In(img)
    assert lib.pp_preprocess_u8(vp(src), vp(out), dtype, batch, h, w, pad_to, 128, flip, stream()) == 0
    slots = np.full((batch, hp, wp, 3), 0xFF, np.uint8)
    slots[:, :h, :w] = img
    check_preprocess(out.read(), slots, ([h] * batch, [w] * batch), 128, flip, "pp_preprocess_u8")


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("dtype", [PP_F16, PP_F32])
@pytest.mark.parametrize("shape", [dict(batch=3, hp=8, wp=12, sizes=[(8, 12), (5, 7), (1, 1)]), ref.RAGGED_LARGE], ids=["small", "second pass"])
def test_preprocess_ragged(lib, shape, dtype, flip):
    batch, hp, wp = (shape[k] for k in ("batch", "hp", "wp"))
    hs = [shape["sizes"][b % len(shape["sizes"])][0] for b in range(batch)]
    ws = [shape["sizes"][b % len(shape["sizes"])][1] for b in range(batch)]
    slots = bytes_with_every_value(np.random.default_rng([72, hp, wp]), (batch, hp, wp, 3))
    for b in range(batch):                                           # garbage outside every image's corner: must not be read
        slots[b, hs[b]:] = 0xFF
        slots[b, :, ws[b]:] = 0xFF
    assert np.unique(slots[0, :hs[0], :ws[0]]).size == 256
    out, src, sizes = Out((batch * (2 if flip else 1), hp, wp, 3), NP_OF[dtype]), In(slots), In(np.array([hs, ws], np.int32))
    assert lib.pp_preprocess_u8_ragged(vp(src), vp(sizes), vp(out), dtype, batch, hp, wp, 128, flip, stream()) == 0
    check_preprocess(out.read(), slots, (hs, ws), 128, flip, "pp_preprocess_u8_ragged")


# ------------------------------------------------------------------------------------------------ pp_flip_average

def flip_operands(dtype, samples, h, w):
    """binary16: N(0, 1), an eighth +-50000 .. 65504 (sums of two overflow to infinity), an eighth on the subnormal grid with |k| <= 5
    (sums of two halve to a subnormal, ties included), and both pairs once at fixed places; float32: N(0, 1) and an eighth +-3e38"""
    rng = np.random.default_rng([81, samples, h, w, dtype])
    shape = (samples, ref.NUM_CH, h, w)
    net = rng.standard_normal(shape).astype(NP_OF[dtype])
    kind, sign = rng.random(shape), rng.choice(np.array([-1.0, 1.0]), shape)
    if dtype == PP_F16:
        net = np.where(kind < 1 / 8, sign * rng.integers(50000, 65505, shape), net)
        net = np.where(kind > 7 / 8, rng.integers(-5, 6, shape) * ref.SUB, net).astype(np.float16)
        if samples > 1:
            net[0, 0, 0, 0], net[1, ref.FLIP_CH[0], 0, w - 1] = 60000.0, 60000.0
            net[0, 49, 0, 0], net[1, ref.FLIP_CH[49], 0, w - 1] = 3 * ref.SUB, 2 * ref.SUB
    else:
        net = np.where(kind < 1 / 8, sign * 3e38, net).astype(np.float32)
    return net


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("dtype", [PP_F16, PP_F32])
@pytest.mark.parametrize("shape", ref.FLIP_SHAPES, ids=str)
def test_flip_average(lib, shape, dtype, flip):
    batch, h, w = shape
    net = flip_operands(dtype, batch * (2 if flip else 1), h, w)
    want_heat, want_paf = ref.flip_average(net, flip)
    if flip:
        assert np.isinf(want_paf[0, 0, 0, 0]) or dtype == PP_F32
        assert want_heat[0, 0, 0, 19] == 2 * ref.SUB or dtype == PP_F32
    heat, paf, src = Out((batch, h, w, ref.NUM_HEAT), np.float32), Out((batch, h, w, ref.NUM_LIMB), np.float32), In(net)
    assert lib.pp_flip_average(vp(src), dtype, batch, h, w, flip, vp(heat), vp(paf), stream()) == 0
    assert_bits(heat.read(), want_heat, "heat")
    assert_bits(paf.read(), want_paf, "paf")


# ------------------------------------------------------------------------------------------------ the second pass of the entries that
# already have a float64 reference (tests/test_gpu_rotation.py, tests/test_gpu_cubic.py: no shape there reaches 2,097,152 pixels)

def test_preprocess_affine_second_pass(lib):
    """pp_preprocess_u8_affine on one 1445 x 1447 image padded to 1449 x 1449 (2,099,601 pixels), against the NumPy restatement of
    cv2.warpAffine (tests/rotation_reference.py), bit for bit as tests/test_gpu_rotation.py asks"""
    from posepaf.rotation import as_c_doubles, invert_affine, reference_center, rotation_matrix
    from rotation_reference import warp_affine
    h, w, side = 1445, 1447, 1449
    assert side * side > ref.WORK_ITEMS_FIRST_PASS and side * side % 256
    img = bytes_with_every_value(np.random.default_rng(91), (1, h, w, 3))
    padded = np.full((side, side, 3), 128, np.uint8)
    padded[:h, :w] = img[0]
    m_in = invert_affine(rotation_matrix(reference_center(side, side), 7.5))
    want = warp_affine(np.float32(padded / 255), m_in)
    out, src = Out((2, side, side, 3), np.float32), In(img)
    assert lib.pp_preprocess_u8_affine(vp(src), vp(out), PP_F32, 1, h, w, side, 128, 1, as_c_doubles(m_in), stream()) == 0
    got = out.read()
    assert_bits(got[0], ref.f64(want), "the warped image")
    assert_bits(got[1], ref.f64(want[:, ::-1]), "its mirror")


def test_image_resize_second_pass(lib):
    """k_resize_u8 and k_resize_u8_ragged with 1450 x 1450 destination slots (2,102,500 pixels in the first), within one count of the
    bicubic in real arithmetic (tests/cubic_reference.py), as tests/test_gpu_cubic.py asks"""
    import cubic_reference as cr
    side, scale = 967, 1.5
    dside = round(side * scale)
    assert dside * dside > ref.WORK_ITEMS_FIRST_PASS and dside * dside % 256
    img = np.random.default_rng(92).integers(0, 256, (side, side, 3), dtype=np.uint8)
    out, src = Out((1, dside, dside, 3), np.uint8), In(img)
    assert lib.pp_resize_u8_cubic(vp(src), vp(out), 1, side, side, dside, dside, 1.0 / scale, 1.0 / scale, stream()) == 0
    plain = out.read()
    cr.assert_u8_close(plain[0], img, scale, "k_resize_u8")
    small = np.ascontiguousarray(img[:49, :65])                      # the second slot lies behind 2,097,152 slot pixels
    sh, sw = round(49 * scale), round(65 * scale)
    slots = np.full((2, side, side, 3), 0xA5, np.uint8)
    slots[0] = img
    slots[1, :49, :65] = small
    out, src = Out((2, dside, dside, 3), np.uint8), In(slots)
    src_sizes, dst_sizes = In(np.array([[side, 49], [side, 65]], np.int32)), In(np.array([[dside, sh], [dside, sw]], np.int32))
    assert lib.pp_resize_u8_cubic_ragged(vp(src), vp(out), 2, side, side, dside, dside, vp(src_sizes), vp(dst_sizes), 1.0 / scale, 1.0 / scale,
                                         stream()) == 0
    ragged = out.read()
    assert np.array_equal(ragged[0], plain[0])                       # the same image through the other kernel: the same bytes
    cr.assert_u8_close(ragged[1, :sh, :sw], small, scale, "k_resize_u8_ragged")
    assert (ragged[1, sh:] == FILL).all() and (ragged[1, :, sw:] == FILL).all()
