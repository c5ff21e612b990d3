"""GPU: pp_conv3x3_dgrad_f16 (csrc/posepaf_convgrad.hip) against the float64 restatement of tests/conv_dgrad_reference.py: bit for bit
on the integer cases that tests/test_conv_dgrad_reference_cpu.py proves exact, with and without y; inside the derived rounding bound
on real-valued operands with subnormals; and the header's further promises (nothing of a neighbouring image is read, equal bits from
call to call and from a captured replay, the refusals in their order).
Before every launch the buffers around the operands hold NaN, and dx and a 64-byte guard behind it NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_dgrad_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD16, FRAME = 32, 64            # guard elements (64 bytes) behind dx; NaN elements around an operand
BAD_ARG, TOO_LARGE, UNSUPPORTED = -2, -3, -6
NAN16 = 0x7E00
LEAK = 0.01                        # fused_model.LEAK; the entry receives its float32


@pytest.fixture(scope="module")
def lib():
    from posepaf import _lib
    return _lib.load()


def bits16(a):
    return np.ascontiguousarray(a).view(np.uint16)


def framed(a):
    """a device copy of the binary16 array `a` with FRAME NaN elements in front and behind, 16-byte aligned"""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float16
    buf = torch.full((a.size + 2 * FRAME,), NAN16, dtype=torch.int16, device=DEV)
    view = buf[FRAME:FRAME + a.size].view(torch.float16).view(a.shape)
    view.copy_(torch.from_numpy(a.copy()))
    return buf, view


class Call:
    def __init__(self, lib, dy, w, y, shape):
        self.lib, (self.n, self.h, self.w), self.c_out, self.c_in = lib, shape, w.shape[0], w.shape[3]
        self._dy, self.dy = framed(dy)
        self._wt, self.wt = framed(w)
        self._y, self.y = framed(y) if y is not None else (None, None)
        self.size = self.n * self.h * self.w * self.c_in
        self.dx = torch.empty(self.size + GUARD16, dtype=torch.int16, device=DEV)
        assert all(t.data_ptr() % 16 == 0 for t in (self.dy, self.wt, self.dx))

    def launch(self, slope=ref.SLOPE, **over):
        a = dict(dy=self.dy.data_ptr(), w=self.wt.data_ptr(), y=self.y.data_ptr() if self.y is not None else None, n=self.n, h=self.h,
                 wd=self.w, c_in=self.c_in, c_out=self.c_out, dx=self.dx.data_ptr())
        a.update(over)
        return self.lib.pp_conv3x3_dgrad_f16(C.c_void_p(a["dy"]), C.c_void_p(a["w"]), C.c_void_p(a["y"]), a["n"], a["h"], a["wd"], a["c_in"],
                                             a["c_out"], slope, C.c_void_p(a["dx"]), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def poison(self):
        self.dx.fill_(NAN16)

    def result(self):
        out = self.dx.cpu().numpy().view(np.uint16)
        assert (out[self.size:] == NAN16).all(), "the guard behind dx was written"
        return out[:self.size].view(np.float16).reshape(self.n, self.h, self.w, self.c_in).copy()

    def run(self, slope=ref.SLOPE):
        self.poison()
        assert self.launch(slope) == 0
        return self.result()

    def untouched(self):
        return bool((self.dx == NAN16).all())


def assert_bits(got, want, what):
    bad = bits16(got) != bits16(want)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements differ, first (b, i, j, c) {np.argwhere(bad)[0].tolist()}: "
                           f"{got[bad][0]!r} for {want[bad][0]!r}")


# ------------------------------------------------------------------------------------------------ bit equality on integer operands

@pytest.mark.parametrize("case", ref.EXACT_CASES, ids=ref.case_id)
def test_dgrad_exact(lib, case):
    shape = case[0]
    dy, w, y = ref.int_operands(case)
    assert_bits(Call(lib, dy, w, y, shape).run(), ref.to_half(ref.conv3x3_dgrad(dy, w, y, shape, ref.SLOPE)), "with y")
    no_y = Call(lib, dy, w, None, shape)
    want = ref.to_half(ref.conv3x3_dgrad(dy, w, None, shape, ref.SLOPE))
    assert_bits(no_y.run(), want, "y = NULL")
    assert_bits(no_y.run(slope=float("nan")), want, "y = NULL, the slope is not looked at")
    if shape == (1, 1, 1):                                       # only the centre tap contributes
        centre = dy[0].astype(np.float64) @ w[:, 1, 1, :].astype(np.float64)
        assert_bits(no_y.result()[0, 0, 0], ref.to_half(centre), "the centre tap")


@pytest.mark.parametrize("channels", [(128, 64), (128, 192), (64, 256)], ids=str)
def test_dgrad_exact_at_the_other_channel_counts(lib, channels):
    """c_in = 128 (the one instance the cases above do not reach) and a c_out that is no multiple of 128, at two ragged shapes"""
    for shape in ((2, 3, 5), (1, 5, 29)):
        dy, w, y = ref.int_operands((shape, channels))
        assert_bits(Call(lib, dy, w, y, shape).run(), ref.to_half(ref.conv3x3_dgrad(dy, w, y, shape, ref.SLOPE)), f"{shape}")


# ------------------------------------------------------------------------------------------------ nothing leaks between images

@pytest.mark.parametrize("shape", [(2, 3, 5), (3, 8, 8)], ids=str)
def test_no_leak_between_images(lib, shape):
    n, h, w = shape
    dy, wt, y = ref.int_operands((shape, (64, 64)))
    dy = dy.reshape(n, h * w, 64).copy()
    dy[0] = np.nan
    got = Call(lib, dy.reshape(n * h * w, 64), wt, y, shape).run()
    assert np.isnan(got[0]).all()
    assert np.isfinite(got[1:]).all()
    for b in range(1, n):                                        # bit-equal to the same image run alone
        alone = Call(lib, dy[b], wt, y[b:b + 1], (1, h, w)).run()
        assert_bits(got[b:b + 1], alone, f"image {b}")


# ------------------------------------------------------------------------------------------------ real operands and the promises

@pytest.fixture(scope="module")
def real():
    """random binary16 operands with a tenth of subnormals, the float64 result and the bound: computed once"""
    out = {}
    for shape, (c_in, c_out) in (((2, 9, 11), (256, 256)), ((1, 5, 29), (192, 128))):
        n, h, w = shape
        rng = np.random.default_rng(c_in)
        dy = (rng.standard_normal((n * h * w, c_out)) * 2.0 ** -3).astype(np.float16)
        wt = (rng.standard_normal((c_out, 3, 3, c_in)) * 0.1).astype(np.float16)
        sub = rng.integers(1, 0x400, dy.shape).astype(np.uint16).view(np.float16)                    # subnormals, a tenth of dy and of w
        dy = np.where(rng.random(dy.shape) < 0.1, sub * rng.choice(np.array([-1, 1], np.float16), dy.shape), dy).astype(np.float16)
        subw = rng.integers(1, 0x400, wt.shape).astype(np.uint16).view(np.float16)
        wt = np.where(rng.random(wt.shape) < 0.1, subw, wt).astype(np.float16)
        assert ((np.abs(dy) < 2.0 ** -14) & (dy != 0)).mean() > 0.05 and ((np.abs(wt) < 2.0 ** -14) & (wt != 0)).mean() > 0.05
        y = rng.standard_normal((n, h, w, c_in)).astype(np.float16)
        y[0, 0, 0, :4] = np.array([0x0000, 0x8000, 0x8001, 0x0001], np.uint16).view(np.float16)
        out[(c_in, c_out)] = dict(shape=shape, dy=dy, w=wt, y=y, want=ref.conv3x3_dgrad(dy, wt, y, shape, LEAK),
                                  bound=ref.conv3x3_dgrad_bound(dy, wt, y, shape, LEAK))
    return out


@pytest.mark.parametrize("channels", [(256, 256), (192, 128)], ids=str)
def test_dgrad_rounding_bound(lib, real, channels):
    c = real[channels]
    got = Call(lib, c["dy"], c["w"], c["y"], c["shape"]).run(LEAK).astype(np.float64)
    err = np.abs(got - c["want"])
    print(f"{channels}: largest |dx - ref| / bound = {(err / c['bound']).max():.4f}")
    assert np.isfinite(got).all()
    assert (err <= c["bound"]).all()


def test_dgrad_two_calls_and_a_replay(lib, real):
    c = real[(256, 256)]
    call = Call(lib, c["dy"], c["w"], c["y"], c["shape"])
    first, second = call.run(LEAK), call.run(LEAK)
    assert np.array_equal(bits16(first), bits16(second))
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    call.poison()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            assert call.launch(LEAK) == 0
    call.poison()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits16(first), bits16(call.result()))


def test_dgrad_refusals_in_order(lib):
    shape = (2, 3, 5)
    dy, w, y = ref.int_operands((shape, (64, 64)))
    call = Call(lib, dy, w, y, shape)
    call.poison()
    nan = float("nan")
    p = lambda t, off: t.data_ptr() + off
    steps = [  # each entry breaks one rule and, where it can, also every LATER one: the earlier refusal must win
        (dict(dy=None, n=0, c_in=65), BAD_ARG), (dict(w=None, n=0), BAD_ARG), (dict(dx=None, n=0), BAD_ARG),
        (dict(n=0, dy=p(call.dy, 2), c_in=65), BAD_ARG), (dict(h=-1, dy=p(call.dy, 2)), BAD_ARG), (dict(wd=0, dy=p(call.dy, 2)), BAD_ARG),
        (dict(dy=p(call.dy, 8), slope=nan, c_in=65), BAD_ARG), (dict(w=p(call.wt, 2), slope=nan), BAD_ARG), (dict(y=p(call.y, 4), slope=nan), BAD_ARG),
        (dict(dx=p(call.dx, 8), slope=nan), BAD_ARG),
        (dict(slope=nan, c_in=65), BAD_ARG), (dict(slope=float("inf"), c_in=65), BAD_ARG), (dict(slope=0.0, c_in=65), BAD_ARG),
        (dict(slope=-0.01, c_in=65), BAD_ARG),
        (dict(c_in=65, n=2 ** 16, h=2 ** 15, wd=1), UNSUPPORTED), (dict(c_in=320), UNSUPPORTED), (dict(c_out=32), UNSUPPORTED),
        (dict(c_out=320), UNSUPPORTED), (dict(c_out=96), UNSUPPORTED), (dict(c_in=0), UNSUPPORTED),
        (dict(n=2 ** 16, h=2 ** 15, wd=1), TOO_LARGE), (dict(n=2 ** 30, h=2 ** 30, wd=2 ** 30), TOO_LARGE),
    ]
    for over, want in steps:
        assert call.launch(over.pop("slope", ref.SLOPE), **over) == want, over
    assert all(lib.pp_conv3x3_dgrad_supported(ci, co) == 1 for ci in (64, 128, 192, 256) for co in (64, 128, 192, 256))
    torch.cuda.synchronize()
    assert call.untouched()
