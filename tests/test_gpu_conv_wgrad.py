"""GPU: pp_conv3x3_wgrad_f16 and pp_head_dgrad_f16 (csrc/posepaf_convgrad.hip) against the float64 restatements of
tests/conv_wgrad_reference.py: bit for bit on the integer cases that tests/test_conv_wgrad_reference_cpu.py proves exact, inside the
derived rounding bounds on real-valued operands with subnormals, and the header's further promises (equal bits from call to call
and from a captured replay, the device factor, a NaN that stays in its row, the refusals in their order).
Before every launch the buffers around the operands hold NaN, the workspace 0xFF bytes, and the outputs and a 64-byte guard behind
each NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_wgrad_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD32, GUARD16, FRAME = 16, 32, 64            # guard elements behind a float32 / binary16 output; NaN elements around an operand
BAD_ARG, TOO_LARGE, UNSUPPORTED = -2, -3, -6
NAN16 = 0x7E00


@pytest.fixture(scope="module")
def lib():
    from posepaf import _lib
    return _lib.load()


def bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bits16(a):
    return np.ascontiguousarray(a).view(np.uint16)


def framed(a, extra=0):
    """a device copy of the binary16 array `a` with FRAME NaN elements in front and behind (+ extra bytes of shift), 16-byte aligned"""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float16
    buf = torch.full((a.size + 2 * FRAME,), NAN16, dtype=torch.int16, device=DEV)
    view = buf[FRAME + extra // 2:FRAME + extra // 2 + a.size].view(torch.float16).view(a.shape)
    view.copy_(torch.from_numpy(a.copy()))
    return buf, view


class ConvCall:
    def __init__(self, lib, dy, x):
        self.lib = lib
        (self.n, self.h, self.w, self.c_in), self.c_out = x.shape, dy.shape[1]
        self._dy, self.dy = framed(dy)
        self._x, self.x = framed(x)
        assert self.dy.data_ptr() % 16 == 0 and self.x.data_ptr() % 16 == 0
        self.ws_bytes = int(lib.pp_conv3x3_wgrad_workspace_bytes(self.n, self.h, self.w, self.c_in, self.c_out))
        assert self.ws_bytes > 0
        self.ws = torch.empty(self.ws_bytes + 16, dtype=torch.uint8, device=DEV)
        self.n_dw = self.c_out * 9 * self.c_in
        self.dw = torch.empty(self.n_dw + GUARD32, dtype=torch.float32, device=DEV)
        self.db = torch.empty(self.c_out + GUARD32, dtype=torch.float32, device=DEV)

    def poison(self):
        self.ws.fill_(0xFF), self.dw.fill_(float("nan")), self.db.fill_(float("nan"))

    def launch(self, inv=1.0, inv_dev=None, **over):
        a = dict(dy=self.dy.data_ptr(), x=self.x.data_ptr(), n=self.n, h=self.h, w=self.w, c_in=self.c_in, c_out=self.c_out, inv=inv,
                 inv_dev=inv_dev, ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes, dw=self.dw.data_ptr(), db=self.db.data_ptr())
        a.update(over)
        return self.lib.pp_conv3x3_wgrad_f16(C.c_void_p(a["dy"]), C.c_void_p(a["x"]), a["n"], a["h"], a["w"], a["c_in"], a["c_out"], a["inv"],
                                             C.c_void_p(a["inv_dev"]), C.c_void_p(a["ws"]), a["ws_bytes"], C.c_void_p(a["dw"]),
                                             C.c_void_p(a["db"]), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def results(self):
        dw, db = self.dw.cpu().numpy(), self.db.cpu().numpy()
        nan = bits32(np.full(GUARD32, np.nan, np.float32))
        assert np.array_equal(bits32(dw[self.n_dw:]), nan) and np.array_equal(bits32(db[self.c_out:]), nan), "a guard behind dw / db was written"
        return dw[:self.n_dw].reshape(self.c_out, 3, 3, self.c_in).copy(), db[:self.c_out].copy()

    def run(self, **kw):
        self.poison()
        assert self.launch(**kw) == 0
        return self.results()

    def untouched(self):
        return bool(torch.isnan(self.dw).all()) and bool(torch.isnan(self.db).all())


# ------------------------------------------------------------------------------------------------ bit equality on integer operands

@pytest.mark.parametrize("case", ref.EXACT_CASES, ids=ref.case_id)
def test_wgrad_exact(lib, case):
    dy, x = ref.int_operands(case)
    want_dw, want_db = ref.conv3x3_wgrad(dy, x)
    dw, db = ConvCall(lib, dy, x).run()
    bad = bits32(dw) != bits32(want_dw.astype(np.float32))
    where = np.argwhere(bad)
    assert not bad.any(), (f"dw differs in {int(bad.sum())} of {bad.size} elements, first (k, r, s, c) {where[0].tolist()}: "
                           f"{dw[tuple(where[0])]!r} for {want_dw[tuple(where[0])]!r}; taps {np.unique(where[:, 1] * 3 + where[:, 2]).tolist()}")
    assert np.array_equal(bits32(db), bits32(want_db.astype(np.float32))), f"db: {np.abs(db - want_db).max()}"
    if case[0] == (1, 1, 1):
        off = np.ones((3, 3), bool)
        off[1, 1] = False
        assert not bits32(dw[:, off, :]).any()               # +0.0, bit for bit


# ------------------------------------------------------------------------------------------------ real operands and the promises

@pytest.fixture(scope="module")
def real():
    """random binary16 operands with subnormals, the float64 result, the bounds, and the device's result: computed once"""
    out = {}
    for shape, (c_in, c_out) in (((2, 9, 11), (256, 256)), ((1, 5, 29), (128, 192))):
        n, h, w = shape
        rng = np.random.default_rng(c_in)
        dy = (rng.standard_normal((n * h * w, c_out)) * 2.0 ** -3).astype(np.float16)
        x = rng.standard_normal((n, h, w, c_in)).astype(np.float16)
        sub = rng.integers(1, 0x400, (n * h * w, c_out)).astype(np.uint16).view(np.float16)          # subnormals, a tenth of dy and of x
        dy = np.where(rng.random(dy.shape) < 0.1, sub * np.float16(1) * rng.choice(np.array([-1, 1], np.float16), dy.shape), dy)
        subx = rng.integers(1, 0x400, x.shape).astype(np.uint16).view(np.float16)
        x = np.where(rng.random(x.shape) < 0.1, subx, x).astype(np.float16)
        dy = dy.astype(np.float16)
        assert ((np.abs(dy) < 2.0 ** -14) & (dy != 0)).mean() > 0.05 and ((np.abs(x) < 2.0 ** -14) & (x != 0)).mean() > 0.05
        out[(c_in, c_out)] = dict(dy=dy, x=x, inv=2.0 ** -7, want=ref.conv3x3_wgrad(dy, x, 2.0 ** -7), bound=ref.conv3x3_bounds(dy, x, 2.0 ** -7))
    return out


@pytest.mark.parametrize("channels", [(256, 256), (128, 192)], ids=str)
def test_wgrad_rounding_bound(lib, real, channels):
    c = real[channels]
    dw, db = ConvCall(lib, c["dy"], c["x"]).run(inv=c["inv"])
    ew, eb = np.abs(dw.astype(np.float64) - c["want"][0]), np.abs(db.astype(np.float64) - c["want"][1])
    print(f"{channels}: largest |dw - ref| / bound = {(ew / c['bound'][0]).max():.4f}, |db - ref| / bound = {(eb / c['bound'][1]).max():.4f}")
    assert np.isfinite(dw).all() and np.isfinite(db).all()
    assert (ew <= c["bound"][0]).all() and (eb <= c["bound"][1]).all()


def test_wgrad_two_calls_replay_and_device_factor(lib, real):
    c = real[(256, 256)]
    call = ConvCall(lib, c["dy"], c["x"])
    first = call.run(inv=c["inv"])
    second = call.run(inv=c["inv"])
    assert np.array_equal(bits32(first[0]), bits32(second[0])) and np.array_equal(bits32(first[1]), bits32(second[1]))
    inv_dev = torch.tensor([c["inv"]], dtype=torch.float32, device=DEV)
    on_dev = call.run(inv=float("nan"), inv_dev=inv_dev.data_ptr())         # the host value is ignored
    assert np.array_equal(bits32(first[0]), bits32(on_dev[0])) and np.array_equal(bits32(first[1]), bits32(on_dev[1]))
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    call.poison()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            assert call.launch(inv=1.0, inv_dev=inv_dev.data_ptr()) == 0
    call.poison()
    graph.replay()
    torch.cuda.synchronize()
    replayed = call.results()
    assert np.array_equal(bits32(first[0]), bits32(replayed[0])) and np.array_equal(bits32(first[1]), bits32(replayed[1]))
    inv_dev.fill_(2.0 * c["inv"])                                             # the replay reads the factor when it runs
    call.poison()
    graph.replay()
    torch.cuda.synchronize()
    doubled = call.results()
    assert np.array_equal(bits32(2.0 * first[0]), bits32(doubled[0])) and np.array_equal(bits32(2.0 * first[1]), bits32(doubled[1]))


def test_wgrad_nan_stays_in_its_row(lib, real):
    c = real[(256, 256)]
    base = ConvCall(lib, c["dy"], c["x"]).run(inv=c["inv"])
    dy = c["dy"].copy()
    k0, pixel = 97, 1 * 9 * 11 + 4 * 11 + 5                  # an interior pixel of the second image: all nine taps see it
    dy[pixel, k0] = np.nan
    dw, db = ConvCall(lib, dy, c["x"]).run(inv=c["inv"])
    assert not np.isfinite(dw[k0]).any() and not np.isfinite(db[k0])
    keep = np.arange(256) != k0
    assert np.array_equal(bits32(dw[keep]), bits32(base[0][keep])) and np.array_equal(bits32(db[keep]), bits32(base[1][keep]))


def test_wgrad_refusals_in_order(lib):
    dy, x = ref.int_operands(((2, 3, 5), (64, 64)))
    call = ConvCall(lib, dy, x)
    call.poison()
    nan, inf = float("nan"), float("inf")
    ok = torch.zeros(1, dtype=torch.float32, device=DEV).data_ptr()
    steps = [  # each entry breaks one rule and, where it can, also every LATER one: the earlier refusal must win
        (dict(dy=None, n=0, c_in=65), BAD_ARG), (dict(x=None, n=0), BAD_ARG), (dict(dw=None, n=0), BAD_ARG), (dict(db=None, n=0), BAD_ARG),
        (dict(ws=None, n=0), BAD_ARG),
        (dict(n=0, dy=call.dy.data_ptr() + 2, c_in=65), BAD_ARG), (dict(h=-1, c_in=65), BAD_ARG), (dict(w=0, c_in=65), BAD_ARG),
        (dict(dy=call.dy.data_ptr() + 8, inv=nan, c_in=65), BAD_ARG), (dict(x=call.x.data_ptr() + 2, c_in=65), BAD_ARG),
        (dict(dw=call.dw.data_ptr() + 2, c_in=65), BAD_ARG), (dict(db=call.db.data_ptr() + 1, c_in=65), BAD_ARG),
        (dict(ws=call.ws.data_ptr() + 2, c_in=65), BAD_ARG), (dict(inv_dev=ok + 2, c_in=65), BAD_ARG),
        (dict(inv=nan, c_in=65), BAD_ARG), (dict(inv=inf, c_in=65), BAD_ARG), (dict(inv=0.0, c_in=65), BAD_ARG), (dict(inv=-1.0, c_in=65), BAD_ARG),
        (dict(c_in=65, n=2 ** 16, h=2 ** 15, w=1), UNSUPPORTED), (dict(c_in=320), UNSUPPORTED), (dict(c_out=32), UNSUPPORTED),
        (dict(c_out=320), UNSUPPORTED), (dict(c_out=96), UNSUPPORTED), (dict(c_in=0), UNSUPPORTED),
        (dict(n=2 ** 16, h=2 ** 15, w=1, ws_bytes=0), TOO_LARGE), (dict(n=2 ** 30, h=2 ** 30, w=2 ** 30), TOO_LARGE),
        (dict(ws_bytes=call.ws_bytes - 1), BAD_ARG), (dict(ws_bytes=0), BAD_ARG),
    ]
    for over, want in steps:
        assert call.launch(**over) == want, over
    assert lib.pp_conv3x3_wgrad_workspace_bytes(0, 3, 5, 64, 64) == BAD_ARG
    assert lib.pp_conv3x3_wgrad_workspace_bytes(2, 3, 5, 64, 50) == UNSUPPORTED
    assert lib.pp_conv3x3_wgrad_workspace_bytes(2 ** 16, 2 ** 15, 1, 64, 64) == TOO_LARGE
    assert all(lib.pp_conv3x3_wgrad_supported(ci, co) == 1 for ci in (64, 128, 192, 256) for co in (64, 128, 192, 256))
    torch.cuda.synchronize()
    assert call.untouched()
    assert call.launch(inv=nan, inv_dev=ok) == 0                    # a device factor: the host value is not looked at
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ pp_head_dgrad_f16

class DgradCall:
    def __init__(self, lib, g, w, y, c_out, g_extra=0):
        self.lib, self.m, self.ldg, self.c_in, self.c_out = lib, g.shape[0], g.shape[1], y.shape[1], c_out
        self._g, self.g = framed(g, g_extra)
        self._w, self.wt = framed(w)
        self._y, self.y = framed(y)
        self.n = self.m * self.c_in
        self.dx = torch.empty(self.n + GUARD16, dtype=torch.int16, device=DEV)

    def launch(self, slope, **over):
        a = dict(g=self.g.data_ptr(), ldg=self.ldg, w=self.wt.data_ptr(), y=self.y.data_ptr(), m=self.m, c_in=self.c_in, c_out=self.c_out,
                 slope=slope, dx=self.dx.data_ptr())
        a.update(over)
        return self.lib.pp_head_dgrad_f16(C.c_void_p(a["g"]), a["ldg"], C.c_void_p(a["w"]), C.c_void_p(a["y"]), a["m"], a["c_in"], a["c_out"],
                                          a["slope"], C.c_void_p(a["dx"]), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def run(self, slope):
        self.dx.fill_(NAN16)
        assert self.launch(slope) == 0
        out = self.dx.cpu().numpy().view(np.uint16)
        assert (out[self.n:] == NAN16).all(), "the guard behind dx was written"
        return out[:self.n].view(np.float16).reshape(self.m, self.c_in).copy()

    def untouched(self):
        return bool((self.dx == NAN16).all())


@pytest.mark.parametrize("c_in", [64, 128, 192, 256])
def test_dgrad_exact(lib, c_in):
    for m in ref.DGRAD_MS:
        for c_out in ref.DGRAD_C_OUTS:
            for ldg in ref.DGRAD_LDGS:
                if ldg < c_out or (c_in != 128 and (m, c_out, ldg) not in ((145, 50, 64), (63, 64, 64), (1, 1, 50))):
                    continue                                    # the whole grid at one c_in, three corners at the others
                for extra in (0, 2):                            # g on a 16-byte boundary and 2 bytes off it
                    g, w, y = ref.dgrad_int_operands(m, c_in, c_out, ldg)
                    want = ref.to_half(ref.head_dgrad(g, w, y, c_out, ref.DGRAD_SLOPE))
                    got = DgradCall(lib, g, w, y, c_out, extra).run(ref.DGRAD_SLOPE)
                    bad = bits16(got) != bits16(want)
                    assert not bad.any(), (f"m {m}, c_out {c_out}, ldg {ldg}, g + {extra}: {int(bad.sum())} elements differ, first "
                                           f"{np.argwhere(bad)[0].tolist()}: {got[bad][0]!r} for {want[bad][0]!r}")


@pytest.mark.parametrize("c_in,c_out,ldg", [(256, 50, 64), (192, 64, 64), (64, 50, 50)])
def test_dgrad_rounding_bound(lib, c_in, c_out, ldg):
    LEAK = 0.01                                                 # fused_model.LEAK; the entry receives its float32
    m = 64 * 3 + 17
    rng = np.random.default_rng(c_in + c_out)
    g = np.full((m, ldg), np.nan, np.float16)                   # the padding channels hold NaN
    g[:, :c_out] = (rng.standard_normal((m, c_out)) * 2.0 ** -3).astype(np.float16)
    g[::7, :c_out:3] = np.array([0x0203], np.uint16).view(np.float16)[0]        # subnormals
    w = (rng.standard_normal((c_out, c_in)) * 0.1).astype(np.float16)
    w[::5, ::9] = np.array([0x8155], np.uint16).view(np.float16)[0]
    y = rng.standard_normal((m, c_in)).astype(np.float16)
    y[0, :4] = np.array([0x0000, 0x8000, 0x8001, 0x0001], np.uint16).view(np.float16)
    got = DgradCall(lib, g, w, y, c_out).run(LEAK).astype(np.float64)
    t, bound = ref.head_dgrad(g, w, y, c_out, LEAK), ref.head_dgrad_bound(g, w, y, c_out, LEAK)
    err = np.abs(got - t)
    print(f"c_in {c_in}, c_out {c_out}: largest |dx - ref| / bound = {(err / bound).max():.4f}")
    assert np.isfinite(got).all() and (err <= bound).all()


def test_dgrad_refusals_in_order(lib):
    g, w, y = ref.dgrad_int_operands(63, 64, 50, 64)
    call = DgradCall(lib, g, w, y, 50)
    call.dx.fill_(NAN16)
    nan = float("nan")
    steps = [
        (dict(g=None, m=0), BAD_ARG), (dict(w=None, m=0), BAD_ARG), (dict(y=None, m=0), BAD_ARG), (dict(dx=None, m=0), BAD_ARG),
        (dict(m=0, ldg=1), BAD_ARG), (dict(m=-5, ldg=1), BAD_ARG),
        (dict(ldg=49, g=call.g.data_ptr() + 1), BAD_ARG),
        (dict(g=call.g.data_ptr() + 1, slope=nan), BAD_ARG), (dict(w=call.wt.data_ptr() + 2, slope=nan), BAD_ARG),
        (dict(y=call.y.data_ptr() + 8, slope=nan), BAD_ARG), (dict(dx=call.dx.data_ptr() + 4, slope=nan), BAD_ARG),
        (dict(slope=nan, c_in=65), BAD_ARG), (dict(slope=float("inf"), c_in=65), BAD_ARG), (dict(slope=0.0, c_in=65), BAD_ARG),
        (dict(slope=-0.01, c_in=65), BAD_ARG),
        (dict(c_in=65, m=2 ** 31), UNSUPPORTED), (dict(c_in=320), UNSUPPORTED), (dict(c_in=0), UNSUPPORTED), (dict(c_out=0), UNSUPPORTED),
        (dict(c_out=65, ldg=65), UNSUPPORTED),
        (dict(m=2 ** 31), TOO_LARGE),
    ]
    for over, want in steps:
        assert call.launch(over.pop("slope", 0.01), **over) == want, over
    assert all(lib.pp_head_dgrad_supported(ci, co) == 1 for ci in (64, 128, 192, 256) for co in (1, 50, 64))
    torch.cuda.synchronize()
    assert call.untouched()
