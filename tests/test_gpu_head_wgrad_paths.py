"""GPU: every code path of pp_head_wgrad_f16 (csrc/posepaf_headgrad.hip) that tests/test_gpu_head_wgrad.py does not launch --
c_in = 192, odd and small c_out, the element-load path with padding in the row, gains with more chunks than workgroups, operands
whose bfloat16 split has non-zero low parts -- bit for bit against the float64 restatement (tests/head_wgrad_reference.py) on the
cases of tests/head_wgrad_cases.py, which tests/test_head_wgrad_cases_cpu.py proves exact and classifies on the CPU.  Then the
header's promises: the same bits at every pointer alignment and row pitch the entry accepts, the derived rounding bound on every
instantiation, and non-finite inputs that stay non-finite and stay in their own row or column.
Before every launch the whole buffer around g holds NaN (its padding channels, the half of a straddled pair, the bytes in front of
a shifted base), the workspace 0xFF bytes, and the outputs and a 64-byte guard behind each NaN.
What no test of results can see: whether the kernel zeroes the channels of g at or behind c_out before
the MFMA or lets them in -- they are rows >= c_out of the A operand, which reach only accumulator rows that are never stored.
"""
import time

import numpy as np
import pytest
import torch

import head_wgrad_cases as hc
import head_wgrad_reference as ref
from test_gpu_head_wgrad import DEV, GUARD, Call, bits

pytestmark = pytest.mark.gpu

P, G = hc.P_DEFAULT, hc.G_DEFAULT
CASES = hc.exact_cases(P, G)
C_OUT = 50
T0 = time.perf_counter()


@pytest.fixture(scope="module")
def lib():
    from posepaf import _lib
    lib = _lib.load()
    assert lib.pp_head_wgrad_chunk_pixels() == P and lib.pp_head_wgrad_max_workgroups() == G, "the cases were built for other constants"
    yield lib
    torch.cuda.synchronize()
    print(f"\ntest_gpu_head_wgrad_paths.py: {time.perf_counter() - T0:.1f} s from import to the last test")


def _place(a, byte_offset, fill):
    """a device copy of `a` that starts byte_offset bytes into a buffer filled with `fill` (a binary16 bit pattern)"""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float16 and byte_offset % 2 == 0
    buf = torch.full((a.size + byte_offset // 2,), fill, dtype=torch.int16, device=DEV)
    view = buf[byte_offset // 2:].view(torch.float16).view(a.shape)
    view.copy_(torch.tensor(a))             # a copy: the cases' arrays are shared and read-only
    assert view.data_ptr() == buf.data_ptr() + byte_offset and buf.data_ptr() % 128 == 0
    return buf, view


NAN16 = 0x7E00


class PlacedCall(Call):
    """Call with g, x and scale at chosen byte offsets from a 128-byte boundary; the buffers end with the operands' last element"""

    def __init__(self, lib, g, x, scale, hw, c_out, g_off=0, x_off=0, s_off=0):
        self.lib, self.m, self.ldg, self.c_in, self.c_out, self.hw = lib, g.shape[0], g.shape[1], x.shape[1], c_out, hw
        self._g_buf, self.g = _place(g, g_off, NAN16)
        self._x_buf, self.x = _place(x, x_off, NAN16)
        self._s_buf, self.scale = (None, None) if scale is None else _place(scale, s_off, NAN16)
        self.ws_bytes = int(lib.pp_head_wgrad_workspace_bytes(self.m, self.c_in, c_out))
        assert self.ws_bytes > 0
        self.ws = torch.empty(self.ws_bytes + 16, dtype=torch.uint8, device=DEV)
        self.dw = torch.empty(c_out * self.c_in + GUARD, dtype=torch.float32, device=DEV)
        self.db = torch.empty(c_out + GUARD, dtype=torch.float32, device=DEV)


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ every exact case, bit for bit

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_exact(lib, case):
    g, x, scale = case.operands()
    want_dw, want_db = hc.expected(case)
    call = PlacedCall(lib, g, x, scale, case.hw, case.c_out, g_off=case.g_byte_offset)
    assert (call.g.data_ptr() % 16 == 0 and case.ldg % 8 == 0) == (case.paths(P, G)["load"] == "vector")
    dw, db = call.run()                     # asserts the guards
    bad_w, bad_b = bits(dw) != bits(want_dw.astype(np.float32)), bits(db) != bits(want_db.astype(np.float32))
    where = np.argwhere(bad_w)
    assert not bad_w.any(), (f"dw differs in {int(bad_w.sum())} of {bad_w.size} elements, first (row, column) {where[0].tolist()}: "
                             f"{dw[tuple(where[0])]!r} for {want_dw[tuple(where[0])]!r}; rows {np.unique(where[:, 0]).tolist()[:8]}, "
                             f"columns {np.unique(where[:, 1]).tolist()[:8]}; {case.paths(P, G)}")
    assert not bad_b.any(), f"db differs at {np.flatnonzero(bad_b).tolist()[:8]}: {db[bad_b][:4]} for {want_db[bad_b][:4]}"


# ------------------------------------------------------------------------------------------------ alignment invariance

@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("c_in", hc.C_INS)
def test_same_bits_at_every_alignment_and_pitch(lib, c_in, scaled):
    """the header: bit-equal at every pointer alignment the entry accepts.  The base call has g on a 16-byte boundary with
    ldg = 64 (16-byte loads); the same values from a base 2 bytes further (element loads), in rows of 50, 51 and 72 elements, and
    with x and the gains 16, 48 and 80 bytes off a 128-byte line must give its bits."""
    c = hc.real_case(c_in, scaled, P)
    base = PlacedCall(lib, c["g"], c["x"], c["scale"], c["hw"], C_OUT).run()
    assert np.isfinite(base[0]).all() and np.isfinite(base[1]).all()
    layouts = [("g + 2 bytes, ldg 64", 64, dict(g_off=2)), ("ldg 50", 50, {}), ("ldg 51", 51, {}), ("ldg 72", 72, {}),
               ("ldg 51, g + 6 bytes", 51, dict(g_off=6)), ("ldg 72, g + 16 bytes", 72, dict(g_off=16)),
               ("x + 16, scale + 48 bytes", 64, dict(x_off=16, s_off=48)), ("x + 80, scale + 16 bytes, g + 2", 64, dict(x_off=80, s_off=16, g_off=2)),
               ("x + 48 bytes, ldg 50", 50, dict(x_off=48, s_off=80))]
    for name, ldg, off in layouts:
        call = PlacedCall(lib, hc.relayout(c["g"], C_OUT, ldg), c["x"], c["scale"], c["hw"], C_OUT, **off)
        assert call.x.data_ptr() % 16 == 0 and (off.get("x_off", 0) == 0 or call.x.data_ptr() % 128 != 0)
        got = call.run()
        assert _same(got[0], base[0]) and _same(got[1], base[1]), f"{name}: |dw - base| max {np.abs(got[0] - base[0]).max()}"


# ------------------------------------------------------------------------------------------------ the bound on every instantiation

@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("c_in", [64, 128, 192])
def test_rounding_bound_on_every_instantiation(lib, c_in, scaled):
    c = hc.real_case(c_in, scaled, P)
    dw, db = PlacedCall(lib, c["g"], c["x"], c["scale"], c["hw"], C_OUT).run()
    bw, bb = ref.rounding_bound(c["m"], c["absprod"][0]), ref.rounding_bound(c["m"], c["absprod"][1])
    ew, eb = np.abs(dw.astype(np.float64) - c["want"][0]), np.abs(db.astype(np.float64) - c["want"][1])
    print(f"c_in {c_in}, m = {c['m']}, {'gains' if scaled else 'no gains'}: largest |dw - ref| / bound = {(ew / bw).max():.4f}, "
          f"|db - ref| / bound = {(eb / bb).max():.4f}")
    assert np.isfinite(dw).all() and np.isfinite(db).all()
    assert (ew <= bw).all() and (eb <= bb).all()


# ------------------------------------------------------------------------------------------------ non-finite inputs

M0, K0, C0 = P + 5, C_OUT - 1, 37           # a pixel of the second chunk, the last real channel of g, a column of the second tile


def _nonfinite_reference(g, x, scale, hw):
    with np.errstate(invalid="ignore", over="ignore"):
        dw, db = ref.head_wgrad(g, x, C_OUT, scale, hw)
    return ~np.isfinite(dw), ~np.isfinite(db)


def _perturbed(c, what):
    g, x, scale = c["g"].copy(), c["x"].copy(), c["scale"].copy()
    if what == "g inf":
        g[M0, K0] = np.inf
    elif what == "g nan":
        g[M0, K0] = np.nan
    elif what == "x inf":
        x[M0, C0] = np.inf
    else:                                   # the gain makes the infinity: 60000 * 1.5 is above the largest binary16 number
        x[M0, C0], scale[M0 // c["hw"], C0] = 60000.0, 1.5
        xs = ref.scaled_input(x, scale, c["hw"])
        assert np.isposinf(xs[M0, C0]) and np.isfinite(np.delete(xs.ravel(), M0 * x.shape[1] + C0)).all()
    return g, x, scale


@pytest.mark.parametrize("g_off", [0, 2], ids=["vector", "element"])
@pytest.mark.parametrize("c_in", [192, 256])
def test_non_finite_inputs_stay_in_their_row_or_column(lib, c_in, g_off):
    """the header's rule: an element of dw / db is non-finite exactly where the float64 restatement's is (which of inf or NaN is
    unspecified), and every other element has the bits of the call without the non-finite input"""
    c = hc.real_case(c_in, True, P)
    base = PlacedCall(lib, c["g"], c["x"], c["scale"], c["hw"], C_OUT, g_off=g_off).run()
    assert np.isfinite(base[0]).all() and np.isfinite(base[1]).all()
    got = {}
    for what in ("g inf", "g nan", "x inf", "x * gain overflows"):
        g, x, scale = _perturbed(c, what)
        want_w, want_b = _nonfinite_reference(g, x, scale, c["hw"])
        dw, db = got[what] = PlacedCall(lib, g, x, scale, c["hw"], C_OUT, g_off=g_off).run()
        bad_w, bad_b = ~np.isfinite(dw), ~np.isfinite(db)
        assert np.array_equal(bad_w, want_w) and np.array_equal(bad_b, want_b), what
        row, col = np.zeros_like(bad_w), np.zeros_like(bad_w)
        row[K0], col[:, C0] = True, True
        if what.startswith("g"):
            assert np.array_equal(bad_w, row) and np.array_equal(np.flatnonzero(bad_b), [K0]), what
        else:
            assert np.array_equal(bad_w, col) and not bad_b.any(), what
        assert _same(dw[~bad_w], base[0][~bad_w]) and _same(db[~bad_b], base[1][~bad_b]), what
    a, b = got["x inf"], got["x * gain overflows"]
    keep = np.isfinite(a[0])
    assert np.array_equal(keep, np.isfinite(b[0])) and _same(a[0][keep], b[0][keep]) and _same(a[1], b[1])
