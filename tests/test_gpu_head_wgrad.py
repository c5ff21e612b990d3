"""GPU: pp_head_wgrad_f16, the weight and bias gradient of a 1 x 1 head, against the float64 restatement tests/head_wgrad_reference.py.

Exact cases: g and x are small integers and the gains are in {0.5, 1, 1.5, 3}, so every xs is a multiple of 1/2 and
sum_m |g| |xs| < 2^23 per element: every float32 partial sum is exact in ANY order, and dw / db must be BIT-equal to the restatement
(compared as unsigned integers).  Rounding cases: real-valued inputs against the derived bound  m * 2^-23 * (|g|^T |xs|)
(head_wgrad_reference.rounding_bound); the largest observed ratio is printed, not asserted on beyond the bound.
Before every call the padding channels of g hold NaN, the workspace 0xFF bytes, and the outputs and a 64-byte guard behind each NaN.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import head_wgrad_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 16            # float32 elements: 64 bytes
BAD_ARG, TOO_LARGE, UNSUPPORTED = -2, -3, -6


@pytest.fixture(scope="module")
def lib():
    from posepaf import _lib
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_ints(rng, m, c_in, c_out, ldg, n_img=None, g_max=3, x_max=15, gains=(0.5, 1.0, 1.5, 3.0)):
    g = np.full((m, ldg), np.nan, np.float16)
    g[:, :c_out] = rng.integers(-g_max, g_max + 1, (m, c_out)).astype(np.float16)
    x = rng.integers(-x_max, x_max + 1, (m, c_in)).astype(np.float16)
    scale = None if n_img is None else rng.choice(np.asarray(gains, np.float16), (n_img, c_in))
    return g, x, scale


def make_reals(rng, m, c_in, c_out, ldg, n_img=None):
    g = np.full((m, ldg), np.nan, np.float16)
    g[:, :c_out] = (rng.standard_normal((m, c_out)) * 2.0 ** -3).astype(np.float16)
    x = rng.standard_normal((m, c_in)).astype(np.float16)
    scale = None if n_img is None else rng.uniform(0.5, 1.5, (n_img, c_in)).astype(np.float16)
    return g, x, scale


class Call:
    """device buffers of one shape: inputs, a workspace with 4 spare bytes in front, outputs with guards"""

    def __init__(self, lib, g, x, scale, hw, c_out):
        self.lib, self.m, self.ldg, self.c_in, self.c_out, self.hw = lib, g.shape[0], g.shape[1], x.shape[1], c_out, hw
        self.g, self.x = torch.from_numpy(g).to(DEV), torch.from_numpy(x).to(DEV)
        self.scale = None if scale is None else torch.from_numpy(scale).to(DEV)
        self.ws_bytes = int(lib.pp_head_wgrad_workspace_bytes(self.m, self.c_in, c_out))
        assert self.ws_bytes > 0
        self.ws = torch.empty(self.ws_bytes + 16, dtype=torch.uint8, device=DEV)
        self.dw = torch.empty(c_out * self.c_in + GUARD, dtype=torch.float32, device=DEV)
        self.db = torch.empty(c_out + GUARD, dtype=torch.float32, device=DEV)

    def poison(self):
        self.ws.fill_(0xFF)
        self.dw.fill_(float("nan"))
        self.db.fill_(float("nan"))

    def launch(self, inv=1.0, ws_offset=0, stream=None, **over):
        a = dict(g=self.g.data_ptr(), ldg=self.ldg, x=self.x.data_ptr(), scale=None if self.scale is None else self.scale.data_ptr(),
                 m=self.m, hw=self.hw, c_in=self.c_in, c_out=self.c_out, inv=inv, ws=self.ws.data_ptr() + ws_offset, ws_bytes=self.ws_bytes,
                 dw=self.dw.data_ptr(), db=self.db.data_ptr())
        a.update(over)
        st = torch.cuda.current_stream() if stream is None else stream
        return self.lib.pp_head_wgrad_f16(C.c_void_p(a["g"]), a["ldg"], C.c_void_p(a["x"]), C.c_void_p(a["scale"]), a["m"], a["hw"], a["c_in"],
                                          a["c_out"], a["inv"], C.c_void_p(a["ws"]), a["ws_bytes"], C.c_void_p(a["dw"]), C.c_void_p(a["db"]),
                                          C.c_void_p(st.cuda_stream))

    def results(self):
        """(dw (c_out, c_in), db (c_out,)) as NumPy; asserts that both guards still hold the poison"""
        dw, db = self.dw.cpu().numpy(), self.db.cpu().numpy()
        n = self.c_out * self.c_in
        nan = bits(np.full(GUARD, np.nan, np.float32))
        assert np.array_equal(bits(dw[n:]), nan) and np.array_equal(bits(db[self.c_out:]), nan), "a guard behind dw / db was written"
        return dw[:n].reshape(self.c_out, self.c_in).copy(), db[:self.c_out].copy()

    def run(self, **kw):
        self.poison()
        assert self.launch(**kw) == 0
        return self.results()

    def untouched(self):
        return bool(torch.isnan(self.dw).all()) and bool(torch.isnan(self.db).all())


def exact_shapes(lib):
    P, G = lib.pp_head_wgrad_chunk_pixels(), lib.pp_head_wgrad_max_workgroups()
    shapes = [(1, 1, 256, 50, 50, False), (32, 16, 256, 50, 50, False)]
    shapes += [(m, m, 256, 64, 64, False) for m in (63, 64, 65)]
    shapes += [(192, 64, 256, 50, 64, True), (512, 256, 64, 50, 64, True)]
    shapes += [(m, m, 128, 50, 64, False) for m in (P - 1, P, P + 1, 2 * P + 17)]
    return shapes, (2 * G * P + 17, 2 * G * P + 17, 256, 50, 64, False)


def check_exact(lib, g, x, scale, hw, c_out):
    call = Call(lib, g, x, scale, hw, c_out)
    dw, db = call.run()
    want_dw, want_db = ref.head_wgrad(g, x, c_out, scale, hw)
    adw, adb = ref.abs_products(g, x, c_out, scale, hw)
    assert adw.max() < 2.0 ** 23 and adb.max() < 2.0 ** 23, "the case is not exact in every order"
    assert np.array_equal(want_dw, want_dw.astype(np.float32)) and np.array_equal(want_db, want_db.astype(np.float32))
    assert np.array_equal(bits(dw), bits(want_dw.astype(np.float32))), f"dw: {np.abs(dw - want_dw).max()}"
    assert np.array_equal(bits(db), bits(want_db.astype(np.float32))), f"db: {np.abs(db - want_db).max()}"


def test_exact_small_integers(lib):
    shapes, _ = exact_shapes(lib)
    for i, (m, hw, c_in, c_out, ldg, scaled) in enumerate(shapes):
        rng = np.random.default_rng(100 + i)
        g, x, scale = make_ints(rng, m, c_in, c_out, ldg, m // hw if scaled else None)
        check_exact(lib, g, x, scale, hw, c_out)


def test_exact_product_needs_its_rounding(lib):
    """x up to 2047 times a gain of 3: the exact product needs more than 11 bits and is rounded to binary16 once"""
    rng = np.random.default_rng(7)
    g, x, scale = make_ints(rng, 192, 256, 50, 64, 3, x_max=2047, gains=(3.0,))
    xs = ref.scaled_input(x, scale, 64).astype(np.float64)
    assert (xs != x.astype(np.float64) * 3.0).any()
    check_exact(lib, g, x, scale, 64, 50)


def test_exact_every_workgroup_two_chunks_and_a_tail(lib):
    m, hw, c_in, c_out, ldg, _ = exact_shapes(lib)[1]
    g, x, _ = make_ints(np.random.default_rng(11), m, c_in, c_out, ldg, None, g_max=1, x_max=31)
    check_exact(lib, g, x, None, hw, c_out)


@pytest.fixture(scope="module")
def real_cases(lib):
    P = lib.pp_head_wgrad_chunk_pixels()
    out = []
    for i, (m, hw, n_img) in enumerate([(2 * P + 17, 2 * P + 17, None), (4 * 256, 256, 4)]):
        g, x, scale = make_reals(np.random.default_rng(200 + i), m, 256, 50, 64, n_img)
        out.append(dict(g=g, x=x, scale=scale, hw=hw, m=m, want=ref.head_wgrad(g, x, 50, scale, hw), absprod=ref.abs_products(g, x, 50, scale, hw)))
    return out


def test_rounding_bound(lib, real_cases):
    for c in real_cases:
        dw, db = Call(lib, c["g"], c["x"], c["scale"], c["hw"], 50).run()
        bw, bb = ref.rounding_bound(c["m"], c["absprod"][0]), ref.rounding_bound(c["m"], c["absprod"][1])
        ew, eb = np.abs(dw.astype(np.float64) - c["want"][0]), np.abs(db.astype(np.float64) - c["want"][1])
        print(f"m = {c['m']}: largest |dw - ref| / bound = {(ew / bw).max():.4f}, |db - ref| / bound = {(eb / bb).max():.4f}")
        assert np.isfinite(dw).all() and np.isfinite(db).all()
        assert (ew <= bw).all() and (eb <= bb).all()


def test_rounding_bound_with_subnormal_inputs(lib):
    """binary16 subnormals in both operands (a few percent of a real feature map are): their products are as exact as any other,
    so the same bound holds -- down to m = 2, where it leaves room for one float32 addition"""
    P = lib.pp_head_wgrad_chunk_pixels()
    worst = 0.0
    for i, (m, hw, n_img) in enumerate([(2, 1, None), (2 * P + 17, 2 * P + 17, None), (128, 64, 2)]):
        rng = np.random.default_rng(400 + i)
        g, x, scale = make_reals(rng, m, 256, 50, 64, n_img)
        x = (x.astype(np.float32) * np.where(rng.random(x.shape) < 0.3, 2.0 ** -17, 1.0)).astype(np.float16)
        g[:, :50] = (g[:, :50].astype(np.float32) * np.where(rng.random((m, 50)) < 0.3, 2.0 ** -13, 1024.0)).astype(np.float16)
        sub = lambda a: int(((np.abs(a) > 0) & (np.abs(a) < 2.0 ** -14)).sum())
        assert sub(x) > x.size // 8 and sub(g[:, :50]) > m * 50 // 8
        dw, db = Call(lib, g, x, scale, hw, 50).run()
        want, ap = ref.head_wgrad(g, x, 50, scale, hw), ref.abs_products(g, x, 50, scale, hw)
        bw, bb = ref.rounding_bound(m, ap[0]), ref.rounding_bound(m, ap[1])
        ew, eb = np.abs(dw.astype(np.float64) - want[0]), np.abs(db.astype(np.float64) - want[1])
        worst = max(worst, float((ew / np.maximum(bw, 1e-300)).max()), float((eb / np.maximum(bb, 1e-300)).max()))
        assert (ew <= bw).all() and (eb <= bb).all(), m
    print(f"subnormal inputs: largest error / bound = {worst:.4f}")


def test_inv_loss_scale_is_applied_once(lib, real_cases):
    c = real_cases[1]
    call = Call(lib, c["g"], c["x"], c["scale"], c["hw"], 50)
    dw1, db1 = call.run()
    dw2, db2 = call.run(inv=2.0 ** -12)
    assert np.array_equal(bits(dw2), bits(dw1 * np.float32(2.0 ** -12))) and np.array_equal(bits(db2), bits(db1 * np.float32(2.0 ** -12)))


def test_deterministic_eager_graph_and_workspace_offset(lib, real_cases):
    c = real_cases[1]
    call = Call(lib, c["g"], c["x"], c["scale"], c["hw"], 50)
    other = make_reals(np.random.default_rng(300), c["m"], 256, 50, 64, 4)
    inputs = [(call.g.clone(), call.x.clone()), (torch.from_numpy(other[0]).to(DEV), torch.from_numpy(other[1]).to(DEV))]
    eager = []
    for g, x in inputs:
        call.g.copy_(g), call.x.copy_(x)
        first, second = call.run(), call.run()
        shifted = call.run(ws_offset=4)
        for a, b in zip(first, second):
            assert np.array_equal(bits(a), bits(b))
        for a, b in zip(first, shifted):
            assert np.array_equal(bits(a), bits(b))
        eager.append(first)
    assert not np.array_equal(bits(eager[0][0]), bits(eager[1][0]))
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert call.launch(stream=side) == 0
    torch.cuda.current_stream().wait_stream(side)
    for replay in range(5):
        g, x = inputs[replay % 2]
        call.g.copy_(g), call.x.copy_(x)
        call.poison()
        graph.replay()
        for a, b in zip(call.results(), eager[replay % 2]):
            assert np.array_equal(bits(a), bits(b)), f"replay {replay}"


def test_refusals_leave_the_outputs_alone(lib):
    g, x, scale = make_ints(np.random.default_rng(5), 128, 256, 50, 64, 2)
    call = Call(lib, g, x, scale, 64, 50)
    cases = [(BAD_ARG, dict(g=None)), (BAD_ARG, dict(x=None)), (BAD_ARG, dict(dw=None)), (BAD_ARG, dict(db=None)), (BAD_ARG, dict(ws=None)),
             (BAD_ARG, dict(m=0)), (BAD_ARG, dict(m=-64)), (BAD_ARG, dict(hw=0)), (BAD_ARG, dict(hw=-64)), (BAD_ARG, dict(m=127)),
             (BAD_ARG, dict(ldg=49)),
             (BAD_ARG, dict(x=call.x.data_ptr() + 8)), (BAD_ARG, dict(scale=call.scale.data_ptr() + 8)), (BAD_ARG, dict(g=call.g.data_ptr() + 1)),
             (BAD_ARG, dict(dw=call.dw.data_ptr() + 2)), (BAD_ARG, dict(db=call.db.data_ptr() + 2)), (BAD_ARG, dict(ws=call.ws.data_ptr() + 2)),
             (BAD_ARG, dict(ws_bytes=call.ws_bytes - 1)), (BAD_ARG, dict(ws_bytes=0)),
             (BAD_ARG, dict(inv=0.0)), (BAD_ARG, dict(inv=-1.0)), (BAD_ARG, dict(inv=float("inf"))), (BAD_ARG, dict(inv=float("nan"))),
             (UNSUPPORTED, dict(c_in=320)), (UNSUPPORTED, dict(c_in=32)), (UNSUPPORTED, dict(c_in=96)), (UNSUPPORTED, dict(c_out=0)),
             (UNSUPPORTED, dict(c_out=65, ldg=65)), (UNSUPPORTED, dict(hw=32)),
             (TOO_LARGE, dict(m=2 ** 31, scale=None)), (TOO_LARGE, dict(m=2 ** 31, hw=2 ** 30))]
    call.poison()
    for want, over in cases:
        assert call.launch(**over) == want, over
    torch.cuda.synchronize()
    assert call.untouched()
    # the same call without an override is accepted
    assert call.launch() == 0
    torch.cuda.synchronize()
    assert not call.untouched()


def test_supported(lib):
    assert lib.pp_head_wgrad_supported(320, 50) == 0
    assert lib.pp_head_wgrad_supported(256, 50) == 1 and lib.pp_head_wgrad_supported(64, 64) == 1 and lib.pp_head_wgrad_supported(192, 1) == 1
    assert lib.pp_head_wgrad_supported(256, 65) == 0 and lib.pp_head_wgrad_supported(0, 50) == 0 and lib.pp_head_wgrad_supported(100, 50) == 0
    assert lib.pp_head_wgrad_chunk_pixels() >= 16 and 1 <= lib.pp_head_wgrad_max_workgroups() <= 1024
