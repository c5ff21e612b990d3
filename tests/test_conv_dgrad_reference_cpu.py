"""CPU: the float64 restatement of tests/conv_dgrad_reference.py against torch's own conv2d_input, the proof that the integer cases of
tests/test_gpu_conv_dgrad.py are exact in float32 in every order of addition, and the new symbols' refusals on a machine without a
device."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_dgrad_reference as ref

NO_DEVICE, BAD_ARG, TOO_LARGE, UNSUPPORTED = -1, -2, -3, -6


@pytest.mark.parametrize("case", [c for c in ref.EXACT_CASES if c[1] == (64, 64) and c[0] != ref.LARGE_SHAPE] + [((2, 3, 5), (192, 128)), ((1, 5, 29), (64, 128))],
                         ids=ref.case_id)
def test_restatement_equals_torch_conv2d_input(case):
    (n, h, w), (c_in, c_out) = case
    rng = np.random.default_rng(9)
    dy = (rng.standard_normal((n * h * w, c_out)) * 0.25).astype(np.float16)
    wt = rng.standard_normal((c_out, 3, 3, c_in)).astype(np.float16)
    got = ref.conv3x3_dgrad(dy, wt, None, (n, h, w), 0.01)
    dt = torch.from_numpy(dy.astype(np.float64)).view(n, h, w, c_out).permute(0, 3, 1, 2)
    want = torch.nn.grad.conv2d_input((n, c_in, h, w), torch.from_numpy(wt.astype(np.float64)).permute(0, 3, 1, 2), dt, stride=1, padding=1)
    want = want.permute(0, 2, 3, 1).numpy()
    assert got.shape == (n, h, w, c_in) and np.abs(got - want).max() <= 1e-12 * (np.abs(want).max() + 1e-30)
    s, _ = ref.conv3x3_dgrad_sums(dy, wt, (n, h, w))
    assert np.array_equal(s, got)


def test_restatement_equals_autograd_through_the_activation():
    n, h, w, c_in, c_out, slope = 2, 3, 5, 64, 64, 0.01
    rng = np.random.default_rng(4)
    dy = (rng.standard_normal((n * h * w, c_out)) * 0.25).astype(np.float16)
    wt = rng.standard_normal((c_out, 3, 3, c_in)).astype(np.float16)
    pre = torch.from_numpy(rng.standard_normal((n, c_in, h, w))).requires_grad_(True)
    pre.data[0, :4, 0, 0] = torch.tensor([0.0, -0.0, -1e-7, 1e-7], dtype=torch.float64)
    y = torch.nn.functional.leaky_relu(pre, float(np.float32(slope)))
    out = torch.nn.functional.conv2d(y, torch.from_numpy(wt.astype(np.float64)).permute(0, 3, 1, 2), padding=1)
    out.backward(torch.from_numpy(dy.astype(np.float64)).view(n, h, w, c_out).permute(0, 3, 1, 2))
    y16 = y.detach().permute(0, 2, 3, 1).numpy().astype(np.float16)
    pre_n = pre.detach().permute(0, 2, 3, 1).numpy()
    keep = (y16 != 0) | (pre_n == 0)              # the entry sees the activation's OUTPUT as binary16: its sign unless it rounds to zero
    got, want = ref.conv3x3_dgrad(dy, wt, y16, (n, h, w), slope), pre.grad.permute(0, 2, 3, 1).numpy()
    assert keep.mean() > 0.99 and np.abs(got - want)[keep].max() <= 1e-12 * np.abs(want).max()
    assert got[0, 0, 0, 0] == want[0, 0, 0, 0] and got[0, 0, 0, 1] == want[0, 0, 0, 1]      # y = +-0: the slope, as torch's backward


def test_single_pixel_has_only_the_centre_tap():
    dy, wt, _ = ref.int_operands(((1, 1, 1), (64, 64)))
    t = ref.conv3x3_dgrad(dy, wt, None, (1, 1, 1), ref.SLOPE)
    assert np.array_equal(t[0, 0, 0], dy[0].astype(np.float64) @ wt[:, 1, 1, :].astype(np.float64))


@pytest.mark.parametrize("case", ref.EXACT_CASES, ids=ref.case_id)
def test_integer_cases_are_exact_in_float32(case):
    (n, h, w), (c_in, c_out) = case
    dy, wt, y = ref.int_operands(case)
    assert 9 * c_out * ref.INT_MAX * ref.INT_MAX < 2 ** 24
    assert np.abs(dy).max() <= ref.INT_MAX and np.abs(wt).max() <= ref.INT_MAX and np.array_equal(dy, np.rint(dy)) and np.array_equal(wt, np.rint(wt))
    s, absprod = ref.conv3x3_dgrad_sums(dy, wt, (n, h, w))
    assert absprod.max() <= 9 * c_out * 16 < 2.0 ** 24      # integers: every partial sum of every order is an integer below 2^24
    t = ref.conv3x3_dgrad(dy, wt, y, (n, h, w), ref.SLOPE)
    assert np.array_equal(s, s.astype(np.float32)) and np.array_equal(t, t.astype(np.float32))     # and slope * s is exact
    bits = y.view(np.uint16)
    assert y.size < 400 or all((bits == v).any() for v in ref.SPECIALS.view(np.uint16))
    assert np.isfinite(ref.to_half(t)).all()
    # an element is exact, so the bound holds the binary16 rounding alone
    assert (np.abs(ref.to_half(t).astype(np.float64) - t) <= ref.conv3x3_dgrad_bound(dy, wt, y, (n, h, w), ref.SLOPE)).all()


# ------------------------------------------------------------------------------------------------ the symbols, without a device

@pytest.fixture(scope="module")
def lib():
    from posepaf import _lib
    return _lib.load()


def _no_device():
    return not torch.cuda.is_available()


def test_dgrad_symbol_refuses_in_order(lib):
    a = 1 << 20                                          # a 16-byte aligned address that is never dereferenced: every call is refused
    call = lambda dy=a, w=a, y=a, n=2, h=3, wd=5, c_in=64, c_out=64, slope=0.01, dx=a: lib.pp_conv3x3_dgrad_f16(
        C.c_void_p(dy), C.c_void_p(w), C.c_void_p(y), n, h, wd, c_in, c_out, slope, C.c_void_p(dx), None)
    nan = float("nan")
    steps = [
        (dict(dy=None, n=0), BAD_ARG), (dict(w=None, n=0), BAD_ARG), (dict(dx=None, n=0), BAD_ARG),
        (dict(n=0, dy=a + 2), BAD_ARG), (dict(h=-1, dy=a + 2), BAD_ARG), (dict(wd=0, dy=a + 2), BAD_ARG),
        (dict(dy=a + 8, slope=nan), BAD_ARG), (dict(w=a + 2, slope=nan), BAD_ARG), (dict(y=a + 4, slope=nan), BAD_ARG), (dict(dx=a + 8, slope=nan), BAD_ARG),
        (dict(slope=nan, c_in=65), BAD_ARG), (dict(slope=float("inf"), c_in=65), BAD_ARG), (dict(slope=0.0, c_in=65), BAD_ARG),
        (dict(slope=-0.01, c_in=65), BAD_ARG),
        (dict(c_in=65, n=2 ** 16, h=2 ** 15, wd=1), UNSUPPORTED), (dict(c_in=320), UNSUPPORTED), (dict(c_out=32), UNSUPPORTED),
        (dict(c_out=96), UNSUPPORTED), (dict(c_out=320), UNSUPPORTED), (dict(c_in=0), UNSUPPORTED),
        (dict(n=2 ** 16, h=2 ** 15, wd=1), TOO_LARGE), (dict(n=2 ** 30, h=2 ** 30, wd=2 ** 30), TOO_LARGE),
    ]
    for over, want in steps:
        assert call(**over) == want, over
    assert all(lib.pp_conv3x3_dgrad_supported(ci, co) == lib.pp_conv3x3_wgrad_supported(ci, co) for ci in range(0, 321, 32) for co in range(0, 321, 32))
    assert all(lib.pp_conv3x3_dgrad_supported(ci, co) == 1 for ci in (64, 128, 192, 256) for co in (64, 128, 192, 256))
    if _no_device():
        assert call() == NO_DEVICE
        assert call(y=None, slope=nan) == NO_DEVICE      # without y the slope is not looked at


def test_layer_update_symbol_refuses_in_order(lib):
    from posepaf import _lib
    assert lib.pp_layer_update_max_segments() == 256 and C.sizeof(_lib.UpdateSegment) == 32
    a = 1 << 20
    names = ("masters", "grads", "momentum", "n", "segments", "n_segments", "hyper", "state", "workspace")

    def call(**over):
        v = dict(masters=a, grads=a, momentum=a, n=100, segments=a, n_segments=2, hyper=a, state=a, workspace=a)
        v.update(over)
        args = [v[k] if k in ("n", "n_segments") else C.c_void_p(v[k]) for k in names]
        return lib.pp_layer_update_f32(*args, None)
    for k in names:
        if k not in ("n", "n_segments"):
            assert call(**{k: None, "n": 0}) == BAD_ARG, k
    assert call(n=0, n_segments=300) == BAD_ARG and call(n=-1, n_segments=300) == BAD_ARG and call(n_segments=-1, masters=a + 2) == BAD_ARG
    for k, off in (("masters", 2), ("grads", 1), ("momentum", 2), ("hyper", 2), ("workspace", 2), ("segments", 4), ("state", 4)):
        assert call(**{k: a + off, "n_segments": 300}) == BAD_ARG, k
    assert call(n_segments=257, n=2 ** 31) == UNSUPPORTED
    assert call(n=2 ** 31) == TOO_LARGE
    if _no_device():
        assert call() == NO_DEVICE and call(n_segments=0) == NO_DEVICE and call(n_segments=256) == NO_DEVICE
