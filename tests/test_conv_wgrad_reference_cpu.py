"""CPU: the float64 restatements of tests/conv_wgrad_reference.py against torch's own formulations, and the proof that the integer
cases of tests/test_gpu_conv_wgrad.py are exact in float32 in every order of addition."""
import numpy as np
import pytest
import torch

import conv_wgrad_reference as ref


def _real_operands(case, seed):
    (n, h, w), (c_in, c_out) = case
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n * h * w, c_out)) * 0.25).astype(np.float16), rng.standard_normal((n, h, w, c_in)).astype(np.float16)


@pytest.mark.parametrize("case", [c for c in ref.EXACT_CASES if c[1] == (64, 64)] + [((2, 3, 5), (192, 128))], ids=ref.case_id)
def test_wgrad_restatement_equals_torch(case):
    (n, h, w), (c_in, c_out) = case
    dy, x = _real_operands(case, 5)
    dw, db = ref.conv3x3_wgrad(dy, x, 0.5)
    xt = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    dt = torch.from_numpy(dy.astype(np.float64)).view(n, h, w, c_out).permute(0, 3, 1, 2)
    want = torch.nn.grad.conv2d_weight(xt, (c_out, c_in, 3, 3), dt, stride=1, padding=1).permute(0, 2, 3, 1).numpy() * 0.5
    scale = np.abs(want).max() + 1e-30
    assert dw.shape == (c_out, 3, 3, c_in) and np.abs(dw - want).max() <= 1e-12 * scale
    assert np.abs(db - dt.sum(dim=(0, 2, 3)).numpy() * 0.5).max() <= 1e-12 * (np.abs(db).max() + 1e-30)


def test_single_pixel_has_only_the_centre_tap():
    dy, x = ref.int_operands(((1, 1, 1), (64, 64)))
    dw, _ = ref.conv3x3_wgrad(dy, x)
    off = np.ones((3, 3), bool)
    off[1, 1] = False
    assert not dw[:, off, :].any() and not np.signbit(dw[:, off, :]).any()
    assert np.array_equal(dw[:, 1, 1, :], np.outer(dy[0].astype(np.float64), x[0, 0, 0].astype(np.float64)))
    assert np.array_equal(ref.contributing_pixels(1, 1, 1), off == False)      # noqa: E712


def test_a_nan_outside_the_window_is_never_multiplied():
    """the restatement takes only neighbours inside the image: embedding x in a NaN frame and slicing it out changes nothing"""
    dy, x = ref.int_operands(((2, 3, 5), (64, 64)))
    framed = np.full((2, 5, 7, 64), np.nan, np.float16)
    framed[:, 1:4, 1:6, :] = x
    a, b = ref.conv3x3_wgrad(dy, x), ref.conv3x3_wgrad(dy, np.ascontiguousarray(framed[:, 1:4, 1:6, :]))
    assert np.array_equal(a[0], b[0]) and np.isfinite(a[0]).all()


@pytest.mark.parametrize("c_out,ldg", [(1, 50), (50, 50), (50, 64), (64, 64)])
def test_dgrad_restatement_equals_autograd(c_out, ldg):
    m, c_in, slope = 145, 64, 0.01
    rng = np.random.default_rng(c_out)
    g = np.full((m, ldg), np.nan, np.float16)
    g[:, :c_out] = rng.standard_normal((m, c_out)).astype(np.float16)
    w = rng.standard_normal((c_out, c_in)).astype(np.float16)
    pre = torch.from_numpy(rng.standard_normal((m, c_in))).requires_grad_(True)
    pre.data[0, :4] = torch.tensor([0.0, -0.0, -1e-7, 1e-7], dtype=torch.float64)
    y = torch.nn.functional.leaky_relu(pre, float(np.float32(slope)))
    out = torch.nn.functional.conv2d(y.t().reshape(1, c_in, m, 1), torch.from_numpy(w.astype(np.float64)).view(c_out, c_in, 1, 1))
    out.backward(torch.from_numpy(g[:, :c_out].astype(np.float64)).t().reshape(1, c_out, m, 1))
    # the entry sees y, the activation's OUTPUT, as binary16; its sign is the pre-activation's as long as it does not round to zero
    y16 = y.detach().numpy().astype(np.float16)
    keep = (y16 != 0) | (pre.detach().numpy() == 0)
    got = ref.head_dgrad(g, w, y16, c_out, slope)
    want = pre.grad.numpy()
    assert keep.mean() > 0.99 and np.abs(got - want)[keep].max() <= 1e-12 * np.abs(want).max()
    assert got[0, 0] == want[0, 0] and got[0, 1] == want[0, 1]               # y = +-0: the slope, as torch's backward


@pytest.mark.parametrize("case", ref.EXACT_CASES, ids=ref.case_id)
def test_integer_wgrad_cases_are_exact_in_float32(case):
    dy, x = ref.int_operands(case)
    assert np.abs(dy).max() <= ref.INT_MAX and np.abs(x).max() <= ref.INT_MAX and np.array_equal(dy, np.rint(dy))
    aw, ab = ref.conv3x3_abs_products(dy, x)
    assert aw.max() < 2.0 ** 24 and ab.max() < 2.0 ** 24        # integers: every partial sum of every order is an integer below 2^24
    dw, db = ref.conv3x3_wgrad(dy, x)
    assert np.array_equal(dw, dw.astype(np.float32)) and np.array_equal(db, db.astype(np.float32))
    (n, h, w), _ = case
    assert ref.contributing_pixels(n, h, w)[1, 1] == n * h * w


def test_integer_dgrad_cases_are_exact():
    for m in ref.DGRAD_MS:
        for c_out in ref.DGRAD_C_OUTS:
            for ldg in ref.DGRAD_LDGS:
                if ldg < c_out:
                    continue
                g, w, y = ref.dgrad_int_operands(m, 128, c_out, ldg)
                assert np.isnan(g[:, c_out:]).all()
                absprod = np.abs(g[:, :c_out].astype(np.float64)) @ np.abs(w.astype(np.float64))
                assert absprod.max() < 2.0 ** 11             # s is an integer below 2^11, slope * s a multiple of 1/8: binary16 holds it
                t = ref.head_dgrad(g, w, y, c_out, ref.DGRAD_SLOPE)
                assert np.array_equal(t, ref.to_half(t).astype(np.float64))
                bits = y.view(np.uint16)
                assert m * 128 < 40 or all((bits == v).any() for v in (0x0000, 0x8000, 0x8001, 0x83FF))
