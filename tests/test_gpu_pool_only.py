"""GPU: the streaming 1x1 kernel's pooled output WITHOUT the full-resolution tensor (pp_pw_cat_f16 / pp_pw_pool_f16 with y = NULL) --
the backbone reads only maxpool2(res1(x)), so res1's 256 x 256 x 128-channel output is never written.

The pooled output must be bit-equal to the call that also writes y; a NaN-filled buffer of y's size (with guards), allocated where the
caching allocator would otherwise place y, must come back intact; y = NULL without a pooled output stays PP_ERR_BAD_ARG."""
import ctypes as C

import pytest
import torch

import conv_reference as cr

pytestmark = pytest.mark.gpu

N = 2
GUARD = 64 * 1024 // 2
NAN16 = 0x7E00
BAD_ARG = -2
CASES = [(64, 64, 128, 2, 32), (64, 64, 128, 4, 64), (192, 256, 384, 2, 32)]   # (c1, c2, k, h, w); the last splits k over grid.y


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _nan(numel):
    return torch.full((GUARD + numel + GUARD,), float("nan"), dtype=torch.float16, device="cuda")


def _all_nan(buf):
    return bool((buf.view(torch.int16) == NAN16).all())


def _cat(L, ops, wcat, bias, y, pool, spec, slope, width=None):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.pp_pw_cat_f16(_p(ops["t"]), _p(ops["x"]), _p(wcat), _p(bias), None, _p(y), _p(pool), spec.n * spec.h * spec.w, spec.h * spec.w,
                         (spec.w if pool is not None else 0) if width is None else width, spec.c1, spec.c2, spec.k, spec.k, 0, slope, st)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", CASES, ids=[f"{a}+{b}to{k}-{h}x{w}" for a, b, k, h, w in CASES])
def test_pooled_output_without_y_is_bit_equal_and_writes_nothing_else(case):
    from posepaf import _lib, fused_model as fm
    L = _lib.load()
    c1, c2, k, h, w = case
    spec = cr.parse_key(("cat", N, c1, c2, h, w, k, True, True))
    ops = cr.make_operands(spec, seed=100 + c1 + h, device="cuda")
    wcat = ops["w"].detach().flatten(1).contiguous()
    ny, npool = N * h * w * k, N * (h // 2) * (w // 2) * k

    ybuf, pbuf = _nan(ny), _nan(npool)
    y = ybuf[GUARD:GUARD + ny].view(N, h, w, k).permute(0, 3, 1, 2)
    pool = pbuf[GUARD:GUARD + npool].view(N, h // 2, w // 2, k).permute(0, 3, 1, 2)
    assert _cat(L, ops, wcat, ops["b"], y, pool, spec, fm.LEAK) == 0
    ref, _ = cr.reference32(spec, ops)
    cr.assert_close(pool, ref["pool"], cr.bound_for(float(ref["pool"].abs().max())), "pooled output (with y)")
    cr.assert_close(y, ref["y"], cr.bound_for(float(ref["y"].abs().max())), "y")

    guard_y, pbuf2 = _nan(ny), _nan(npool)         # where y would be: must stay NaN
    pool2 = pbuf2[GUARD:GUARD + npool].view(N, h // 2, w // 2, k).permute(0, 3, 1, 2)
    assert _cat(L, ops, wcat, ops["b"], None, pool2, spec, fm.LEAK) == 0
    assert _all_nan(guard_y), "the call without y wrote into the buffer where y would be"
    assert _all_nan(pbuf2[:GUARD]) and _all_nan(pbuf2[GUARD + npool:]), "a store landed outside the pooled output"
    assert not bool(torch.isnan(pool2).any()), "pooled output not fully written"
    assert torch.equal(pool2, pool), "pooled output differs from the call that also writes y"
    assert _all_nan(ybuf[:GUARD]) and _all_nan(ybuf[GUARD + ny:]) and _all_nan(pbuf[:GUARD]) and _all_nan(pbuf[GUARD + npool:])


def test_no_output_at_all_is_a_bad_argument():
    from posepaf import _lib, fused_model as fm
    L = _lib.load()
    spec = cr.parse_key(("cat", N, 64, 64, 2, 32, 128, True, False))
    ops = cr.make_operands(spec, seed=3, device="cuda")
    wcat = ops["w"].detach().flatten(1).contiguous()
    assert _cat(L, ops, wcat, ops["b"], None, None, spec, fm.LEAK) == BAD_ARG
    assert _cat(L, ops, wcat, ops["b"], None, None, spec, fm.LEAK, width=32) == BAD_ARG
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.cat([ops["t"], ops["x"]], dim=1).contiguous(memory_format=torch.channels_last)
    assert L.pp_pw_pool_f16(_p(x), None, _p(wcat), _p(ops["b"]), None, None, None, None, None, N * 64, 64, 32, 128, 128, 128, 0, fm.LEAK,
                            st) == BAD_ARG
    assert L.pp_pw_f16(_p(x), None, _p(wcat), _p(ops["b"]), None, None, None, None, N * 64, 64, 128, 128, 128, 0, fm.LEAK, st) == BAD_ARG


def test_res1_hands_over_the_same_pooled_tensor_without_writing_its_output(monkeypatch):
    """model level: FResidual.forward_pool(x, pooled_only=True) on the backbone's res1 (64 -> 128 channels, skip convolution) against
    the form that also returns the block output"""
    from posepaf import fused_model as fm
    model = fm.build_inference_model("cuda")
    x = torch.rand((2, 64, 64, 64), generator=torch.Generator(device="cuda").manual_seed(4), device="cuda").half()
    x = x.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        y, pooled = model.res1.forward_pool(x)                   # (tunes the shape on first use)
        nothing, only = model.res1.forward_pool(x, pooled_only=True)
        monkeypatch.setattr(fm, "USE_POOL_ONLY", False)
        y_off, pooled_off = model.res1.forward_pool(x, pooled_only=True)
    torch.cuda.synchronize()
    key = ("cat", 2, 64, 64, 64, 64, 128, bool(model.res1.c3.act), True)
    assert key in fm.conv_choices(), "res1 did not go through the [t ; x] form's tuner"
    if fm.conv_choices()[key] == 1:
        assert nothing is None, "the one-launch form still returned (and wrote) the block output"
    assert y is not None and y_off is not None
    assert torch.equal(only, pooled) and torch.equal(pooled_off, pooled)
    assert torch.equal(pooled, fm.maxpool2(y))
