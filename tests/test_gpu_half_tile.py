"""GPU: variant 106 of the plain 3x3 convolution -- the halo-tile kernel's instances for C_out = 64 mod 128, which run the half-empty
last channel tile on all four SIMDs (csrc/posepaf_conv_own.hip, HALO_HALF) -- against variant 104 and against ground truth.

Every output keeps its accumulation order (channel blocks, then taps), so 106 must be bit-equal to 104.  Shapes (C, K): one and
several channel blocks, a lone half tile (K = 64), full tiles followed by a half tile (K = 192, 320); maps of tile widths 128, 64,
32 and 16, the last one (16 x 16) the stacked-image case, which the variant may refuse; residual modes 0, 1, 2.  Both variants
run through FConv._fused_launch (the product's argument marshalling) into NaN-filled outputs with a 64 KiB NaN guard on both sides."""
import zlib

import pytest
import torch

import conv_reference as cr

pytestmark = pytest.mark.gpu

N = 2
SHAPES = [(32, 64), (64, 64), (64, 192), (192, 192), (64, 320)]
MAPS = [(8, 128), (16, 64), (32, 32), (64, 64), (16, 16)]
GUARD = 64 * 1024 // 2
NAN16 = 0x7E00
UNSUPPORTED = -6


def _fconv(spec, ops):
    from posepaf import fused_model as fm
    conv = torch.nn.Conv2d(spec.c, spec.k, spec.r, 1, spec.pad, spec.dil, bias=True)
    with torch.no_grad():
        conv.weight.copy_(ops["w"].float().cpu())
        conv.bias.copy_(ops["b"].float().cpu())
    f = fm.FConv(conv, None, spec.act).cuda().half()
    f.weight.data = f.weight.data.contiguous(memory_format=torch.channels_last)
    assert torch.equal(f.weight, ops["w"]) and torch.equal(f.bias, ops["b"])
    return f


def _guarded(n, k, h, w):
    """-> (NaN-filled buffer, its (n, k, h, w) channels-last view behind a guard)"""
    body = n * h * w * k
    buf = torch.full((GUARD + body + GUARD,), float("nan"), dtype=torch.float16, device="cuda")
    return buf, buf.as_strided((n, k, h, w), (h * w * k, 1, w * k, k), GUARD)


def _guards_intact(buf, body):
    bits = buf.view(torch.int16)
    return bool((bits[:GUARD] == NAN16).all()) and bool((bits[GUARD + body:] == NAN16).all())


def _run(f, cfg, spec, ops):
    buf, y = _guarded(spec.n, spec.k, spec.H, spec.W)
    rc = f._fused_launch(cfg, ops["x"], ops.get("e1"), spec.mode, y)
    torch.cuda.synchronize()
    return rc, buf, y


@pytest.mark.parametrize("hw", MAPS, ids=[f"{h}x{w}" for h, w in MAPS])
@pytest.mark.parametrize("ck", SHAPES, ids=[f"{c}to{k}" for c, k in SHAPES])
def test_variant_106_is_bit_equal_to_104_and_within_tolerance(ck, hw):
    (c, k), (h, w) = ck, hw
    for mode in (0, 1, 2):
        spec = cr.parse_key((N, c, h, w, k, 3, 1, 1, mode, True))
        label = f"{c}->{k} at {h}x{w} mode {mode}"
        ops = cr.make_operands(spec, seed=zlib.crc32(label.encode()), device="cuda")
        ref, _ = cr.reference32(spec, ops)
        bound = cr.bound_for(float(ref["y"].abs().max()), cr.TOL)
        f = _fconv(spec, ops)
        body = spec.n * spec.H * spec.W * spec.k
        rc, buf4, y4 = _run(f, 104, spec, ops)
        assert rc == 0, f"{label}: 104 rc {rc}"
        assert _guards_intact(buf4, body), f"{label}: 104 wrote outside its output"
        cr.assert_close(y4, ref["y"], bound, label + " variant 104")
        rc, buf6, y6 = _run(f, 106, spec, ops)
        if (h, w) == (16, 16) and rc == UNSUPPORTED:
            continue                      # whole images stacked in one tile: correct or refused
        assert rc == 0, f"{label}: 106 rc {rc}"
        assert _guards_intact(buf6, body), f"{label}: 106 wrote outside its output"
        assert not bool(torch.isnan(y6).any()), f"{label}: 106 left output elements unwritten"
        cr.assert_close(y6, ref["y"], bound, label + " variant 106")
        assert torch.equal(y6, y4), f"{label}: 106 differs from 104"
        rc, _, again = _run(f, 106, spec, ops)
        assert rc == 0 and torch.equal(again, y6), f"{label}: two runs of 106 differ (race?)"


@pytest.mark.parametrize("ck", [(64, 128), (64, 256), (32, 384)], ids=lambda v: f"{v[0]}to{v[1]}")
def test_variant_106_refuses_shapes_without_a_half_empty_tile(ck):
    c, k = ck
    spec = cr.parse_key((N, c, 32, 32, k, 3, 1, 1, 0, True))
    ops = cr.make_operands(spec, seed=5, device="cuda")
    f = _fconv(spec, ops)
    rc, buf, y = _run(f, 106, spec, ops)
    assert rc == UNSUPPORTED, rc
    assert bool((buf.view(torch.int16) == NAN16).all()), "a refused call wrote something"
    rc, _, _ = _run(f, 104, spec, ops)
    assert rc == 0
