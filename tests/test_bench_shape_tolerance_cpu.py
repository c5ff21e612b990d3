"""CPU: the comparison of tests/test_gpu_bench_shapes.py can tell a subtly wrong kernel from a right one at every layer key of the
bench geometry (profiles/conv_choice_b128.json).  Per key, on the same operand recipe at 2 samples: a "kernel" that drops ONE input
channel at ONE tap over ONE tile of the last image must be rejected, and the float64 truth rounded to fp16 must be accepted.
The tolerance scale max |ref| comes from an fp32 torch.nn.functional pass over the whole 2-sample output; float64 is computed
for the mutated tile only.
The keys on the `strengthened` printout are where this bar cannot see ONE missing term: tests/test_gpu_conv_exact.py (exact
operands, bit equality; tests/test_conv_exact_reference_cpu.py shows one missing term changes a bit at every key) closes that gap."""
import pytest
import torch

import conv_reference as cr

ENTRIES = cr.table_entries()


def _tile_pix(spec):
    th, tw, tx = cr.tile_geometry(spec.H, spec.W)
    last = tx * (-(-spec.H // th)) - 1
    q = cr.tile_pixels(spec.H, spec.W, last)
    return torch.cat([torch.full((len(q), 1), spec.n - 1), q], 1)


def test_the_comparison_rejects_one_missing_term_and_accepts_fp16_rounding():
    torch.manual_seed(0)
    strengthened, report = [], []
    for key, _ in ENTRIES:
        spec = cr.parse_key(key, n=2)
        ops = cr.make_operands(spec, seed=11)
        ref32, _ = cr.reference32(spec, ops)
        tol = cr.TOL_COLLAPSED if spec.up else cr.TOL            # the looser of the form's candidates
        bound = cr.bound_for(ref32["y"].abs().max(), tol)
        pix = _tile_pix(spec)
        exact = cr.outputs64_at(spec, ops, pix)["y"]
        label = f"{cr.key_id(key)} (n = 2)"
        assert cr.mismatch(exact.half().double(), exact, bound, label, pix) is None, "fp16 rounding of the truth rejected"
        # one input channel at the centre tap: a channel drawn per key (the same every run)
        c = int(torch.randint(0, spec.c, (1,), generator=torch.Generator().manual_seed(len(report))))
        tap = (spec.r // 2) * spec.r + spec.r // 2
        wrong = cr.outputs64_at(spec, ops, pix, drop=(c, tap))["y"].half().double()
        msg = cr.mismatch(wrong, exact, bound, label, pix)
        if msg is None:
            # one term is below the bound at this fan-in: a block of 32 channels at that tap must still be caught
            strengthened.append(cr.key_id(key))
            block = cr.outputs64_at(spec, ops, pix, drop=(slice(c - c % 32, c - c % 32 + 32), tap))["y"]
            msg = cr.mismatch(block.half().double(), exact, bound, label, pix)
            assert msg is not None, f"{label}: neither one missing term nor a missing block of 32 channels is detected"
        assert f"image {spec.n - 1}" in msg, msg
        report.append((cr.key_id(key), round(float((wrong - exact).abs().max()) / bound, 2)))
    print("missing-term error / bound per key:", report)
    print("keys that needed the 32-channel mutation:", strengthened or "none")
    assert len(report) == len(ENTRIES) == 71


def test_the_float64_and_fp32_references_agree_at_the_sampled_pixels():
    """The two references of the GPU test, on the CPU at 2 samples: conv + bias of the fp32 pass within 1e-5 of float64 at every
    sampled pixel, and every output (pooled and channel-mean forms included) within the kernel tolerance of float64."""
    for key, _ in ENTRIES:
        spec = cr.parse_key(key, n=2)
        ops = cr.make_operands(spec, seed=12)
        pix = cr.sample_pixels(spec.n, spec.H, spec.W)
        ref32, at32 = cr.reference32(spec, ops, pix, chunk=1)
        a64 = cr.acc64_at(spec, ops, pix)
        label = cr.key_id(key)
        cr.assert_close(at32.double(), a64, cr.TOL_FP32 * max(1.0, float(a64.abs().max())), label + " fp32 conv", pix)
        o64 = cr.outputs64_at(spec, ops, pix)
        for name in [o for o in spec.outputs() if o in o64]:
            bound = cr.bound_for(ref32[name].abs().max())
            cr.assert_close(cr.values_at(ref32[name], pix), o64[name], bound, f"{label} {name}", pix)
        if spec.pooled:
            q = cr.sample_pixels(spec.n, spec.H // 2, spec.W // 2)
            cr.assert_close(cr.values_at(ref32["pool"], q), cr.pooled64_at(spec, ops, q), cr.bound_for(ref32["pool"].abs().max()),
                            label + " pool", q)
        if spec.has_mean:
            assert ref32["mean"].shape == (spec.n, spec.k)
