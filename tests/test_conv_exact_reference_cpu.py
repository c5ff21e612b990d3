"""CPU: the exact-operand sweep of tests/test_gpu_conv_exact.py stands on firm ground -- the key selection
(tests/conv_exact_cases.py) is deterministic, covers the launcher cells and forms it is meant to and stays within its budget; every
selected key satisfies, under every recipe it gets, the conditions under which bit equality may be asked of any summation order
(conv_reference.assert_exact_case); the float64 expectation equals the fp32 torch.nn.functional reference rounded to binary16 bit
for bit (two independent restatements of the contract); and ONE missing term changes an expected bit at every key, the bench
geometry's included -- the mutation the 2e-3 bar of tests/test_bench_shape_tolerance_cpu.py accepts at its `strengthened` keys."""
import pytest
import torch

import conv_exact_cases as cases
import conv_reference as cr
from test_bench_shape_tolerance_cpu import _tile_pix
from test_gpu_offbench_shapes import WANTED

SELECTION = cases.select()
IDS = [cr.key_id(k) for k, _ in SELECTION]
_shares: dict = {}


def test_the_selection_is_deterministic_covers_the_cells_and_stays_in_budget():
    entries = cr.table_entries(cr.OFFBENCH)
    again = cases.select(list(reversed(entries)))
    assert [k for k, _ in again] == [k for k, _ in SELECTION], "the selection depends on the order of the key file"
    assert len(set(IDS)) == len(IDS)
    have = cases.selected_cells(SELECTION)
    missing = [what for what, hit in WANTED if not any(hit(c) for c in have)]
    assert not missing, f"no selected key reaches {missing}"
    forms = {cr.parse_key(k).form for k, _ in entries}
    assert {s.form for _, s in SELECTION} == forms, "a form of the key file has no selected key"
    for tw in (128, 64, 32, 16):
        assert any(f" tw{tw} " in c + " " for c in have), f"no {tw}-wide tile"
    assert any(c.endswith(" x2") for c in have) and any(c.endswith(" x4") for c in have)
    small_rows = [(k, cr.parse_key(k)) for k, _ in entries if cr.parse_key(k).n <= cases.MAX_N]
    assert have == cases.selected_cells(small_rows), "a launcher cell of the rows with n <= 4 has no selected key"
    assert sum(c.startswith("pwpool") for c in have) >= 5 and "pwpre" in have and any(c.startswith("sums") for c in have)
    each = [cases.macs(s) for _, s in SELECTION]
    print(f"{len(SELECTION)} keys, {sum(each):.3g} multiply-adds in all, the largest key {max(each):.3g}; cells: {sorted(have)}")
    assert all(s.n <= cases.MAX_N for _, s in SELECTION)
    assert len(SELECTION) <= cases.MAX_KEYS and max(each) <= cases.MAX_KEY_MACS and sum(each) <= cases.MAX_TOTAL_MACS


@pytest.mark.parametrize("case", SELECTION, ids=IDS)
def test_every_recipe_is_valid_and_small_equals_the_fp32_reference_bit_for_bit(case):
    key, spec = case
    label = cr.key_id(key)
    for recipe in cr.recipes_for(spec):
        ops = cr.make_exact_operands(spec, cases.seed_of(label, recipe), recipe)
        want = cr.expected_exact(spec, ops)
        assert sorted(want) == sorted(spec.outputs())
        facts = cr.assert_exact_case(spec, ops, recipe, want, label)
        if recipe == "rounding":
            _shares.setdefault(spec.form, []).append(facts["shares"])
        if recipe != "small":
            continue
        ref32, _ = cr.reference32(spec, ops)
        for name in spec.outputs():
            if name == "mean":       # the contract's mean sums the ROUNDED outputs: taken from the fp32 pass' y, rounded
                r = cr.mean_binary16(ref32["y"].half())
            else:
                r = ref32[name].half()
            msg = cr.first_bit_difference(want[name], r, f"{label} {name}: float64 expectation against the fp32 reference")
            assert msg is None, msg


def test_the_rounding_recipe_report():
    """printout (after the per-key tests of this file): per form, the share of elements at which the contract's rounding order and the
    order without each inner rounding differ"""
    if not _shares:
        pytest.skip("the per-key tests did not run in this session")
    for form, rows in sorted(_shares.items()):
        names = sorted({n for r in rows for n in r})
        print(f"{form}: {len(rows)} keys; share of order-sensitive elements, least .. most per rounding: " +
              ", ".join(f"{n} {min(r[n] for r in rows if n in r):.1%} .. {max(r[n] for r in rows if n in r):.1%}" for n in names))
        assert all(r["any"] >= 0.01 for r in rows)


def _one_missing_term_changes_a_bit(spec, label, seed):
    ops = cr.make_exact_operands(spec, seed, "small")
    pix = _tile_pix(spec)
    e = {n_: cr._nhwc_at(ops[n_], pix[:, 0], pix[:, 1], pix[:, 2]) if n_ in ops else None for n_ in ("e1", "e2")}
    # one input channel at the centre tap (always inside the image), drawn among the channels whose input is not zero at every pixel
    # of the tile: a term that is zero everywhere is not missing (a 1 x 1 map has ONE pixel, and x = 0 is one value of seven)
    d = 2 if spec.up else 1
    xc = cr._nhwc_at(ops["x"], pix[:, 0], pix[:, 1] // d, pix[:, 2] // d)
    if spec.form == "cat":
        xc = torch.cat([cr._nhwc_at(ops["t"], pix[:, 0], pix[:, 1], pix[:, 2]), xc], 1)
    live = (xc != 0).any(0).nonzero().flatten()
    c = int(live[torch.randint(0, len(live), (1,), generator=torch.Generator().manual_seed(seed))])
    tap = (spec.r // 2) * spec.r + spec.r // 2
    right = cr.exact_epilogue(spec, cr.acc64_at(spec, ops, pix), e["e1"], e["e2"])
    wrong = cr.exact_epilogue(spec, cr.acc64_at(spec, ops, pix, drop=(c, tap)), e["e1"], e["e2"])
    changed = sum(int((right[n_].view(torch.int16) != wrong[n_].view(torch.int16)).sum()) for n_ in right)
    assert changed > 0, f"{label}: dropping input channel {c} at tap {tap} over the last tile changes no expected bit"
    return changed / sum(v.numel() for v in right.values())


def test_one_missing_term_changes_an_expected_bit_at_every_key():
    """the mirror of test_the_comparison_rejects_one_missing_term_and_accepts_fp16_rounding: under `small` a kernel that drops ONE
    input channel at ONE tap over one tile differs from the expectation in at least one bit -- at every selected key and at every key
    of the bench geometry at n = 2, the keys of that test's `strengthened` list among them"""
    least = 1.0
    for key, spec in SELECTION:
        least = min(least, _one_missing_term_changes_a_bit(spec, cr.key_id(key), cases.seed_of(cr.key_id(key), "drop")))
    bench = cr.table_entries()
    for key, _ in bench:
        label = cr.key_id(key) + " (n = 2)"
        least = min(least, _one_missing_term_changes_a_bit(cr.parse_key(key, n=2), label, cases.seed_of(label, "drop")))
    print(f"{len(SELECTION)} selected + {len(bench)} bench keys: one missing term changes at least {least:.1%} of the mutated tile's elements")
    assert len(bench) == 71


def test_the_stem_cases_are_valid():
    for shape in cases.STEM_IMAGES:
        for recipe in cr.RECIPES:
            label = f"stem {shape}"
            y = cases.stem_expected(cases.stem_operands(shape, cases.seed_of(label, recipe), recipe), recipe, label)
            assert y.shape == (shape[0], 64, shape[1] // 2, shape[2] // 2)
