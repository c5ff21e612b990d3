"""GPU: every fused convolution form held to BIT equality on exact operands.

The sweeps of tests/test_gpu_bench_shapes.py and tests/test_gpu_offbench_shapes.py judge N(0, 1) operands with
|y - ref| <= 2e-3 max(1, max |ref|): one missing term at a large fan-in, an extra binary16 rounding in an epilogue, or a flushed
subnormal pass below that bar.  Here the operands are chosen so that every fp32 partial sum is exact in any order
(conv_reference.make_exact_operands: `small`, `rounding`, `subnormal`); the only roundings left are the ones the contract in
conv_reference's docstring names, the expectation (conv_reference.expected_exact, float64 on the CPU) is known to the last bit, and
the tolerance is zero.  Per selected layer key (tests/conv_exact_cases.py: recorded keys, one per launch path), per recipe, every
candidate of conv_candidates.candidates -- MIOpen's candidate -1 is not this library's arithmetic and stays out -- writes guarded
NaN-filled outputs, and every output that ran must equal the expectation as int16 bit patterns with the guards intact.
The validity conditions of a case are asserted on the reference before anything is compared (conv_reference.assert_exact_case).
The stem runs the same recipes through pp_stem7x7_f16 and the product's FStem, which prepares its weights.
Last: pp_pw_f16's dynamic-LDS limit is raised once per k_pw instance with the FIRST caller's size; two fresh child processes call
the same instance small-then-large and large-then-small (tests/pw_lds_order_child.py)."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

import conv_exact_cases as cases
import conv_reference as cr
from conv_candidates import REFUSED, Out, _outputs, _p, _view, candidates, cells
from test_gpu_offbench_shapes import WANTED

pytestmark = pytest.mark.gpu

SELECTION = cases.select()
IDS = [cr.key_id(k) for k, _ in SELECTION]
_ran_cells: set = set()          # launcher cells of every candidate that ran under `small`
_report: dict = {}               # key id -> (form, {recipe: (ran, refused)})


@pytest.mark.parametrize("case", SELECTION, ids=IDS)
def test_every_candidate_equals_the_exact_expectation_bit_for_bit(case):
    key, spec = case
    label = cr.key_id(key)
    assert cases.macs(spec) <= cases.MAX_KEY_MACS        # the float64 expectation of the whole batch is affordable on the CPU
    failures, per_recipe = [], {}
    for recipe in cr.recipes_for(spec):
        ops = cr.make_exact_operands(spec, cases.seed_of(label, recipe), recipe, device="cuda")
        want = cr.expected_exact(spec, ops)
        cr.assert_exact_case(spec, ops, recipe, want, label)
        want = {name: v.cuda() for name, v in want.items()}
        ran, refused = [], []
        for cand, _, launch, shapes in candidates(spec, ops):
            o = _outputs(spec, shapes)
            rc = launch({name: _view(spec, name, v) for name, v in o.items()})
            torch.cuda.synchronize()
            if rc in REFUSED:
                refused.append(cand)
                continue
            assert rc == 0, f"{label} [{recipe}] candidate {cand}: rc {rc}"
            ran.append(cand)
            for name in shapes:
                what = f"{label} [{recipe}] candidate {cand} output {name}"
                hit = o[name].intact()
                assert hit is None, f"{what}: a store landed in {hit}"
                msg = cr.first_bit_difference(_view(spec, name, o[name]), want[name], what)
                if msg is not None:
                    failures.append(msg)
            if recipe == "small":
                _ran_cells.update(cells(spec, cand))
            del o
        print(f"{label} [{recipe}]: {len(ran)} candidates ran {ran}, refused {refused}")
        per_recipe[recipe] = (ran, refused)
        # (a channel-sums key at which halo_geometry refuses the batch -- no launcher cell on the CPU replay -- runs on MIOpen's
        # path in the product, and nothing of this library's is left to compare)
        assert ran or not cases.selected_cells([case]), f"{label} [{recipe}]: no candidate ran"
    _report[label] = (spec.form, per_recipe)
    assert not failures, f"{len(failures)} outputs differ from the exact expectation:\n" + "\n".join(failures)


@pytest.mark.parametrize("shape", cases.STEM_IMAGES, ids=[f"{n}x{h}x{w}" for n, h, w in cases.STEM_IMAGES])
def test_the_stem_equals_the_exact_expectation_bit_for_bit(shape):
    from posepaf import _lib, fused_model as fm
    L = _lib.load()
    n, h, w = shape
    failures = []
    for recipe in cr.RECIPES:
        label = f"stem {shape}"
        ops = cases.stem_operands(shape, cases.seed_of(label, recipe), recipe)
        want = cases.stem_expected(ops, recipe, label).cuda()
        conv = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=True)
        with torch.no_grad():
            conv.weight.copy_(ops["w"].float())
            conv.bias.copy_(ops["b"].float())
        stem = fm.FStem(conv, None, True).cuda().half()
        assert torch.equal(stem.weight.cpu(), ops["w"]) and torch.equal(stem.bias.cpu(), ops["b"])
        x = ops["x"].cuda()
        o = Out(n, 64, h // 2, w // 2)
        rc = L.pp_stem7x7_f16(_p(x), _p(stem.prepared), _p(stem.bias), _p(o.t), n, h, w, fm.LEAK,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0, f"{label} [{recipe}]: rc {rc}"
        assert o.intact() is None, f"{label} [{recipe}]: a store landed in {o.intact()}"
        msg = cr.first_bit_difference(o.t, want, f"{label} [{recipe}] pp_stem7x7_f16")
        if msg is None and recipe == "small":       # the product's call, which allocates its own output
            msg = cr.first_bit_difference(stem(x.permute(0, 3, 1, 2)), want, f"{label} [{recipe}] FStem.forward")
        if msg is not None:
            failures.append(msg)
    assert not failures, "\n".join(failures)


def test_the_sweep_ran_the_cells_of_the_offbench_rows_under_small():
    if len(_report) != len(SELECTION):
        pytest.skip(f"only {len(_report)} of the {len(SELECTION)} selected keys were swept in this session")
    for form in sorted({f for f, _ in _report.values()}):
        for recipe in cr.RECIPES:
            rows = [r[recipe] for f, r in _report.values() if f == form and recipe in r]
            if rows:
                print(f"{form} [{recipe}]: {len(rows)} keys, {sum(len(a) for a, _ in rows)} candidates ran, "
                      f"{sum(len(b) for _, b in rows)} refused")
    print("cells that ran under `small`:", sorted(_ran_cells))
    missing = [what for what, hit in WANTED if not any(hit(c) for c in _ran_cells)]
    assert not missing, f"no candidate of the sweep ran {missing} (cells that ran: {sorted(_ran_cells)})"


@pytest.mark.parametrize("mode", [0, 1], ids=["EX0", "EX1"])
def test_pw_lds_limit_holds_in_either_call_order(mode):
    """k_pw<8, 2, EX, false> at c_in = 256: 32 KiB of LDS at c_out = 64, 128 KiB at 256.  If the runtime enforces the limit the first
    call set, the larger second launch is refused (PP_ERR_HIP), and the tuner would drop the kernel silently."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pw_lds_order_child.py")
    for order in ("small-first", "large-first"):
        r = subprocess.run([sys.executable, child, order, str(mode)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, f"{order}, mode {mode}: the child ended with {r.returncode}\n{r.stdout}\n{r.stderr}"
        res = json.loads(r.stdout.strip().splitlines()[-1])
        print(res)
        assert res["rc"] == [0, 0], f"{order}, mode {mode}: return codes {res['rc']} at c_out {res['c_out']}"
        assert res["equal"] == [True, True] and res["intact"] == [True, True], res
