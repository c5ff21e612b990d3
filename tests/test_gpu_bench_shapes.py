"""GPU: every kernel the per-shape tuner could pick, at every layer shape of the bench geometry (512 x 512, 256 samples = 128 images
and their flips; profiles/conv_choice_b128.json) and at the batch-1-with-flip geometry (2 samples), against ground truth over the
WHOLE batch.  Which candidate wins a shape changes from box to box inside the timing noise, so any candidate that takes a shape
can end up in the product.

Per key and candidate: the whole output (and the second / pooled / channel-mean output where the form has one) against an fp32
torch.nn.functional reference that is itself checked against float64 at a stratified pixel sample (tests/conv_reference.py), the
sample against float64 directly, two runs bit-identical, outputs pre-filled with NaN so that an unwritten element fails, and every
output a view into a buffer with a 64 KiB NaN guard on both sides (and, for a channel slice, the other channels of the wider
tensor) that must come back intact.  The plain keys run through FConv._fused_launch, the product's own argument marshalling;
the other forms allocate their outputs themselves in posepaf/fused_model.py, so their C entry points are called here with the
NaN-filled guarded outputs instead -- an element a kernel never writes cannot hold an earlier candidate's value."""
import json
import zlib

import pytest
import torch

import conv_reference as cr
from conv_candidates import REFUSED, _outputs, _view, candidates      # (shared with tests/test_gpu_offbench_shapes.py)

pytestmark = pytest.mark.gpu

ENTRIES = cr.table_entries()


def test_the_table_lists_every_shape_of_the_bench_geometry():
    """Census: with the committed table installed, one forward of the bench model (256 x 512 x 512 x 3) tunes no new shape -- the
    sweep below covers every shape the bench runs."""
    from posepaf import fused_model as fm
    saved = (fm._conv_choice, fm._conv_timing, fm._conv_calls)

    class Recording(dict):
        looked_up = set()

        def get(self, key, default=None):
            self.looked_up.add(key)
            return super().get(key, default)

    try:
        fm._conv_choice, fm._conv_timing, fm._conv_calls = Recording(), {}, {}
        fm.install_entries(json.load(open(cr.TABLE))["entries"])   # (the library hash it was tuned on does not matter here)
        before = set(fm._conv_choice)
        model = fm.build_inference_model("cuda")
        x = torch.rand((256, 512, 512, 3), generator=torch.Generator(device="cuda").manual_seed(1), device="cuda").half()
        with torch.no_grad():
            y = model(x)
        torch.cuda.synchronize()
        assert y.shape == (256, 50, 128, 128)
        new = set(fm._conv_choice) - before
        assert not new, (f"the bench geometry tuned {len(new)} shapes the committed table does not list: {sorted(map(str, new))}; "
                         "regenerate profiles/conv_choice_b128.json (bench.py at 128 images, fused_model.save_table)")
        # (keys not looked up here are the inner convolutions of fused forms: the tuner times them on the way, see forward_up2)
        print(f"{len(before - Recording.looked_up)} of {len(before)} table keys are not looked up with every choice installed")
    finally:
        fm._conv_choice, fm._conv_timing, fm._conv_calls = saved


@pytest.mark.parametrize("samples", [256, 2])
@pytest.mark.parametrize("entry", ENTRIES, ids=[cr.key_id(k) for k, _ in ENTRIES])
def test_every_tuner_candidate_at_the_bench_shapes_over_the_whole_batch(entry, samples):
    key, committed = entry
    spec = cr.parse_key(key, n=samples)
    label = f"{cr.key_id(key)} at n = {samples}"
    ops = cr.make_operands(spec, seed=zlib.crc32(label.encode()), device="cuda")
    pix = cr.sample_pixels(spec.n, spec.H, spec.W)
    ref, at32 = cr.reference32(spec, ops, pix)
    # the fp32 reference is proven against float64 before it judges a kernel
    a64 = cr.acc64_at(spec, ops, pix)
    cr.assert_close(at32.double(), a64, cr.TOL_FP32 * max(1.0, float(a64.abs().max())), label + ": fp32 reference", pix)
    o64 = cr.outputs64_at(spec, ops, pix)
    qpix = cr.sample_pixels(spec.n, spec.H // 2, spec.W // 2) if spec.pooled else None
    p64 = cr.pooled64_at(spec, ops, qpix) if spec.pooled else None
    scale = {name: float(v.abs().max()) for name, v in ref.items()}
    nb = cr.chunk_images(spec)

    ran, refused = [], []
    for cand, tol, launch, shapes in candidates(spec, ops):
        runs = []
        for rep in range(2):
            o = _outputs(spec, shapes)
            rc = launch({name: v.t if name != "mean" else v.t[:, :, 0, 0] for name, v in o.items()})
            torch.cuda.synchronize()
            if rc in REFUSED and rep == 0:
                break
            assert rc == 0, f"{label} candidate {cand}: rc {rc}"
            runs.append(o)
        if not runs:
            refused.append(cand)
            continue
        ran.append(cand)
        first, second = runs
        for name in shapes:
            what = f"{label} candidate {cand} output {name}"
            for o in (first[name], second[name]):
                hit = o.intact()
                assert hit is None, f"{what}: a store landed in {hit}"
            got, bound = _view(spec, name, first[name]), cr.bound_for(scale[name], tol)
            for i0 in range(0, spec.n, nb):
                cr.assert_close(got[i0:i0 + nb], ref[name][i0:i0 + nb], bound, what, img0=i0)
            if name in o64:
                cr.assert_close(cr.values_at(got, pix), o64[name], bound, what + " (float64 sample)", pix)
            elif name == "pool":
                cr.assert_close(cr.values_at(got, qpix), p64, bound, what + " (float64 sample)", qpix)
            assert torch.equal(got, _view(spec, name, second[name])), f"{what}: two runs differ (race?)"
        del runs, first, second
    print(f"{label}: {len(ran)} candidates ran {ran}, refused {refused}, committed {committed}")
    assert ran, f"{label}: no candidate ran"
    if spec.form == "plain" or committed != 0:     # 0 of a fused form = its separate path: plain keys of the table
        assert committed in ran, f"{label}: the committed choice {committed} did not run (ran {ran}, refused {refused})"
