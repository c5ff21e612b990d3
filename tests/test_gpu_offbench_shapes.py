"""GPU: every kernel the per-shape tuner could pick, at the layer shapes of image geometries OFF the bench's 512 x 512, against
ground truth over the whole batch -- the protocol of tests/test_gpu_bench_shapes.py at the maps evaluate.py, demo_image.py and the
multi-scale path produce (any image padded to a multiple of 64: maps 16a x 16b down to a x b).  The keys are recorded, not typed:
profiles/conv_keys_offbench.json (tools/offbench_keys.py), one eager forward per row on an empty choice table.

What each row reaches (csrc/posepaf_conv_own.hip: halo_geometry, replayed by conv_reference.halo_cell; n counts samples):
  64 x 64    n 1, 2, 3  the smallest image, maps 16 .. 1; scale 0 is two stacked 16 x 16 images for n = 2, refused for odd n
  64 x 256   n 2, 4     16 x 64: the 64-wide tile, 2 tiles; 8 x 32: TWO images stacked on the 32-wide tile; dilated 64- / 32-wide
  128 x 192  n 2, 44    32 x 48: the 16-wide tile unstacked, 3 tiles; below, refused; n = 44: 132 tiles x 2 channel tiles = 272 ids
                        on a persistent grid of 256, some workgroups walk a second tile
  192 x 128  n 2        48 x 32: the 32-wide tile, 3 tile rows; 24 x 16: stacking refused (32 % 24)
  128 x 256  n 2, 4     32 x 64 / 16 x 32: 64- and 32-wide tiles; 8 x 16: FOUR stacked images for n = 4, refused for n = 2
  256 x 320  n 2        64 x 80: the 16-wide tile, 5 x 2 tiles; 32 x 40 and below refused; the pooled 1x1 forms refused at width 80
  384 x 384  n 2        96 x 96: the 32-wide tile, 18 tiles; 48 x 48 refused; pooled forms taken for c != 64, refused for c == 64
  256 x 384  n 2        (added) the collapsed upsample convolution walks the HALF-resolution grid, and 32 x 48 -- the input of scale
                        0's 64 x 96 -- is the only such grid of the set that is cut into unstacked 16-wide tiles
"posenet" at every row, "final" (the published variant) at n = 2 of 64 x 64, 128 x 192, 128 x 256 and 384 x 384.

Every candidate is launched whether or not the Python eligibility tests of FConv.forward_* would try it: a kernel that accepts a
shape must be right on it.  A plain key also gets candidate -1, MIOpen's convolution + the k_bias_act pass, which the product runs
where nothing else takes a shape (torch's convolution pinned to its deterministic algorithms, conv_candidates._miopen_bias_act:
MIOpen's default is not reproducible from call to call on these maps, and the two-runs comparison is about this library's
kernels); an `rmean` key, whose one-launch form the launcher can refuse by batch size, also gets the separate form on that path.
The float64 truth covers every pixel where n * H * W <= 4096, a stratified sample elsewhere.
The last test asserts that the named launcher cells really ran: a refusal must not silently empty the sweep."""
import zlib

import pytest
import torch

import conv_reference as cr
from conv_candidates import MIOPEN, REFUSED, _outputs, _view, candidates, cells

pytestmark = pytest.mark.gpu

ENTRIES = cr.table_entries(cr.OFFBENCH)
ROWS, LOOKUPS = cr.offbench_rows()
_ran_cells: set = set()          # launcher cells (conv_candidates.cells) of every candidate that ran
_report: dict = {}               # key id -> (ran, refused)
_models: dict = {}


def _row_id(r):
    return f"{r['arch']}-{r['image'][0]}x{r['image'][1]}-n{r['n']}"


@pytest.mark.parametrize("row", range(len(ROWS)), ids=[_row_id(r) for r in ROWS])
def test_the_key_file_lists_every_shape_of_the_row(row):
    """Census: with the file's entries installed, the first forward at the row's geometry (the one that runs every scale) records
    no key the file does not list, and looks up exactly the keys the file says the row looks up."""
    from posepaf import fused_model as fm
    saved = (fm._conv_choice, fm._conv_timing, fm._conv_calls)
    r = ROWS[row]
    (h, w), n = r["image"], r["n"]

    class Recording(dict):
        looked_up = set()

        def get(self, key, default=None):
            self.looked_up.add(key)
            return super().get(key, default)

    try:
        fm._conv_choice, fm._conv_timing, fm._conv_calls = Recording(), {}, {}
        fm.install_entries([[fm._key_to_json(k), v] for k, v in ENTRIES])
        before = set(fm._conv_choice)
        if r["arch"] not in _models:
            _models[r["arch"]] = fm.build_inference_model("cuda", arch=r["arch"])
        x = torch.rand((n, h, w, 3), generator=torch.Generator(device="cuda").manual_seed(1), device="cuda").half()
        with torch.no_grad():
            y = _models[r["arch"]](x)
        torch.cuda.synchronize()
        assert y.shape == (n, 50, h // 4, w // 4)
        new = set(fm._conv_choice) - before
        assert not new, (f"{_row_id(r)} tuned {len(new)} shapes profiles/conv_keys_offbench.json does not list: "
                         f"{sorted(map(str, new))}; regenerate it (tools/offbench_keys.py)")
        listed = {k for (k, _), rows in zip(ENTRIES, LOOKUPS) if row in rows}
        assert Recording.looked_up == listed, (f"{_row_id(r)}: looked up but not recorded for the row "
                                               f"{sorted(map(str, Recording.looked_up - listed))}, recorded but not looked up "
                                               f"{sorted(map(str, listed - Recording.looked_up))}")
    finally:
        fm._conv_choice, fm._conv_timing, fm._conv_calls = saved


@pytest.mark.parametrize("entry", ENTRIES, ids=[cr.key_id(k) for k, _ in ENTRIES])
def test_every_tuner_candidate_at_the_offbench_shapes_over_the_whole_batch(entry):
    key, _ = entry
    spec = cr.parse_key(key)                  # at the key's own batch size
    label = cr.key_id(key)
    ops = cr.make_operands(spec, seed=zlib.crc32(label.encode()), device="cuda")
    pix = cr.truth_pixels(spec.n, spec.H, spec.W)
    ref, at32 = cr.reference32(spec, ops, pix)
    # the fp32 reference is proven against float64 before it judges a kernel
    a64 = cr.acc64_at(spec, ops, pix)
    cr.assert_close(at32.double(), a64, cr.TOL_FP32 * max(1.0, float(a64.abs().max())), label + ": fp32 reference", pix)
    o64 = cr.outputs64_at(spec, ops, pix)
    qpix = cr.truth_pixels(spec.n, spec.H // 2, spec.W // 2) if spec.pooled else None
    p64 = cr.pooled64_at(spec, ops, qpix) if spec.pooled else None
    scale = {name: float(v.abs().max()) for name, v in ref.items()}
    nb = cr.chunk_images(spec)

    ran, refused = [], []
    for cand, tol, launch, shapes in candidates(spec, ops, miopen=True):
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
        _ran_cells.update(cells(spec, cand))
        del runs, first, second
    print(f"{label}: {len(ran)} candidates ran {ran}, refused {refused}")
    _report[label] = (ran, refused)
    assert ran, f"{label}: no candidate ran"


# the cells the rows were chosen for: (what, predicate on a cell name of conv_candidates.cells)
WANTED = [("the 16-wide tile unstacked, variant 104", lambda c: c == "halo104 tw16 x1"),
          ("the 16-wide tile unstacked, variant 106 (half channel tile)", lambda c: c == "halo106 tw16 x1"),
          ("the 16-wide tile unstacked, channel sums", lambda c: c == "sums tw16 x1"),
          ("the 16-wide tile unstacked, upsampled input", lambda c: c == "up tw16 x1"),
          ("the 16-wide tile unstacked, collapsed upsample convolution", lambda c: c == "collapsed tw16 x1"),
          ("two images stacked on the 32-wide tile", lambda c: c.endswith(" tw32 x2")),
          ("four images stacked on the 16-wide tile", lambda c: c.endswith(" tw16 x4")),
          ("the 64-wide dilated instance", lambda c: c == "halo104 tw64 x1 dil"),
          ("the 32-wide dilated instance", lambda c: c == "halo104 tw32 x1 dil"),
          ("k_conv_igemm at a map with W % 16 != 0", lambda c: c == "igemm ragged"),
          ("pp_pw_pool_f16 at 96 wide", lambda c: c == "pwpool W96"),
          ("pp_pw_pre_f16", lambda c: c == "pwpre"),
          ("the residual sums form", lambda c: c.startswith("rsums "))]


def test_the_sweep_ran_the_cells_the_rows_were_chosen_for():
    if len(_report) != len(ENTRIES):
        pytest.skip(f"only {len(_report)} of the file's {len(ENTRIES)} keys were swept in this session")
    for i, r in enumerate(ROWS):
        mine = [_report[cr.key_id(k)] for (k, _), rows in zip(ENTRIES, LOOKUPS) if i in rows]
        print(f"{_row_id(r)}: {len(mine)} keys, {sum(len(a) for a, _ in mine)} candidates ran, {sum(len(b) for _, b in mine)} refused")
    only = sorted(label for label, (ran, _) in _report.items() if ran == [MIOPEN])
    print(f"{len(only)} keys where only candidate -1 (MIOpen + k_bias_act) ran: {only}")
    print("cells that ran:", sorted(_ran_cells))
    missing = [what for what, hit in WANTED if not any(hit(c) for c in _ran_cells)]
    assert not missing, f"no candidate of the sweep ran {missing} (cells that ran: {sorted(_ran_cells)})"
