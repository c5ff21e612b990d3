"""CPU: the comparison of tests/test_gpu_offbench_shapes.py can tell a subtly wrong kernel from a right one at every recorded layer
key of the image geometries off the bench's (profiles/conv_keys_offbench.json), each at its own batch size -- the two tests of
tests/test_bench_shape_tolerance_cpu.py over those keys, the published variant's `rmean`, `pre` and `up2 ... nopost` included.
Per key: a "kernel" that drops ONE input channel at the centre tap over the last tile of the last image (conv_reference.tile_geometry:
the halo kernel's real tile where it takes the map) must be rejected, and the float64 truth rounded to fp16 must be accepted; the
fp32 and float64 references agree at the pixels the GPU test computes the truth at.  Also here: tile_geometry returns what it
returned before it followed halo_geometry for every key of the bench table, and the geometry the rows were chosen for."""
import pytest
import torch

import conv_reference as cr

ENTRIES = cr.table_entries(cr.OFFBENCH)
ROWS, LOOKUPS = cr.offbench_rows()
# a key shared between rows is checked once, with the first row that looks it up
BY_ROW = [[k for (k, _), rows in zip(ENTRIES, LOOKUPS) if rows[0] == i] for i in range(len(ROWS))]
ROW_IDS = [f"{r['arch']}-{r['image'][0]}x{r['image'][1]}-n{r['n']}" for r in ROWS]


def _tile_pix(spec):
    th, tw, tx = cr.tile_geometry(spec.H, spec.W)
    last = tx * (-(-spec.H // th)) - 1
    q = cr.tile_pixels(spec.H, spec.W, last)
    return torch.cat([torch.full((len(q), 1), spec.n - 1), q], 1)


def test_the_file_holds_the_rows_and_the_new_key_kinds():
    assert len(ENTRIES) == len(LOOKUPS) == len({k for k, _ in ENTRIES}) and sum(map(len, BY_ROW)) == len(ENTRIES)
    assert all(rows and all(0 <= i < len(ROWS) for i in rows) for rows in LOOKUPS)
    want = {("posenet", h, w, n) for h, w, ns in ((64, 64, (1, 2, 3)), (64, 256, (2, 4)), (128, 192, (2, 44)), (192, 128, (2,)),
                                                  (128, 256, (2, 4)), (256, 320, (2,)), (384, 384, (2,))) for n in ns}
    want |= {("final", h, w, 2) for h, w in ((64, 64), (128, 192), (128, 256), (384, 384))}
    have = {(r["arch"], r["image"][0], r["image"][1], r["n"]) for r in ROWS}
    assert want <= have and (512, 512) not in {(h, w) for _, h, w, _ in have}
    kinds = {k[0] if isinstance(k[0], str) else "plain" for k, _ in ENTRIES}
    assert kinds >= {"plain", "up2", "dual", "mean", "pool", "cat", "rmean", "pre"}
    assert any(k[0] == "up2" and k[-1] == "nopost" for k, _ in ENTRIES)
    for k, _ in ENTRIES:       # every key at its own n, and every key parses
        assert cr.parse_key(k).n == (k[1] if isinstance(k[0], str) else k[0])


def test_tile_geometry_is_unchanged_at_every_bench_key():
    """the rule before it followed halo_geometry: TW = min(W, 128), TH = min(512 / TW, H)"""
    bench = cr.table_entries()
    assert len(bench) == 71
    for key, _ in bench:
        s = cr.parse_key(key)
        tw = min(s.W, 128)
        assert cr.tile_geometry(s.H, s.W) == (max(1, min(512 // tw, s.H)), tw, -(-s.W // tw)), key


def test_tile_geometry_follows_the_halo_kernel_off_the_bench_maps():
    # (tile height, width, tiles per row): the 16-wide tile unstacked, the 32-wide one, stacked images, refused maps, one band
    for (H, W), want in {(32, 48): (32, 16, 3), (64, 80): (32, 16, 5), (96, 96): (16, 32, 3), (48, 32): (16, 32, 1),
                         (16, 64): (8, 64, 1), (64, 96): (16, 32, 3), (8, 32): (8, 32, 1), (8, 16): (8, 16, 1), (16, 16): (16, 16, 1),
                         (24, 16): (24, 16, 1), (16, 24): (16, 24, 1), (48, 48): (10, 48, 1), (32, 40): (12, 40, 1),
                         (12, 8): (12, 8, 1), (3, 2): (3, 2, 1), (1, 1): (1, 1, 1), (32, 192): (8, 64, 3)}.items():
        assert cr.tile_geometry(H, W) == want, (H, W)
    # halo_cell: (tile width, tile height, images per tile, tiles per image), None where the launcher refuses
    assert cr.halo_cell(2, 32, 48) == (16, 32, 1, 3) and cr.halo_cell(44, 32, 48) == (16, 32, 1, 3)
    assert cr.halo_cell(2, 8, 32) == (32, 16, 2, 1) and cr.halo_cell(3, 8, 32) is None
    assert cr.halo_cell(4, 8, 16) == (16, 32, 4, 1) and cr.halo_cell(2, 8, 16) is None
    assert cr.halo_cell(2, 16, 16) == (16, 32, 2, 1) and cr.halo_cell(1, 16, 16) is None and cr.halo_cell(3, 16, 16) is None
    assert cr.halo_cell(2, 24, 16) is None and cr.halo_cell(2, 48, 48) is None and cr.halo_cell(2, 16, 24) is None
    assert cr.halo_cell(2, 4, 16) is None                       # H % (128 / tw): a wave's 128 pixels would span two images
    assert cr.halo_cell(2, 16, 16, csum=True, mode=0) is None and cr.halo_cell(2, 16, 16, csum=True, mode=1) == (16, 32, 2, 1)
    assert cr.halo_cell(2, 16, 64, dil=5) == (64, 8, 1, 5) and cr.halo_cell(2, 8, 32, dil=3) == (32, 16, 1, 3)
    assert cr.halo_cell(2, 32, 48, dil=3) is None and cr.halo_cell(2, 16, 64, dil=2) is None
    # every real tile's first and last pixel of image 0 is in the sample
    pix = {tuple(p) for p in cr.sample_pixels(2, 32, 48).tolist()}
    assert {(0, 0, 0), (0, 31, 15), (0, 0, 16), (0, 31, 31), (0, 0, 32), (0, 31, 47)} <= pix
    # the float64 truth covers every pixel of a small map
    assert len(cr.truth_pixels(4, 8, 16)) == 4 * 8 * 16 and len(cr.truth_pixels(2, 32, 64)) == 4096
    assert len(cr.truth_pixels(2, 64, 80)) == len(cr.sample_pixels(2, 64, 80)) < 2 * 64 * 80


@pytest.mark.parametrize("row", range(len(ROWS)), ids=ROW_IDS)
def test_the_comparison_rejects_one_missing_term_and_accepts_fp16_rounding(row):
    torch.manual_seed(0)
    strengthened, report = [], []
    for key in BY_ROW[row]:
        spec = cr.parse_key(key)
        ops = cr.make_operands(spec, seed=11)
        ref32, _ = cr.reference32(spec, ops)
        tol = cr.TOL_COLLAPSED if spec.up else cr.TOL            # the looser of the form's candidates
        bound = cr.bound_for(ref32["y"].abs().max(), tol)
        pix = _tile_pix(spec)
        exact = cr.outputs64_at(spec, ops, pix)["y"]
        label = f"{cr.key_id(key)} (n = {spec.n})"
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
    assert len(report) == len(BY_ROW[row])


@pytest.mark.parametrize("row", range(len(ROWS)), ids=ROW_IDS)
def test_the_float64_and_fp32_references_agree_at_the_truth_pixels(row):
    """The two references of the GPU test, on the CPU: conv + bias of the fp32 pass within 1e-5 of float64 at every pixel the GPU
    test takes the truth at, and every output (pooled and channel-mean forms included) within the kernel tolerance of float64."""
    for key in BY_ROW[row]:
        spec = cr.parse_key(key)
        ops = cr.make_operands(spec, seed=12)
        pix = cr.truth_pixels(spec.n, spec.H, spec.W)
        ref32, at32 = cr.reference32(spec, ops, pix, chunk=1)
        a64 = cr.acc64_at(spec, ops, pix)
        label = cr.key_id(key)
        cr.assert_close(at32.double(), a64, cr.TOL_FP32 * max(1.0, float(a64.abs().max())), label + " fp32 conv", pix)
        o64 = cr.outputs64_at(spec, ops, pix)
        for name in [o for o in spec.outputs() if o in o64]:
            bound = cr.bound_for(ref32[name].abs().max())
            cr.assert_close(cr.values_at(ref32[name], pix), o64[name], bound, f"{label} {name}", pix)
        if spec.pooled:
            q = cr.truth_pixels(spec.n, spec.H // 2, spec.W // 2)
            cr.assert_close(cr.values_at(ref32["pool"], q), cr.pooled64_at(spec, ops, q), cr.bound_for(ref32["pool"].abs().max()),
                            label + " pool", q)
        if spec.has_mean:
            assert ref32["mean"].shape == (spec.n, spec.k)
