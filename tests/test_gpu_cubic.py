"""GPU: every kernel that resamples bicubically against the independent float64 reference (tests/cubic_reference.py, pinned
to torch's float64 bicubic by test_cubic_reference_cpu.py) -- not against the oracle, which was written from the same
reading of resize.cpp as the kernels.  The tolerances are those of a float32 implementation against the reference
(cubic_reference.DYADIC_TOL / GENERAL_TOL); the negative controls of the CPU module show that a wrong constant, centre
convention, tap window or phase table misses them by more than 1000x.

  accumulators  k_accumulate_scales (fused), the k_resize_cubic chain, the ragged launch
  image resize  k_resize_u8, k_resize_u8_ragged
  K_A           the x4 peak-patch refinement, maps staged in LDS and maps kept in device memory
  K_B           the on-the-fly x4 limb-map sample (bicubic4_at, d_cubic4)"""
import numpy as np
import pytest

import cubic_reference as cr
import ragged_cases as rc
from conftest import load_scene
from test_gpu_parity import SCORE_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


# ---- a. accumulators

@pytest.mark.parametrize("fused", [True, False], ids=["fused", "chain"])
@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("flip", [True, False], ids=["flip", "noflip"])
def test_accumulators_against_the_reference(torch_cuda, fused, dtype, flip):
    """a batch of two different images; proc.fused picks k_accumulate_scales or the per-scale k_resize_cubic chain (only the
    chain allocates the x4 scratch maps, which is how the test knows which one ran)"""
    from posepaf.api import PosePostProcessor
    from posepaf.original_path import OriginalPathProcessor
    torch = torch_cuda
    post = PosePostProcessor(max_batch=2, max_h=24, max_w=36, max_peaks_per_part=64)
    try:
        for name, (H, W), entries in cr.PREDICT_CASES:
            inputs = [cr.predict_inputs(entries, dtype, flip, seed) for seed in (77, 78)]
            proc = OriginalPathProcessor(post, H, W, 2)
            proc.fused = fused
            proc.reset()
            keep = []
            for k, (_, (pd, pr)) in enumerate(inputs[0]):
                keep.append(torch.from_numpy(np.stack([inputs[b][k][0] for b in range(2)])).cuda())
                proc.accumulate(keep[-1], pd, pr, len(entries), flip=flip)
            heat, paf = proc.heat_acc.cpu().numpy(), proc.paf_acc.cpu().numpy()
            assert bool(proc._scratch) == (not fused), "the other accumulation ran"
            for b in range(2):
                want_h, want_p = np.zeros((20, H, W)), np.zeros((30, H, W))
                for net, (pd, pr) in inputs[b]:
                    h_, p_ = cr.predict_entry(net, pd, pr, H, W, len(entries), flip)
                    want_h += h_
                    want_p += p_
                err = max(float(np.abs(heat[b] - want_h).max()), float(np.abs(paf[b] - want_p).max()))
                print(f"{name}, image {b}: {err:.3g}")
                assert err <= cr.GENERAL_TOL, (name, b)
    finally:
        post.close()


def test_ragged_accumulators_against_the_reference(torch_cuda):
    """one ragged bucket of two image sizes (tests/ragged_cases.py): each image cropped and resized at its own size"""
    from posepaf.api import PosePostProcessor
    from posepaf.original_path import OriginalPathProcessor, RaggedBucket
    torch = torch_cuda
    picks = [0, 2]                                             # (120, 100) and (97, 115): neither fills its slot
    sizes = [rc.SIZES[k] for k in picks]
    per_image = [rc.scene_maps(rc.SIZES[k], *rc.SCENES[k], np.float16) for k in picks]
    post = PosePostProcessor(max_batch=2, max_h=48, max_w=48, max_peaks_per_part=64)
    try:
        rg = RaggedBucket(sizes, rc.SCALES, torch.device("cuda", post.device))
        proc = OriginalPathProcessor(post, None, None, 2, slot_area=rg.slot_area)
        proc.reset(rg)
        maps = [torch.from_numpy(np.stack([m[i] for m in per_image])).cuda() for i in range(len(rc.SCALES))]
        for i, m in enumerate(maps):
            proc.accumulate(m, *rg.pads(i), len(maps))
        for b, (h, w) in enumerate(sizes):
            want_h, want_p = np.zeros((20, h, w)), np.zeros((30, h, w))
            for net, (pd, pr) in zip(per_image[b], rc.pads((h, w))):
                h_, p_ = cr.predict_entry(net, pd, pr, h, w, len(rc.SCALES), True)
                want_h += h_
                want_p += p_
            err = max(float(np.abs(proc.heat_view(b).cpu().numpy() - want_h).max()),
                      float(np.abs(proc.paf_view(b).cpu().numpy() - want_p).max()))
            print(f"ragged image {b} {(h, w)}: {err:.3g}")
            assert err <= cr.GENERAL_TOL, b
            assert float(np.abs(want_h).max()) > 0.3
    finally:
        post.close()


# ---- b. image resize

@pytest.mark.parametrize("scale", cr.U8_SCALES)
def test_image_resize_against_real_arithmetic(torch_cuda, scale):
    """k_resize_u8 on a batch of two, and k_resize_u8_ragged on a bucket of a 50 x 66 and a 49 x 65 image (one padded shape
    at every scale of the list; 49 * 1.5 and 65 * 1.5 round half to even)"""
    from posepaf.original_path import RaggedBucket, resize_images_u8, scaled_size
    torch = torch_cuda
    imgs = cr.u8_images()
    batch = np.stack([imgs["noise"], imgs["smooth"]])
    got = resize_images_u8(torch.from_numpy(batch).cuda(), scale).cpu().numpy()
    for b, name in enumerate(("noise", "smooth")):
        cr.assert_u8_close(got[b], batch[b], scale, f"{name} x{scale}")
    small = np.ascontiguousarray(imgs["noise"][1:50, 1:66])
    slots = np.full((2, 50, 66, 3), 0xA5, np.uint8)
    slots[0] = imgs["smooth"]
    slots[1, :49, :65] = small
    dev = torch.from_numpy(slots).cuda()
    rg = RaggedBucket([(50, 66), (49, 65)], [scale], dev.device)
    out = torch.full((2,) + rg.key[0] + (3,), 0x3C, dtype=torch.uint8, device=dev.device)
    got = resize_images_u8(dev, scale, ragged=rg, out=out).cpu().numpy()
    for b, (name, img) in enumerate((("smooth, ragged", imgs["smooth"]), ("noise 49 x 65, ragged", small))):
        dh, dw = scaled_size(img.shape[0], img.shape[1], scale)
        cr.assert_u8_close(got[b, :dh, :dw], img, scale, f"{name} x{scale}")
        assert (got[b, dh:] == 0x3C).all() and (got[b, :, dw:] == 0x3C).all()


# ---- c. K_A

def _ka_maps(dtype):
    from posepaf import synth
    return [("corner / edge 24x32", cr.corner_edge_map(dtype=dtype), False),
            ("16x24", synth.make_net_output(2, 11, h=16, w=24, dtype=dtype), True),
            ("40x56", synth.make_net_output(5, 12, h=40, w=56, dtype=dtype), True)]


@pytest.mark.parametrize("residency", ["auto", "hbm"], ids=["lds", "hbm"])
@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["f16", "f32"])
def test_peak_refinement_against_the_reference(torch_cuda, oracle, residency, dtype):
    """every refined peak on the reference's arg-max pixel of its clipped patch (replication at the PATCH edge), score within
    DYADIC_TOL.  The integer peaks come from the unrefined NMS, which the reference's own outputs pin (golden G1 / G2)."""
    from posepaf.api import PosePostProcessor
    torch = torch_cuda
    post = PosePostProcessor(max_batch=1, max_h=40, max_w=56, max_peaks_per_part=64)
    try:
        post.set_map_residency(residency)
        for name, net, flip in _ka_maps(dtype):
            h, w = net.shape[-2:]
            assert post.map_residency(dtype, h, w) == ("lds" if residency == "auto" else "hbm")
            heat, _ = cr.flip_average(net, flip)
            jl0, _ = oracle.heatmap_nms(heat, 4, refine=False)
            assert len(jl0) >= 18
            got = post.nms(torch.from_numpy(net).cuda()[None], flip=flip, refine=True)[0]
            gap = cr.assert_refined_peaks(got, jl0, heat, f"{name} {residency}")
            assert gap > 4 * cr.DYADIC_TOL, "the scene has a tie the reference itself cannot decide: pick another"
    finally:
        post.set_map_residency("auto")
        post.close()


# ---- d. K_B

@pytest.mark.parametrize("key", ["P6_s0_f16", "P15_s1_f32"])
def test_limb_scores_against_the_reference_map(torch_cuda, oracle, key):
    """K_B samples the x4 limb map on the fly; the oracle's process_paf, given the REFERENCE's x4 map, must connect the same
    peak pairs with scores within SCORE_TOL"""
    from posepaf.api import PosePostProcessor
    torch = torch_cuda
    net, g = load_scene(key)
    _, paf = cr.flip_average(net)
    up = np.ascontiguousarray(cr.upsample4(paf).transpose(1, 2, 0), np.float32)
    want = oracle.process_paf(g["joint_list"][None], up, 512)
    assert not want["sort_oob"]
    post = PosePostProcessor(max_batch=1, max_h=128, max_w=128, max_peaks_per_part=64)
    try:
        rec = post.process(torch.from_numpy(net).cuda()[None], 512)[0]
        assert rec["status"] == 0
        total, worst = 0, 0.0
        for limb in range(30):
            got = post.read_connections(0, limb)
            exp = np.array([(c[0], c[1], c[2], c[5]) for c in want["connections"][limb]], np.float64).reshape(-1, 4)
            assert len(got) == len(exp), limb
            got = got[np.lexsort((got[:, 1], got[:, 0]))].astype(np.float64)
            exp = exp[np.lexsort((exp[:, 1], exp[:, 0]))]
            assert np.array_equal(got[:, :2], exp[:, :2]), limb
            if len(got):
                worst = max(worst, float(np.abs(got[:, 2] - exp[:, 2]).max()))
            total += len(got)
        print(f"{key}: {total} connections, score error max {worst:.3g}")
        assert total >= 30 and worst <= SCORE_TOL
        n = int(rec["n_humans"])
        assert np.array_equal(rec["humans"]["peak_id"][:n], want["ids"])
    finally:
        post.close()
