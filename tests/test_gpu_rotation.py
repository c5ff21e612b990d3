"""GPU: the test-time rotation search (utils/parse_skeletons.py rotation_search) against the NumPy restatement of
cv2.warpAffine (tests/rotation_reference.py) and the oracle's restatement of predict's other steps.  Bar: bit-equal, except
where the network runs twice (its output is compared with the tolerance the existing predict test uses)."""
import ctypes as C

import numpy as np
import pytest

from rotation_reference import warp_affine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _padded(h, w):
    return -(-h // 64) * 64, -(-w // 64) * 64


def _compose(oracle, net, pd, pr, img_h, img_w, n, m_rev, heat_acc, paf_acc, flip=True):
    """one entry of predict by composition: flip-average -> x4 bicubic -> warpAffine(M_rev) -> crop -> resize -> += v / n"""
    if m_rev is None:
        oracle.predict_accumulate(net, pd, pr, img_h, img_w, n, heat_acc, paf_acc, flip=flip)
        return
    heat, paf = oracle.flip_average(net, flip)
    for planar, acc in ((heat, heat_acc), (paf, paf_acc)):
        up = warp_affine(oracle.upsample4_hwc(planar), m_rev)
        ch, cw = up.shape[0] - pd, up.shape[1] - pr
        crop = up[:ch, :cw]
        for c in range(planar.shape[0]):
            v = oracle.resize_cubic(np.ascontiguousarray(crop[:, :, c]), img_w / cw, img_h / ch)
            assert v.shape == (img_h, img_w)
            acc[c] += (v / np.float32(n)).astype(np.float64)


@pytest.mark.parametrize("batch,h,w", [(3, 37, 50), (3, 64, 64), (1, 130, 71)])
def test_preprocess_affine_matches_the_numpy_warp(torch_cuda, batch, h, w):
    from posepaf.pipeline import preprocess_batch
    from posepaf.rotation import invert_affine, reference_center, rotation_matrix
    torch = torch_cuda
    img = np.random.default_rng(h * w).integers(0, 256, (batch, h, w, 3), dtype=np.uint8)
    hp, wp = _padded(h, w)
    pad = np.full((batch, hp, wp, 3), 128, np.uint8)
    pad[:, :h, :w] = img
    flt = np.float32(pad / 255)
    dimg = torch.from_numpy(img).cuda()
    for ang in (7.5, -30.0, 90.0, 180.0):
        m_in = invert_affine(rotation_matrix(reference_center(hp, wp), ang))
        want = np.stack([warp_affine(flt[b], m_in) for b in range(batch)])
        got = preprocess_batch(dimg, True, torch.float32, m_inv=m_in).cpu().numpy()
        assert got.shape == (2 * batch, hp, wp, 3)
        assert np.array_equal(got[0::2], want), ang
        assert np.array_equal(got[1::2], want[:, :, ::-1]), ang
        got16 = preprocess_batch(dimg, True, torch.float16, m_inv=m_in).cpu().numpy()
        assert np.array_equal(got16[0::2], want.astype(np.float16)), ang
        assert np.array_equal(got16[1::2], want[:, :, ::-1].astype(np.float16)), ang
        assert (got[0] == 0).any() and not (got[0] == np.float32(128 / 255)).all()   # black corners, not pad grey
        assert np.array_equal(preprocess_batch(dimg, False, torch.float32, m_inv=m_in).cpu().numpy(), want)


IMG_H, IMG_W = 120, 136
ENTRIES = [(s, a) for s in (0.5, 1.0, 1.5) for a in (0.0, 15.0)]


def _entries(dtype, seed=3, entries=ENTRIES, img_h=IMG_H, img_w=IMG_W):
    from posepaf.original_path import scaled_size
    from posepaf.rotation import input_and_map_inverses
    g = np.random.default_rng(seed)
    out = []
    for s, a in entries:
        sh, sw = scaled_size(img_h, img_w, s)
        hp, wp = _padded(sh, sw)
        net = (g.random((2, 2, 50, hp // 4, wp // 4)) * 0.8).astype(dtype)
        out.append((net, hp - sh, wp - sw, input_and_map_inverses(hp, wp, a)[1]))
    return out


def _accumulate(torch, post, entries, fused, img_h=IMG_H, img_w=IMG_W):
    from posepaf.original_path import OriginalPathProcessor
    proc = OriginalPathProcessor(post, img_h, img_w, 2)
    proc.fused = fused
    proc.reset()
    keep = []
    for net, pd, pr, m_rev in entries:
        keep.append(torch.from_numpy(net).cuda())
        proc.accumulate(keep[-1], pd, pr, len(entries), m_inv=m_rev)
    return proc.heat_acc.clone(), proc.paf_acc.clone()


@pytest.fixture(scope="module")
def post(torch_cuda):
    from posepaf.api import PosePostProcessor
    p = PosePostProcessor(max_batch=2, max_h=64, max_w=64, max_peaks_per_part=64)
    yield p
    p.close()


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_fused_rotated_accumulation_equals_the_composition(torch_cuda, oracle, post, dtype):
    entries = _entries(dtype)
    heat, paf = _accumulate(torch_cuda, post, entries, fused=True)
    heat, paf = heat.cpu().numpy(), paf.cpu().numpy()
    for b in range(2):
        hw = np.zeros((20, IMG_H, IMG_W)); pw = np.zeros((30, IMG_H, IMG_W))
        for net, pd, pr, m_rev in entries:
            _compose(oracle, net[b], pd, pr, IMG_H, IMG_W, len(entries), m_rev, hw, pw)
        assert np.array_equal(heat[b], hw) and np.array_equal(paf[b], pw), (dtype, b)
    assert float(np.abs(paf).max()) > 0.1


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_fused_rotated_accumulation_equals_the_chain(torch_cuda, post, dtype):
    entries = _entries(dtype, seed=11)
    fused = _accumulate(torch_cuda, post, entries, fused=True)
    chain = _accumulate(torch_cuda, post, entries, fused=False)
    assert torch_cuda.equal(fused[0], chain[0]) and torch_cuda.equal(fused[1], chain[1])
    # and the rotated entries change the result
    plain = _accumulate(torch_cuda, post, [(n, pd, pr, None) for n, pd, pr, _ in entries], fused=True)
    assert not torch_cuda.equal(fused[1], plain[1])


def test_an_entry_too_large_for_lds_falls_back_to_the_chain(torch_cuda, post):
    from posepaf import _lib
    torch = torch_cuda
    entries = _entries(np.float16, seed=5, entries=[(1.0, 0.0), (3.0, 45.0)], img_h=64, img_w=64)
    L = _lib.load()
    nets = [torch.from_numpy(n).cuda() for n, *_ in entries]
    acc_h = torch.zeros((2, 20, 64, 64), dtype=torch.float64, device="cuda")
    acc_p = torch.zeros((2, 30, 64, 64), dtype=torch.float64, device="cuda")
    dp = C.POINTER(C.c_double)
    mats = [None if m is None else np.ascontiguousarray(m.reshape(6)) for *_, m in entries]
    rc = L.pp_original_accumulate_all_affine(
        post.ctx, 2, 2, (C.c_void_p * 2)(*[t.data_ptr() for t in nets]), _lib.PP_F16,
        (C.c_int * 2)(*[t.shape[3] for t in nets]), (C.c_int * 2)(*[t.shape[4] for t in nets]), 1,
        (C.c_int * 2)(*[e[1] for e in entries]), (C.c_int * 2)(*[e[2] for e in entries]),
        (dp * 2)(*[dp() if m is None else m.ctypes.data_as(dp) for m in mats]), 64, 64,
        C.c_void_p(acc_h.data_ptr()), C.c_void_p(acc_p.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -6                                   # PP_ERR_UNSUPPORTED: the rotated scale-3 entry does not fit LDS
    fused = _accumulate(torch, post, entries, fused=True, img_h=64, img_w=64)
    chain = _accumulate(torch, post, entries, fused=False, img_h=64, img_w=64)
    assert torch.equal(fused[0], chain[0]) and torch.equal(fused[1], chain[1])
    assert float(fused[1].abs().max()) > 0.1


@pytest.fixture(scope="module")
def model(torch_cuda):
    from posepaf.fused_model import build_inference_model
    return build_inference_model(torch_cuda.device("cuda", 0))


def _forward(torch, model, x):
    from posepaf.fused_model import to_planes
    with torch.no_grad():
        out = model(x)
        return to_planes(out[-1][0] if isinstance(out, (list, tuple)) else out).float().cpu().numpy()


def test_predict_with_rotation_search(torch_cuda, oracle, model):
    from posepaf import skeleton as sk
    from posepaf.original_path import resize_images_u8
    from posepaf.pipeline import preprocess_batch
    from posepaf.rotation import input_and_map_inverses
    from utils import parse_skeletons as ps
    torch = torch_cuda
    cfg = dict(sk.default_test_cfg())
    cfg["rotation_search"] = [0, 15]
    cfg["multiplier"] = [1.0, 0.5]
    img = np.random.default_rng(4).integers(0, 256, (120, 200, 3), dtype=np.uint8)
    heat, paf = ps.predict(img, model, cfg, sk.default_model_cfg(), "x.jpg", flip_avg=True)
    assert heat.shape == (120, 200, 20) and heat.dtype == np.float64
    h0 = np.zeros((20, 120, 200)); p0 = np.zeros((30, 120, 200))
    for s in cfg["multiplier"]:
        scaled = resize_images_u8(torch.from_numpy(img).cuda()[None], s)
        sh, sw = scaled.shape[1:3]
        hp, wp = _padded(sh, sw)
        for a in cfg["rotation_search"]:
            m_in, m_rev = input_and_map_inverses(hp, wp, a)
            net = _forward(torch, model, preprocess_batch(scaled, True, torch.float16, m_inv=m_in))
            _compose(oracle, net.reshape(2, 50, hp // 4, wp // 4), hp - sh, wp - sw, 120, 200, 4, m_rev, h0, p0)
    assert np.allclose(heat, h0.transpose(1, 2, 0), rtol=0, atol=2e-2)
    assert np.allclose(paf, p0.transpose(1, 2, 0), rtol=0, atol=2e-2)


def test_predict_refactor_returns_the_last_angle_warped_at_feature_resolution(torch_cuda, oracle, model):
    from posepaf import skeleton as sk
    from posepaf.pipeline import preprocess_batch
    from posepaf.rotation import input_and_map_inverses
    from utils import parse_skeletons as ps
    torch = torch_cuda
    cfg = dict(sk.default_test_cfg())
    cfg["rotation_search"] = [0, 20]
    img = np.random.default_rng(6).integers(0, 256, (120, 200, 3), dtype=np.uint8)
    heat, paf = ps.predict_refactor(img, model, cfg, sk.default_model_cfg(), "x.jpg", flip_avg=True)
    assert heat.shape == (32, 64, 20) and paf.shape == (32, 64, 30) and heat.dtype == np.float32
    m_in, m_rev = input_and_map_inverses(128, 256, 20.0)      # centre of the padded INPUT, applied at feature resolution
    net = _forward(torch, model, preprocess_batch(torch.from_numpy(img).cuda()[None], True, torch.float16, m_inv=m_in))
    hw, pw = oracle.flip_average(net.reshape(2, 50, 32, 64).astype(np.float16))
    want_h = warp_affine(hw.transpose(1, 2, 0), m_rev)
    want_p = warp_affine(pw.transpose(1, 2, 0), m_rev)
    assert np.allclose(heat, want_h, rtol=0, atol=2e-2) and np.allclose(paf, want_p, rtol=0, atol=2e-2)
    # the warp itself, bit-exact on the GPU's own flip-average
    unrot = ps.predict_refactor(img, model, dict(cfg, rotation_search=[0]), sk.default_model_cfg(), "x.jpg")
    assert unrot[0].shape == heat.shape and not np.array_equal(unrot[0], heat)


def test_warp_kernel_hwc_and_planar_bit_exact(torch_cuda):
    from posepaf import _lib
    from posepaf.rotation import input_and_map_inverses
    torch = torch_cuda
    src = np.random.default_rng(8).standard_normal((2, 33, 47, 30)).astype(np.float32)
    m = input_and_map_inverses(128, 192, -12.5)[1]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    md = (C.c_double * 6)(*m.reshape(6))
    for hwc in (1, 0):
        arr = src if hwc else np.ascontiguousarray(src.transpose(0, 3, 1, 2))
        d_src = torch.from_numpy(arr).cuda()
        d_dst = torch.empty_like(d_src)
        n = 2 if hwc else 60
        _lib.check(_lib.load().pp_warp_affine_f32(C.c_void_p(d_src.data_ptr()), C.c_void_p(d_dst.data_ptr()), n, 33, 47, 30, hwc,
                                                  md, st))
        got = d_dst.cpu().numpy()
        if not hwc:
            got = got.transpose(0, 2, 3, 1)
        for b in range(2):
            assert np.array_equal(got[b], warp_affine(src[b], m)), hwc


class _PoolNet:
    """Stand-in network for the determinism check: 4 x 4 average pooling of the (rotated, mirrored) input mixed elementwise
    into 50 channels.  The real network's MIOpen fp16 convolutions may accumulate with atomics, so a random-weight network's
    noise-level output is not bit-reproducible between calls (tests/test_gpu_model.py, test_pipeline_end_to_end_runs)."""

    def __call__(self, x):
        import torch
        import torch.nn.functional as F
        p = F.avg_pool2d(x.permute(0, 3, 1, 2).float(), 4)
        k = torch.arange(50, device=x.device, dtype=torch.float32)
        return (p[:, k.long() % 3] * ((k + 1) / 50)[None, :, None, None]).to(x.dtype).contiguous()


def test_original_path_run_with_angles_is_deterministic(torch_cuda):
    from posepaf.api import PosePostProcessor
    from posepaf.original_path import OriginalPathProcessor
    torch = torch_cuda
    imgs = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (2, 128, 128, 3), dtype=np.uint8)).cuda()
    post = PosePostProcessor(max_batch=2, max_h=48, max_w=48, max_peaks_per_part=64)
    proc = OriginalPathProcessor(post, 128, 128, 2)
    net = _PoolNet()
    r1 = proc.run(net, imgs, [1.0, 0.5], angles=[0, 15])
    h1, p1 = proc.heat_acc.clone(), proc.paf_acc.clone()
    r2 = proc.run(net, imgs, [1.0, 0.5], angles=[0, 15])
    assert r1.tobytes() == r2.tobytes()
    assert torch.equal(h1, proc.heat_acc) and torch.equal(p1, proc.paf_acc)
    proc.run(net, imgs, [1.0, 0.5])
    assert not torch.equal(h1, proc.heat_acc)
    post.close()
