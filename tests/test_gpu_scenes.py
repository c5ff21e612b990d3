"""GPU: pp_render_scenes (csrc/posepaf_synth.hip) against the float64 restatement of the reference's training-target recipe
(tests/scene_reference.py, pinned to the reference's own Heatmapper by tests/test_scene_reference_cpu.py), its mirrored sample,
background channels and noise, and the engine / evaluate.py plumbing that renders one scene per image inside the batch's graph.

Tolerances (fixed by the number formats, not by what the kernel gives):
  fp32   1e-6 absolute outside the floor mask: values are <= 1, half a float32 ulp at 1 is 6e-8, and a few-ulp expf on an
         argument <= 4.2, the product and the division stay within ~16 of those
  fp16   2^-11 |ref| + 1e-6: one binary16 rounding of a value that was within 1e-6
  mask   pixels with a limb contribution within 0.015 (1 +- 1e-4) of the floor's step, at most 1e-4 of a scene's limb pixels
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scene_cases
import scene_reference as ref
from conftest import PKG

pytestmark = pytest.mark.gpu
GUARD = 4096                     # elements behind the output that no launch may touch
SENTINEL = -7.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_REF = {}


def reference_batch(h, w):
    """(people of the four images, float64 (4, 2, 50, h, w) with channel 49 left zero, mask (4, 2, 50, h, w)): computed once"""
    if (h, w) not in _REF:
        people = scene_cases.batch_people(h, w)
        maps, masks = [], []
        for pj in people:
            m, k = ref.render(pj, h, w)
            k50 = ref.full_mask(k)
            assert ref.masked_share(k) <= ref.MASK_CAP
            maps.append(np.stack([m, ref.mirror(m)]))
            masks.append(np.stack([k50, ref.mirror_mask(k50)]))
        want, mask = np.stack(maps), np.stack(masks)
        want.setflags(write=False)
        mask.setflags(write=False)
        _REF[(h, w)] = (people, want, mask)
    return _REF[(h, w)]


def upload(torch, people, max_people):
    from posepaf import synth_device
    joints, n = synth_device.pack_joints(people, max_people)
    return torch.from_numpy(joints).cuda(), torch.from_numpy(n).cuda()


def render_raw(torch, joints, n, h, w, n_samples=2, dtype=None, flags=0, sigma=0.0, seed=0, ids=None):
    """pp_render_scenes through ctypes into a buffer with a sentinel-filled guard behind it -> (output numpy, guard intact)"""
    from posepaf import _lib
    dtype = dtype or torch.float32
    b = joints.shape[0]
    count = b * n_samples * 50 * h * w
    buf = torch.full((count + GUARD,), SENTINEL, dtype=dtype, device="cuda")
    _lib.check(_lib.load().pp_render_scenes(
        C.c_void_p(joints.data_ptr()), C.c_void_p(n.data_ptr()), C.c_void_p(ids.data_ptr()) if ids is not None else None, b,
        joints.shape[1], h, w, n_samples, _lib.PP_F16 if dtype == torch.float16 else _lib.PP_F32, flags, sigma, seed,
        C.c_void_p(buf.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return host[:count].reshape(b, n_samples, 50, h, w), bool((host[count:] == SENTINEL).all())


@pytest.mark.parametrize("h,w", scene_cases.SHAPES)
def test_fp32_and_fp16_match_the_restatement(torch_cuda, h, w):
    """0, 1, 9 and 12 people in one batch (tests/scene_cases.py: borders on all four sides, off-frame people, ties, a zero-length
    limb, coincident limbs; joint flags 0, 1 and 2), both samples, launch flags 0 / 1 / 2.
    Measured on the MI355X, max |fp32 - restatement| outside the mask: 8.9e-8 (16 x 24), 9.1e-8 (33 x 47), 9.3e-8 (128 x 128), no
    pixel masked; fp16 stays 9.8e-7 inside its bound."""
    from posepaf import synth_device
    torch = torch_cuda
    people, want, mask = reference_batch(h, w)
    joints, n = upload(torch, people, scene_cases.BATCH_MAX_PEOPLE)
    assert n.cpu().tolist() == [0, 1, 9, scene_cases.BATCH_MAX_PEOPLE]
    for b in (2, 3):   # the joint flag takes 0, 1 and 2 in the edge scene and in the crowd: "< 2 means annotated", 0 included
        assert set(np.unique(people[b][:, :, 2]).tolist()) == {0.0, 1.0, 2.0} and (people[b][:, :, 2] == 0).sum() >= 6
    got32, intact = render_raw(torch, joints, n, h, w)
    assert intact
    err = ref.max_err_outside(got32, want, mask)
    print(f"{h}x{w}: fp32 max err outside the mask {err:.3e}; masked share {ref.masked_share(mask[:, :, :30]):.2e}; "
          f"inside the mask {float(np.abs(got32 - want)[mask].max()) if mask.any() else 0.0:.3e}")
    assert err <= ref.TOL
    assert not got32[0].any() and got32[2].max() > 0.99          # no people: zeros; the edge scene has peaks
    # the wrapper gives the same bytes
    via = synth_device.render_scenes(joints, n, h, w, dtype=torch.float32)
    assert via.shape == (4, 2, 50, h, w) and np.array_equal(via.cpu().numpy(), got32)
    # flags: bit 1 (PP_SCENE_REVERSE_KP) fills channel 49 only; reserved bits change nothing
    rev, intact = render_raw(torch, joints, n, h, w, flags=1)
    assert intact and np.array_equal(rev[:, :, :49], got32[:, :, :49])
    assert np.array_equal(rev[:, :, 49], rev[:, :, 30:48].max(axis=2)) and rev[2, 0, 49].max() > 0.99
    assert not rev[:, :, 48].any() and not got32[:, :, 48:].any()
    other, intact = render_raw(torch, joints, n, h, w, flags=2)
    assert intact and np.array_equal(other, got32)
    # fp16: one rounding of the same values
    got16, intact = render_raw(torch, joints, n, h, w, dtype=torch.float16)
    assert intact
    excess = np.abs(got16.astype(np.float64) - want) - (2.0 ** -11 * np.abs(want) + 1e-6)
    excess[mask] = -1.0
    print(f"{h}x{w}: fp16 worst excess over 2^-11 |ref| + 1e-6: {float(excess.max()):.3e}")
    assert excess.max() <= 0.0
    assert np.array_equal(got16, got32.astype(np.float16))           # the same float32 value, rounded once
    rev16, _ = render_raw(torch, joints, n, h, w, dtype=torch.float16, flags=1)
    assert np.array_equal(rev16[:, :, 49], rev16[:, :, 30:48].max(axis=2)) and not rev16[:, :, 48].any()


@pytest.mark.parametrize("h,w", scene_cases.SHAPES[:2])
@pytest.mark.parametrize("half", (False, True))
def test_mirrored_sample_and_single_sample(torch_cuda, h, w, half):
    """sample 1 is the channel-permuted mirror of sample 0 byte for byte; n_samples = 1 gives sample 0 and stays in its extent"""
    torch = torch_cuda
    dtype = torch.float16 if half else torch.float32
    people, _, _ = reference_batch(h, w)
    joints, n = upload(torch, people, scene_cases.BATCH_MAX_PEOPLE)
    for flags in (0, 1):
        both, intact = render_raw(torch, joints, n, h, w, dtype=dtype, flags=flags)
        assert intact
        for b in range(4):
            assert np.array_equal(both[b, 1], ref.mirror(both[b, 0])), (b, flags)
        one, intact = render_raw(torch, joints, n, h, w, n_samples=1, dtype=dtype, flags=flags)
        assert intact and np.array_equal(one[:, 0], both[:, 0])


def test_sixty_four_people_fit(torch_cuda):
    """the documented capacity: 64 people of one image staged in LDS, against the restatement; 65 are refused"""
    from posepaf import _lib
    torch = torch_cuda
    h = w = 64
    people = [scene_cases.random_people(64, 77, h, w), scene_cases.random_people(3, 78, h, w)]
    joints, n = upload(torch, people, 64)
    got, intact = render_raw(torch, joints, n, h, w, n_samples=1)
    assert intact
    for b in range(2):
        m, k = ref.render(people[b], h, w)
        assert ref.masked_share(k) <= ref.MASK_CAP
        err = ref.max_err_outside(got[b, 0], m, ref.full_mask(k))
        print(f"{people[b].shape[0]} people at 64x64: fp32 max err {err:.3e}")
        assert err <= ref.TOL
    big = torch.zeros((1, 65, 18, 3), dtype=torch.float32, device="cuda")
    out = torch.zeros(50 * 8 * 8, dtype=torch.float32, device="cuda")
    rc = _lib.load().pp_render_scenes(C.c_void_p(big.data_ptr()), C.c_void_p(n.data_ptr()), None, 1, 65, 8, 8, 1, _lib.PP_F32, 0, 0.0,
                                      0, C.c_void_p(out.data_ptr()), None)
    assert rc == -6                                                # PP_ERR_UNSUPPORTED


def test_noise_is_counter_based(torch_cuda):
    """same (seed, scene ids) -> same bytes, in any launch, batch composition and slot; other ids -> other noise; the moments
    of out(noise) - out(0) over N = 4 * 2 * 50 * 33 * 47 values are a normal's within 4 standard errors; noise = 0 is the
    noiseless call"""
    from posepaf import synth_device
    torch = torch_cuda
    h, w, sigma, seed = 33, 47, 0.05, 1234
    people, _, _ = reference_batch(h, w)
    joints, n = upload(torch, people, scene_cases.BATCH_MAX_PEOPLE)
    ids = torch.tensor([10, 11, 12, 13], dtype=torch.int64, device="cuda")
    clean, _ = render_raw(torch, joints, n, h, w)
    a1, intact = render_raw(torch, joints, n, h, w, sigma=sigma, seed=seed, ids=ids)
    a2, _ = render_raw(torch, joints, n, h, w, sigma=sigma, seed=seed, ids=ids)
    assert intact and np.array_equal(a1, a2)
    # another composition: two of the images, other slots, another batch size (another launch geometry)
    j2, n2 = upload(torch, [people[3], people[0]], scene_cases.BATCH_MAX_PEOPLE)
    b1, intact = render_raw(torch, j2, n2, h, w, sigma=sigma, seed=seed, ids=torch.tensor([13, 10], dtype=torch.int64, device="cuda"))
    assert intact and np.array_equal(b1[0], a1[3]) and np.array_equal(b1[1], a1[0])
    j3, n3 = upload(torch, [people[1]] * 5 + [people[2]], scene_cases.BATCH_MAX_PEOPLE)
    c1, _ = render_raw(torch, j3, n3, h, w, sigma=sigma, seed=seed,
                       ids=torch.tensor([1, 2, 3, 11, 4, 12], dtype=torch.int64, device="cuda"))
    assert np.array_equal(c1[3], a1[1]) and np.array_equal(c1[5], a1[2])
    assert not np.array_equal(c1[0], c1[1])                        # the same scene under another id: other noise
    # without ids the id is the image's index
    d1, _ = render_raw(torch, joints, n, h, w, sigma=sigma, seed=seed)
    d2, _ = render_raw(torch, joints, n, h, w, sigma=sigma, seed=seed, ids=torch.arange(4, dtype=torch.int64, device="cuda"))
    assert np.array_equal(d1, d2) and not np.array_equal(d1, a1)
    e1, _ = render_raw(torch, joints, n, h, w, sigma=sigma, seed=seed + 1, ids=ids)
    assert not np.array_equal(e1, a1)
    # fp16 output: the same noise, rounded once
    f1, _ = render_raw(torch, joints, n, h, w, dtype=torch.float16, sigma=sigma, seed=seed, ids=ids)
    assert np.array_equal(f1, a1.astype(np.float16))
    # moments (the noise reaches every channel and both samples, and is not clipped)
    diff = a1.astype(np.float64) - clean.astype(np.float64)
    N = diff.size
    assert N == 4 * 2 * 50 * 33 * 47
    mean, std = float(diff.mean()), float(diff.std())
    print(f"noise: N {N}, mean {mean:.3e} (bound {4 * sigma / np.sqrt(N):.3e}), std {std:.6f} (sigma {sigma}, bound "
          f"{4 * sigma / np.sqrt(2 * N):.3e}); min {diff.min():.3f} max {diff.max():.3f}")
    assert abs(mean) <= 4 * sigma / np.sqrt(N)
    assert abs(std - sigma) <= 4 * sigma / np.sqrt(2 * N)
    assert a1.min() < 0.0 and a1.max() > 1.0                       # no second clip
    # noise = 0
    z = synth_device.render_scenes(joints, n, h, w, dtype=torch.float32, noise=0.0, seed=seed, scene_ids=ids)
    assert np.array_equal(z.cpu().numpy(), clean)


class _TinyModel:
    """a deterministic stand-in network: NHWC fp16 image batch -> (N, 50, h / 4, w / 4) fp16, elementwise work and a fixed-order
    mean only, so two runs on the same images give the same bits"""

    def __init__(self, torch):
        self.torch = torch
        g = torch.Generator().manual_seed(3)
        self.weight = torch.rand((1, 50, 3, 1, 1), generator=g).cuda()

    def __call__(self, x):
        torch = self.torch
        y = torch.nn.functional.avg_pool2d(x.permute(0, 3, 1, 2).float(), 4)
        return (y.unsqueeze(1) * self.weight).sum(dim=2).half()


def test_engine_device_scenes_equal_a_bank_of_the_same_scenes(torch_cuda):
    """InferenceEngine(scenes="device") against scenes="bank" holding render_scenes' own output for the same joints / seed / ids:
    byte-equal records, eagerly and under graph replay -- the plumbing (slot layout, upload, render inside the graph, addcmul)
    isolated from rounding.  Two batches through the same plan: the joints really travel with each slot."""
    from posepaf import synth_device
    from posepaf.api import PosePostProcessor, records_to_numpy
    from posepaf.engine import InferenceEngine
    torch = torch_cuda
    B, H, W, MP, noise, seed = 4, 256, 256, 12, 0.02, 99
    model = _TinyModel(torch)
    rng = np.random.default_rng(4)
    batches = []
    for k in range(2):
        people = [scene_cases.random_people(p, 500 + 10 * k + j, H // 4, W // 4) for j, p in enumerate((3, 0, 5, 2) if k == 0 else (1, 4, 2, 6))]
        hw = [(256, 256), (200, 251), (193, 256), (256, 197)]
        batches.append((hw, [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in hw], people, [100 * k + j for j in range(4)]))
    # the bank: what render_scenes gives for every image of both batches, brought to the host and back
    bank = []
    for _, _, people, ids in batches:
        j, n = upload(torch, people, MP)
        bank.append(synth_device.render_scenes(j, n, H // 4, W // 4, noise=noise, seed=seed,
                                               scene_ids=torch.tensor(ids, dtype=torch.int64, device="cuda")).cpu().numpy())
    bank = np.concatenate(bank)
    assert bank.shape == (8, 2, 50, 64, 64) and bank.dtype == np.float16
    post = PosePostProcessor(max_batch=B, max_h=H // 4, max_w=W // 4, max_peaks_per_part=64)
    try:
        results = {}
        for scenes in ("device", "bank"):
            for use_graph in (True, False):
                eng = InferenceEngine(model, post, B, 0, rules="cpp", use_graph=use_graph, inject_scale=1e-3, max_image_hw=(H, W),
                                      scenes=scenes, max_people=MP, scene_noise=noise, scene_seed=seed)
                plan = eng.plan(H, W)
                if scenes == "bank":
                    eng.set_bank(plan, bank)
                    assert plan.scenes is None and plan.nbytes == 256 + B * H * W * 3
                eng.prepare(plan)
                assert (plan.graph is not None) == use_graph
                eng.sync()
                plan.records.zero_()     # the warm-up saw bank scene 0 in one mode and no people in the other: its humans past
                out = []                 # n_humans would stay behind in the buffer
                for k, (hw, imgs, people, ids) in enumerate(batches):
                    slot = eng.acquire()
                    sizes, idx, slot_imgs = slot.views(B, H, W)
                    for j, ((h, w), im) in enumerate(zip(hw, imgs)):
                        slot_imgs[j] = 0
                        slot_imgs[j, :h, :w] = im
                        sizes[0, j], sizes[1, j] = h, w
                        idx[j] = ids[j] if scenes == "device" else 4 * k + j
                    if scenes == "device":
                        n_people, joints = slot.scene_views(B, H, W, MP)
                        synth_device.pack_joints(people, MP, joints_out=joints, n_out=n_people)
                    rec_dev = eng.submit(slot, plan)
                    eng.sync()
                    out.append(rec_dev.cpu().numpy().tobytes())
                    assert sum(int(r["n_humans"]) for r in records_to_numpy(rec_dev)) > 0
                    if scenes == "device":
                        assert np.array_equal(plan.scenes.cpu().numpy(), bank[4 * k: 4 * k + 4])
                results[(scenes, use_graph)] = out
        assert results[("device", True)] == results[("bank", True)] == results[("device", False)] == results[("bank", False)]
        assert results[("device", True)][0] != results[("device", True)][1]
    finally:
        post.close()


_RUNS = {}


def _evaluate(tmp, name, extra, timeout=240):
    """one evaluate.py child under its own time limit -> its JSON summary line; a finished run is reused"""
    if name not in _RUNS:
        dump = os.path.join(tmp, name + ".json")
        r = subprocess.run([sys.executable, os.path.join(PKG, "evaluate.py"), "--run_refactor", "--run_cpp", "--batch", "32",
                            "--dump_name", dump] + extra, capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, r.stderr[-3000:]
        _RUNS[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return _RUNS[name]


def test_evaluate_end_to_end_with_device_scenes(torch_cuda, tmp_path_factory):
    """evaluate.py --scenes device: 96 images, 96 distinct scenes (the bank's period of 64 is gone), no overflow status; the
    synthetic OKS AP is printed next to the bank run's (not asserted: the scenes differ by construction beyond image 63)."""
    tmp = str(tmp_path_factory.mktemp("scene_runs"))
    dev = _evaluate(tmp, "device", ["--synthetic", "96", "--scenes", "device"])
    assert dev["status_or"] == 0 and dev["scenes"] == "device" and dev["distinct_scenes"] == 96 and dev["images"] == 96
    bank = _evaluate(tmp, "bank", ["--synthetic", "96", "--scenes", "bank"])
    assert bank["scenes"] == "bank" and bank["distinct_scenes"] == 64
    print("synthetic OKS AP, 96 images: device", dev.get("synthetic_oks"), "bank", bank.get("synthetic_oks"))
