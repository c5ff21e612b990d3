"""GPU: the device data transformer (pp_augment_batch, posepaf/augment.py) against the NumPy restatement of its contract
(tests/augment_reference.py).

Bound: none.  The arithmetic is integer plus one correctly rounded division (and float64 products rounded one by one for the
joints), so every output is compared BIT for bit, with no exclusions.
Shapes: sources of 37 x 53, 96 x 80 and 64 x 64 in a 96 x 96 slot, outputs of 64 x 64 (16 x 16 cells: one block) and 64 x 128
(16 x 32 cells: two blocks, and non-square); 8 x 12 and 72 x 68 outputs for the cells-per-block tail (18 x 17 cells: four blocks, the
erode's halo crossing block borders inside the frame)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_reference as ar
from conftest import PKG
from posepaf import augment, rotation, synth_device, val_loss

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SLOT = (96, 96)
SRC = ((37, 53), (96, 80), (64, 64))
AUGS = (augment.AugmentSelection(False, False, 40.0, (50, -50), 1.3), augment.AugmentSelection(True, False, -17.3, (0, 0), 0.7),
        augment.AugmentSelection.unrandom())
OBJPOS = ((25.0, 20.0), (40.5, 50.0), (31.5, 31.5))
SCALE_PROVIDED = (0.45, 0.7, 0.6)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want))


def block_mask(h, w, seed, lo, hi):
    """seeded random blocks of `lo` on a plane of `hi`, with a few soft values between"""
    rng = np.random.default_rng(seed)
    m = np.full((h, w), hi, np.uint8)
    m[h // 4:3 * h // 4, w // 3:2 * w // 3] = lo             # one block large enough to survive the reduction and the erode
    for _ in range(4):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        m[y:y + int(rng.integers(3, 24)), x:x + int(rng.integers(3, 24))] = lo
    y, x = int(rng.integers(0, h - 2)), int(rng.integers(0, w - 2))
    m[y:y + 2, x:x + 2] = rng.integers(0, 256, (2, 2), dtype=np.uint8)
    return m


def sources(srcs=SRC, seed=0):
    out = []
    for i, (h, w) in enumerate(srcs):
        rng = np.random.default_rng(100 * seed + i)
        out.append((rng.integers(0, 256, (h, w, 3), dtype=np.uint8), block_mask(h, w, 1000 * seed + i, 0, 255),
                    block_mask(h, w, 2000 * seed + i, 255, 0)))
    return out


def slots(srcs, slot=SLOT, pad=(0, 0, 0)):
    """[(image, mask_miss, mask_all)] -> the three slot arrays and sizes (2, B); pad: what the rest of a slot holds"""
    b = len(srcs)
    img = np.full((b,) + slot + (3,), pad[0], np.uint8)
    miss, all_ = np.full((b,) + slot, pad[1], np.uint8), np.full((b,) + slot, pad[2], np.uint8)
    sizes = np.zeros((2, b), np.int32)
    for i, (im, mm, ma) in enumerate(srcs):
        h, w = im.shape[:2]
        img[i, :h, :w], miss[i, :h, :w], all_[i, :h, :w] = im, mm, ma
        sizes[:, i] = h, w
    return img, miss, all_, sizes


def people(b, p, seed):
    """float64 (b, p, 18, 3): joints around the sources, a few flags 0 and 2, one joint far away"""
    rng = np.random.default_rng(seed)
    j = np.zeros((b, p, 18, 3))
    j[..., :2] = rng.uniform(-10.0, 100.0, (b, p, 18, 2))
    j[..., 2] = rng.integers(0, 3, (b, p, 18))
    j[0, 0, 4] = (1.0e5 + 0.123, -7.5e4, 1.0)
    j[0, min(1, p - 1), 6, 2] = 2.0
    j[b - 1, p - 1, 3] = (12.25, 13.5, 2.0)
    return j


def to_dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def raw_params(m_inv, m_fwd, flips):
    """the bytes pack_params makes, from explicit inverses"""
    d = np.stack([np.asarray(m_inv, np.float64).reshape(-1, 6), np.asarray(m_fwd, np.float64).reshape(-1, 6)])
    return np.concatenate([d.reshape(-1).view(np.uint8), np.asarray(flips, np.int32).view(np.uint8)])


def reference(srcs, m_inv, m_fwd, flips, joints, n_people, out_hw, half=False, use_miss=True, use_all=True):
    res = [ar.transform(im, mm if use_miss else None, ma if use_all else None, m_inv[i], m_fwd[i], flips[i], joints[i], n_people[i],
                        out_hw[0], out_hw[1], half=half) for i, (im, mm, ma) in enumerate(srcs)]
    return [np.stack([r[k] for r in res]) for k in range(4)]


def device(img, miss, all_, sizes, joints, n_people, params, out_hw, **kw):
    got = augment.augment_device(to_dev(img), to_dev(miss), to_dev(all_), to_dev(sizes), to_dev(joints), to_dev(np.asarray(n_people, np.int32)),
                                 to_dev(params), out_hw, **kw)
    torch.cuda.synchronize(DEV)
    return got


def matrices(out_hw, augs=AUGS, objpos=OBJPOS, scale_provided=SCALE_PROVIDED):
    m_fwd = [augment.affine_matrix(a, o, s, out_hw[0], out_hw[1])[0] for a, o, s in zip(augs, objpos, scale_provided)]
    return [rotation.invert_affine(m) for m in m_fwd], m_fwd, [a.flip for a in augs]


# ---------------------------------------------------------------------------------------------- the ragged batch, through transform_batch
@pytest.mark.parametrize("out_hw", [(64, 64), (64, 128)])
def test_ragged_batch_matches_the_restatement_and_writes_channel_48_in_place(out_hw):
    srcs = sources()
    img, miss, all_, sizes = slots(srcs)
    joints, n_people = people(3, 3, 7), [3, 1, 0]
    m_inv, m_fwd, flips = matrices(out_hw)
    want = reference(srcs, m_inv, m_fwd, flips, joints, n_people, out_hw)
    assert len({w.tobytes() for w in want[0]}) == 3 and want[1].min() < 1.0 and 0.0 < want[2].max() and want[2].min() == 0.0
    ch, cw = out_hw[0] // 4, out_hw[1] // 4
    target = torch.full((3, 1, 50, ch, cw), 0.625, dtype=torch.float16, device=DEV)
    got = augment.transform_batch(to_dev(img), to_dev(miss), to_dev(all_), to_dev(sizes), to_dev(joints), to_dev(np.asarray(n_people, np.int32)),
                                  list(AUGS), list(OBJPOS), list(SCALE_PROVIDED), out_hw, target=target)
    torch.cuda.synchronize(DEV)
    assert same(got[0], want[0]) and same(got[1], want[1]) and same(got[3], want[3])
    assert got[2].data_ptr() == target[:, 0, 48].data_ptr() and same(got[2], want[2].astype(np.float16))
    t = target.cpu().numpy()
    assert same(t[:, 0, 48], want[2].astype(np.float16))
    assert (np.delete(t, 48, axis=2) == np.float16(0.625)).all()                 # the sentinel survives everywhere else
    # the joints: rows beyond n_people unchanged, a flag 2 kept, one joint far outside the frame
    j = got[3].cpu().numpy()
    assert np.array_equal(j[1, 1:], joints[1, 1:].astype(np.float32)) and np.array_equal(j[2], joints[2].astype(np.float32))
    assert j[0, 1, 6, 2] == 2.0 and np.abs(j[0, 0, 4, :2]).max() > 5.0e4
    assert not np.array_equal(j[1, 0, :, :2], ar.map_joints(m_fwd[1], joints[1], 1, False)[0, :, :2])      # image 1 is flipped


# ---------------------------------------------------------------------------------------------- dtypes, NULL masks, NULL sizes, tails
@pytest.mark.parametrize("dtype, use_miss, use_all, use_sizes, out_hw", [
    (torch.float16, False, False, True, (64, 64)),
    (torch.float32, True, True, False, (72, 68)),
    (torch.float16, True, False, False, (8, 12)),
    (torch.float32, False, True, True, (72, 68)),
])
def test_sources_and_outputs(dtype, use_miss, use_all, use_sizes, out_hw):
    srcs = sources(SRC if use_sizes else ((96, 96),) * 3, seed=1)
    img, miss, all_, sizes = slots(srcs)
    joints, n_people = people(3, 2, 8), [2, 2, 1]
    m_inv, m_fwd, flips = matrices(out_hw, objpos=((25.0, 20.0), (40.5, 50.0), (31.5, 31.5)) if use_sizes else ((48.0, 48.0),) * 3)
    half = dtype == torch.float16
    want = reference(srcs, m_inv, m_fwd, flips, joints, n_people, out_hw, half=half, use_miss=use_miss, use_all=use_all)
    got = device(img, miss if use_miss else None, all_ if use_all else None, sizes if use_sizes else None, joints, n_people,
                 augment.pack_params(m_fwd, flips, *out_hw), out_hw, dtype=dtype)
    for g, w in zip(got, want):
        assert same(g, w)
    if not use_miss:
        assert (want[1] == 1.0).all()
    if not use_all:
        assert (want[2] == 0.0).all()
    else:
        assert want[2].max() > 0.0


# ---------------------------------------------------------------------------------------------- extreme placements
def test_extreme_placements_and_pad_bytes_are_never_read():
    srcs = sources(seed=2)
    # pad 255 / 0 / 255: each differs from its plane's border value (124 127 127 / 255 / 0), so a read of the pad would show
    img, miss, all_, sizes = slots(srcs, pad=(255, 0, 255))
    w1, w2 = SRC[1][1], SRC[2][1]
    m_inv = [np.array([[1.0, 0.0, 5000.0], [0.0, 1.0, -3000.0]]),                # wholly outside
             np.array([[1.0, 0.0, w1 - 1.0], [0.0, 1.0, 0.0]]),                   # destination x = 0 reads column w - 1 at fx = 0
             np.array([[1.0, 0.0, w2 - 2.5], [0.0, 1.0, SRC[2][0] - 1.5]])]       # half-weight taps beyond the right and bottom edges
    m_fwd = [np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])] * 3
    joints, n_people, out_hw = people(3, 1, 9), [1, 1, 1], (64, 64)
    want = reference(srcs, m_inv, m_fwd, [0, 0, 0], joints, n_people, out_hw)
    got = device(img, miss, all_, sizes, joints, n_people, raw_params(m_inv, m_fwd, [0, 0, 0]), out_hw)
    for g, w in zip(got, want):
        assert same(g, w)
    border = np.array(ar.BORDER, np.float32) / np.float32(255)
    assert (want[0][0] == border).all() and (want[1][0] == 1.0).all() and (want[2][0] == 0.0).all()
    assert np.array_equal(want[0][1][:37, 0], ar.unit(srcs[1][0][:37, w1 - 1])) and (want[0][1][:, 1:] == border).all()
    assert not (want[0][2][:2, :3] == border).all()


# ---------------------------------------------------------------------------------------------- determinism
def test_an_image_does_not_depend_on_its_batch():
    srcs = sources(seed=3)
    out_hw = (64, 128)
    m_inv, m_fwd, flips = matrices(out_hw)
    joints = people(3, 2, 10)
    img, miss, all_, sizes = slots(srcs)
    full = device(img, miss, all_, sizes, joints, [2, 2, 2], augment.pack_params(m_fwd, flips, *out_hw), out_hw)
    # image 2 alone, in a smaller slot
    h, w = SRC[2]
    img1, miss1, all1, sizes1 = slots(srcs[2:], slot=(h, w + 3))
    one = device(img1, miss1, all1, sizes1, joints[2:], [2], augment.pack_params(m_fwd[2:], flips[2:], *out_hw), out_hw)
    # image 1 first of two
    two = device(img[[1, 0]], miss[[1, 0]], all_[[1, 0]], sizes[:, [1, 0]], joints[[1, 0]], [2, 2],
                 augment.pack_params([m_fwd[1], m_fwd[0]], [flips[1], flips[0]], *out_hw), out_hw)
    for f, o, t in zip(full, one, two):
        assert same(o[0], f[2].cpu().numpy()) and same(t[0], f[1].cpu().numpy()) and same(t[1], f[0].cpu().numpy())


def test_a_captured_graph_replays_with_rewritten_matrices():
    srcs = sources(seed=4)
    out_hw = (64, 64)
    img, miss, all_, sizes = slots(srcs)
    joints, n_people = people(3, 2, 11), [2, 1, 2]
    draws = [matrices(out_hw), matrices(out_hw, augs=(AUGS[1], AUGS[2], AUGS[0]))]
    wants = [reference(srcs, m_inv, m_fwd, flips, joints, n_people, out_hw) for m_inv, m_fwd, flips in draws]
    assert not np.array_equal(wants[0][0], wants[1][0])
    packed = [to_dev(augment.pack_params(m_fwd, flips, *out_hw)) for _, m_fwd, flips in draws]
    args = [to_dev(img), to_dev(miss), to_dev(all_), to_dev(sizes), to_dev(joints), to_dev(np.asarray(n_people, np.int32))]
    params = packed[1].clone()
    out = {"image": torch.empty((3, 64, 64, 3), device=DEV), "mask_miss": torch.empty((3, 16, 16), device=DEV),
           "fg": torch.empty((3, 16, 16), device=DEV), "joints": torch.empty((3, 2, 18, 3), device=DEV)}
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        augment.augment_device(*args, params, out_hw, out=out)                   # warm-up outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        augment.augment_device(*args, params, out_hw, out=out)
    for k in (0, 1, 0):
        params.copy_(packed[k])
        for t in out.values():
            t.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize(DEV)
        for name, w in zip(("image", "mask_miss", "fg", "joints"), wants[k]):
            assert same(out[name], w), (k, name)


# ---------------------------------------------------------------------------------------------- the C entry's refusals
def test_the_entry_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    from posepaf import _lib
    L = _lib.load()
    srcs = sources(seed=5)
    img, miss, all_, sizes = (to_dev(a) for a in slots(srcs))
    joints, n_people = to_dev(people(3, 2, 12)), to_dev(np.array([1, 1, 1], np.int32))
    m_inv, m_fwd, flips = matrices((64, 64))
    params = to_dev(augment.pack_params(m_fwd, flips, 64, 64))
    image, mm = torch.full((3, 64, 64, 3), -1.0, device=DEV), torch.full((3, 16, 16), -1.0, device=DEV)
    fg, jout = torch.full((3, 16, 16), -1.0, device=DEV), torch.full((3, 2, 18, 3), -1.0, device=DEV)
    base = params.data_ptr()
    good = dict(images=img.data_ptr(), sizes=sizes.data_ptr(), miss=miss.data_ptr(), all=all_.data_ptr(), batch=3, slot_h=96, slot_w=96,
                m_inv=base, m_fwd=base + 144, flip=base + 288, jin=joints.data_ptr(), n=n_people.data_ptr(), p=2, out_h=64, out_w=64,
                border=(C.c_ubyte * 3)(124, 127, 127), image=image.data_ptr(), idt=_lib.PP_F32, mm=mm.data_ptr(), fg=fg.data_ptr(),
                fdt=_lib.PP_F32, stride=256, jout=jout.data_ptr(), stream=None)
    bad = [(dict(images=None), -2), (dict(m_inv=None), -2), (dict(m_fwd=None), -2), (dict(flip=None), -2), (dict(jin=None), -2),
           (dict(n=None), -2), (dict(border=None), -2), (dict(image=None), -2), (dict(mm=None), -2), (dict(fg=None), -2),
           (dict(jout=None), -2), (dict(batch=0), -2), (dict(slot_h=0), -2), (dict(slot_w=-1), -2), (dict(p=0), -2), (dict(out_h=0), -2),
           (dict(out_h=62), -2), (dict(out_w=66), -2), (dict(idt=2), -2), (dict(fdt=-1), -2), (dict(stride=255), -2),
           (dict(image=image.data_ptr() + 4), -2), (dict(p=65), -6), (dict(out_w=32772, stride=1 << 20), -3)]
    for change, code in bad:
        kw = dict(good)
        kw.update(change)
        assert L.pp_augment_batch(*kw.values()) == code, change
    torch.cuda.synchronize(DEV)
    assert all(bool((t == -1.0).all()) for t in (image, mm, fg, jout))            # nothing was launched
    assert L.pp_augment_batch(*good.values()) == 0
    torch.cuda.synchronize(DEV)
    assert not bool((image == -1.0).any())


# ---------------------------------------------------------------------------------------------- end to end
def test_transform_render_loss_equals_the_restatement_fed_to_the_same_entries():
    out_hw = (64, 64)
    srcs = sources(seed=6)
    img, miss, all_, sizes = slots(srcs)
    joints, n_people = people(3, 3, 13), [3, 2, 1]
    joints[..., :2] = np.clip(joints[..., :2], 0.0, 90.0)
    m_inv, m_fwd, flips = matrices(out_hw)
    want = reference(srcs, m_inv, m_fwd, flips, joints, n_people, out_hw)
    n_dev = to_dev(np.asarray(n_people, np.int32))
    rng = np.random.default_rng(14)
    preds = [[to_dev(rng.uniform(0.0, 1.0, (3, 50, 16 >> s, 16 >> s)).astype(np.float32)) for s in range(3)] for _ in range(2)]

    def loss(jts, fg, mask):
        target = synth_device.render_scenes(jts, n_dev, 16, 16, dtype=torch.float16, flip=False, reverse_kp=True)
        target[:, 0, 48].copy_(fg)                   # after the render: the renderer zeroes the channel
        return target, val_loss.focal_l2_terms(preds, target, mask=mask)
    x, mask, fg, jts = augment.transform_batch(to_dev(img), to_dev(miss), to_dev(all_), to_dev(sizes), to_dev(joints), n_dev, list(AUGS),
                                               list(OBJPOS), list(SCALE_PROVIDED), out_hw)
    t_dev, terms_dev = loss(jts, fg, mask)
    t_ref, terms_ref = loss(to_dev(want[3]), to_dev(want[2]), to_dev(want[1]))
    torch.cuda.synchronize(DEV)
    assert same(x, want[0]) and same(t_dev, t_ref.cpu().numpy()) and same(terms_dev, terms_ref.cpu().numpy())
    assert bool((t_dev[:, 0, 48] > 0).any()) and bool((t_dev[:, 0, 30:48] > 0).any()) and bool((mask < 1).any())
    assert np.isfinite(terms_dev.cpu().numpy()).all() and float(terms_dev.sum()) > 0
    # the in-place form: channel 48 written into a rendered target gives the same target
    augment.transform_batch(to_dev(img), to_dev(miss), to_dev(all_), to_dev(sizes), to_dev(joints), n_dev, list(AUGS), list(OBJPOS),
                            list(SCALE_PROVIDED), out_hw, target=t_ref)
    torch.cuda.synchronize(DEV)
    assert same(t_ref, t_dev.cpu().numpy())


FT_BOUND = 2.0 ** -23        # the bound of the existing finetune A/B test (tests/test_gpu_loss_grad.py): one float32 ulp, relative


def run_finetune(loss):
    r = subprocess.run([sys.executable, os.path.join(PKG, "finetune.py"), "--augment", "--synthetic", "8", "--batch", "4", "--sizes", "64x64",
                        "--src_sizes", "80x96,64x64", "--steps", "3", "--train", "heads", "--loss", loss],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_finetune_augment_runs_and_agrees_with_the_torch_formulation():
    """finetune.py --augment as a child process with --loss device and --loss torch: finite losses, "augment": true, and step 0 --
    the same weights, the same transformed batch, the same mask -- agrees on loss_first within the existing A/B test's bound.
    Measured on the MI355X over two pairs of runs: 1.1e-9 and 3.9e-9 relative (MIOpen's convolutions are not bit-reproducible from
    process to process)."""
    dev, tor = run_finetune("device"), run_finetune("torch")
    for out, name in ((dev, "device"), (tor, "torch")):
        assert out["augment"] is True and out["loss"] == name and out["images_per_step"] == 4 and len(out["losses"]) == 3
        assert np.isfinite(out["losses"]).all() and out["loss_first"] == out["losses"][0] and out["loss_first"] > 0
    rel = abs(dev["loss_first"] - tor["loss_first"]) / tor["loss_first"]
    print(f"finetune --augment step 0, device against torch: loss {rel:.3e}; losses device {dev['losses']}, torch {tor['losses']}")
    assert rel <= FT_BOUND
