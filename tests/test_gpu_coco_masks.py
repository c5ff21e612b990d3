"""GPU: COCO person masks on the device (pp_coco_masks_u8, posepaf/coco_masks.py) against the restatement of their contract
(tests/coco_mask_reference.py), and the two consumers (finetune.py --ann_file, evaluate.py --mask_miss segm).

Bound: none.  The contract is integer and float64 arithmetic with every operation rounded on its own, so every byte of both masks is
compared, and the slot bytes outside the images must keep a sentinel.
Shapes: 37 x 53, 70 x 150 (two row tiles of 64) and 64 x 64 in a 96 x 160 slot (rows on 16-byte boundaries: vector stores), the same
in a 75 x 157 slot (byte stores), and 70 x 300 (two column tiles of 256)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_reference as ar
import coco_mask_cases as cases
import coco_mask_reference as cr
from conftest import PKG
from posepaf import augment, coco_masks, rotation

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = 77


@pytest.fixture(scope="module")
def restated():
    """the restatement of both batches, computed once: [[(mask_miss, mask_all) per image] per batch]"""
    return [[cr.make_mask(anns, h, w) for anns, (h, w) in zip(batch, cases.SIZES)] for batch in cases.batches()]


def rasterise(anns_per_image, sizes, slot, capacity=None):
    packed = coco_masks.to_device(coco_masks.pack_segmentations(anns_per_image, sizes), DEV, capacity)
    out = tuple(torch.full((len(sizes),) + tuple(slot), SENTINEL, dtype=torch.uint8, device=DEV) for _ in range(2))
    coco_masks.masks_device(packed, slot, out=out)
    torch.cuda.synchronize(DEV)
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def check(got, want, sizes):
    """every byte inside the images equals the restatement, every byte outside is the sentinel"""
    for plane, name in ((0, "mask_miss"), (1, "mask_all")):
        for i, (h, w) in enumerate(sizes):
            g = got[plane][i]
            bad = np.argwhere(g[:h, :w] != want[i][plane])
            assert len(bad) == 0, (name, i, len(bad), bad[:5].tolist())
            rest = g.copy()
            rest[:h, :w] = SENTINEL
            assert (rest == SENTINEL).all(), (name, i, "bytes outside the image were written")


@pytest.mark.parametrize("k", [0, 1])
def test_batches_equal_the_restatement(restated, k):
    got = rasterise(cases.batches()[k], cases.SIZES, cases.SLOT)
    check(got, restated[k], cases.SIZES)
    if k == 0:
        miss, all_ = restated[0][1]
        assert 0 < (miss == 0).sum() < miss.size and 0 < (all_ == 255).sum() < all_.size       # the case is not trivial
        assert (restated[0][0][0] == 255).all() and (restated[0][0][1] == 0).all()             # an image with nothing: 255 / 0


def test_unaligned_slot_and_two_column_tiles(restated):
    got = rasterise(cases.batches()[0], cases.SIZES, (75, 157))
    check(got, restated[0], cases.SIZES)
    want = [cr.make_mask(cases.wide(), 70, 300)]
    for slot in ((70, 300), (72, 304)):
        check(rasterise([cases.wide()], [(70, 300)], slot), want, [(70, 300)])


def test_an_image_does_not_depend_on_its_batch_or_slot(restated):
    first, _ = cases.batches()
    alone = rasterise([first[1]], [cases.SIZES[1]], (70, 150))
    check(alone, [restated[0][1]], [cases.SIZES[1]])
    moved = rasterise([first[2], first[0], first[1]], [cases.SIZES[2], cases.SIZES[0], cases.SIZES[1]], (128, 208))
    check(moved, [restated[0][2], restated[0][0], restated[0][1]], [cases.SIZES[2], cases.SIZES[0], cases.SIZES[1]])


def test_a_captured_graph_replays_with_rewritten_tables(restated):
    host = [coco_masks.pack_segmentations(b, cases.SIZES) for b in cases.batches()]
    assert not np.array_equal(restated[0][1][0], restated[1][1][0])
    cap = {k: max(len(p[k]) for p in host) for k in ("verts", "rings", "runs")}
    packed = [coco_masks.to_device(p, DEV, cap) for p in host]
    live = {k: v.clone() for k, v in packed[1].items()}
    out = tuple(torch.empty((3,) + cases.SLOT, dtype=torch.uint8, device=DEV) for _ in range(2))
    work = torch.empty(coco_masks.workspace_bytes(cap["verts"]), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        coco_masks.masks_device(live, cases.SLOT, out=out, workspace=work)          # warm-up outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        coco_masks.masks_device(live, cases.SLOT, out=out, workspace=work)
    for k in (0, 1, 0):
        for name, t in live.items():
            t.copy_(packed[k][name])
        for t in out:
            t.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize(DEV)
        check((out[0].cpu().numpy(), out[1].cpu().numpy()), restated[k], cases.SIZES)


def test_masks_through_the_transformer_equal_the_restatement(restated):
    """the device masks fed to transform_batch against tests/augment_reference.py fed the restated masks, bit for bit"""
    first, _ = cases.batches()
    out_hw = (64, 64)
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in cases.SIZES]
    slot_img = np.zeros((3,) + cases.SLOT + (3,), np.uint8)
    for i, im in enumerate(imgs):
        slot_img[i, :im.shape[0], :im.shape[1]] = im
    packed = coco_masks.to_device(coco_masks.pack_segmentations(first, cases.SIZES), DEV)
    miss, all_ = coco_masks.masks_device(packed, cases.SLOT)
    joints = np.zeros((3, 2, 18, 3))
    joints[..., :2], joints[..., 2] = rng.uniform(0.0, 60.0, (3, 2, 18, 2)), rng.integers(0, 3, (3, 2, 18))
    n_people = np.array([2, 1, 2], np.int32)
    augs = [augment.AugmentSelection(False, False, 25.0, (10, -5), 1.1), augment.AugmentSelection(True, False, -12.0, (0, 0), 0.8),
            augment.AugmentSelection.unrandom()]
    objpos, scale_provided = [(25.0, 18.0), (75.0, 35.0), (32.0, 32.0)], [0.5, 0.9, 0.8]
    got = augment.transform_batch(torch.from_numpy(slot_img).to(DEV), miss, all_, packed["sizes"], torch.from_numpy(joints).to(DEV),
                                  torch.from_numpy(n_people).to(DEV), augs, objpos, scale_provided, out_hw)
    torch.cuda.synchronize(DEV)
    for i in range(3):
        m_fwd = augment.affine_matrix(augs[i], objpos[i], scale_provided[i], *out_hw)[0]
        want = ar.transform(imgs[i], restated[0][i][0], restated[0][i][1], rotation.invert_affine(m_fwd), m_fwd, augs[i].flip, joints[i],
                            int(n_people[i]), *out_hw)
        for g, w, name in zip(got, want, ("image", "mask_miss", "fg", "joints")):
            g = g[i].cpu().numpy()
            assert g.dtype == w.dtype and np.array_equal(g.view(np.uint32), np.ascontiguousarray(w).view(np.uint32)), (i, name)
    assert bool((got[1] < 1).any()) and bool((got[2] > 0).any())


def test_the_entry_refuses_bad_arguments_before_any_launch():
    from posepaf import _lib
    L = _lib.load()
    p = coco_masks.to_device(coco_masks.pack_segmentations(cases.batches()[0], cases.SIZES), DEV)
    out = tuple(torch.full((3,) + cases.SLOT, SENTINEL, dtype=torch.uint8, device=DEV) for _ in range(2))
    nv, nr, nn = (int(p[k].shape[0]) for k in ("verts", "rings", "runs"))
    work = torch.empty(coco_masks.workspace_bytes(nv), dtype=torch.uint8, device=DEV)
    good = dict(verts=p["verts"].data_ptr(), nv=nv, rings=p["rings"].data_ptr(), nr=nr, images=p["images"].data_ptr(),
                runs=p["runs"].data_ptr(), nn=nn, sizes=p["sizes"].data_ptr(), batch=3, slot_h=cases.SLOT[0], slot_w=cases.SLOT[1],
                work=work.data_ptr(), wb=work.numel(), miss=out[0].data_ptr(), all=out[1].data_ptr(), stream=None)
    bad = [(dict(verts=None), -2), (dict(rings=None), -2), (dict(images=None), -2), (dict(runs=None), -2), (dict(work=None), -2),
           (dict(miss=None), -2), (dict(all=None), -2), (dict(all=good["miss"]), -2), (dict(batch=0), -2), (dict(slot_h=0), -2),
           (dict(slot_w=-1), -2), (dict(nv=-1), -2), (dict(nr=-1), -2), (dict(nn=-1), -2), (dict(wb=work.numel() - 1), -2),
           (dict(verts=good["verts"] + 4), -2), (dict(rings=good["rings"] + 4), -2), (dict(work=good["work"] + 4), -2),
           (dict(batch=65536), -3), (dict(slot_w=32769), -3), (dict(nv=(1 << 24) + 1), -3), (dict(nr=(1 << 20) + 1), -3),
           (dict(nn=(1 << 24) + 1), -3)]
    for change, code in bad:
        kw = dict(good)
        kw.update(change)
        assert L.pp_coco_masks_u8(*kw.values()) == code, change
    assert L.pp_coco_masks_workspace_bytes(-1) == -2 and L.pp_coco_masks_workspace_bytes((1 << 24) + 1) == -3
    torch.cuda.synchronize(DEV)
    assert all(bool((t == SENTINEL).all()) for t in out)                          # nothing was launched
    assert L.pp_coco_masks_u8(*good.values()) == 0
    torch.cuda.synchronize(DEV)
    assert not bool((out[0][1, :70, :150] == SENTINEL).any())
    with pytest.raises(coco_masks.PosePafError, match="HIP device"):
        coco_masks.masks_device({k: v.cpu() for k, v in p.items()}, cases.SLOT)


# ---------------------------------------------------------------------------------------------- evaluate.py --mask_miss segm
def test_evaluate_val_loss_with_the_segmentation_mask(tmp_path, monkeypatch):
    """evaluate.py --val_loss --mask_miss segm as a child process reports another loss than --mask_miss ones; in this process, its
    run_val_loss gives the same loss when the stride-4 mask is the restated one (make_mask, padded with 255 to the bucket's shape,
    through the 4 x 4 area rule of tests/augment_reference.py) -- and the device's stride-4 mask equals that one bit for bit."""
    import importlib.util
    ann, img_dir, doc = cases.write_annotation_fixture(str(tmp_path))
    common = ["--val_loss", "--ann_file", ann, "--img_dir", img_dir, "--batch", "2"]
    ones, segm = run_script("evaluate.py", common), run_script("evaluate.py", common + ["--mask_miss", "segm"])
    assert ones["mask_miss"] == "none" and segm["mask_miss"] == "segm" and ones["images"] == segm["images"] == 3
    assert segm["images_skipped_multi_crowd"] == 0 and "images_skipped_multi_crowd" not in ones
    assert np.isfinite(segm["val_loss"]) and 0 < segm["val_loss"] < ones["val_loss"]              # masked terms only leave the sum

    spec = importlib.util.spec_from_file_location("pp_evaluate", os.path.join(PKG, "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    from posepaf.fused_model import FusedIMHN
    from posepaf.model_init import build_network
    model = FusedIMHN.from_network(build_network("posenet", None, 7)[0]).eval().to(DEV).half().to(memory_format=torch.channels_last)
    a, src = ev.parse(common + ["--mask_miss", "segm"]), ev.CocoSource(ann, img_dir)
    device_mask, compared = ev.segm_mask_stride4, []

    def restated_mask(anns_per_image, staged, sizes, dev):
        n, hp, wp, _ = staged.shape
        hw = sizes.cpu().numpy()
        planes = []
        for j, anns in enumerate(anns_per_image):
            full = np.full((hp, wp), 255, np.uint8)
            full[:hw[0, j], :hw[1, j]] = cr.make_mask(anns, int(hw[0, j]), int(hw[1, j]))[0]
            planes.append(ar.area4(full).astype(np.float32) / np.float32(255))
        want = np.stack(planes)
        got = device_mask(anns_per_image, staged, sizes, dev).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        compared.append(int((want < 1).sum()))
        return torch.from_numpy(want).to(dev)
    pinned = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True      # torch's own small convolutions are not reproducible from call to call otherwise
    try:
        got = ev.run_val_loss(a, src, model, DEV)
        monkeypatch.setattr(ev, "segm_mask_stride4", restated_mask)
        want = ev.run_val_loss(a, src, model, DEV)
    finally:
        torch.backends.cudnn.deterministic = pinned
    assert len(compared) >= 2 and max(compared) > 0          # every batch was compared; the third image has nothing to mask
    assert got["mask_miss"] == "segm" and got["val_loss"] == want["val_loss"] and got["per_stack_scale"] == want["per_stack_scale"]


# ---------------------------------------------------------------------------------------------- finetune.py --ann_file
FT_BOUND = 2.0 ** -23        # the bound of the existing finetune A/B tests (tests/test_gpu_augment.py): one float32 ulp, relative


def run_script(script, args):
    r = subprocess.run([sys.executable, os.path.join(PKG, script)] + args, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_finetune_from_annotations_runs_and_agrees_with_the_torch_formulation(tmp_path):
    """finetune.py --ann_file as a child process with --loss device and --loss torch: finite losses, "source": "annotations", and
    step 0 -- the same weights, instances, masks and draws -- agrees on loss_first within the existing A/B tests' bound."""
    ann, img_dir, _ = cases.write_annotation_fixture(str(tmp_path))
    outs = {}
    for loss in ("device", "torch"):
        outs[loss] = run_script("finetune.py", ["--ann_file", ann, "--img_dir", img_dir, "--batch", "2", "--sizes", "64x64", "--steps", "2",
                                                "--train", "heads", "--loss", loss])
        o = outs[loss]
        assert o["source"] == "annotations" and o["augment"] is True and o["loss"] == loss and len(o["losses"]) == 2
        assert o["instances"] == 6 and o["instances_skipped"] == 0 and o["images_skipped_multi_crowd"] == 0
        assert np.isfinite(o["losses"]).all() and o["loss_first"] > 0
    rel = abs(outs["device"]["loss_first"] - outs["torch"]["loss_first"]) / outs["torch"]["loss_first"]
    print(f"finetune --ann_file step 0, device against torch: {rel:.3e}; device {outs['device']['losses']}, torch {outs['torch']['losses']}")
    assert rel <= FT_BOUND
