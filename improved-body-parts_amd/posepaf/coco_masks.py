"""COCO person masks on the device (pp_coco_masks_u8, csrc/posepaf_segm.hip) and the reference's choice of training instances:
the stage between an annotation file and the data transformer (posepaf/augment.py).

    packed = pack_segmentations(anns_per_image, sizes)             # host: vertices, ring table, crowd runs -- a few KB per batch
    mask_miss, mask_all = masks_device(to_device(packed, dev), (slot_h, slot_w))    # uint8 (B, slot_h, slot_w), as transform_batch reads
    instances, skipped = training_instances(images, anns_per_image)                # main persons, objpos, scale_provided, joints

The reference makes these masks offline (data/coco_masks_hdf5.py: make_mask over pycocotools' annToMask, process_image) into an HDF5
corpus.  The rasteriser's arithmetic is the contract of INTEGRATION section 19: it follows the published maskApi.c (rleFrPoly,
rleMerge, rleDecode), but it is that statement (tests/coco_mask_reference.py) the kernel is held to, not a pycocotools run.  Whatever
the contract does not cover -- compressed run-length strings among it -- is refused with a message, never approximated.  There is
no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._lib import SCENE_MAX_PEOPLE, PosePafError

COORD_LIMIT = float(2 ** 24)          # |x|, |y| of a vertex: 5 x + 0.5 stays far inside int32
MAX_RINGS_PER_IMAGE = 4096            # every workgroup of an image walks all its rings
MAX_VERTS, MAX_RINGS, MAX_RUNS = 1 << 24, 1 << 20, 1 << 24        # per call (include/posepaf.h)
RING_COUNTS_FOR_MISS = 1              # ring flag: the annotation has num_keypoints <= 0


class MultiCrowdError(PosePafError):
    """an image with more than one crowd annotation: the reference's make_mask raises on it, callers skip the image and count it"""


def _ring(coords, where):
    try:
        xy = np.asarray(coords, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise PosePafError(f"{where}: a ring must be a flat list of numbers") from None
    if len(xy) % 2:
        raise PosePafError(f"{where}: a ring with an odd number of coordinates ({len(xy)})")
    if len(xy) < 6:
        raise PosePafError(f"{where}: a ring with fewer than 3 vertices ({len(xy) // 2})")
    if not np.isfinite(xy).all():
        raise PosePafError(f"{where}: a ring with non-finite coordinates")
    if (np.abs(xy) > COORD_LIMIT).any():
        raise PosePafError(f"{where}: a ring with coordinates beyond +-2^24")
    return xy.reshape(-1, 2)


def _crowd_runs(seg, h, w, where):
    if not isinstance(seg, dict):
        raise PosePafError(f"{where}: a crowd annotation must carry a run-length code {{'size', 'counts'}}, not polygons")
    counts = seg.get("counts")
    if isinstance(counts, (str, bytes)):
        raise PosePafError(f"{where}: compressed-string counts are not supported (uncompressed run lengths only)")
    try:
        size = [int(v) for v in seg.get("size", ())]
        runs = np.asarray(counts, np.int64).reshape(-1)
        exact = np.array_equal(runs, np.asarray(counts).reshape(-1))
    except (TypeError, ValueError):
        raise PosePafError(f"{where}: a run-length code needs 'size' [h, w] and 'counts' as a list of integers") from None
    if size != [h, w]:
        raise PosePafError(f"{where}: the run-length code's size {size} is not the image's [{h}, {w}]")
    if not exact or (runs < 0).any():
        raise PosePafError(f"{where}: the run lengths must be non-negative integers")
    if int(runs.sum()) != h * w:
        raise PosePafError(f"{where}: the run lengths sum to {int(runs.sum())}, the image has {h * w} pixels")
    return np.cumsum(runs)


def pack_segmentations(anns_per_image, sizes, names=None):
    """anns_per_image: per image its annotations in annotation order (dicts with 'segmentation', 'iscrowd', 'num_keypoints');
    sizes: per image (h, w); names: what to call the images in messages (default: their index).
    -> {'verts' float64 (V, 2), 'rings' int32 (R, 4), 'images' int64 (B, 5), 'runs' int64 (N,), 'sizes' int32 (2, B)}: the host
    arrays of pp_coco_masks_u8 (include/posepaf.h).  Raises PosePafError for what the contract does not cover and MultiCrowdError
    for an image with more than one crowd annotation."""
    b = len(anns_per_image)
    if b < 1 or len(sizes) != b or (names is not None and len(names) != b):
        raise PosePafError("one annotation list and one (h, w) per image")
    verts, rings, runs = [], [], []
    images, n_verts, n_runs = np.zeros((b, 5), np.int64), 0, 0
    size_arr = np.zeros((2, b), np.int32)
    for i, (anns, hw) in enumerate(zip(anns_per_image, sizes)):
        name = f"image {names[i] if names is not None else i}"
        h, w = int(hw[0]), int(hw[1])
        if not (1 <= h <= 32768 and 1 <= w <= 32768):
            raise PosePafError(f"{name}: sides must be 1..32768, got {h} x {w}")
        size_arr[:, i] = h, w
        images[i, 0] = len(rings)
        crowds = 0
        for q, ann in enumerate(anns):
            where = f"{name}, annotation {q}"
            seg = ann.get("segmentation")
            if int(ann.get("iscrowd", 0)) == 1:
                crowds += 1
                if crowds > 1:
                    raise MultiCrowdError(f"{name}: more than one crowd annotation (the reference's make_mask raises on it)")
                cum = _crowd_runs(seg, h, w, where)
                images[i, 2:5] = n_runs, len(cum), q
                runs.append(cum)
                n_runs += len(cum)
                continue
            if isinstance(seg, dict):
                raise PosePafError(f"{where}: a run-length segmentation on an annotation that is no crowd is not supported")
            if not isinstance(seg, (list, tuple)):
                raise PosePafError(f"{where}: 'segmentation' must be a list of rings")
            flag = RING_COUNTS_FOR_MISS if int(ann.get("num_keypoints", 0)) <= 0 else 0
            for k, coords in enumerate(seg):
                xy = _ring(coords, f"{where}, ring {k}")
                rings.append((n_verts, len(xy), q, flag))
                verts.append(xy)
                n_verts += len(xy)
        images[i, 1] = len(rings) - images[i, 0]
        if images[i, 1] > MAX_RINGS_PER_IMAGE:
            raise PosePafError(f"{name}: {images[i, 1]} rings, at most {MAX_RINGS_PER_IMAGE} per image")
    if n_verts > MAX_VERTS or len(rings) > MAX_RINGS or n_runs > MAX_RUNS:
        raise PosePafError(f"{n_verts} vertices, {len(rings)} rings, {n_runs} runs: at most {MAX_VERTS}, {MAX_RINGS}, {MAX_RUNS} per call")
    return {"verts": np.concatenate(verts) if verts else np.zeros((0, 2), np.float64),
            "rings": np.array(rings, np.int32).reshape(-1, 4),
            "images": images,
            "runs": np.concatenate(runs).astype(np.int64) if runs else np.zeros(0, np.int64),
            "sizes": size_arr}


_KEYS = (("verts", np.float64), ("rings", np.int32), ("images", np.int64), ("runs", np.int64), ("sizes", np.int32))


def to_device(packed, device, capacity=None, stream=None):
    """the arrays of pack_segmentations as device tensors.  capacity: {'verts' | 'rings' | 'runs': rows} pads those arrays (the kernel
    clamps against the lengths, so the padding is never used) -- the tensors of a captured graph keep their sizes between batches"""
    import torch
    out = {}
    st = torch.cuda.current_stream(device) if stream is None else stream
    with torch.cuda.stream(st):
        for key, dt in _KEYS:
            arr = np.ascontiguousarray(packed[key], dt)
            if key in ("verts", "rings", "runs"):               # at least one row: a tensor of no elements has no address
                rows = max(int((capacity or {}).get(key, len(arr))), 1)
                if len(arr) > rows:
                    raise PosePafError(f"{key}: {len(arr)} rows do not fit the capacity {rows}")
                arr = np.concatenate([arr, np.zeros((rows - len(arr),) + arr.shape[1:], dt)])
            out[key] = torch.from_numpy(arr).to(device)
    return out


def workspace_bytes(n_verts: int) -> int:
    from . import _lib
    n = int(_lib.load().pp_coco_masks_workspace_bytes(int(n_verts)))
    if n < 0:
        _lib.check(n)
    return n


def masks_device(packed, slot_hw, out=None, workspace=None, stream=None):
    """packed: the device tensors of to_device; slot_hw: (slot_h, slot_w), every image must fit; out: (mask_miss, mask_all) uint8
    (B, slot_h, slot_w) to write into; workspace: a uint8 device tensor of at least workspace_bytes(len(verts)) bytes (allocated when
    absent -- pass one under graph capture).  -> (mask_miss, mask_all): image b in the top-left corner of its slot, the rest of a
    slot untouched (torch.empty when allocated here).  Asynchronous."""
    import torch
    try:
        slot_h, slot_w = (int(v) for v in slot_hw)
    except (TypeError, ValueError):
        raise PosePafError(f"slot_hw must be (slot_h, slot_w), got {slot_hw!r}") from None
    if not (1 <= slot_h <= 32768 and 1 <= slot_w <= 32768):
        raise PosePafError(f"slot sides must be 1..32768, got {slot_h} x {slot_w}")
    want = {"verts": (torch.float64, 2), "rings": (torch.int32, 4), "images": (torch.int64, 5), "runs": (torch.int64, None),
            "sizes": (torch.int32, None)}
    if not isinstance(packed, dict) or any(k not in packed for k in want):
        raise PosePafError("packed must be the dict of to_device(pack_segmentations(...))")
    for k, (dt, cols) in want.items():
        t = packed[k]
        if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous() \
                or (cols is not None and (t.dim() != 2 or t.shape[1] != cols)):
            raise PosePafError(f"packed[{k!r}] must be a contiguous {dt} tensor of pack_segmentations' layout")
        if not t.is_cuda:
            raise PosePafError(f"packed[{k!r}] must live on the HIP device: the rasteriser has no CPU path")
    dev = packed["images"].device
    b = int(packed["images"].shape[0])
    if b < 1 or b > 65535 or tuple(packed["sizes"].shape) != (2, b) or packed["runs"].dim() != 1:
        raise PosePafError("packed: 1..65535 images, sizes (2, B), runs one-dimensional")
    n_verts, n_rings, n_runs = int(packed["verts"].shape[0]), int(packed["rings"].shape[0]), int(packed["runs"].shape[0])
    if out is None:
        out = (torch.empty((b, slot_h, slot_w), dtype=torch.uint8, device=dev), torch.empty((b, slot_h, slot_w), dtype=torch.uint8, device=dev))
    need = workspace_bytes(n_verts)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    tensors = [("out[0]", out[0]), ("out[1]", out[1]), ("workspace", workspace)]
    for name, t in tensors:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_contiguous():
            raise PosePafError(f"{name} must be a contiguous uint8 tensor")
        if not t.is_cuda:
            raise PosePafError(f"{name} must live on the HIP device: the rasteriser has no CPU path")
    for name, t in tensors + [(f"packed[{k!r}]", packed[k]) for k in want]:
        if t.device != dev:
            raise PosePafError(f"{name} is on {t.device}, the image table on {dev}: one device for all")
    for name, t in tensors[:2]:
        if tuple(t.shape) != (b, slot_h, slot_w):
            raise PosePafError(f"{name} must be ({b}, {slot_h}, {slot_w}), got {tuple(t.shape)}")
    if workspace.numel() < need:
        raise PosePafError(f"workspace holds {workspace.numel()} bytes, {need} are needed")
    from . import _lib
    L = _lib.load()
    st = torch.cuda.current_stream(dev) if stream is None else stream

    def ptr(t):
        return C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(L.pp_coco_masks_u8(ptr(packed["verts"]), n_verts, ptr(packed["rings"]), n_rings, ptr(packed["images"]),
                                      ptr(packed["runs"]), n_runs, ptr(packed["sizes"]), b, slot_h, slot_w, ptr(workspace),
                                      int(workspace.numel()), ptr(out[0]), ptr(out[1]), C.c_void_p(st.cuda_stream)))
    return out[0], out[1]


def training_instances(images, anns_per_image, image_size=512, max_people=SCENE_MAX_PEOPLE):
    """process_image of the reference (data/coco_masks_hdf5.py:126-266) for every image: each "main person" -- num_keypoints >= 5,
    area >= 32 * 32, not within 0.3 * side of an earlier main person's centre -- becomes one training instance, centred on them.
    images: per image a dict with 'height' and 'width' (and 'id', 'file_name', passed through); anns_per_image: its annotations.
    -> (instances, skipped): an instance is {'image': index, 'image_id', 'file_name', 'people_index', 'objpos' [(x, y)],
    'scale_provided' [bbox_h / image_size], 'joints' float64 (P, 18, 3)}, the main person first, then every other person with
    num_keypoints != 0 in annotation order (joints through synth_device.coco_person_to_joints); skipped counts the instances with more
    than max_people people, which are left out, never truncated."""
    from .synth_device import coco_person_to_joints
    if len(images) != len(anns_per_image):
        raise PosePafError("one annotation list per image")
    instances, skipped = [], 0
    for index, (meta, anns) in enumerate(zip(images, anns_per_image)):
        persons = []
        for p in anns:
            bx, by, bw, bh = (float(v) for v in p["bbox"])
            persons.append({"objpos": (bx + bw / 2, by + bh / 2), "area": float(p["area"]), "num_keypoints": int(p["num_keypoints"]),
                            "scale_provided": bh / image_size, "keypoints": p["keypoints"]})
        if not persons:
            continue
        # the reference reads img_anns[p]["bbox"] here with p left over from the loop that built the persons (line 216): the side is
        # max(bbox_w, bbox_h) of the image's LAST annotation, whoever the main person is.  Kept: it decides the instances.
        side = max(float(anns[-1]["bbox"][2]), float(anns[-1]["bbox"][3]))
        main, centres = [], []
        for k, pers in enumerate(persons):
            if pers["num_keypoints"] < 5 or pers["area"] < 32 * 32:
                continue
            cx, cy = pers["objpos"]
            if any(math.sqrt((cx - px) * (cx - px) + (cy - py) * (cy - py)) < ps * 0.3 for px, py, ps in centres):
                continue
            main.append(k)
            centres.append((cx, cy, side))
        for k in main:
            order = [k] + [o for o, pers in enumerate(persons) if o != k and pers["num_keypoints"] != 0]
            if len(order) > max_people:
                skipped += 1
                continue
            instances.append({"image": index, "image_id": meta.get("id"), "file_name": meta.get("file_name"), "people_index": k,
                              "objpos": [persons[o]["objpos"] for o in order],
                              "scale_provided": [persons[o]["scale_provided"] for o in order],
                              "joints": np.stack([coco_person_to_joints(persons[o]["keypoints"]) for o in order])})
    return instances, skipped
