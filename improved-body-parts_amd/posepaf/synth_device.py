"""Ground-truth-style scenes rendered on the device (pp_render_scenes, csrc/posepaf_synth.hip): joint lists in, the
network-output layout (B, 1|2, 50, h, w) out -- the device form of synth.render_maps + synth.mirror_sample (+ noise).

synth.py stays the host restatement (demo_image.py --synthetic, the scene banks, the tests' fixtures); this module is what an
evaluation uses to give every image its own scene without keeping a bank in HBM.  The noise is NOT NumPy's stream: it is a
counter-based generator keyed by (seed, scene id, sample, channel, pixel), so an image gets the same noise in whichever batch
it lands.  There is no CPU path: without a HIP device render_scenes raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import skeleton as sk
from ._lib import PP_F16, PP_F32, SCENE_MAX_PEOPLE, SCENE_REVERSE_KP, PosePafError

MAX_PEOPLE = SCENE_MAX_PEOPLE      # people of one image the kernel stages in LDS (PP_SCENE_MAX_PEOPLE, include/posepaf.h)


def coco_person_to_joints(keypoints) -> np.ndarray:
    """One COCO annotation's 51 numbers -> (18, 3) float64 joints in the CMU order (x, y, flag; 1 = present, 2 = absent):
    COCO order -> the 18 parts through skeleton.ORDER_COCO, neck = shoulder midpoint when both shoulders are labelled, as in
    the reference's data pipeline."""
    kp = np.asarray(keypoints, np.float64).reshape(17, 3)
    j = np.zeros((sk.NUM_PART, 3))
    j[:, 2] = 2
    for coco_i, cmu_i in enumerate(sk.ORDER_COCO):
        if kp[coco_i, 2] > 0:
            j[cmu_i] = (kp[coco_i, 0], kp[coco_i, 1], 1)
    if kp[5, 2] > 0 and kp[6, 2] > 0:
        j[1] = ((kp[5, 0] + kp[6, 0]) / 2, (kp[5, 1] + kp[6, 1]) / 2, 1)
    return j


def coco_to_joints(gts, max_people: int | None = None) -> np.ndarray:
    """The ground truths of ONE image (dicts with a "keypoints" entry, COCO order) -> joints (P, 18, 3) float64 of the people
    with at least one labelled part, in annotation order.  max_people: refuse (never truncate) an image with more."""
    people = []
    for g in gts:
        j = coco_person_to_joints(g["keypoints"])
        if (j[:, 2] < 2).any():
            people.append(j)
    if max_people is not None and len(people) > max_people:
        raise PosePafError(f"{len(people)} annotated people in one image, max_people is {max_people}")
    return np.stack(people) if people else np.zeros((0, sk.NUM_PART, 3))


def pack_joints(people_per_image, max_people: int, joints_out=None, n_out=None):
    """[joints (P_i, 18, 3)] -> (joints float32 (B, max_people, 18, 3) with absent flags past P_i, n_people int32 (B,)), into the
    given arrays (e.g. views of a pinned batch) when passed."""
    b = len(people_per_image)
    joints = np.zeros((b, max_people, sk.NUM_PART, 3), np.float32) if joints_out is None else joints_out
    n = np.zeros(b, np.int32) if n_out is None else n_out
    for i, pj in enumerate(people_per_image):
        p = int(pj.shape[0])
        if p > max_people:
            raise PosePafError(f"image {i} has {p} people, max_people is {max_people}")
        joints[i, :p] = pj
        joints[i, p:, :, :2] = 0
        joints[i, p:, :, 2] = 2
        n[i] = p
    return joints, n


def _check_args(joints, n_people, h, w, dtype, noise, scene_ids, out, flip):
    import torch
    if not (isinstance(joints, torch.Tensor) and isinstance(n_people, torch.Tensor)):
        raise PosePafError("render_scenes takes device tensors (joints float32 (B, P, 18, 3), n_people int32 (B,))")
    if joints.dim() != 4 or tuple(joints.shape[2:]) != (sk.NUM_PART, 3) or joints.dtype != torch.float32:
        raise PosePafError(f"joints must be float32 (B, max_people, 18, 3), got {joints.dtype} {tuple(joints.shape)}")
    b, max_people = int(joints.shape[0]), int(joints.shape[1])
    if b <= 0 or max_people <= 0:
        raise PosePafError(f"joints must hold at least one image and one person slot, got {tuple(joints.shape)}")
    if max_people > MAX_PEOPLE:
        raise PosePafError(f"max_people {max_people} is beyond the {MAX_PEOPLE} the kernel stages in LDS")
    if n_people.dtype != torch.int32 or tuple(n_people.shape) != (b,):
        raise PosePafError(f"n_people must be int32 ({b},), got {n_people.dtype} {tuple(n_people.shape)}")
    if int(h) <= 0 or int(w) <= 0:
        raise PosePafError(f"h and w must be positive, got {h} x {w}")
    if dtype not in (torch.float16, torch.float32):
        raise PosePafError(f"dtype must be torch.float16 or torch.float32, got {dtype}")
    if not (float(noise) >= 0.0):
        raise PosePafError(f"noise must be >= 0, got {noise}")
    if scene_ids is not None and (not isinstance(scene_ids, torch.Tensor) or scene_ids.dtype != torch.int64
                                  or tuple(scene_ids.shape) != (b,)):
        raise PosePafError(f"scene_ids must be an int64 ({b},) tensor")
    want = (b, 2 if flip else 1, sk.NUM_CH, int(h), int(w))
    if out is not None and (tuple(out.shape) != want or out.dtype != dtype or not out.is_contiguous()):
        raise PosePafError(f"out must be a contiguous {dtype} {want} tensor, got {out.dtype} {tuple(out.shape)}")
    for name, t in (("joints", joints), ("n_people", n_people), ("scene_ids", scene_ids), ("out", out)):
        if t is not None and not t.is_cuda:
            raise PosePafError(f"{name} must live on the HIP device: render_scenes has no CPU path")
    for name, t in (("joints", joints), ("n_people", n_people), ("scene_ids", scene_ids)):
        if t is not None and not t.is_contiguous():
            raise PosePafError(f"{name} must be contiguous")
    return want


def render_scenes(joints, n_people, h: int, w: int, dtype=None, flip: bool = True, noise: float = 0.0, seed: int = 0,
                  scene_ids=None, reverse_kp: bool = False, out=None, stream=None):
    """joints: device float32 (B, max_people, 18, 3) (x, y in image pixels, flag < 2 = annotated); n_people: device int32 (B,).
    -> device (B, 2 if flip else 1, 50, h, w) `dtype` (default float16): the maps synth.render_maps gives for each image's first
    n_people[b] people, and with flip their mirror_sample.  noise > 0 adds noise * N(0, 1) keyed by (seed, scene_ids[b] -- the
    image's index without scene_ids --, sample, channel, pixel).  reverse_kp: channel 49 = max over the keypoint channels.
    out: render into this tensor; stream: a torch stream (default: the current one).  Asynchronous."""
    import torch
    dtype = torch.float16 if dtype is None else dtype
    want = _check_args(joints, n_people, h, w, dtype, noise, scene_ids, out, flip)
    from . import _lib
    L = _lib.load()
    dev = joints.device
    for t in (n_people, scene_ids, out):
        if t is not None and t.device != dev:
            raise PosePafError("joints, n_people, scene_ids and out must share one device")
    if out is None:
        out = torch.empty(want, dtype=dtype, device=dev)
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev):
        _lib.check(L.pp_render_scenes(
            C.c_void_p(joints.data_ptr()), C.c_void_p(n_people.data_ptr()),
            C.c_void_p(scene_ids.data_ptr()) if scene_ids is not None else None, want[0], int(joints.shape[1]), int(h), int(w),
            want[1], PP_F16 if dtype == torch.float16 else PP_F32, SCENE_REVERSE_KP if reverse_kp else 0, float(noise),
            int(seed) & 0xFFFFFFFFFFFFFFFF, C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream)))
    return out
