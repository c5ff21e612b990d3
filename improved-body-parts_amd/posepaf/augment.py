"""The reference's training-data transformer on the device (pp_augment_batch, csrc/posepaf_augment.hip): raw uint8 slots in,
(image, mask_miss, foreground, joints) out, one launch chain for a batch and no host round trip.

    aug = AugmentSelection.random(TransformParams(), random.Random(seed))        # the reference's draws, in its order
    x, mask, fg, joints = transform_batch(images, mask_miss, mask_all, sizes, joints64, n_people, augs, objpos, scale_provided,
                                          (out_h, out_w), target=target)          # fg lands in channel 48 of `target`
    target = synth_device.render_scenes(joints, n_people, out_h // 4, out_w // 4, out=target)   # BEFORE transform_batch: it zeroes 48

The host half is the reference's (py_cocodata_server/py_data_transformer.py:9-88): the draws and the one affine matrix per sample,
in float64, inverted as cv2.warpAffine inverts it (rotation.invert_affine).  The device half is the contract of INTEGRATION
section 17: it follows OpenCV 3.4's 8-bit warpAffine / INTER_AREA resize / erode, but it is that statement (tests/augment_reference.py)
the kernels are held to, not a cv2 run.  The HSV colour distortion (aug.tint) is out of scope and refused.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import rotation
from . import skeleton as sk
from ._lib import PP_F16, PP_F32, SCENE_MAX_PEOPLE, PosePafError

BORDER = (124, 127, 127)                       # py_data_transformer.py:132
LEFT_PARTS = [sk.PARTS.index(p) for p in ("Lsho", "Lelb", "Lwri", "Lhip", "Lkne", "Lank", "Leye", "Lear")]
RIGHT_PARTS = [sk.PARTS.index(p) for p in ("Rsho", "Relb", "Rwri", "Rhip", "Rkne", "Rank", "Reye", "Rear")]
# the int32 fixed-point range of the coordinates: (|m0| out_w + |m1| out_h + |m2| + 1) * 1024 < 2^31 for both rows of the inverse
COORD_LIMIT = float(2 ** 21)
PARAM_DOUBLES = 12                             # per image: the inverse, then the forward matrix


class TransformParams:
    """config/config.py:25-38 of the reference (TransformationParams), the fields the transformer reads"""

    def __init__(self, target_dist=0.6, scale_prob=0.8, scale_min=0.7, scale_max=1.3, max_rotate_degree=40.0,
                 center_perterb_max=50.0, flip_prob=0.5, tint_prob=0.2):
        self.target_dist = target_dist
        self.scale_prob = scale_prob
        self.scale_min = scale_min
        self.scale_max = scale_max
        self.max_rotate_degree = max_rotate_degree
        self.center_perterb_max = center_perterb_max
        self.flip_prob = flip_prob
        self.tint_prob = tint_prob


class AugmentSelection:
    """One sample's augmentation draw (py_data_transformer.py:9-40)"""

    def __init__(self, flip=False, tint=False, degree=0.0, crop=(0, 0), scale=1.0):
        self.flip, self.tint, self.degree, self.crop, self.scale = flip, tint, degree, crop, scale

    @staticmethod
    def random(params, rng):
        """rng: a random.Random.  The draws in the reference's order: flip, tint, degree, the scale-probability draw, the scale draw
        only if that fired, x_offset, y_offset -- random.Random(s) gives what the reference gives after random.seed(s)."""
        flip = rng.uniform(0.0, 1.0) < params.flip_prob
        tint = rng.uniform(0.0, 1.0) < params.tint_prob
        degree = rng.uniform(-1.0, 1.0) * params.max_rotate_degree
        if rng.uniform(0.0, 1.0) < params.scale_prob:
            scale = (params.scale_max - params.scale_min) * rng.uniform(0.0, 1.0) + params.scale_min
        else:
            scale = 1.0
        x_offset = int(rng.uniform(-1.0, 1.0) * params.center_perterb_max)
        y_offset = int(rng.uniform(-1.0, 1.0) * params.center_perterb_max)
        return AugmentSelection(flip, tint, degree, (x_offset, y_offset), scale)

    @staticmethod
    def unrandom():
        return AugmentSelection(False, False, 0.0, (0, 0), 1.0)

    def __repr__(self):
        return f"AugmentSelection(flip={self.flip}, tint={self.tint}, degree={self.degree}, crop={self.crop}, scale={self.scale})"


def affine_matrix(aug, objpos, scale_provided, out_h, out_w, params=None):
    """AugmentSelection.affine (py_data_transformer.py:42-88) for an (out_h, out_w) output: -> (M 2 x 3 float64, scale_size).  The
    same five 3 x 3 matrices multiplied in the same order; scale_self *= height / (height - 1) and the width / 2 - 0.5 + crop
    centre included."""
    params = TransformParams() if params is None else params
    scale_self = scale_provided * (out_h / (out_h - 1))
    A = math.cos(aug.degree / 180. * math.pi)
    B = math.sin(aug.degree / 180. * math.pi)
    scale_size = params.target_dist / scale_self * aug.scale
    center_x, center_y = objpos
    center2zero = np.array([[1., 0., -center_x], [0., 1., -center_y], [0., 0., 1.]])
    rotate = np.array([[A, B, 0], [-B, A, 0], [0, 0, 1.]])
    scale = np.array([[scale_size, 0, 0], [0, scale_size, 0], [0, 0, 1.]])
    flip = np.array([[-1 if aug.flip else 1., 0., 0.], [0., 1., 0.], [0., 0., 1.]])
    center2center = np.array([[1., 0., out_w / 2 - 0.5 + aug.crop[0]], [0., 1., out_h / 2 - 0.5 + aug.crop[1]], [0., 0., 1.]])
    combined = center2center.dot(flip).dot(scale).dot(rotate).dot(center2zero)
    return combined[0:2], scale_size


def check_inverse(m_inv, out_h, out_w, what="matrix"):
    """refuse an inverted matrix whose fixed-point coordinates would leave int32 somewhere on an (out_h, out_w) output"""
    m = np.asarray(m_inv, np.float64).reshape(6)
    if not np.isfinite(m).all():
        raise PosePafError(f"{what}: the inverted matrix is not finite (a singular matrix?)")
    for r in (0, 3):
        reach = abs(m[r]) * out_w + abs(m[r + 1]) * out_h + abs(m[r + 2]) + 1.0
        if not reach < COORD_LIMIT:
            raise PosePafError(f"{what}: source coordinates reach {reach:.3g} px, the fixed-point range ends at {COORD_LIMIT:.0f}")


def pack_params(m_fwd, flips, out_h, out_w) -> np.ndarray:
    """B forward matrices (2 x 3) and flips -> one uint8 array: double[B][6] inverses, double[B][6] forward matrices, int[B] flips
    (what augment_device reads from one device tensor)"""
    b = len(m_fwd)
    if b < 1 or len(flips) != b:
        raise PosePafError("one matrix and one flip per image")
    d = np.empty((2, b, 6), np.float64)
    for i, m in enumerate(m_fwd):
        m = np.asarray(m, np.float64)
        if m.shape != (2, 3) or not np.isfinite(m).all():
            raise PosePafError(f"image {i}: the matrix must be a finite 2 x 3 array")
        inv = rotation.invert_affine(m)
        check_inverse(inv, out_h, out_w, f"image {i}")
        d[0, i], d[1, i] = inv.reshape(6), m.reshape(6)
    f = np.array([1 if v else 0 for v in flips], np.int32)
    return np.concatenate([d.reshape(-1).view(np.uint8), f.view(np.uint8)])


def params_bytes(batch: int) -> int:
    return batch * (PARAM_DOUBLES * 8 + 4)


def _check_device_args(images, mask_miss, mask_all, sizes, joints, n_people, params, out_hw, dtype, border, target, out):
    import torch
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8:
        raise PosePafError("images must be a uint8 (B, slot_h, slot_w, 3) device tensor")
    b, slot_h, slot_w = (int(v) for v in images.shape[:3])
    if b < 1 or b > 65535 or slot_h < 1 or slot_w < 1 or slot_h > 32768 or slot_w > 32768:
        raise PosePafError(f"images must hold 1..65535 slots of 1..32768 pixels a side, got {tuple(images.shape)}")
    for name, m in (("mask_miss", mask_miss), ("mask_all", mask_all)):
        if m is not None and (not isinstance(m, torch.Tensor) or m.dtype != torch.uint8 or tuple(m.shape) != (b, slot_h, slot_w)):
            raise PosePafError(f"{name} must be a uint8 ({b}, {slot_h}, {slot_w}) device tensor or None")
    if sizes is not None and (not isinstance(sizes, torch.Tensor) or sizes.dtype != torch.int32 or tuple(sizes.shape) != (2, b)):
        raise PosePafError(f"sizes must be an int32 (2, {b}) device tensor (heights, then widths) or None")
    if not isinstance(joints, torch.Tensor) or joints.dim() != 4 or tuple(joints.shape[2:]) != (sk.NUM_PART, 3) \
            or joints.shape[0] != b or joints.dtype != torch.float64:
        raise PosePafError(f"joints must be a float64 ({b}, max_people, 18, 3) device tensor")
    p = int(joints.shape[1])
    if p < 1 or p > SCENE_MAX_PEOPLE:
        raise PosePafError(f"max_people must be 1..{SCENE_MAX_PEOPLE}, got {p}")
    if not isinstance(n_people, torch.Tensor) or n_people.dtype != torch.int32 or tuple(n_people.shape) != (b,):
        raise PosePafError(f"n_people must be an int32 ({b},) device tensor")
    if params is not None and (not isinstance(params, torch.Tensor) or params.dtype != torch.uint8
                               or tuple(params.shape) != (params_bytes(b),) or params.data_ptr() % 8):
        raise PosePafError(f"params must be the uint8 ({params_bytes(b)},) device tensor of pack_params")
    try:
        out_h, out_w = (int(v) for v in out_hw)
    except (TypeError, ValueError):
        raise PosePafError(f"out_hw must be (out_h, out_w), got {out_hw!r}") from None
    if out_h < 4 or out_w < 4 or out_h % 4 or out_w % 4 or out_h > 32768 or out_w > 32768:
        raise PosePafError(f"out_hw must be positive multiples of 4 up to 32768, got {out_h} x {out_w}")
    if dtype not in (torch.float16, torch.float32):
        raise PosePafError(f"dtype must be torch.float16 or torch.float32, got {dtype}")
    try:
        border = tuple(int(v) for v in border)
    except (TypeError, ValueError):
        border = ()
    if len(border) != 3 or any(not 0 <= v <= 255 for v in border):
        raise PosePafError("border must be three values in 0..255")
    ch, cw = out_h // 4, out_w // 4
    if target is not None:
        if not isinstance(target, torch.Tensor) or target.dim() not in (4, 5) or target.shape[0] != b \
                or tuple(target.shape[-3:]) != (sk.NUM_CH, ch, cw) or target.dtype not in (torch.float16, torch.float32) \
                or not target.is_contiguous():
            raise PosePafError(f"target must be a contiguous float16 / float32 ({b}, 50, {ch}, {cw}) or ({b}, n, 50, {ch}, {cw}) tensor")
    want = {"image": ((b, out_h, out_w, 3), dtype), "mask_miss": ((b, ch, cw), torch.float32), "fg": ((b, ch, cw), torch.float32),
            "joints": ((b, p, sk.NUM_PART, 3), torch.float32)}
    out = dict(out or {})
    for name, t in out.items():
        if name not in want or (name == "fg" and target is not None):
            raise PosePafError(f"out[{name!r}]: out takes 'image', 'mask_miss', 'joints' and, without target, 'fg'")
        shape, dt = want[name]
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
            raise PosePafError(f"out[{name!r}] must be a contiguous {dt} {shape} tensor")
    named = [("images", images), ("mask_miss", mask_miss), ("mask_all", mask_all), ("sizes", sizes), ("joints", joints),
             ("n_people", n_people), ("params", params), ("target", target)] + [(f"out[{k!r}]", v) for k, v in out.items()]
    for name, t in named:
        if t is not None and not t.is_cuda:
            raise PosePafError(f"{name} must live on the HIP device: the transformer has no CPU path")
    for name, t in named:
        if t is not None and t.device != images.device:
            raise PosePafError(f"{name} is on {t.device}, images on {images.device}: one device for all")
    for name, t in named[:7]:
        if t is not None and not t.is_contiguous():
            raise PosePafError(f"{name} must be contiguous")
    return b, slot_h, slot_w, p, out_h, out_w, border, want, out


def augment_device(images, mask_miss, mask_all, sizes, joints, n_people, params, out_hw, dtype=None, border=BORDER, target=None,
                   out=None, stream=None):
    """transform_batch behind the host half: `params` is the device copy of pack_params (rewrite it, e.g. between the replays of a
    captured graph, for new draws).  Everything else as transform_batch.  Asynchronous; allocates only the outputs it is not given."""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    if params is None:
        raise PosePafError("params must be the device copy of pack_params")
    b, slot_h, slot_w, p, out_h, out_w, border, want, out = _check_device_args(
        images, mask_miss, mask_all, sizes, joints, n_people, params, out_hw, dtype, border, target, out)
    from . import _lib
    L = _lib.load()
    dev = images.device
    res = {k: out[k] if k in out else (None if (k == "fg" and target is not None) else torch.empty(s, dtype=dt, device=dev))
           for k, (s, dt) in want.items()}
    ch, cw = out_h // 4, out_w // 4
    if target is not None:
        res["fg"] = target[:, 0, sk.NUM_CH - 2] if target.dim() == 5 else target[:, sk.NUM_CH - 2]
        fg_stride = int(target.stride(0))
    else:
        fg_stride = ch * cw
    fg = res["fg"]
    base = params.data_ptr()
    st = torch.cuda.current_stream(dev) if stream is None else stream

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None
    with torch.cuda.device(dev):
        _lib.check(L.pp_augment_batch(
            ptr(images), ptr(sizes), ptr(mask_miss), ptr(mask_all), b, slot_h, slot_w, C.c_void_p(base), C.c_void_p(base + 48 * b),
            C.c_void_p(base + 96 * b), ptr(joints), ptr(n_people), p, out_h, out_w, (C.c_ubyte * 3)(*border), ptr(res["image"]),
            PP_F16 if dtype == torch.float16 else PP_F32, ptr(res["mask_miss"]), ptr(fg), PP_F16 if fg.dtype == torch.float16 else PP_F32,
            fg_stride, ptr(res["joints"]), C.c_void_p(st.cuda_stream)))
    return res["image"], res["mask_miss"], fg, res["joints"]


def transform_batch(images, mask_miss, mask_all, sizes, joints, n_people, augs, objpos, scale_provided, out_hw, *, dtype=None,
                    border=BORDER, target=None, out=None, stream=None, transform_params=None):
    """One batch through the reference's Transformer.transform.
    images: device uint8 (B, slot_h, slot_w, 3), image b in the top-left corner of its slot; mask_miss / mask_all: device uint8
    (B, slot_h, slot_w) or None (constant 255 / 0, as the reference's read_data_new does without masks); sizes: device int32 (2, B),
    heights then widths, or None (every image fills its slot); joints: device float64 (B, P, 18, 3); n_people: device int32 (B,);
    augs: B AugmentSelection; objpos: B (x, y) centres; scale_provided: B numbers; out_hw: the output size, multiples of 4.
    dtype: of the image (default float32); border: the image's border value; target: a (B, [n,] 50, out_h / 4, out_w / 4) tensor whose
    channel 48 (of sample 0) receives the foreground plane in place -- render into it BEFORE this call, the renderer zeroes that
    channel; out: {'image' | 'mask_miss' | 'fg' | 'joints': tensor} to write into; transform_params: a TransformParams (its
    target_dist enters the matrix; default: the reference's).
    -> (image (B, out_h, out_w, 3), mask_miss float32 (B, out_h / 4, out_w / 4), fg (the view of target, or float32 of the same
    shape), joints float32 (B, P, 18, 3) as render_scenes reads them).  The matrices are built and inverted here in float64 and
    uploaded with the flips as one small tensor.  Asynchronous."""
    import torch
    if not isinstance(images, torch.Tensor):
        raise PosePafError("images must be a uint8 (B, slot_h, slot_w, 3) device tensor: the transformer has no CPU path")
    b = int(images.shape[0]) if images.dim() == 4 else 0
    try:
        augs, objpos, scale_provided = list(augs), [tuple(float(v) for v in o) for o in objpos], [float(s) for s in scale_provided]
        out_h, out_w = (int(v) for v in out_hw)
    except (TypeError, ValueError):
        raise PosePafError("augs, objpos ((x, y) per image), scale_provided and out_hw must be sequences of the batch's length") from None
    if b < 1 or len(augs) != b or len(objpos) != b or len(scale_provided) != b or any(len(o) != 2 for o in objpos):
        raise PosePafError(f"one AugmentSelection, one (x, y) objpos and one scale_provided per image ({b})")
    if out_h < 4 or out_w < 4 or out_h % 4 or out_w % 4:
        raise PosePafError(f"out_hw must be positive multiples of 4, got {out_h} x {out_w}")
    for i, (a, s) in enumerate(zip(augs, scale_provided)):
        if not isinstance(a, AugmentSelection):
            raise PosePafError(f"augs[{i}] is not an AugmentSelection")
        if a.tint:
            raise PosePafError(f"augs[{i}].tint: the HSV colour distortion rests on OpenCV's 8-bit colour-conversion tables, which "
                               "cannot be pinned here; it is out of scope (draw with tint_prob = 0)")
        if not (s > 0 and math.isfinite(s)):
            raise PosePafError(f"scale_provided[{i}] must be a positive number, got {s}")
    host = pack_params([affine_matrix(a, o, s, out_h, out_w, transform_params)[0] for a, o, s in zip(augs, objpos, scale_provided)],
                       [a.flip for a in augs], out_h, out_w)
    # every remaining argument -- shapes and types, then the device -- is checked before the upload and the library call
    dt = torch.float32 if dtype is None else dtype
    _check_device_args(images, mask_miss, mask_all, sizes, joints, n_people, None, (out_h, out_w), dt, border, target, out)
    st = torch.cuda.current_stream(images.device) if stream is None else stream
    with torch.cuda.stream(st):
        dev_params = torch.from_numpy(host).to(images.device)
    return augment_device(images, mask_miss, mask_all, sizes, joints, n_people, dev_params, (out_h, out_w), dt, border, target, out, st)
