"""Skeleton rendering from person records, both styles of the demo for a whole batch on the device, and the NumPy renderings
of ONE record the two kernels are held to, bit for bit.

pp_draw_humans_u8 (csrc/posepaf_draw.hip, draw_records) draws the refactored branch (demo_image.py:174-192): what
utils.draw.draw_humans(canvas, humans, normalized=False) draws -- discs of radius 4.5 on the joints, lines of thickness 3 on
CocoPairsRender, human after human -- straight from pp_record[b] in device memory.  pp_draw_limbs_u8 (csrc/posepaf_limbs.hip,
draw_limbs_records) draws the ellipse / alpha-blend style of the original branch (utils.draw.draw_limbs_original,
demo_image.py:218-240) from the same records: its angle int(degrees(atan2(...))) is found without a device libm, and cos / sin
of that integer come from a 361-entry table the HOST's C library fills (pp_limb_angle_table).  Parity with cv2's own rasteriser
is pinned for neither: the kernels are pinned to utils/draw.py, and draw.py to nothing."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import MAX_HUMANS, NUM_PART, RECORD_BYTES, ST_FLOAT_COORDS, PosePafError


def record_to_humans(rec) -> list:
    """One numpy record (RECORD_DTYPE) -> the Human list demo_image.py:83-92 builds from it: a BodyPart per present part
    (peak_id >= 0) named "<human>-<part>", people without any part dropped.  Integer records give int coordinates; a
    PP_ST_FLOAT_COORDS record (original path) gives the float32 values its x / y bit patterns stand for, which draw_humans
    truncates with int(bp.x)."""
    from utils.common import BodyPart, Human
    is_float = bool(int(rec["status"]) & ST_FLOAT_COORDS)
    humans = []
    for hid in range(min(max(int(rec["n_humans"]), 0), MAX_HUMANS)):
        hm = rec["humans"][hid]
        xs, ys = (hm["x"].view(np.float32), hm["y"].view(np.float32)) if is_float else (hm["x"], hm["y"])
        human = Human([])
        for part in range(NUM_PART):
            if hm["peak_id"][part] >= 0:
                x, y = (float(xs[part]), float(ys[part])) if is_float else (int(xs[part]), int(ys[part]))
                human.body_parts[part] = BodyPart("%d-%d" % (hid, part), part, x, y, float(hm["part_score"][part]))
        if human.body_parts:
            human.score = float(hm["score"])
            humans.append(human)
    return humans


def draw_record_numpy(image, rec):
    """The NumPy rendering of one record on a copy of `image` (BGR uint8, (h, w, 3)): what pp_draw_humans_u8 must equal."""
    from utils import draw
    return draw.draw_humans(np.array(image, dtype=np.uint8, copy=True), record_to_humans(rec))


def _draw_arguments(images_dev, records_dev, sizes_dev, out):
    """the checks both renderers make -> (out, the C arguments up to wp, the stream)"""
    import torch
    if not (torch.is_tensor(images_dev) and images_dev.is_cuda and images_dev.dtype == torch.uint8 and images_dev.dim() == 4
            and images_dev.shape[3] == 3 and images_dev.is_contiguous()):
        raise PosePafError("images_dev must be a contiguous device uint8 tensor (B, hp, wp, 3)")
    b, hp, wp = (int(v) for v in images_dev.shape[:3])
    if not (torch.is_tensor(records_dev) and records_dev.is_cuda and records_dev.dtype == torch.uint8
            and records_dev.is_contiguous() and records_dev.numel() >= b * RECORD_BYTES):
        raise PosePafError(f"records_dev must be a contiguous device uint8 tensor of {b} records ({b * RECORD_BYTES} bytes)")
    if sizes_dev is not None and not (torch.is_tensor(sizes_dev) and sizes_dev.is_cuda and sizes_dev.dtype == torch.int32
                                      and sizes_dev.is_contiguous() and tuple(sizes_dev.shape) == (2, b)):
        raise PosePafError(f"sizes_dev must be a contiguous device int32 tensor (2, {b}): heights, then widths")
    if out is None:
        out = torch.empty_like(images_dev)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
              and out.shape == images_dev.shape):
        raise PosePafError("out must be a contiguous device uint8 tensor of the images' shape")
    stream = torch.cuda.current_stream(images_dev.device).cuda_stream
    args = (C.c_void_p(records_dev.data_ptr()), C.c_void_p(images_dev.data_ptr()), C.c_void_p(out.data_ptr()),
            C.c_void_p(sizes_dev.data_ptr()) if sizes_dev is not None else None, b, hp, wp)
    return out, args, C.c_void_p(stream)


def draw_records(images_dev, records_dev, sizes_dev=None, out=None):
    """Draw every record on its image, one launch on torch's current stream (asynchronous, capturable into a HIP graph).
    images_dev: device uint8 (B, hp, wp, 3) BGR, contiguous; records_dev: device uint8, B packed pp_record (what
    PosePostProcessor.process_async / InferenceEngine.submit return); sizes_dev: device int32 (2, B) heights then widths, or
    None when every image fills its slot; out: the device canvas (same shape as images_dev; may BE images_dev to draw in
    place), allocated when None.  Only each image's own (h, w) corner of `out` is written (with ragged sizes the rest of a
    freshly allocated canvas is uninitialised).  Returns `out`."""
    out, args, stream = _draw_arguments(images_dev, records_dev, sizes_dev, out)
    _lib.check(_lib.load().pp_draw_humans_u8(*args, stream))
    return out


def record_to_persons(rec):
    """One numpy record (RECORD_DTYPE) -> (person_to_joint_assoc (P, 20, 2) float64, joint_candidates (N, 4) float64): what
    find_humans hands to utils.draw.draw_limbs_original (demo_image.py:218-240).  One candidate row (x, y, score, id) per present
    (human, part) in human-then-part order, its id the row's index; person[part, 0] is that id or -1, person[18, 0] the human's
    score times its part count and person[19, 0] the count (demo_image.humans_from_python_rules divides them); people without
    any part are dropped; n_humans is clamped as in record_to_humans.  Integer records give integral coordinates; a
    PP_ST_FLOAT_COORDS record gives the float32 values its x / y bit patterns stand for, widened."""
    is_float = bool(int(rec["status"]) & ST_FLOAT_COORDS)
    persons, cand = [], []
    for hid in range(min(max(int(rec["n_humans"]), 0), MAX_HUMANS)):
        hm = rec["humans"][hid]
        present = [part for part in range(NUM_PART) if hm["peak_id"][part] >= 0]
        if not present:
            continue
        xs, ys = (hm["x"].view(np.float32), hm["y"].view(np.float32)) if is_float else (hm["x"], hm["y"])
        person = np.full((NUM_PART + 2, 2), -1.0)
        for part in present:
            person[part, 0] = len(cand)
            person[part, 1] = float(hm["part_score"][part])
            cand.append((float(xs[part]), float(ys[part]), float(hm["part_score"][part]), float(len(cand))))
        person[NUM_PART] = float(hm["score"]) * len(present)
        person[NUM_PART + 1] = len(present)
        persons.append(person)
    return (np.array(persons, np.float64).reshape(-1, NUM_PART + 2, 2), np.array(cand, np.float64).reshape(-1, 4))


def persons_to_record(person_to_joint_assoc, joint_candidates, float_coords=True):
    """The inverse, for demo_image.py --device_draw: find_humans' persons and candidates -> one numpy record.  At most MAX_HUMANS
    people are kept; with float_coords (the original path) x / y hold float32 bit patterns, so a float64 candidate is ROUNDED to
    float32 on the way."""
    rec = np.zeros((), _lib.RECORD_DTYPE)
    rec["humans"]["peak_id"] = -1
    rec["status"] = ST_FLOAT_COORDS if float_coords else 0
    people = np.asarray(person_to_joint_assoc, np.float64).reshape(-1, NUM_PART + 2, 2)[:MAX_HUMANS]
    cand = np.asarray(joint_candidates, np.float64).reshape(-1, 4)
    rec["n_humans"] = len(people)
    for hid, person in enumerate(people):
        hm = rec["humans"][hid]
        for part in range(NUM_PART):
            cid = int(person[part, 0])
            if cid < 0:
                continue
            x, y, score = cand[cid, :3]
            hm["peak_id"][part] = cid
            if float_coords:
                hm["x"][part], hm["y"][part] = np.float32(x).view(np.int32), np.float32(y).view(np.int32)
            else:
                hm["x"][part], hm["y"][part] = int(x), int(y)
            hm["part_score"][part] = score
        hm["n_parts"] = int((person[:NUM_PART, 0] >= 0).sum())
        hm["score"] = person[NUM_PART, 0] / max(person[NUM_PART + 1, 0], 1.0)
    return rec


def draw_limbs_record_numpy(image, rec):
    """The NumPy rendering of one record in the original branch's style on a copy of `image` (BGR uint8, (h, w, 3)): what
    pp_draw_limbs_u8 must equal."""
    from utils import draw
    from . import skeleton as sk
    persons, cand = record_to_persons(rec)
    return draw.draw_limbs_original(np.array(image, dtype=np.uint8, copy=True), persons, cand, sk.LIMB_PAIRS, sk.DRAW_LIST)


_ANGLE_TABLES = {}


def limb_angle_table():
    """(361, 2) float64: cos and sin of k degrees for k = -180 .. 180 from the host's C library (pp_limb_angle_table)."""
    tab = np.empty((361, 2), np.float64)
    _lib.check(_lib.load().pp_limb_angle_table(tab.ctypes.data_as(C.POINTER(C.c_double))))
    return tab


def limb_angle_table_dev(device):
    """The device copy of limb_angle_table() for `device`, built on first use and kept.  Call it once outside a graph capture;
    draw_limbs_records finds it here and allocates nothing."""
    import torch
    device = torch.device(device)
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _ANGLE_TABLES:
        _ANGLE_TABLES[key] = torch.from_numpy(limb_angle_table()).to(torch.device("cuda", key))
    return _ANGLE_TABLES[key]


def draw_limbs_records(images_dev, records_dev, sizes_dev=None, out=None):
    """draw_records in the original branch's style (pp_draw_limbs_u8): same arguments, same checks, same return value.  The
    device's angle table comes from limb_angle_table_dev (first use builds it: call it, or this function, once before capturing)."""
    out, args, stream = _draw_arguments(images_dev, records_dev, sizes_dev, out)
    table = limb_angle_table_dev(images_dev.device)
    _lib.check(_lib.load().pp_draw_limbs_u8(*args, C.c_void_p(table.data_ptr()), stream))
    return out
