"""Skeleton rendering from person records: the refactored branch of the demo (demo_image.py:174-192) for a whole batch on the
device (pp_draw_humans_u8, csrc/posepaf_draw.hip), and the NumPy rendering of ONE record that kernel is held to, bit for bit.

The kernel draws what utils.draw.draw_humans(canvas, humans, normalized=False) draws -- discs of radius 4.5 on the joints, lines
of thickness 3 on CocoPairsRender, human after human -- straight from pp_record[b] in device memory.  The ellipse / alpha-blend
style of the original branch (utils.draw.draw_limbs_original, demo_image.py:218-240) stays on NumPy: its angle is
int(degrees(atan2(...))) followed by cos / sin, and a device libm does not promise those bits.  Parity with cv2's own rasteriser
is pinned for neither: the kernel is pinned to utils/draw.py, and draw.py to nothing."""
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


def draw_records(images_dev, records_dev, sizes_dev=None, out=None):
    """Draw every record on its image, one launch on torch's current stream (asynchronous, capturable into a HIP graph).
    images_dev: device uint8 (B, hp, wp, 3) BGR, contiguous; records_dev: device uint8, B packed pp_record (what
    PosePostProcessor.process_async / InferenceEngine.submit return); sizes_dev: device int32 (2, B) heights then widths, or
    None when every image fills its slot; out: the device canvas (same shape as images_dev; may BE images_dev to draw in
    place), allocated when None.  Only each image's own (h, w) corner of `out` is written (with ragged sizes the rest of a
    freshly allocated canvas is uninitialised).  Returns `out`."""
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
    _lib.check(_lib.load().pp_draw_humans_u8(
        C.c_void_p(records_dev.data_ptr()), C.c_void_p(images_dev.data_ptr()), C.c_void_p(out.data_ptr()),
        C.c_void_p(sizes_dev.data_ptr()) if sizes_dev is not None else None, b, hp, wp, C.c_void_p(stream)))
    return out
