"""COCO keypoint evaluation with its per-image half on the device (csrc/posepaf_eval.hip).

    ev = DeviceKeypointEval(device, image_ids, gts)      # packs and uploads the ground truth once
    out = ev.match(records_u8_dev)                       # pp_coco_rows_f32 + pp_oks_match over the whole shard, two launches
    ev.summary(out)                                      # stage B on the host: oks_eval.accumulate_ranges

What is pinned to what: the device flags equal stage A of oks_eval.evaluate_keypoints_ranges (match_image) exactly on inputs whose
OKS values keep a margin to the thresholds (tests/test_gpu_ap_device.py); evaluate_keypoints_ranges equals oks_eval.evaluate_keypoints
for the area range `all`; evaluate_keypoints is pinned to nothing: pycocotools is absent, parity with it is UNPINNED.
A missing library or kernel is an error: nothing here computes the matching on the host instead."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, oks_eval
from ._lib import AP_MAX_DETS, AP_MAX_GT, AP_RANGES, AP_THRESHOLDS, COCO_ROW, GT_ANN_DTYPE, MAX_HUMANS, RECORD_BYTES, PosePafError


def pack_ground_truth(image_ids, gts):
    """-> (pp_gt_ann array, int32 offsets [len(image_ids) + 1]); slot k holds the annotations of image_ids[k] in their order"""
    offsets = np.zeros(len(image_ids) + 1, np.int32)
    anns = []
    for k, iid in enumerate(image_ids):
        g = gts.get(iid, [])
        if len(g) > AP_MAX_GT:
            raise PosePafError(f"image {iid!r} has {len(g)} ground-truth annotations; the device matching holds {AP_MAX_GT} per image")
        anns.extend(g)
        offsets[k + 1] = offsets[k] + len(g)
    packed = np.zeros(len(anns), GT_ANN_DTYPE)
    for j, x in enumerate(anns):
        packed["keypoints"][j] = np.asarray(x["keypoints"], np.float64).reshape(17, 3)
        packed["area"][j] = float(x["area"])
        box = x.get("bbox")
        if box is not None:
            packed["bbox"][j] = np.asarray(box, np.float64)
            packed["has_bbox"][j] = 1
        packed["iscrowd"][j] = 1 if x.get("iscrowd", 0) else 0
        packed["num_keypoints"][j] = int(x.get("num_keypoints", 1))
    return packed, offsets


def stage_b_inputs(scores, match, n_det, n_gt, image_order):
    """Per-image device outputs (B, 20) / (B, 3, 10, 20) / (B,) / (B, 3) -> what oks_eval.accumulate_ranges takes, the images
    taken in `image_order` (ascending image id, as evaluate_keypoints walks them)."""
    perm = np.asarray(image_order, np.int64)
    scores, match, n_det, n_gt = (np.asarray(v)[perm] for v in (scores, match, n_det, n_gt))
    keep = np.arange(AP_MAX_DETS)[None, :] < n_det[:, None]
    return scores[keep].astype(np.float64), match.transpose(1, 2, 0, 3)[:, :, keep], n_gt.sum(axis=0, dtype=np.int64)


class DeviceKeypointEval:
    def __init__(self, device, image_ids, gts):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.image_ids = list(image_ids)
        packed, self.offsets = pack_ground_truth(self.image_ids, gts)     # raises for an image beyond the kernel's capacity
        self.n_gt_total = len(packed)
        self._gt = torch.from_numpy(packed.view(np.uint8).reshape(-1).copy()).to(self.device) if len(packed) else None
        self._offsets = torch.from_numpy(self.offsets).to(self.device)
        self._thr = np.ascontiguousarray(oks_eval.OKS_THRESHOLDS, np.float64)       # the host's own np.linspace values
        self._rng = np.ascontiguousarray(oks_eval.AREA_RANGES, np.float64)
        assert self._thr.shape == (AP_THRESHOLDS,) and self._rng.shape == (AP_RANGES, 2)
        self._lib = _lib.load()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def rows(self, records_u8_dev):
        """records (uint8 device tensor, batch * RECORD_BYTES) -> rows float32 (batch, 128, 52), counts int32 (batch,)"""
        rec = records_u8_dev.contiguous().view(-1)
        batch = rec.numel() // RECORD_BYTES
        if rec.device != self.device or rec.dtype != torch.uint8 or rec.numel() != batch * RECORD_BYTES:
            raise PosePafError("records must be a uint8 tensor of whole pp_record structs on the evaluator's device")
        rows = torch.empty((batch, MAX_HUMANS, COCO_ROW), dtype=torch.float32, device=self.device)
        counts = torch.empty((batch,), dtype=torch.int32, device=self.device)
        if batch:
            _lib.check(self._lib.pp_coco_rows_f32(C.c_void_p(rec.data_ptr()), batch, C.c_void_p(rows.data_ptr()),
                                                  C.c_void_p(counts.data_ptr()), self._stream()))
        return rows, counts

    def match(self, records_u8_dev, image_slots=None, want_oks=False):
        """Rows + matching of a whole shard.  image_slots: for every record the index into image_ids of its image (None: record
        b is image_ids[b]).  -> dict of device tensors rows, counts, order, scores, match, n_det, n_gt (+ oks), and "slots"."""
        batch = records_u8_dev.numel() // RECORD_BYTES
        slots = np.arange(batch, dtype=np.int32) if image_slots is None else np.ascontiguousarray(image_slots, np.int32).reshape(-1)
        if len(slots) != batch or (batch and (slots.min() < 0 or slots.max() >= len(self.image_ids))):
            raise PosePafError("image_slots must name one of the evaluator's images for every record")
        rows, counts = self.rows(records_u8_dev)
        dev = self.device
        out = {"rows": rows, "counts": counts, "slots": slots,
               "order": torch.empty((batch, AP_MAX_DETS), dtype=torch.int32, device=dev),
               "scores": torch.empty((batch, AP_MAX_DETS), dtype=torch.float32, device=dev),
               "match": torch.empty((batch, AP_RANGES, AP_THRESHOLDS, AP_MAX_DETS), dtype=torch.int8, device=dev),
               "n_det": torch.empty((batch,), dtype=torch.int32, device=dev),
               "n_gt": torch.empty((batch, AP_RANGES), dtype=torch.int32, device=dev)}
        if want_oks:
            out["oks"] = torch.empty((batch, AP_MAX_DETS, AP_MAX_GT), dtype=torch.float64, device=dev)
        if not batch:
            return out
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        slots_dev = None if image_slots is None else torch.from_numpy(slots).to(dev)
        rc = self._lib.pp_oks_match(
            C.c_void_p(rows.data_ptr()), C.c_void_p(counts.data_ptr()), batch,
            C.c_void_p(self._gt.data_ptr()) if self._gt is not None else None, C.c_void_p(self._offsets.data_ptr()),
            self.offsets.ctypes.data_as(ip), len(self.image_ids),
            C.c_void_p(slots_dev.data_ptr()) if slots_dev is not None else None,
            slots.ctypes.data_as(ip) if slots_dev is not None else None,
            self._thr.ctypes.data_as(dp), self._rng.ctypes.data_as(dp),
            C.c_void_p(out["order"].data_ptr()), C.c_void_p(out["scores"].data_ptr()), C.c_void_p(out["match"].data_ptr()),
            C.c_void_p(out["n_det"].data_ptr()), C.c_void_p(out["n_gt"].data_ptr()),
            C.c_void_p(out["oks"].data_ptr()) if want_oks else None, self._stream())
        _lib.check(rc)
        return out

    def summary(self, match_outputs) -> dict:
        """stage B (oks_eval.accumulate_ranges, the host function's own) over the outputs of match()"""
        host = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in match_outputs.items()
                if k in ("scores", "match", "n_det", "n_gt", "slots")}
        ids = [self.image_ids[int(s)] for s in host["slots"]]
        order = sorted(range(len(ids)), key=ids.__getitem__)
        return oks_eval.accumulate_ranges(*stage_b_inputs(host["scores"], host["match"], host["n_det"], host["n_gt"], order))
