"""The reference's original (non-refactored) inference path with a real scale search (BASELINE config 5):

    predict (utils/parse_skeletons.py:180-283)  ->  find_peaks (:286-321)  ->  find_connections / find_humans (:324-600)

for a batch of equally sized images, everything on the GPU: per scale the uint8 images are resized (bicubic), padded,
normalised and mirrored, run through the network, flip-averaged, up-sampled x4, cropped, resized to the image size and
accumulated in float64 maps that stay in HBM (105 MB per 512x512 image); peaks, matching and assembly then run at image
resolution.  `multiplier` is the list predict builds at :186 (the reference then hard-codes [1.] at :188; config 5 asks
for three scales).

Images of DIFFERENT sizes run in one batch when their scaled sizes pad to one shape at every scale (bucket_key): a ragged
bucket.  Each image is resized, padded, cropped and searched at its own size (RaggedBucket carries the sizes to the
kernels), so it comes out bit for bit as it does alone."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import skeleton as sk
from ._lib import RECORD_BYTES, PosePafError
from .api import PosePostProcessor, records_to_numpy
from .engine import padded_shape
from .pipeline import preprocess_batch
from .fused_model import to_planes
from .rotation import input_and_map_inverses


def _p(t):
    return C.c_void_p(t.data_ptr())


def scaled_size(h: int, w: int, scale: float):
    """cv2.resize(image, (0, 0), fx=scale, fy=scale): dsize = round(size * scale)"""
    return int(round(h * scale)), int(round(w * scale))


def bucket_key(h: int, w: int, multiplier):
    """Per scale, the padded shape of the network input predict builds from an (h, w) image.  Images with equal keys see an
    input of one shape at every scale, each padded as it would be alone: one forward per scale serves them all."""
    return tuple(padded_shape(*scaled_size(int(h), int(w), float(s))) for s in multiplier)


def group_by_bucket_key(shapes, multiplier, exact: bool = False):
    """Indices of `shapes` grouped for the original path -> [(key, indices, ragged)], groups in order of first appearance,
    indices ascending.  A group whose images all have one size is not ragged: it runs the equal-size code.  exact: group by
    (H, W) itself (what a rotation search needs; key = (H, W))."""
    groups = {}
    for k, (h, w) in enumerate(shapes):
        groups.setdefault((int(h), int(w)) if exact else bucket_key(h, w, multiplier), []).append(k)
    return [(key, members, len({tuple(shapes[k]) for k in members}) > 1) for key, members in groups.items()]


class RaggedUnsupported(PosePafError):
    """the one-launch accumulation refused a ragged bucket (PP_ERR_UNSUPPORTED): run its images in exact-size groups"""


class RaggedBucket:
    """Geometry of ONE ragged batch, on the host and (one upload) on the device: the image sizes, every scale's resized
    sizes (scaled_size) and the pads up to the scale's padded shape.  int32 (1 + 2 n, 2, B): row 0 the sizes (heights, then
    widths -- the layout pp_preprocess_u8_ragged reads), rows 1..n the resized sizes, rows n+1..2n (pad_down, pad_right)."""

    def __init__(self, sizes, multiplier, device):
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        self.multiplier = [float(s) for s in multiplier]
        if not self.sizes or min(min(hw) for hw in self.sizes) <= 0:
            raise PosePafError("a ragged bucket needs at least one image, every size positive")
        keys = {bucket_key(h, w, self.multiplier) for h, w in self.sizes}
        if len(keys) != 1:
            raise PosePafError(f"images of one ragged bucket must share bucket_key; got {sorted(keys)}")
        self.key = keys.pop()
        self.B, n = len(self.sizes), len(self.multiplier)
        self.slot_area = max(h * w for h, w in self.sizes)
        self.host = np.empty((1 + 2 * n, 2, self.B), np.int32)
        self.host[0] = np.asarray(self.sizes, np.int32).T
        for i, s in enumerate(self.multiplier):
            self.host[1 + i] = np.asarray([scaled_size(h, w, s) for h, w in self.sizes], np.int32).T
            self.host[1 + n + i] = np.asarray(self.key[i], np.int32)[:, None] - self.host[1 + i]
        self.dev = torch.from_numpy(self.host).to(device)

    def index(self, scale: float) -> int:
        return self.multiplier.index(float(scale))

    def pads(self, i: int):
        """(pad_down, pad_right) of scale i, each a list over the images"""
        n = len(self.multiplier)
        return self.host[1 + n + i, 0].tolist(), self.host[1 + n + i, 1].tolist()


def resize_images_u8(images_u8: torch.Tensor, scale: float, ragged: RaggedBucket = None, out: torch.Tensor = None) -> torch.Tensor:
    """cv2.resize(image, (0, 0), fx=scale, fy=scale, INTER_CUBIC) of a batch.  ragged: the images are the top-left corners of
    (slot_h, slot_w) slots; the result has slots of the scale's padded shape (what the ragged pre-processing reads), image b
    in the top-left scaled_size corner; bytes outside the corners are not written (`out`: write into this tensor)."""
    B, H, W, _ = images_u8.shape
    if ragged is not None:
        i = ragged.index(scale)
        dh, dw = ragged.key[i]
        if B != ragged.B or H * W < ragged.slot_area or any(h > H or w > W for h, w in ragged.sizes):
            raise PosePafError("the image slots do not hold the ragged bucket's images")
        if scale == 1.0 and (H, W) == (dh, dw) and out is None:
            return images_u8
        if out is None:
            out = torch.empty((B, dh, dw, 3), dtype=torch.uint8, device=images_u8.device)
        if tuple(out.shape) != (B, dh, dw, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
            raise PosePafError(f"out must be a contiguous uint8 ({B}, {dh}, {dw}, 3) tensor")
        st = C.c_void_p(torch.cuda.current_stream(images_u8.device).cuda_stream)
        _lib.check(_lib.load().pp_resize_u8_cubic_ragged(_p(images_u8.contiguous()), _p(out), B, H, W, dh, dw, _p(ragged.dev[0]),
                                                         _p(ragged.dev[1 + i]), 1.0 / scale, 1.0 / scale, st))
        return out
    if scale == 1.0:
        return images_u8
    dh, dw = scaled_size(H, W, scale)
    out = torch.empty((B, dh, dw, 3), dtype=torch.uint8, device=images_u8.device)
    st = C.c_void_p(torch.cuda.current_stream(images_u8.device).cuda_stream)
    _lib.check(_lib.load().pp_resize_u8_cubic(_p(images_u8.contiguous()), _p(out), B, H, W, dh, dw, 1.0 / scale, 1.0 / scale, st))
    return out


def preprocess_ragged(scaled_u8: torch.Tensor, sizes_dev: torch.Tensor, dtype=torch.float16) -> torch.Tensor:
    """pad / normalise / mirror of a ragged batch whose slots have the padded shape (pp_preprocess_u8_ragged): image b is
    padded from its own (h_b, w_b) = sizes_dev[:, b] exactly as preprocess_batch pads it alone -> (2B, Hp, Wp, 3)"""
    B, hp, wp, _ = scaled_u8.shape
    x = torch.empty((2 * B, hp, wp, 3), dtype=dtype, device=scaled_u8.device)
    st = C.c_void_p(torch.cuda.current_stream(scaled_u8.device).cuda_stream)
    _lib.check(_lib.load().pp_preprocess_u8_ragged(_p(scaled_u8), _p(sizes_dev), _p(x),
                                                   _lib.PP_F16 if dtype == torch.float16 else _lib.PP_F32, B, hp, wp,
                                                   sk.PAD_VALUE, 1, st))
    return x


class OriginalPathProcessor:
    """Accumulators at image resolution + the kernels behind them.  accumulate() only REGISTERS a scale; the arithmetic of all
    registered scales runs in ONE launch (pp_original_accumulate_all: the accumulators are written once, never re-read) when the
    accumulators are first needed -- by finish(), or by reading .heat_acc / .paf_acc.

    Ragged form (slot_area given, img_h = img_w = None): the accumulators are (max_batch, C, slot_area); reset(ragged) names
    the batch's RaggedBucket, accumulate() takes per-image pads, and image b's maps are heat_view(b) / paf_view(b)."""

    def __init__(self, post: PosePostProcessor, img_h: int, img_w: int, max_batch: int, device=None, slot_area: int = None):
        if post.maxp > 64:
            raise _lib.PosePafError("the original path needs max_peaks_per_part <= 64 (float64 tables in LDS)")
        self.post, self.H, self.W, self.B = post, img_h, img_w, max_batch
        dev = device or torch.device("cuda", post.device)
        self.slot_area = None if slot_area is None else int(slot_area)
        self._ragged = None       # the RaggedBucket of the batch being accumulated
        plane = (img_h, img_w) if slot_area is None else (self.slot_area,)
        self._heat = torch.zeros((max_batch, sk.NUM_HEAT) + plane, dtype=torch.float64, device=dev)
        self._paf = torch.zeros((max_batch, sk.NUM_LIMB) + plane, dtype=torch.float64, device=dev)
        self.mask = torch.empty((max_batch, sk.NUM_PART) + plane, dtype=torch.uint8, device=dev)
        self.peaks64 = torch.empty((max_batch, sk.NUM_PART, post.maxp, 4), dtype=torch.float64, device=dev)
        self.records = torch.empty(max_batch * RECORD_BYTES, dtype=torch.uint8, device=dev)
        self._scratch = {}
        self._pending = []        # [(maps, pad_down, pad_right, n_scales, flip, m_inv)] registered, not yet accumulated
        self._need_zero = False   # reset() was called and nothing has written the accumulators since
        self.fused = True         # False: always the per-scale chain (pp_original_accumulate), for A/B measurements

    @property
    def heat_acc(self) -> torch.Tensor:
        self._flush()
        return self._heat

    @property
    def paf_acc(self) -> torch.Tensor:
        self._flush()
        return self._paf

    def reset(self, ragged: RaggedBucket = None):
        """ragged: the sizes of the batch that follows (a processor built with slot_area); None: the equal-size form"""
        if (ragged is not None) != (self.slot_area is not None):
            raise PosePafError("a ragged bucket runs on a processor built with slot_area, and only there")
        if ragged is not None and (ragged.B > self.B or ragged.slot_area > self.slot_area):
            raise PosePafError(f"the ragged bucket ({ragged.B} images, {ragged.slot_area} pixels) exceeds the processor's slots")
        self._ragged = ragged
        self._pending = []
        self._need_zero = True

    def heat_view(self, b: int) -> torch.Tensor:
        """image b's (20, H_b, W_b) heat accumulator of the ragged batch: the dense head of its slot"""
        h, w = self._ragged.sizes[b]
        return self.heat_acc[b, :, : h * w].view(sk.NUM_HEAT, h, w)

    def paf_view(self, b: int) -> torch.Tensor:
        """image b's (30, H_b, W_b) limb accumulator of the ragged batch"""
        h, w = self._ragged.sizes[b]
        return self.paf_acc[b, :, : h * w].view(sk.NUM_LIMB, h, w)

    def accumulate(self, maps: torch.Tensor, pad_down, pad_right, n_scales: int, flip: bool = True, m_inv=None):
        """maps: (B, 2|1, 50, h, w) network output of ONE scale (padded input).  The tensor must stay alive until finish().
        n_scales: the divisor, len(multiplier) * len(rotation_search).  m_inv: a rotated entry (utils/parse_skeletons.py:265-267):
        the x4 map is warped with cv2.warpAffine(M_rev) before the crop, m_inv = invert_affine(M_rev) (posepaf.rotation).
        Ragged batch: pad_down / pad_right are sequences, one value per image; a rotated entry is refused."""
        if self._ragged is not None:
            if m_inv is not None:
                raise PosePafError("a ragged bucket takes no rotated entry: group images by exact size for a rotation search")
            pad_down, pad_right = [int(v) for v in pad_down], [int(v) for v in pad_right]
            if len(pad_down) != self._ragged.B or len(pad_right) != self._ragged.B or maps.shape[0] != self._ragged.B:
                raise PosePafError("a ragged accumulate needs the bucket's batch and one (pad_down, pad_right) per image")
            self._pending.append((maps, pad_down, pad_right, int(n_scales), bool(flip), None))
            return
        if m_inv is not None:
            m_inv = np.ascontiguousarray(np.asarray(m_inv, np.float64).reshape(6))
        self._pending.append((maps, int(pad_down), int(pad_right), int(n_scales), bool(flip), m_inv))

    def _flush_ragged(self, pend):
        """every registered scale of a ragged batch in one launch (pp_original_accumulate_all_ragged); there is no per-scale
        form: RaggedUnsupported tells the caller to run exact-size groups"""
        rg = self._ragged
        maps0, _, _, n_scales, flip, _ = pend[0]
        n = len(pend)
        if not (n == n_scales and all(m.dtype == maps0.dtype and q == n_scales and f == flip and m.is_contiguous()
                                      for m, _, _, q, f, _ in pend)):
            raise PosePafError("a ragged batch accumulates the complete scale list, one dtype and flip setting, in one launch")
        if n > 6:
            raise RaggedUnsupported("more than 6 scales")
        pads = np.ascontiguousarray([[p[1], p[2]] for p in pend], np.int32)            # (n, 2, B)
        pads_dev = torch.from_numpy(pads).to(maps0.device)
        ptrs = (C.c_void_p * n)(*[m.data_ptr() for m, *_ in pend])
        hs = (C.c_int * n)(*[m.shape[3] for m, *_ in pend])
        ws = (C.c_int * n)(*[m.shape[4] for m, *_ in pend])
        ip = C.POINTER(C.c_int)
        code = _lib.PP_F16 if maps0.dtype == torch.float16 else _lib.PP_F32
        st = C.c_void_p(torch.cuda.current_stream(maps0.device).cuda_stream)
        rc = _lib.load().pp_original_accumulate_all_ragged(self.post.ctx, rg.B, n, ptrs, code, hs, ws, int(flip),
                                                           rg.host[0].ctypes.data_as(ip), _p(rg.dev[0]), pads.ctypes.data_as(ip),
                                                           _p(pads_dev), self.slot_area, _p(self._heat), _p(self._paf), st)
        if rc == -6:
            raise RaggedUnsupported("a scale's tiles do not fit LDS for an image of the bucket")
        _lib.check(rc, self.post.ctx)
        self._need_zero = False

    def _chain(self, maps, pad_down, pad_right, n_scales, flip, m_inv=None):
        """one scale through the round-2 chain: flip-average -> x4 map -> crop -> resize -> read-modify-write accumulate"""
        if m_inv is not None:
            return self._chain_affine(maps, pad_down, pad_right, n_scales, flip, m_inv)
        B, _, _, h, w = maps.shape
        key = (B, h, w)
        if key not in self._scratch:
            self._scratch[key] = (torch.empty((B, sk.NUM_CH, h, w), dtype=torch.float32, device=maps.device),
                                  torch.empty((B, sk.NUM_CH, 4 * h, 4 * w), dtype=torch.float32, device=maps.device))
        planar, up = self._scratch[key]
        code = _lib.PP_F16 if maps.dtype == torch.float16 else _lib.PP_F32
        st = C.c_void_p(torch.cuda.current_stream(maps.device).cuda_stream)
        _lib.check(_lib.load().pp_original_accumulate(self.post.ctx, B, _p(maps), code, h, w, int(flip), pad_down, pad_right,
                                                      self.H, self.W, n_scales, _p(planar), _p(up), _p(self._heat),
                                                      _p(self._paf), st), self.post.ctx)

    def _chain_affine(self, maps, pad_down, pad_right, n_scales, flip, m_inv):
        """one rotated entry through the chain: flip-average -> x4 map -> warpAffine(M_rev) -> crop -> resize -> accumulate"""
        B, _, _, h, w = maps.shape
        key = (B, h, w, "warp")
        if key not in self._scratch:
            self._scratch[key] = tuple(torch.empty(shape, dtype=torch.float32, device=maps.device) for shape in
                                       ((B, sk.NUM_CH, h, w), (B, sk.NUM_CH, 4 * h, 4 * w), (B, sk.NUM_CH, 4 * h, 4 * w)))
        planar, up, warped = self._scratch[key]
        code = _lib.PP_F16 if maps.dtype == torch.float16 else _lib.PP_F32
        st = C.c_void_p(torch.cuda.current_stream(maps.device).cuda_stream)
        _lib.check(_lib.load().pp_original_accumulate_affine(self.post.ctx, B, _p(maps), code, h, w, int(flip), pad_down, pad_right,
                                                             self.H, self.W, n_scales, m_inv.ctypes.data_as(C.POINTER(C.c_double)),
                                                             _p(planar), _p(up), _p(warped), _p(self._heat), _p(self._paf), st),
                   self.post.ctx)

    def _flush(self):
        pend, self._pending = self._pending, []
        if not pend:
            if self._need_zero:
                self._heat.zero_()
                self._paf.zero_()
                self._need_zero = False
            return
        if self._ragged is not None:
            return self._flush_ragged(pend)
        maps0, _, _, n_scales, flip, _ = pend[0]
        B = maps0.shape[0]
        same = all(m.shape[0] == B and m.dtype == maps0.dtype and n == n_scales and f == flip and m.is_contiguous()
                   for m, _, _, n, f, _ in pend)
        rotated = any(p[5] is not None for p in pend)
        if self.fused and self._need_zero and same and len(pend) <= 6 and B <= self.B:
            L = _lib.load()
            n = len(pend)
            ptrs = (C.c_void_p * n)(*[m.data_ptr() for m, *_ in pend])
            hs = (C.c_int * n)(*[m.shape[3] for m, *_ in pend])
            ws = (C.c_int * n)(*[m.shape[4] for m, *_ in pend])
            pd = (C.c_int * n)(*[p[1] for p in pend])
            pr = (C.c_int * n)(*[p[2] for p in pend])
            code = _lib.PP_F16 if maps0.dtype == torch.float16 else _lib.PP_F32
            st = C.c_void_p(torch.cuda.current_stream(maps0.device).cuda_stream)
            # n_div of the kernel is the number of scales it is given: only the complete set goes through it
            if n == n_scales and rotated:   # the warped instance; entries without a matrix take the plain steps in it
                dp = C.POINTER(C.c_double)
                mats = (dp * n)(*[(p[5].ctypes.data_as(dp) if p[5] is not None else dp()) for p in pend])
                rc = L.pp_original_accumulate_all_affine(self.post.ctx, B, n, ptrs, code, hs, ws, int(flip), pd, pr, mats, self.H,
                                                         self.W, _p(self._heat), _p(self._paf), st)
                if rc == 0:
                    self._need_zero = False
                    return
                if rc != -6:
                    _lib.check(rc, self.post.ctx)
            elif n == n_scales:
                rc = L.pp_original_accumulate_all(self.post.ctx, B, n, ptrs, code, hs, ws, int(flip), pd, pr, self.H, self.W,
                                                  _p(self._heat), _p(self._paf), st)
                if rc == 0:
                    self._need_zero = False
                    return
                if rc != -6:   # PP_ERR_UNSUPPORTED (a scale too large for the tiles): fall through to the chain
                    _lib.check(rc, self.post.ctx)
        if self._need_zero:
            self._heat.zero_()
            self._paf.zero_()
            self._need_zero = False
        for m, pdn, prt, n, f, mi in pend:
            self._chain(m, pdn, prt, n, f, mi)

    def finish(self, batch: int, thre1: float = 0.1, test_cfg=None) -> torch.Tensor:
        """test_cfg: None = what the post-processor's context holds; a dict = set it on the context first (keys moved off the
        INI defaults, see PosePostProcessor.set_test_cfg) and take thre1 from it when it has one."""
        self._flush()
        if test_cfg is not None:
            self.post.set_test_cfg(test_cfg)
            if "thre1" in test_cfg:
                thre1 = float(test_cfg["thre1"])
        st = C.c_void_p(torch.cuda.current_stream(self._heat.device).cuda_stream)
        if self._ragged is not None:
            rg = self._ragged
            if batch != rg.B:
                raise PosePafError(f"finish({batch}) of a ragged batch of {rg.B} images")
            _lib.check(_lib.load().pp_original_finish_ragged(self.post.ctx, batch, rg.host[0].ctypes.data_as(C.POINTER(C.c_int)),
                                                             _p(rg.dev[0]), self.slot_area, float(thre1), _p(self._heat),
                                                             _p(self._paf), _p(self.mask), _p(self.peaks64), _p(self.records), st),
                       self.post.ctx)
            return self.records[: batch * RECORD_BYTES]
        _lib.check(_lib.load().pp_original_finish(self.post.ctx, batch, self.H, self.W, float(thre1), _p(self._heat),
                                                  _p(self._paf), _p(self.mask), _p(self.peaks64), _p(self.records), st),
                   self.post.ctx)
        return self.records[: batch * RECORD_BYTES]

    @torch.no_grad()
    def run(self, model, images_u8: torch.Tensor, multiplier, dtype=torch.float16, thre1: float = 0.1,
            angles=(0.0,), test_cfg=None, sizes=None) -> np.ndarray:
        """images (B, H, W, 3) uint8 on the GPU -> records (float coordinates, PP_ST_FLOAT_COORDS).
        Every (scale, angle) of product(multiplier, angles) is one entry (utils/parse_skeletons.py:196), each divided by
        len(multiplier) * len(angles); angle 0 takes the unrotated steps.
        sizes: HOST list of (H_b, W_b): a ragged bucket, image b in the top-left corner of its (H, W) slot; no rotation."""
        B = images_u8.shape[0]
        angles = [float(a) for a in angles]
        n_div = len(multiplier) * len(angles)
        if sizes is not None:
            if any(a != 0.0 for a in angles):
                raise PosePafError("a ragged bucket runs without rotation search: group images by exact size for that")
            rg = RaggedBucket(sizes, multiplier, images_u8.device)
            self.reset(rg)
            for i, scale in enumerate(rg.multiplier):
                scaled = resize_images_u8(images_u8, scale, ragged=rg)
                out = model(preprocess_ragged(scaled, rg.dev[1 + i], dtype))
                maps = to_planes(out[-1][0] if isinstance(out, (list, tuple)) else out)
                maps = maps.view(B, 2, sk.NUM_CH, maps.shape[-2], maps.shape[-1])
                self.accumulate(maps, *rg.pads(i), n_div)
            return records_to_numpy(self.finish(B, thre1, test_cfg))
        self.reset()
        for scale in multiplier:
            scaled = resize_images_u8(images_u8, float(scale))
            sh, sw = scaled.shape[1:3]
            for angle in angles:
                ph, pw = -(-sh // sk.MAX_DOWNSAMPLE) * sk.MAX_DOWNSAMPLE, -(-sw // sk.MAX_DOWNSAMPLE) * sk.MAX_DOWNSAMPLE
                m_in, m_rev = input_and_map_inverses(ph, pw, angle)
                x = preprocess_batch(scaled, True, dtype, m_inv=m_in)       # pad to /64, /255, rotate, mirror
                out = model(x)
                maps = to_planes(out[-1][0] if isinstance(out, (list, tuple)) else out)
                maps = maps.view(B, 2, sk.NUM_CH, maps.shape[-2], maps.shape[-1])
                self.accumulate(maps, ph - sh, pw - sw, n_div, m_inv=m_rev)
        return records_to_numpy(self.finish(B, thre1, test_cfg))


def record_float_coords(rec):
    """x / y of a PP_ST_FLOAT_COORDS record as float32 arrays (n_humans, 18)."""
    n = int(rec["n_humans"])
    return rec["humans"]["x"][:n].view(np.float32), rec["humans"]["y"][:n].view(np.float32)
