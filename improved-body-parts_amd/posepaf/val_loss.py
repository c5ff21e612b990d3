"""The reference's validation loss on the device (pp_focal_l2_terms, csrc/posepaf_loss.hip): MultiTaskLoss.focal_l2_loss summed over
stacks and scales (models/loss_model.py:23-81, :133-161) as per-image terms, their weighted combination and a running meter.

    terms = focal_l2_terms(preds, target)          # device float64 (T, K, B): stack, scale, image
    loss = combine(terms)                          # 0-d device float64: the scalar MultiTaskLoss.forward returns
    loss.backward()                                # when a prediction requires grad: pp_focal_l2_grad (focal_l2_grad is the raw entry)
    meter = ValLossMeter(); meter.update(terms); meter.summary()

preds is what FusedIMHN.forward(x, all_preds=True) returns (or any list of lists of (B, 50, h_s, w_s) device tensors), target what
synth_device.render_scenes renders.  The contract -- pooling, the float32 foreground comparison, the exact-mean definition of a
0.01f plateau, the mask -- is INTEGRATION section 15.  There is no CPU path: host tensors are refused.
"""
from __future__ import annotations

import ctypes as C

from . import skeleton as sk
from ._lib import LOSS_MAX_SCALES, LOSS_MAX_STACKS, LOSS_PLAIN_L2, PP_F16, PP_F32, PosePafError

NSTACK_WEIGHT = (1, 1, 1, 1)                      # config/config.py:17-20 of the reference
SCALE_WEIGHT = (0.1, 0.2, 0.4, 1.6, 6.4)
MULTI_TASK_WEIGHT, KEYPOINT_TASK_WEIGHT = 0.1, 3.0


def _layout(t):
    """0: planes; S >= 50: pixel-major with S elements per pixel (50 = channels_last, 64 = the [:, :50] view of a fused head's
    output); None: neither.  Strides of extent-1 dimensions say nothing and are not looked at."""
    if t.is_contiguous():
        return 0
    b, c, h, w = t.shape
    sb, sc, sh, sw = t.stride()
    if sc != 1 or sw < c or sw > (1 << 20):
        return None
    if (h > 1 and sh != w * sw) or (b > 1 and sb != h * w * sw):
        return None
    return int(sw)


def _check_args(preds, target, mask, out, workspace):
    import torch
    if not isinstance(preds, (list, tuple)) or not preds or not all(isinstance(p, (list, tuple)) and p for p in preds):
        raise PosePafError("preds must be a non-empty list (stacks) of non-empty lists (scales) of device tensors")
    T, K = len(preds), len(preds[0])
    if T > LOSS_MAX_STACKS or K > LOSS_MAX_SCALES:
        raise PosePafError(f"at most {LOSS_MAX_STACKS} stacks and {LOSS_MAX_SCALES} scales, got {T} x {K}")
    if any(len(p) != K for p in preds):
        raise PosePafError("every stack must hold the same number of scales")
    if not isinstance(target, torch.Tensor) or target.dim() not in (4, 5) or target.shape[-3] != sk.NUM_CH:
        raise PosePafError("target must be a (B, 50, H, W) or (B, n, 50, H, W) device tensor")
    if target.dtype not in (torch.float16, torch.float32):
        raise PosePafError(f"target must be float16 or float32, got {target.dtype}")
    B, (H, W) = int(target.shape[0]), (int(v) for v in target.shape[-2:])
    if B < 1 or B > 65535 or H < 1 or W < 1:
        raise PosePafError(f"target must hold 1..65535 images of at least one pixel, got {tuple(target.shape)}")
    dtype = preds[0][0].dtype if isinstance(preds[0][0], torch.Tensor) else None
    if dtype not in (torch.float16, torch.float32):
        raise PosePafError(f"predictions must be float16 or float32 tensors, got {dtype}")
    sizes = []
    for t_, stack in enumerate(preds):
        for s_, p in enumerate(stack):
            if not isinstance(p, torch.Tensor) or p.dim() != 4 or p.shape[0] != B or p.shape[1] != sk.NUM_CH:
                raise PosePafError(f"preds[{t_}][{s_}] must be a ({B}, 50, h, w) tensor")
            if p.dtype != dtype:
                raise PosePafError(f"preds[{t_}][{s_}] is {p.dtype}, preds[0][0] is {dtype}: one dtype for all predictions")
            h, w = int(p.shape[2]), int(p.shape[3])
            if not (1 <= h <= H and 1 <= w <= W):
                raise PosePafError(f"preds[{t_}][{s_}] is {h} x {w}: outside 1..{H} x 1..{W} of the target")
            if t_ == 0:
                sizes.append((h, w))
            elif sizes[s_] != (h, w):
                raise PosePafError(f"preds[{t_}][{s_}] is {h} x {w}, preds[0][{s_}] is {sizes[s_][0]} x {sizes[s_][1]}")
    if mask is not None and (not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (B, H, W) or mask.dtype != torch.float32):
        raise PosePafError(f"mask must be a float32 ({B}, {H}, {W}) tensor or None")
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (T, K, B) or out.dtype != torch.float64
                            or not out.is_contiguous()):
        raise PosePafError(f"out must be a contiguous float64 ({T}, {K}, {B}) tensor")
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1
                                  or not workspace.is_contiguous()):
        raise PosePafError("workspace must be a contiguous 1-d uint8 tensor")
    named = [("target", target), ("mask", mask), ("out", out), ("workspace", workspace)]
    named += [(f"preds[{t_}][{s_}]", p) for t_, stack in enumerate(preds) for s_, p in enumerate(stack)]
    for name, t in named:
        if t is not None and not t.is_cuda:
            raise PosePafError(f"{name} must live on the HIP device: focal_l2_terms has no CPU path")
    for name, t in named:
        if t is not None and t.device != target.device:
            raise PosePafError(f"{name} is on {t.device}, target on {target.device}: one device for all")
    return T, K, B, H, W, sizes, dtype


def workspace_bytes(batch: int, n_stacks: int, sizes) -> int:
    """bytes of the workspace focal_l2_terms needs for predictions of `sizes` [(h_s, w_s)] (pp_focal_l2_workspace_bytes)"""
    from . import _lib
    k = len(sizes)
    hs, ws = (C.c_int * k)(*[int(h) for h, _ in sizes]), (C.c_int * k)(*[int(w) for _, w in sizes])
    n = int(_lib.load().pp_focal_l2_workspace_bytes(int(batch), int(n_stacks), k, hs, ws))
    if n < 0:
        _lib.check(n)
    return n


def _prepare(preds, target, mask, T, K, H, W, esz):
    """-> target and its image stride as the library reads them, the contiguous mask, keep[s][t] (the tensors the kernel reads: the
    caller's where their layout is one it takes, contiguous copies elsewhere), layout[s] and {layout: [scales]}"""
    if target.dim() == 5:
        image_stride = int(target.shape[1]) * sk.NUM_CH * H * W
        if not target.is_contiguous():
            target, image_stride = target[:, 0].contiguous(), sk.NUM_CH * H * W
    else:
        target, image_stride = target.contiguous(), sk.NUM_CH * H * W
    mask = mask.contiguous() if mask is not None else None
    # one library call per layout: the scales whose tensors (of every stack) share a pixel stride go together
    keep, layout = [], []
    for s in range(K):
        ls = {_layout(preds[t][s]) for t in range(T)}
        ok = len(ls) == 1 and None not in ls and all(preds[t][s].data_ptr() % esz == 0 for t in range(T))
        layout.append(ls.pop() if ok else 0)
        keep.append([preds[t][s] if ok else preds[t][s].contiguous() for t in range(T)])
    groups = {}
    for s in range(K):
        groups.setdefault(layout[s], []).append(s)
    return target, image_stride, mask, keep, layout, groups


def _check_weights(multi_task_weight, keypoint_task_weight):
    if not (float(multi_task_weight) == float(multi_task_weight) and float(keypoint_task_weight) == float(keypoint_task_weight)):
        raise PosePafError("the task weights must be numbers")


def _terms(shape, preds, target, mask, multi_task_weight, keypoint_task_weight, plain_l2, out, workspace, stream):
    """focal_l2_terms behind its argument checks"""
    import torch
    T, K, B, H, W, sizes, dtype = shape
    from . import _lib
    L = _lib.load()
    dev = target.device
    esz = 2 if dtype == torch.float16 else 4
    target, image_stride, mask, keep, layout, groups = _prepare(preds, target, mask, T, K, H, W, esz)
    if out is None:
        out = torch.empty((T, K, B), dtype=torch.float64, device=dev)
    need = max(workspace_bytes(B, T, [sizes[s] for s in members]) for members in groups.values())
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.numel() < need or workspace.data_ptr() % 8:
        raise PosePafError(f"workspace must hold {need} bytes on an 8-byte boundary, got {workspace.numel()}")
    st = torch.cuda.current_stream(dev) if stream is None else stream
    flags = LOSS_PLAIN_L2 if plain_l2 else 0
    with torch.cuda.device(dev), torch.cuda.stream(st):
        for stride, members in groups.items():
            k = len(members)
            whole = k == K
            dst = out if whole else torch.empty((T, k, B), dtype=torch.float64, device=dev)
            table = (C.c_void_p * (T * k))(*[keep[s][t].data_ptr() for t in range(T) for s in members])
            hs, ws = (C.c_int * k)(*[sizes[s][0] for s in members]), (C.c_int * k)(*[sizes[s][1] for s in members])
            _lib.check(L.pp_focal_l2_terms(
                table, PP_F16 if dtype == torch.float16 else PP_F32, int(stride), C.c_void_p(target.data_ptr()),
                PP_F16 if target.dtype == torch.float16 else PP_F32, image_stride, C.c_void_p(mask.data_ptr()) if mask is not None else None,
                B, H, W, T, k, hs, ws, float(multi_task_weight), float(keypoint_task_weight), flags, C.c_void_p(workspace.data_ptr()),
                C.c_void_p(dst.data_ptr()), C.c_void_p(st.cuda_stream)))
            if not whole and torch.cuda.is_current_stream_capturing():
                for j, s in enumerate(members):        # (an index list is a host tensor the capture could not transfer)
                    out[:, s].copy_(dst[:, j])
            elif not whole:
                out[:, members] = dst
    return out


def focal_l2_terms(preds, target, mask=None, multi_task_weight: float = MULTI_TASK_WEIGHT, keypoint_task_weight: float = KEYPOINT_TASK_WEIGHT,
                   plain_l2: bool = False, out=None, workspace=None, stream=None):
    """preds[t][s]: device (B, 50, h_s, w_s) float16 / float32 -- planes, channels_last or the [:, :50] view of a fused head's
    64-channel output are read where they lie, anything else through a contiguous copy; target: device (B, 50, H, W), or
    (B, n, 50, H, W) of which sample 0 is read in place; mask: device float32 (B, H, W) or None (all ones).
    -> device float64 (T, K, B).  plain_l2: the reference's l2_loss (no focal factor).  out / workspace (uint8, at least
    workspace_bytes): reuse these; stream: a torch stream (default: the current one).  Asynchronous.
    Differentiable with respect to the predictions: with grad mode on and a prediction that requires grad the result is an autograd
    node whose backward is focal_l2_grad (once differentiable; `out` is refused there, and so is a target or mask that requires
    grad: the loss has no derivative with respect to either).  Otherwise the result has no grad_fn."""
    import torch
    shape = _check_args(preds, target, mask, out, workspace)
    _check_weights(multi_task_weight, keypoint_task_weight)
    if torch.is_grad_enabled() and any(p.requires_grad for stack in preds for p in stack):
        if out is not None:
            raise PosePafError("out= cannot receive a result that autograd tracks: leave it out when a prediction requires grad")
        if target.requires_grad or (mask is not None and mask.requires_grad):
            raise PosePafError("the loss has no gradient with respect to the target or the mask: detach them")
        T, K, dtype = shape[0], shape[1], shape[6]
        # a layout the kernel does not take becomes a contiguous copy HERE, outside the node: torch differentiates the copy
        keep = _prepare(preds, target, mask, T, K, shape[3], shape[4], 2 if dtype == torch.float16 else 4)[3]
        flat = [keep[s][t] for t in range(T) for s in range(K)]
        return _function()(target, mask, shape, float(multi_task_weight), float(keypoint_task_weight), bool(plain_l2), workspace, stream, *flat)
    return _terms(shape, preds, target, mask, multi_task_weight, keypoint_task_weight, plain_l2, out, workspace, stream)


def focal_l2_grad(preds, target, term_weights, mask=None, multi_task_weight: float = MULTI_TASK_WEIGHT,
                  keypoint_task_weight: float = KEYPOINT_TASK_WEIGHT, plain_l2: bool = False, stream=None):
    """The gradient of sum(term_weights * focal_l2_terms(preds, target, mask, ...)) with respect to every prediction
    (pp_focal_l2_grad; the arithmetic: INTEGRATION section 16).  term_weights: device float64 (T, K, B); a zero masks an image.
    -> grads[t][s], each with the shape, dtype and strides of preds[t][s]: planes and channels_last tensors get a buffer of their
    own geometry; the [:, :50] view of an S-channel pixel-major tensor gets the same view of a fresh S-channel buffer whose padding
    channels are zeroed once here (the kernel never writes them); any other layout is read through a contiguous copy and gets a
    contiguous gradient.  Nothing is tracked by autograd.  Asynchronous."""
    import torch
    T, K, B, H, W, sizes, dtype = _check_args(preds, target, mask, None, None)
    _check_weights(multi_task_weight, keypoint_task_weight)
    if not isinstance(term_weights, torch.Tensor) or tuple(term_weights.shape) != (T, K, B) or term_weights.dtype != torch.float64:
        raise PosePafError(f"term_weights must be a float64 ({T}, {K}, {B}) tensor")
    if not term_weights.is_cuda or term_weights.device != target.device:
        raise PosePafError(f"term_weights must live on the target's device {target.device}: focal_l2_grad has no CPU path")
    from . import _lib
    L = _lib.load()
    dev = target.device
    esz = 2 if dtype == torch.float16 else 4
    with torch.no_grad():
        target, image_stride, mask, keep, layout, groups = _prepare(preds, target, mask, T, K, H, W, esz)
        st = torch.cuda.current_stream(dev) if stream is None else stream
        flags = LOSS_PLAIN_L2 if plain_l2 else 0
        grads = [[None] * K for _ in range(T)]
        with torch.cuda.device(dev), torch.cuda.stream(st):
            tw = term_weights.detach().contiguous()
            for stride, members in groups.items():
                k = len(members)
                for s in members:
                    h, w = sizes[s]
                    for t in range(T):
                        if stride == 0:
                            grads[t][s] = torch.empty((B, sk.NUM_CH, h, w), dtype=dtype, device=dev)
                        else:
                            buf = torch.empty((B, h, w, stride), dtype=dtype, device=dev)
                            if stride > sk.NUM_CH:
                                buf[..., sk.NUM_CH:].zero_()
                            grads[t][s] = buf.permute(0, 3, 1, 2)[:, :sk.NUM_CH]
                if k == K:
                    part = tw
                elif torch.cuda.is_current_stream_capturing():     # as in _terms: no index list inside a capture
                    part = torch.stack([tw[:, s] for s in members], dim=1)
                else:
                    part = tw[:, members].contiguous()
                table = (C.c_void_p * (T * k))(*[keep[s][t].data_ptr() for t in range(T) for s in members])
                gtable = (C.c_void_p * (T * k))(*[grads[t][s].data_ptr() for t in range(T) for s in members])
                hs, ws = (C.c_int * k)(*[sizes[s][0] for s in members]), (C.c_int * k)(*[sizes[s][1] for s in members])
                _lib.check(L.pp_focal_l2_grad(
                    table, PP_F16 if dtype == torch.float16 else PP_F32, int(stride), C.c_void_p(target.data_ptr()),
                    PP_F16 if target.dtype == torch.float16 else PP_F32, image_stride, C.c_void_p(mask.data_ptr()) if mask is not None else None,
                    B, H, W, T, k, hs, ws, float(multi_task_weight), float(keypoint_task_weight), flags, C.c_void_p(part.data_ptr()),
                    gtable, C.c_void_p(st.cuda_stream)))
    return grads


_FUNCTION = None


def _function():
    """the autograd node of focal_l2_terms (built on first use: this module imports without torch)"""
    global _FUNCTION
    if _FUNCTION is not None:
        return _FUNCTION
    import torch
    from torch.autograd.function import once_differentiable

    class FocalL2Terms(torch.autograd.Function):
        @staticmethod
        def forward(ctx, target, mask, shape, multi_task_weight, keypoint_task_weight, plain_l2, workspace, stream, *flat):
            T, K = shape[0], shape[1]
            preds = [[flat[t * K + s] for s in range(K)] for t in range(T)]
            ctx.save_for_backward(target, mask, *flat)
            ctx.call = (T, K, multi_task_weight, keypoint_task_weight, plain_l2, stream)
            return _terms(shape, preds, target, mask, multi_task_weight, keypoint_task_weight, plain_l2, None, workspace, stream)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_terms):
            T, K, multi_task_weight, keypoint_task_weight, plain_l2, stream = ctx.call
            target, mask, *flat = ctx.saved_tensors
            preds = [[flat[t * K + s] for s in range(K)] for t in range(T)]
            grads = focal_l2_grad(preds, target, grad_terms, mask, multi_task_weight, keypoint_task_weight, plain_l2, stream)
            wanted = ctx.needs_input_grad[8:]
            return (None,) * 8 + tuple(grads[t][s] if wanted[t * K + s] else None for t in range(T) for s in range(K))

    _FUNCTION = FocalL2Terms.apply
    return _FUNCTION


def _weights(values, n, name, ref):
    import torch
    if len(values) < n:
        raise PosePafError(f"{name} has {len(values)} entries, the terms hold {n}")
    if isinstance(values, torch.Tensor):       # the caller's own device copy: no transfer here (a stream capture allows none)
        if values.dim() != 1 or values.dtype != torch.float64 or values.device != ref.device:
            raise PosePafError(f"{name} as a tensor must be 1-D float64 on {ref.device}")
        return values[:n]
    return torch.tensor([float(v) for v in values[:n]], dtype=torch.float64, device=ref.device)


def _check_terms(terms):
    import torch
    if not isinstance(terms, torch.Tensor) or terms.dim() != 3 or terms.dtype != torch.float64:
        raise PosePafError("terms must be a float64 (T, K, B) tensor")


def combine(terms, nstack_weight=NSTACK_WEIGHT, scale_weight=SCALE_WEIGHT, n_images=None):
    """sum_s scale_weight[s] * (sum_t nstack_weight[t] * sum_b terms[t][s][b] / sum nstack_weight) / sum scale_weight / n_images
    (models/loss_model.py:34-40, :156-160) -> 0-d float64 tensor on the terms' device.  n_images: default the terms' batch."""
    _check_terms(terms)
    T, K, B = terms.shape
    nw, sw = _weights(nstack_weight, T, "nstack_weight", terms), _weights(scale_weight, K, "scale_weight", terms)
    per_scale = (nw[:, None] * terms.sum(dim=2)).sum(dim=0) / nw.sum()
    return (sw * per_scale).sum() / sw.sum() / float(B if n_images is None else n_images)


class ValLossMeter:
    """Running sums of the terms over the batches of an evaluation (on the device; one synchronisation, in summary())."""

    def __init__(self, nstack_weight=NSTACK_WEIGHT, scale_weight=SCALE_WEIGHT):
        self.nstack_weight, self.scale_weight = tuple(nstack_weight), tuple(scale_weight)
        self.sums, self.images = None, 0

    def update(self, terms, n_valid=None):
        """terms (T, K, B); n_valid: only the first n_valid images count (a padded last batch)"""
        _check_terms(terms)
        n = int(terms.shape[2]) if n_valid is None else int(n_valid)
        if not 0 <= n <= terms.shape[2]:
            raise PosePafError(f"n_valid {n} outside 0..{terms.shape[2]}")
        part = terms[:, :, :n].sum(dim=2)
        if self.sums is None:
            self.sums = part.clone()
        elif self.sums.shape != part.shape:
            raise PosePafError(f"terms of {tuple(part.shape)} stacks x scales after {tuple(self.sums.shape)}")
        else:
            self.sums += part
        self.images += n

    def summary(self) -> dict:
        """val_loss: combine() over every image seen; per_stack[T] / per_scale[K]: the same with one stack / one scale alone (their
        own weight cancels); per_stack_scale[T][K]: mean term per image"""
        if self.sums is None or self.images == 0:
            raise PosePafError("no image has been added")
        T, K = self.sums.shape
        n = float(self.images)
        cell = self.sums.unsqueeze(2)                       # (T, K, 1): the sums as one "image"
        return {
            "val_loss": float(combine(cell, self.nstack_weight, self.scale_weight, n)),
            "per_stack": [float(combine(cell[t:t + 1], (1,), self.scale_weight, n)) for t in range(T)],
            "per_scale": [float(combine(cell[:, s:s + 1], self.nstack_weight, (1,), n)) for s in range(K)],
            "per_stack_scale": (self.sums / n).tolist(),
            "images": self.images,
        }
