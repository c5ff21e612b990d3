"""Training the twenty 1 x 1 prediction heads on the fused fp16 forward.

Everything but the heads (`outs[t][s]`: 256 -> 50, no BN, no activation) is frozen, so a step needs the forward, the loss gradient
with respect to the predictions (val_loss.focal_l2_grad) and, per head, the weight and bias gradient of a 1 x 1 convolution
(pp_head_wgrad_f16).  The data gradient of no layer is needed: the plain `finetune.py --train heads` detaches the chain between the
stages in the same way.

    tr = HeadTrainer(net, device, lr=2.5e-5, momentum=0.9, weight_decay=1e-4, loss_scale="auto", wgrad="device", arch=None)
    loss = tr.step(x, target, mask=None)         # 0-d float64 device tensor, the UNSCALED combine(terms); asynchronous
    grads = tr.gradients(x, target, mask=None)   # {(t, s): (dw float32 (50, 256), db float32 (50,))}; no update
    sd = tr.state_dict()                         # the plain network's keys, outs.* replaced by the float32 masters

The fused model is built with the prediction-merge fold OFF (FusedIMHN(net, folded_merge=False)): a head's new weights reach the
next stage through the prediction-merge convolution itself, with no re-fold per step.  The fold happens when a deployment model is
later built from state_dict().  The masters are float32; after every update they are rounded to binary16 IN PLACE into the fused
heads' tensors (weight, bias, and the zero-padded 64-output copies the streaming kernel reads), so pointers and layouts stay.

Loss scale.  The binary16 gradient pp_focal_l2_grad stores is  tw * cw * M * (2 d f + d^2 f')  per element.  For a background
element d = p, f = |p|, so the gradient is cubic in p and falls below the binary16 normal range (6.1e-5) for |p| of a few percent at
scale 1 -- the reason apex.amp scales the loss in the reference's train_distributed.py.  tw is therefore multiplied by a power of two
S and pp_head_wgrad_f16 multiplies the float32 sums by 1 / S once (exact).  "auto" is the largest power of two with

    S * tw_max * KEYPOINT_TASK_WEIGHT * ELEMENT_BOUND <= 65504        (the largest finite binary16)

where tw_max = max(nw) / sum(nw) * max(sw) / sum(sw) / B is the largest term weight of this batch size, KEYPOINT_TASK_WEIGHT = 3.0
the largest channel weight, M <= 1, and ELEMENT_BOUND = 12 bounds |2 d f + d^2 f'| for predictions in [-1, 2] and targets in [0, 1]
(|d| <= 2, f <= 2, |f'| = 1: 2 * 2 * 2 + 4).  A prediction outside that range can still overflow: then dw / db are not finite, the
step's update is masked out on the device and `skipped_steps` counts it.  The scale is static (no dynamic scaling).
"""
import ctypes as C
import math

from . import val_loss
from ._lib import PosePafError

KEYPOINT_TASK_WEIGHT = val_loss.KEYPOINT_TASK_WEIGHT      # the largest channel weight of the loss
ELEMENT_BOUND = 12.0      # |2 d f + d^2 f'| <= 2 * 2 * 2 + 4 for p in [-1, 2], G in [0, 1]  (module docstring)
HALF_MAX = 65504.0


def term_weights(batch, stages, scales, nstack_weight=val_loss.NSTACK_WEIGHT, scale_weight=val_loss.SCALE_WEIGHT):
    """d combine / d terms[t][s][b] = nw[t] / sum(nw) * sw[s] / sum(sw) / B -> nested list [t][s] (the same for every b)"""
    nw, sw = [float(v) for v in nstack_weight[:stages]], [float(v) for v in scale_weight[:scales]]
    if len(nw) < stages or len(sw) < scales:
        raise PosePafError(f"the loss weights hold {len(nw)} stages and {len(sw)} scales, the model has {stages} and {scales}")
    return [[nw[t] / sum(nw) * sw[s] / sum(sw) / batch for s in range(scales)] for t in range(stages)]


def auto_loss_scale(batch, stages, scales=5, nstack_weight=val_loss.NSTACK_WEIGHT, scale_weight=val_loss.SCALE_WEIGHT):
    """the largest power of two S with S * tw_max * KEYPOINT_TASK_WEIGHT * ELEMENT_BOUND <= 65504 (module docstring)"""
    tw_max = max(max(row) for row in term_weights(batch, stages, scales, nstack_weight, scale_weight))
    limit = HALF_MAX / (tw_max * KEYPOINT_TASK_WEIGHT * ELEMENT_BOUND)
    return 2.0 ** math.floor(math.log2(limit))


def is_power_of_two(v) -> bool:
    try:
        v = float(v)
    except (TypeError, ValueError):
        return False
    return math.isfinite(v) and v > 0 and math.frexp(v)[0] == 0.5 and 2.0 ** -24 <= v <= 2.0 ** 24


def _pixel_major(grad):
    """a (B, 50, h, w) gradient as (tensor whose data_ptr is pixel 0, ldg): in place where it is pixel-major with one pixel stride"""
    B, k, h, w = grad.shape
    t = grad.permute(0, 2, 3, 1)
    if t.stride(3) == 1 or k == 1:
        ldg = t.stride(2) if w > 1 else (t.stride(1) if h > 1 else (t.stride(0) if B > 1 else k))
        want = (h * w * ldg, w * ldg, ldg)
        if ldg >= k and all(t.shape[d] == 1 or t.stride(d) == want[d] for d in range(3)):
            return grad, int(ldg)
    return t.contiguous(), k


class HeadTrainer:
    def __init__(self, net, device, lr=2.5e-5, momentum=0.9, weight_decay=1e-4, loss_scale="auto", wgrad="device", arch=None):
        import torch
        from . import fused_model
        pn = getattr(net, "posenet", None)
        if pn is None or not hasattr(pn, "outs"):
            raise PosePafError("net must be a NetworkEval (model_init.build_network)")
        try:
            device = torch.device(device)
        except (TypeError, RuntimeError) as e:
            raise PosePafError(f"device: {e}")
        if device.type != "cuda":
            raise PosePafError(f"device {device}: the trainer has no CPU path")
        for name, v, ok in (("lr", lr, lambda v: v > 0), ("momentum", momentum, lambda v: 0 <= v < 1), ("weight_decay", weight_decay, lambda v: v >= 0)):
            if not (isinstance(v, (int, float)) and math.isfinite(v) and ok(v)):
                raise PosePafError(f"{name} = {v!r} is out of range")
        if loss_scale != "auto" and not is_power_of_two(loss_scale):
            raise PosePafError(f"loss_scale = {loss_scale!r}: 'auto' or a power of two in 2^-24 .. 2^24")
        if wgrad not in ("device", "torch"):
            raise PosePafError(f"wgrad = {wgrad!r}: 'device' (pp_head_wgrad_f16) or 'torch' (the A/B formulation)")
        from models import posenet_final
        found = "final" if isinstance(pn, posenet_final.PoseNet) else "posenet"
        if arch not in (None, found):
            raise PosePafError(f"arch = {arch!r}, the network is {found!r}")
        for t, stage in enumerate(pn.outs):
            for s, c in enumerate(stage):
                if c.bn is not None or c.relu is not None or tuple(c.conv.kernel_size) != (1, 1) or c.conv.bias is None:
                    raise PosePafError(f"outs[{t}][{s}] is not a bare 1 x 1 convolution with a bias: a head with BN or an activation is refused")
        self.net, self.device, self.arch, self.wgrad = net, device, found, wgrad
        self.loss_scale_arg = loss_scale
        self.model = fused_model.FusedIMHN.from_network(net, folded_merge=False).eval().to(device).half().to(memory_format=torch.channels_last)
        self.T, self.K = self.model.S, self.model.K
        self.heads = {(t, s): self.model.head[t][s] for t in range(self.T) for s in range(self.K)}
        # the reference's configuration weighs its four stages alike; a deeper stack keeps doing so
        self.nstack_weight = tuple(val_loss.NSTACK_WEIGHT) + (1,) * max(0, self.T - len(val_loss.NSTACK_WEIGHT))
        # float32 masters, their gradients and momentum buffers as views of three flat tensors: one finite test, one masked restore
        sizes = {}
        for key in self.heads:
            conv = pn.outs[key[0]][key[1]].conv
            sizes[key] = (conv.weight.numel(), conv.bias.numel())
        total = sum(a + b for a, b in sizes.values())
        self._flat = torch.empty(total, dtype=torch.float32, device=device)
        self._flat_grad = torch.zeros(total, dtype=torch.float32, device=device)
        self._flat_buf = torch.zeros(total, dtype=torch.float32, device=device)
        self.masters, self._grads, params, at = {}, {}, [], 0
        for key, (nw, nb) in sizes.items():
            conv = pn.outs[key[0]][key[1]].conv
            pair, gpair = [], []
            for n, src in ((nw, conv.weight), (nb, conv.bias)):
                view = self._flat[at:at + n].view(src.shape)
                view.copy_(src.detach().float())
                p = torch.nn.Parameter(view, requires_grad=True)
                p.grad = self._flat_grad[at:at + n].view(src.shape)
                pair.append(p), gpair.append(p.grad), params.append((p, self._flat_buf[at:at + n].view(src.shape)))
                at += n
            self.masters[key], self._grads[key] = tuple(pair), tuple(gpair)
        self.opt = torch.optim.SGD([p for p, _ in params], lr=lr, momentum=momentum, weight_decay=weight_decay)
        if momentum:      # a zero buffer is SGD's "no buffer yet": 0 * momentum + grad = grad
            for p, buf in params:
                self.opt.state[p]["momentum_buffer"] = buf
        self.skipped_steps = torch.zeros((), dtype=torch.int64, device=device)
        self.last_inputs, self._seen, self._workspace = {}, {}, None
        for key, head in self.heads.items():
            head.register_forward_pre_hook(lambda mod, args, key=key: self._seen.__setitem__(key, args[0]))
        self._push_masters()

    # ---- pieces of a step

    def loss_scale_for(self, batch):
        return auto_loss_scale(batch, self.T, self.K, self.nstack_weight) if self.loss_scale_arg == "auto" else float(self.loss_scale_arg)

    def _check_inputs(self, x, target, mask):
        import torch
        for name, t in (("x", x), ("target", target)) + ((("mask", mask),) if mask is not None else ()):
            if not isinstance(t, torch.Tensor):
                raise PosePafError(f"{name} must be a torch tensor")
            if not t.is_cuda or t.device != self.device:
                raise PosePafError(f"{name} must live on {self.device}: host tensors are refused")
        if x.dim() != 4 or x.shape[3] != 3 or x.dtype not in (torch.float16, torch.float32):
            raise PosePafError("x must be a (B, H, W, 3) float16 / float32 image batch in [0, 1]")
        B, H, W, _ = x.shape
        if B < 1 or H < 64 or W < 64 or H % 64 or W % 64:
            raise PosePafError(f"x is {tuple(x.shape)}: both sides must be positive multiples of 64")
        if target.shape[0] != B or tuple(target.shape[-2:]) != (H // 4, W // 4):
            raise PosePafError(f"target is {tuple(target.shape)}: expected batch {B} and {H // 4} x {W // 4} maps")

    def _head_inputs(self, key, grad):
        """(g 2-D strided view (m, 50), ldg, x 2-D (m, c_in), scale (B, c_in) or None) of one head from the captured forward input"""
        import torch
        from .fused_model import Scaled
        head, seen = self.heads[key], self._seen[key]
        scaled = isinstance(seen, Scaled)
        if head.last_padded is not None:          # the fast path: the gains (if any) were multiplied in the kernel's input read
            x, scale = (seen.y, seen.s.contiguous()) if scaled else (seen, None)
        else:
            x, scale = (seen.materialize() if scaled else seen), None
        B, c, h, w = x.shape
        x2 = x.permute(0, 2, 3, 1).contiguous().view(B * h * w, c)
        g, ldg = _pixel_major(grad)
        g2 = torch.as_strided(g, (B * h * w, grad.shape[1]), (ldg, 1), g.storage_offset())
        return g2, ldg, x2, scale

    def _wgrad(self, key, g2, ldg, x2, scale, inv):
        import torch
        from . import _lib
        dw, db = self._grads[key]
        m, c_in = x2.shape
        k = g2.shape[1]
        hw = m // (scale.shape[0] if scale is not None else 1)
        if self.wgrad == "torch":
            xs = x2 if scale is None else (x2.float().view(scale.shape[0], hw, c_in) * scale.float()[:, None, :]).half().view(m, c_in)
            dw.view(k, c_in).copy_((g2.double().t() @ xs.double()).float() * inv)
            db.copy_(g2.double().sum(dim=0).float() * inv)
            return
        L = _lib.load()
        need = int(L.pp_head_wgrad_workspace_bytes(m, c_in, k))
        if need < 0:
            _lib.check(need)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        _lib.check(L.pp_head_wgrad_f16(C.c_void_p(g2.data_ptr()), ldg, C.c_void_p(x2.data_ptr()),
                                       C.c_void_p(scale.data_ptr()) if scale is not None else None, m, hw, c_in, k, inv,
                                       C.c_void_p(self._workspace.data_ptr()), need, C.c_void_p(dw.data_ptr()), C.c_void_p(db.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _backward(self, x, target, mask):
        """forward, loss terms, scaled loss gradient, every head's dw / db into the masters' .grad -> the unscaled loss"""
        import torch
        self._check_inputs(x, target, mask)
        B = x.shape[0]
        S = self.loss_scale_for(B)
        self._last_batch = B
        with torch.no_grad(), torch.cuda.device(self.device):
            self._seen.clear()
            preds = self.model(x.half() if x.dtype != torch.float16 else x, all_preds=True)
            terms = val_loss.focal_l2_terms(preds, target, mask=mask)
            loss = val_loss.combine(terms, self.nstack_weight)
            tw = torch.tensor(term_weights(B, self.T, self.K, self.nstack_weight), dtype=torch.float64, device=self.device)[:, :, None].expand(self.T, self.K, B)
            grads = val_loss.focal_l2_grad(preds, target, (tw * S).contiguous(), mask)
            self.last_inputs = {}
            for key in self.heads:
                g2, ldg, x2, scale = self._head_inputs(key, grads[key[0]][key[1]])
                self.last_inputs[key] = (g2, ldg, x2, scale)
                self._wgrad(key, g2, ldg, x2, scale, 1.0 / S)
            self._seen.clear()
        return loss

    def _push_masters(self):
        """the masters, rounded to binary16, in place into the fused heads' tensors"""
        import torch
        with torch.no_grad():
            for key, (w, b) in self.masters.items():
                head = self.heads[key]
                k = head.k_real
                head.weight.copy_(w), head.bias.copy_(b)
                head.wpad[:k].copy_(w), head.bpad[:k].copy_(b)

    # ---- the public calls

    def gradients(self, x, target, mask=None):
        """{(t, s): (dw float32 (50, c_in), db float32 (50,))} of the UNSCALED loss, copies; no update.  Keeps
        last_inputs[(t, s)] = (g, ldg, x, scale): what the head's pp_head_wgrad_f16 call read (g as a (m, 50) view with row stride ldg)"""
        self._backward(x, target, mask)
        return {key: (dw.detach().clone().view(dw.shape[0], -1), db.detach().clone()) for key, (dw, db) in self._grads.items()}

    def gradients_from_last(self, wgrad):
        """dw / db once more from last_inputs -- the tensors the last gradients() / step() captured, no forward -- in the named
        formulation ("device" or "torch"), for A/B on identical inputs -> the dictionary gradients() returns"""
        import torch
        if wgrad not in ("device", "torch") or not self.last_inputs:
            raise PosePafError("gradients_from_last needs 'device' or 'torch' and a previous gradients() or step()")
        S = self.loss_scale_for(self._last_batch)
        keep, self.wgrad = self.wgrad, wgrad
        try:
            with torch.no_grad(), torch.cuda.device(self.device):
                for key, (g2, ldg, x2, scale) in self.last_inputs.items():
                    self._wgrad(key, g2, ldg, x2, scale, 1.0 / S)
        finally:
            self.wgrad = keep
        return {key: (dw.detach().clone().view(dw.shape[0], -1), db.detach().clone()) for key, (dw, db) in self._grads.items()}

    def step(self, x, target, mask=None):
        import torch
        loss = self._backward(x, target, mask)
        with torch.no_grad():
            finite = torch.isfinite(self._flat_grad).all()
            old, old_buf = self._flat.clone(), self._flat_buf.clone()
            self.opt.step()
            # a non-finite gradient: the masters and the momentum come back, on the device (no host synchronisation)
            self._flat.copy_(torch.where(finite, self._flat, old))
            self._flat_buf.copy_(torch.where(finite, self._flat_buf, old_buf))
            self.skipped_steps += (~finite).to(torch.int64)
        self._push_masters()
        return loss

    def grad_norm(self):
        """the L2 norm of the heads' gradients of the last gradients() / step() -> 0-d float64 device tensor"""
        import torch
        return torch.sqrt((self._flat_grad.double() ** 2).sum())

    def state_dict(self):
        """the plain network's state dict (its keys; tensors on their devices) with outs.* replaced by copies of the float32 masters"""
        sd = {k: v.detach() for k, v in self.net.state_dict().items()}
        for (t, s), (w, b) in self.masters.items():
            for name, p in ((f"posenet.outs.{t}.{s}.conv.weight", w), (f"posenet.outs.{t}.{s}.conv.bias", b)):
                if name not in sd:
                    raise PosePafError(f"the network has no {name}")
                sd[name] = p.detach().clone()
        return sd
