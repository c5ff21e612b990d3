"""Training the twenty 1 x 1 prediction heads on the fused fp16 forward.

Everything but the heads (`outs[t][s]`: 256 -> 50, no BN, no activation) is frozen, so a step needs the forward, the loss gradient
with respect to the predictions (val_loss.focal_l2_grad) and, per head, the weight and bias gradient of a 1 x 1 convolution
(pp_head_wgrad_f16).  The data gradient of no layer is needed: the plain `finetune.py --train heads` detaches the chain between the
stages in the same way.

    tr = HeadTrainer(net, device, lr=2.5e-5, momentum=0.9, weight_decay=1e-4, loss_scale="auto", wgrad="device", arch=None,
                     update="torch", graph=False, growth_interval=2000, init_scale=None)
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
step's update is masked out on the device and `skipped_steps` counts it.  "auto" and a given power of two are static scales.

The captured step.  wgrad="multi" forms every head's dw / db in one pp_head_wgrad_multi_f16 call (the bits of
"device").  update="device" replaces torch.optim.SGD.step(), the masked restore and the 80 fp16 copies by pp_head_update_f32: finite
test, SGD (torch's roundings), fp16 copies and the loss-scale state in two launches; lr, momentum and weight decay live in a device
block set_lr() writes.  loss_scale="dynamic" (needs update="device" and wgrad "multi" or "torch") is apex's dynamic scaler on that
state: halve on a non-finite gradient (the step is skipped), double after growth_interval finite steps, between 2^-24 and 2^24,
from init_scale or, without one, "auto" of the first batch; loss_scale_now() reads it.  graph=True (needs update="device"): the first
step() of a signature -- (shape and dtype of x, shape and dtype of target, mask given or not) -- runs eagerly (the tuner times its
candidates there), the second captures forward, loss, gradients and update into one torch.cuda.CUDAGraph over static copies of the
inputs and replays it, later ones copy the inputs in and replay: the same bits as graph=False, step for step.  graph=True sets
torch.backends.cudnn.deterministic (the few MIOpen layers must add in one order for that to hold).

train="heads+conv" (the 'final' architecture only: on 'posenet' an SE block stands in between).  The 3 x 3
convolution in front of every head (features[t].before_regress[s][2]: conv, frozen BN, LeakyReLU) is trained as well.  Its masters are
the weight and bias with the BN FOLDED in float32 (fused_model._fold of the plain layer), the weight in (K, 3, 3, C) order -- the memory
of the fused layer's channels-last binary16 tensor, which receives the rounded master in place.  Per layer, after the heads:
pp_head_dgrad_f16 takes the loss gradient through the head's current binary16 weight and the activation (dY, binary16),
pp_conv3x3_wgrad_f16 forms dw / db from dY and the convolution's captured input with the heads' loss-scale factor.  wgrad="torch"
forms both in float64 with the contract's roundings.  The same flat tensors, finite test, update paths, dynamic scale and capture
cover them.  gradients() returns them under ("conv", t, s); state_dict() writes the folded master as the plain convolution's weight
behind a BN whose fold is exact (identity_bn_var), so a model rebuilt from it runs the trainer's binary16 bits.

train="heads+conv2" ('final' only).  The 3 x 3 convolution in front of that one (before_regress[s][1], the
fused model's feat[t][s].c2) is trained as well.  Its masters lie BEHIND the heads' and the ("conv", t, s) ones in the flat tensors,
so the ranges of those keys are the ones of "heads+conv".  Per (t, s), after c3's gradients: pp_conv3x3_dgrad_f16 takes c3's dY
through c3's CURRENT binary16 weight -- the layer's own channels-last memory, no rotated copy -- and the LeakyReLU whose output is
c3's captured input (dY2, binary16); pp_conv3x3_wgrad_f16 forms c2's dw / db from dY2 and c2's captured input with the same factor
and workspace.  wgrad="torch": torch.nn.grad.conv2d_input in float64 with the contract's roundings, then conv2d_weight as for c3.
update="device" goes through pp_layer_update_f32 in this mode (60 layers at four stages; pp_head_update_f32 takes 40): a head is two
segments with its padded copy as the second destination, a convolution two with dst2 = dst.  gradients() returns ("conv2", t, s)
next to the others; last_inputs[("conv2", t, s)] = (c3's binary16 weight (K, 3, 3, C) copy, c2's NHWC input, dY2).
"""
import ctypes as C
import math

import numpy as np

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


def identity_bn_var(eps):
    """a float32 running_var v next to 1 - eps with sqrt(fl32(v + eps)) == 1.0f: with running_mean 0 and weight 1, fused_model._fold
    then multiplies the convolution's weight by exactly 1 and returns the BN bias as the folded bias, bit for bit"""
    import torch
    v = np.float32(1.0) - np.float32(eps)
    candidates, up, down = [v], v, v
    for _ in range(8):              # the nearest first
        up, down = np.nextafter(up, np.float32(2.0)), np.nextafter(down, np.float32(0.0))
        candidates += [up, down]
    for c in (float(c) for c in candidates):
        if float(torch.sqrt(torch.tensor(c, dtype=torch.float32) + eps)) == 1.0:
            return c
    raise PosePafError(f"no float32 running_var folds to the identity with eps = {eps!r}")


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
    def __init__(self, net, device, lr=2.5e-5, momentum=0.9, weight_decay=1e-4, loss_scale="auto", wgrad="device", arch=None,
                 update="torch", graph=False, growth_interval=2000, init_scale=None, train="heads"):
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
        dynamic = isinstance(loss_scale, str) and loss_scale == "dynamic"
        if not dynamic and loss_scale != "auto" and not is_power_of_two(loss_scale):
            raise PosePafError(f"loss_scale = {loss_scale!r}: 'auto', 'dynamic' or a power of two in 2^-24 .. 2^24")
        if wgrad not in ("device", "torch", "multi"):
            raise PosePafError(f"wgrad = {wgrad!r}: 'device' (pp_head_wgrad_f16), 'multi' (pp_head_wgrad_multi_f16) or 'torch' (the A/B formulation)")
        if update not in ("torch", "device"):
            raise PosePafError(f"update = {update!r}: 'torch' (torch.optim.SGD) or 'device' (pp_head_update_f32)")
        if graph and update != "device":
            raise PosePafError("graph=True needs update='device': torch.optim.SGD.step() is not captured")
        if dynamic and (update != "device" or wgrad == "device"):
            raise PosePafError("loss_scale='dynamic' needs update='device' and wgrad 'multi' or 'torch': pp_head_wgrad_f16 takes its "
                               "factor from the host")
        if isinstance(growth_interval, bool) or not isinstance(growth_interval, int) or not 0 <= growth_interval < 2 ** 31:
            raise PosePafError(f"growth_interval = {growth_interval!r}: an integer >= 0 (0: the scale never moves)")
        if init_scale is not None and not is_power_of_two(init_scale):
            raise PosePafError(f"init_scale = {init_scale!r}: None or a power of two in 2^-24 .. 2^24")
        from models import posenet_final
        found = "final" if isinstance(pn, posenet_final.PoseNet) else "posenet"
        if arch not in (None, found):
            raise PosePafError(f"arch = {arch!r}, the network is {found!r}")
        if train not in ("heads", "heads+conv", "heads+conv2"):
            raise PosePafError(f"train = {train!r}: 'heads', 'heads+conv' (the 3 x 3 convolution in front of every head as well) or "
                               "'heads+conv2' (both 3 x 3 convolutions below every head)")
        if train != "heads" and found != "final":
            raise PosePafError(f"train={train!r} needs the 'final' architecture: on 'posenet' an SE block stands between the "
                               "convolution and the head, and it has no backward here")
        for t, stage in enumerate(pn.outs):
            for s, c in enumerate(stage):
                if c.bn is not None or c.relu is not None or tuple(c.conv.kernel_size) != (1, 1) or c.conv.bias is None:
                    raise PosePafError(f"outs[{t}][{s}] is not a bare 1 x 1 convolution with a bias: a head with BN or an activation is refused")
        self.net, self.device, self.arch, self.wgrad = net, device, found, wgrad
        self.loss_scale_arg = loss_scale
        self.update, self.graph, self.dynamic, self.graph_replays = update, bool(graph), dynamic, 0
        if graph:
            torch.backends.cudnn.deterministic = True
        self.model = fused_model.FusedIMHN.from_network(net, folded_merge=False).eval().to(device).half().to(memory_format=torch.channels_last)
        self.T, self.K = self.model.S, self.model.K
        self.heads = {(t, s): self.model.head[t][s] for t in range(self.T) for s in range(self.K)}
        # the reference's configuration weighs its four stages alike; a deeper stack keeps doing so
        self.nstack_weight = tuple(val_loss.NSTACK_WEIGHT) + (1,) * max(0, self.T - len(val_loss.NSTACK_WEIGHT))
        self.train, self.convs = train, {}
        # float32 masters, their gradients and momentum buffers as views of three flat tensors: one finite test, one masked restore
        sources = {}
        for key in self.heads:
            conv = pn.outs[key[0]][key[1]].conv
            sources[key] = (conv.weight.detach(), conv.bias.detach())
        if train != "heads":            # behind the heads, so that their ranges are those of train='heads'
            for t, s in self.heads:
                sources[("conv", t, s)] = self._conv_source(pn, t, s)
                self.convs[("conv", t, s)] = self.model.feat[t][s].c3
        if train == "heads+conv2":      # and behind those: the ranges of the keys above are the ones of train='heads+conv'
            for t, s in self.heads:
                sources[("conv2", t, s)] = self._conv_source(pn, t, s, 1)
                self.convs[("conv2", t, s)] = self.model.feat[t][s].c2
        sizes = {key: (w.numel(), b.numel()) for key, (w, b) in sources.items()}
        total = sum(a + b for a, b in sizes.values())
        self._flat = torch.empty(total, dtype=torch.float32, device=device)
        self._flat_grad = torch.zeros(total, dtype=torch.float32, device=device)
        self._flat_buf = torch.zeros(total, dtype=torch.float32, device=device)
        self.masters, self._grads, params, at = {}, {}, [], 0
        for key, (nw, nb) in sizes.items():
            pair, gpair = [], []
            for n, src in zip((nw, nb), sources[key]):
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
        self._tw, self._graphs, self._last_batch = {}, {}, None
        self._nw = torch.tensor([float(v) for v in self.nstack_weight[:self.T]], dtype=torch.float64, device=device)
        self._sw = torch.tensor([float(v) for v in val_loss.SCALE_WEIGHT[:self.K]], dtype=torch.float64, device=device)
        if update == "device":
            self._init_device_update(sizes, lr, momentum, weight_decay, growth_interval if dynamic else 0, init_scale if dynamic else None)
        for key, layer in list(self.heads.items()) + list(self.convs.items()):
            layer.register_forward_pre_hook(lambda mod, args, key=key: self._seen.__setitem__(key, args[0]))
        self._push_masters()

    def _conv_source(self, pn, t, s, layer=2):
        """(weight (K, 3, 3, C), bias (K,)) float32 of before_regress[s][layer] of stage t (2: the convolution in front of the head, 1:
        the one in front of that) with its BN folded in float32 (fused_model._fold on the plain layer, not the fused model's binary16
        copy), the weight in the memory order of the fused layer's channels-last tensor"""
        import torch
        from . import _lib, fused_model
        blk = pn.features[t].before_regress[s][layer]
        fused, conv = getattr(self.model.feat[t][s], f"c{layer + 1}"), blk.conv
        plain = (tuple(conv.kernel_size), tuple(conv.stride), tuple(conv.padding), tuple(conv.dilation), conv.groups)
        if plain != ((3, 3), (1, 1), (1, 1), (1, 1), 1) or blk.relu is None or not fused.act:
            raise PosePafError(f"before_regress[{s}][{layer}] of stage {t} is not a 3 x 3 / pad 1 / stride 1 convolution with a LeakyReLU")
        k, c = conv.weight.shape[:2]
        L = _lib.load()
        # what takes the gradient to this layer's output: the head's data gradient, or the data gradient of the 3 x 3 above
        reach = L.pp_head_dgrad_supported(k, self.heads[(t, s)].k_real) if layer == 2 else L.pp_conv3x3_dgrad_supported(
            k, self.model.feat[t][s].c3.weight.shape[0])
        if not L.pp_conv3x3_wgrad_supported(c, k) or not reach:
            raise PosePafError(f"before_regress[{s}][{layer}] of stage {t}: {c} -> {k} channels are outside the gradient kernels' shapes")
        if fused.weight.dtype != torch.float16 or not fused.weight.is_contiguous(memory_format=torch.channels_last):
            raise PosePafError("the fused 3 x 3 layer does not keep its weight as one channels-last binary16 tensor")
        w, b = fused_model._fold(conv, blk.bn)
        return w.permute(0, 2, 3, 1).contiguous(), b

    # ---- pieces of a step

    def loss_scale_for(self, batch):
        """the static scale of a batch size ("auto" or the given power of two); the dynamic one lives on the device: loss_scale_now()"""
        if self.dynamic:
            raise PosePafError("loss_scale='dynamic' has no per-batch value: read loss_scale_now()")
        return auto_loss_scale(batch, self.T, self.K, self.nstack_weight) if self.loss_scale_arg == "auto" else float(self.loss_scale_arg)

    def loss_scale_now(self):
        """the loss scale the next step multiplies by -> 0-d float32 device tensor (a copy).  Dynamic: the device state; static: the
        scale of the last batch size (before any step: PosePafError)"""
        import torch
        if self.dynamic:
            if not self._scale_set:
                raise PosePafError("without init_scale the dynamic scale starts at 'auto' of the first batch: no step was made yet")
            return self._scale.clone()
        if self._last_batch is None:
            raise PosePafError("no step was made yet: loss_scale_for(batch) gives the static scale of a batch size")
        return torch.tensor(self.loss_scale_for(self._last_batch), dtype=torch.float32, device=self.device)

    def set_lr(self, lr):
        """a new learning rate from the next step on: the optimiser's group, or with update='device' the device block (a captured step
        reads it when it runs)"""
        if not (isinstance(lr, (int, float)) and math.isfinite(lr) and lr > 0):
            raise PosePafError(f"lr = {lr!r} is out of range")
        if self.update == "device":
            self._hyper[0] = float(lr)
        else:
            for group in self.opt.param_groups:
                group["lr"] = float(lr)

    # ---- update='device': pp_head_update_f32 and its blocks

    def _init_device_update(self, sizes, lr, momentum, weight_decay, growth_interval, init_scale):
        import torch
        from . import _lib
        L = _lib.load()
        self._segments = self.train == "heads+conv2"      # this mode always updates through pp_layer_update_f32
        if self._segments and 2 * len(sizes) > L.pp_layer_update_max_segments():
            raise PosePafError(f"{len(sizes)} trained layers: pp_layer_update_f32 takes {L.pp_layer_update_max_segments()} segments")
        if not self._segments and len(sizes) > L.pp_head_wgrad_multi_max_heads():
            raise PosePafError(f"{len(sizes)} trained layers: pp_head_update_f32 takes {L.pp_head_wgrad_multi_max_heads()}")
        dev = self.device
        self._hyper = torch.tensor([lr, momentum, weight_decay], dtype=torch.float32, device=dev)
        self._state = torch.zeros(_lib.HEAD_UPDATE_STATE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        f = self._state.view(torch.float32)
        self._scale, self._inv_scale = f[0], f[1]                    # 0-d views of the block the kernel updates
        self.skipped_steps = self._state[24:32].view(torch.int64)[0]
        self._growth_interval, self._scale_set = growth_interval, False
        self._write_scale(float(init_scale) if init_scale is not None else 1.0)
        self._scale_set = init_scale is not None or not self.dynamic
        self._ranges, at = [], 0
        for key in sizes:               # the heads, then the convolutions: the order of the flat tensors
            nw, nb = sizes[key]
            self._ranges.append((at, nw, at + nw, nb))
            at += nw + nb
        entry = 2 * C.sizeof(_lib.UpdateSegment) if self._segments else C.sizeof(_lib.HeadUpdateDesc)
        self._table = torch.zeros(len(sizes) * entry, dtype=torch.uint8, device=dev)
        self._table_ptrs = None
        self._update_ws = torch.empty(int(L.pp_head_update_workspace_bytes(self._flat.numel())), dtype=torch.uint8, device=dev)

    def _write_scale(self, scale):
        """(re)starts the state block at `scale`: good_steps 0, the skip count kept"""
        import torch
        from . import _lib
        st = np.zeros(1, _lib.HEAD_UPDATE_STATE_DTYPE)
        st["scale"], st["inv_scale"], st["growth_interval"] = scale, 1.0 / scale, self._growth_interval
        st["min_scale"], st["max_scale"] = 2.0 ** -24, 2.0 ** 24
        skipped = self.skipped_steps.clone()
        self._state.copy_(torch.from_numpy(st.view(np.uint8)))
        self.skipped_steps.copy_(skipped)
        self._scale_set = True

    def _sync_table(self):
        """the device table of pp_head_update_f32 names the heads' fp16 tensors where they lie now (a layer re-lays its weight at its
        first forward): rewritten, in place, when one moved -- never inside a capture"""
        import torch
        from . import _lib
        # a convolution has no padded copies: its descriptor names the weight and the bias twice, and the second store of an element
        # writes the value the first one wrote
        ptrs = tuple((h.weight.data_ptr(), h.bias.data_ptr(), h.wpad.data_ptr(), h.bpad.data_ptr()) for h in self.heads.values())
        ptrs += tuple((c.weight.data_ptr(), c.bias.data_ptr()) * 2 for c in self.convs.values())
        if ptrs == self._table_ptrs:
            return
        if torch.cuda.is_current_stream_capturing():
            raise PosePafError("a head's fp16 tensor moved after the eager step: the captured update would write the old one")
        # pp_head_update_f32's descriptors, or the same ranges as single segments (pp_layer_update_f32): the one this mode calls
        table = (_lib.UpdateSegment * (2 * len(ptrs)))() if self._segments else (_lib.HeadUpdateDesc * len(ptrs))()
        layers = list(self.heads.values()) + list(self.convs.values())
        for i, (layer, (w_off, w_len, b_off, b_len), (pw, pb, pwp, pbp)) in enumerate(zip(layers, self._ranges, ptrs)):
            if hasattr(layer, "wpad"):
                k = layer.k_real
                for t, n in ((layer.weight, w_len), (layer.bias, b_len), (layer.wpad[:k], w_len), (layer.bpad[:k], b_len)):
                    dense = t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))
                    if t.dtype != torch.float16 or t.numel() != n or not dense or tuple(t.shape[2:]) not in ((), (1, 1)):
                        raise PosePafError("a head's fp16 tensor is not the dense binary16 image of its master")
            else:       # (K, C, 3, 3) channels-last is the master's (K, 3, 3, C) element by element
                w, b = layer.weight, layer.bias
                if (w.dtype != torch.float16 or b.dtype != torch.float16 or w.numel() != w_len or b.numel() != b_len
                        or not w.is_contiguous(memory_format=torch.channels_last) or not b.is_contiguous()):
                    raise PosePafError("a convolution's fp16 tensor is not the dense binary16 image of its master")
            if self._segments:
                sw, sb = table[2 * i], table[2 * i + 1]
                sw.off, sw.len, sw.dst, sw.dst2 = w_off, w_len, pw, pwp
                sb.off, sb.len, sb.dst, sb.dst2 = b_off, b_len, pb, pbp
            else:
                d = table[i]
                d.w_off, d.w_len, d.b_off, d.b_len, d.weight, d.bias, d.wpad, d.bpad = w_off, w_len, b_off, b_len, pw, pb, pwp, pbp
        self._table.copy_(torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()))
        self._table_ptrs = ptrs

    def _device_update(self):
        import torch
        from . import _lib
        self._sync_table()
        ptr = lambda t: C.c_void_p(t.data_ptr())
        L, layers = _lib.load(), len(self.heads) + len(self.convs)
        entry, n = (L.pp_layer_update_f32, 2 * layers) if self._segments else (L.pp_head_update_f32, layers)
        _lib.check(entry(ptr(self._flat), ptr(self._flat_grad), ptr(self._flat_buf), self._flat.numel(), ptr(self._table), n,
                         ptr(self._hyper), ptr(self._state), ptr(self._update_ws),
                         C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

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

    def _grow_workspace(self, need):
        """the weight gradients' workspace, replaced by a larger one when a call needs more.  A captured graph holds the address of
        the one it was captured with: its entry in _graphs keeps that tensor alive (_graphed_step), so a replacement here never
        returns memory that a later replay still writes"""
        import torch
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)

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
        self._grow_workspace(need)
        _lib.check(L.pp_head_wgrad_f16(C.c_void_p(g2.data_ptr()), ldg, C.c_void_p(x2.data_ptr()),
                                       C.c_void_p(scale.data_ptr()) if scale is not None else None, m, hw, c_in, k, inv,
                                       C.c_void_p(self._workspace.data_ptr()), need, C.c_void_p(dw.data_ptr()), C.c_void_p(db.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _wgrad_multi(self, inv):
        """every head of last_inputs in one pp_head_wgrad_multi_f16 call; inv: a host float or the device float of the state block"""
        import torch
        from . import _lib
        L = _lib.load()
        table = (_lib.HeadWgradDesc * len(self.heads))()
        for d, key in zip(table, self.heads):
            g2, ldg, x2, scale = self.last_inputs[key]
            dw, db = self._grads[key]
            m, c_in = x2.shape
            d.g, d.ldg, d.x, d.scale = g2.data_ptr(), ldg, x2.data_ptr(), scale.data_ptr() if scale is not None else None
            d.m, d.hw, d.c_in, d.c_out = m, m // (scale.shape[0] if scale is not None else 1), c_in, g2.shape[1]
            d.dw, d.db = dw.data_ptr(), db.data_ptr()
        need = int(L.pp_head_wgrad_multi_workspace_bytes(len(table), table))
        if need < 0:
            _lib.check(need)
        self._grow_workspace(need)
        on_device = isinstance(inv, torch.Tensor)
        _lib.check(L.pp_head_wgrad_multi_f16(len(table), table, 1.0 if on_device else inv, C.c_void_p(inv.data_ptr()) if on_device else None,
                                             C.c_void_p(self._workspace.data_ptr()), need,
                                             C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _scales(self, B):
        """(what the term weights are multiplied by, what the sums are multiplied by): host floats, or with the dynamic scale the two
        device floats of the state block"""
        if not self.dynamic:
            S = self.loss_scale_for(B)
            return S, 1.0 / S
        if not self._scale_set:
            self._write_scale(auto_loss_scale(B, self.T, self.K, self.nstack_weight))
        return self._scale, self._inv_scale

    def _backward(self, x, target, mask):
        """forward, loss terms, scaled loss gradient, every head's dw / db into the masters' .grad -> the unscaled loss"""
        import torch
        self._check_inputs(x, target, mask)
        B = x.shape[0]
        S, inv = self._scales(B)
        self._last_batch = B
        if B not in self._tw:
            self._tw[B] = torch.tensor(term_weights(B, self.T, self.K, self.nstack_weight), dtype=torch.float64, device=self.device)
        with torch.no_grad(), torch.cuda.device(self.device):
            self._seen.clear()
            preds = self.model(x.half() if x.dtype != torch.float16 else x, all_preds=True)
            terms = val_loss.focal_l2_terms(preds, target, mask=mask)
            loss = val_loss.combine(terms, self._nw, self._sw)
            tw = self._tw[B][:, :, None].expand(self.T, self.K, B)
            grads = val_loss.focal_l2_grad(preds, target, (tw * S).contiguous(), mask)       # a power of two: exact
            self.last_inputs = {}
            for key in self.heads:
                g2, ldg, x2, scale = self._head_inputs(key, grads[key[0]][key[1]])
                self.last_inputs[key] = (g2, ldg, x2, scale)
                if self.wgrad != "multi":
                    self._wgrad(key, g2, ldg, x2, scale, inv)
            if self.wgrad == "multi":
                self._wgrad_multi(inv)
            for key, c3 in self.convs.items():      # every ("conv", t, s) before the first ("conv2", t, s)
                if key[0] == "conv2":
                    above = self.convs[("conv",) + key[1:]]
                    self.last_inputs[key] = (above.weight.detach().permute(0, 2, 3, 1).contiguous().clone(),
                                             self._seen[key].permute(0, 2, 3, 1).contiguous(), None)
                    self._conv2_grads(key, inv, self.wgrad)
                    continue
                head = self.heads[key[1:]]
                self.last_inputs[key] = (head.weight.detach().reshape(head.k_real, -1).clone(),
                                         self._seen[key].permute(0, 2, 3, 1).contiguous(), None)
                self._conv_grads(key, inv, self.wgrad)
            self._seen.clear()
        return loss

    def _conv_grads(self, key, inv, how):
        """("conv", t, s): dY = the loss gradient through head (t, s) and the LeakyReLU in front of it, then the convolution's dw / db
        into the masters' .grad, from last_inputs: the head's (g, ldg, y, None) and this key's (head weight, NHWC input, .); the third
        element becomes dY.  how 'torch': both steps in float64 with the contract's roundings; else pp_head_dgrad_f16 and
        pp_conv3x3_wgrad_f16.  inv: a host float or the device float of the state block"""
        import torch
        from . import _lib, fused_model
        g2, ldg, y2, scale = self.last_inputs[key[1:]]
        w16, x_in = self.last_inputs[key][:2]
        dw, db = self._grads[key]
        B, h, w, c_in = x_in.shape
        m, c_mid = y2.shape
        if scale is not None or m != B * h * w or tuple(dw.shape) != (c_mid, 3, 3, c_in):
            raise PosePafError(f"{key}: the head's captured input is not this convolution's output")
        if how == "torch":
            s = g2.double() @ w16.double()
            dy = torch.where(y2 > 0, s, float(np.float32(fused_model.LEAK)) * s).half()
            d64 = dy.double()
            g64 = torch.nn.grad.conv2d_weight(x_in.double().permute(0, 3, 1, 2), (c_mid, c_in, 3, 3),
                                              d64.view(B, h, w, c_mid).permute(0, 3, 1, 2), stride=1, padding=1)
            dw.copy_(g64.permute(0, 2, 3, 1).float() * inv)
            db.copy_(d64.sum(dim=0).float() * inv)
            self.last_inputs[key] = (w16, x_in, dy)
            return
        L = _lib.load()
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        dy = torch.empty((m, c_mid), dtype=torch.float16, device=self.device)
        _lib.check(L.pp_head_dgrad_f16(C.c_void_p(g2.data_ptr()), ldg, C.c_void_p(w16.data_ptr()), C.c_void_p(y2.data_ptr()), m, c_mid,
                                       g2.shape[1], fused_model.LEAK, C.c_void_p(dy.data_ptr()), stream))
        need = int(L.pp_conv3x3_wgrad_workspace_bytes(B, h, w, c_in, c_mid))
        if need < 0:
            _lib.check(need)
        self._grow_workspace(need)
        on_device = isinstance(inv, torch.Tensor)
        _lib.check(L.pp_conv3x3_wgrad_f16(C.c_void_p(dy.data_ptr()), C.c_void_p(x_in.data_ptr()), B, h, w, c_in, c_mid,
                                          1.0 if on_device else inv, C.c_void_p(inv.data_ptr()) if on_device else None,
                                          C.c_void_p(self._workspace.data_ptr()), need, C.c_void_p(dw.data_ptr()), C.c_void_p(db.data_ptr()),
                                          stream))
        self.last_inputs[key] = (w16, x_in, dy)

    def _conv2_grads(self, key, inv, how):
        """("conv2", t, s): dY2 = ("conv", t, s)'s dY through that convolution and the LeakyReLU in front of it, then this
        convolution's dw / db into the masters' .grad, from last_inputs: ("conv", t, s)'s (., NHWC input = the activation's output, dY)
        and this key's (c3 weight (K, 3, 3, C), NHWC input, .); the third element becomes dY2.  how 'torch': both steps in float64
        with the contract's roundings; else pp_conv3x3_dgrad_f16 and pp_conv3x3_wgrad_f16.  inv as in _conv_grads"""
        import torch
        from . import _lib, fused_model
        _, y_mid, dy = self.last_inputs[("conv",) + key[1:]]
        w16, x_in = self.last_inputs[key][:2]
        dw, db = self._grads[key]
        B, h, w, c_in = x_in.shape
        c_top, c_mid = w16.shape[0], w16.shape[3]
        m = B * h * w
        if (dy is None or tuple(dy.shape) != (m, c_top) or tuple(y_mid.shape) != (B, h, w, c_mid) or tuple(w16.shape[1:3]) != (3, 3)
                or tuple(dw.shape) != (c_mid, 3, 3, c_in)):
            raise PosePafError(f"{key}: the captured input of the convolution above is not this convolution's output")
        if how == "torch":
            s = torch.nn.grad.conv2d_input((B, c_mid, h, w), w16.double().permute(0, 3, 1, 2),
                                           dy.double().view(B, h, w, c_top).permute(0, 3, 1, 2), stride=1, padding=1).permute(0, 2, 3, 1)
            t = torch.where(y_mid > 0, s, (float(np.float32(fused_model.LEAK)) * s).float().double())       # fl32(slope * s)
            dy2 = t.half().reshape(m, c_mid)
            d64 = dy2.double()
            g64 = torch.nn.grad.conv2d_weight(x_in.double().permute(0, 3, 1, 2), (c_mid, c_in, 3, 3),
                                              d64.view(B, h, w, c_mid).permute(0, 3, 1, 2), stride=1, padding=1)
            dw.copy_(g64.permute(0, 2, 3, 1).float() * inv)
            db.copy_(d64.sum(dim=0).float() * inv)
            self.last_inputs[key] = (w16, x_in, dy2)
            return
        L = _lib.load()
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        dy2 = torch.empty((m, c_mid), dtype=torch.float16, device=self.device)
        _lib.check(L.pp_conv3x3_dgrad_f16(C.c_void_p(dy.data_ptr()), C.c_void_p(w16.data_ptr()), C.c_void_p(y_mid.data_ptr()), B, h, w, c_mid,
                                          c_top, fused_model.LEAK, C.c_void_p(dy2.data_ptr()), stream))
        need = int(L.pp_conv3x3_wgrad_workspace_bytes(B, h, w, c_in, c_mid))
        if need < 0:
            _lib.check(need)
        self._grow_workspace(need)
        on_device = isinstance(inv, torch.Tensor)
        _lib.check(L.pp_conv3x3_wgrad_f16(C.c_void_p(dy2.data_ptr()), C.c_void_p(x_in.data_ptr()), B, h, w, c_in, c_mid,
                                          1.0 if on_device else inv, C.c_void_p(inv.data_ptr()) if on_device else None,
                                          C.c_void_p(self._workspace.data_ptr()), need, C.c_void_p(dw.data_ptr()), C.c_void_p(db.data_ptr()),
                                          stream))
        self.last_inputs[key] = (w16, x_in, dy2)

    def _push_masters(self):
        """the masters, rounded to binary16, in place into the fused heads' tensors"""
        import torch
        with torch.no_grad():
            for key, (w, b) in self.masters.items():
                if key in self.convs:       # (K, 3, 3, C) into the channels-last (K, C, 3, 3): element by element, pointers stay
                    self.convs[key].weight.copy_(w.permute(0, 3, 1, 2)), self.convs[key].bias.copy_(b)
                    continue
                head = self.heads[key]
                k = head.k_real
                head.weight.copy_(w), head.bias.copy_(b)
                head.wpad[:k].copy_(w), head.bpad[:k].copy_(b)

    # ---- the public calls

    def gradients(self, x, target, mask=None):
        """{(t, s): (dw float32 (50, c_in), db float32 (50,))} of the UNSCALED loss, copies; no update.  Keeps
        last_inputs[(t, s)] = (g, ldg, x, scale): what the head's pp_head_wgrad_f16 call read (g as a (m, 50) view with row stride ldg)"""
        self._backward(x, target, mask)
        return self._grad_copies()

    def _grad_copies(self):
        """a head's dw as (50, c_in); with train='heads+conv' also ("conv", t, s): (dw float32 (K, 3, 3, C), db float32 (K,)), and
        last_inputs[("conv", t, s)] = (the head's binary16 weight (50, K), the convolution's NHWC input, dY (m, K)): what
        pp_head_dgrad_f16 read besides the head's entry, and what pp_conv3x3_wgrad_f16 read"""
        return {key: (dw.detach().clone() if key in self.convs else dw.detach().clone().view(dw.shape[0], -1), db.detach().clone())
                for key, (dw, db) in self._grads.items()}

    def gradients_from_last(self, wgrad):
        """dw / db once more from last_inputs -- the tensors the last gradients() / step() captured, no forward -- in the named
        formulation ("device" or "torch"), for A/B on identical inputs -> the dictionary gradients() returns"""
        import torch
        if wgrad not in ("device", "torch", "multi") or not self.last_inputs:
            raise PosePafError("gradients_from_last needs 'device', 'multi' or 'torch' and a previous gradients() or step()")
        if self.dynamic and wgrad == "device":
            raise PosePafError("loss_scale='dynamic': pp_head_wgrad_f16 takes its factor from the host, use 'multi' or 'torch'")
        inv = self._scales(self._last_batch)[1]       # (dynamic: the scale as it is NOW, which a step since may have moved)
        keep, self.wgrad = self.wgrad, wgrad
        try:
            with torch.no_grad(), torch.cuda.device(self.device):
                if wgrad == "multi":
                    self._wgrad_multi(inv)
                else:
                    for key in self.heads:
                        g2, ldg, x2, scale = self.last_inputs[key]
                        self._wgrad(key, g2, ldg, x2, scale, inv)
                for key in self.convs:
                    (self._conv2_grads if key[0] == "conv2" else self._conv_grads)(key, inv, wgrad)
        finally:
            self.wgrad = keep
        return self._grad_copies()

    def step(self, x, target, mask=None):
        """one training step -> the unscaled loss, a 0-d float64 device tensor; asynchronous"""
        if self.graph:
            return self._graphed_step(x, target, mask)
        return self._step(x, target, mask)

    def _graphed_step(self, x, target, mask):
        """the first call of a signature: eager.  The second: capture over static copies of the inputs, then as every later one:
        copy the inputs in, replay, return a copy of the graph's loss scalar"""
        import torch
        self._check_inputs(x, target, mask)
        sig = (tuple(x.shape), x.dtype, tuple(target.shape), target.dtype, mask is not None)
        entry = self._graphs.get(sig)
        if entry is None:
            self._graphs[sig] = "seen"
            return self._step(x, target, mask)
        with torch.cuda.device(self.device):
            if entry == "seen":
                sx, st, sm = x.clone(), target.clone(), mask.clone() if mask is not None else None
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    loss = self._step(sx, st, sm)
                # the last element pins what the graph addresses beyond its own pool: the workspace of this capture, which a
                # later, larger eager call (another signature, gradients(), gradients_from_last("multi")) replaces in self
                entry = self._graphs[sig] = (graph, sx, st, sm, loss, self._workspace)
            graph, sx, st, sm, loss = entry[:5]
            sx.copy_(x), st.copy_(target)
            if sm is not None:
                sm.copy_(mask)
            graph.replay()
            self.graph_replays += 1
            return loss.clone()

    def _step(self, x, target, mask):
        loss = self._backward(x, target, mask)
        if self.update == "device":
            self._device_update()
        else:
            self._torch_update()
        return loss

    def _torch_update(self):
        import torch
        with torch.no_grad():
            finite = torch.isfinite(self._flat_grad).all()
            old, old_buf = self._flat.clone(), self._flat_buf.clone()
            self.opt.step()
            # a non-finite gradient: the masters and the momentum come back, on the device (no host synchronisation)
            self._flat.copy_(torch.where(finite, self._flat, old))
            self._flat_buf.copy_(torch.where(finite, self._flat_buf, old_buf))
            self.skipped_steps += (~finite).to(torch.int64)
        self._push_masters()

    def grad_norm(self):
        """the L2 norm of the heads' gradients of the last gradients() / step() -> 0-d float64 device tensor"""
        import torch
        return torch.sqrt((self._flat_grad.double() ** 2).sum())

    def state_dict(self):
        """the plain network's state dict (its keys; tensors on their devices) with outs.* replaced by copies of the float32 masters"""
        import torch
        sd = {k: v.detach() for k, v in self.net.state_dict().items()}
        for (t, s), (w, b) in ((k, v) for k, v in self.masters.items() if k in self.heads):
            for name, p in ((f"posenet.outs.{t}.{s}.conv.weight", w), (f"posenet.outs.{t}.{s}.conv.bias", b)):
                if name not in sd:
                    raise PosePafError(f"the network has no {name}")
                sd[name] = p.detach().clone()
        # a trained convolution: the folded master as the plain weight behind a BN whose fold is the identity in float32, so a model
        # rebuilt from this dictionary rounds the master's own bits (dividing by the old BN scale would round twice)
        for (kind, t, s), (w, b) in ((k, v) for k, v in self.masters.items() if k in self.convs):
            layer = 1 if kind == "conv2" else 2
            base = f"posenet.features.{t}.before_regress.{s}.{layer}."
            bn = self.net.posenet.features[t].before_regress[s][layer].bn
            new = {"conv.weight": w.detach().permute(0, 3, 1, 2).contiguous()}
            if bn is None:
                new["conv.bias"] = b.detach().clone()
            else:
                new.update({"bn.weight": torch.ones_like(b), "bn.bias": b.detach().clone(), "bn.running_mean": torch.zeros_like(b),
                            "bn.running_var": torch.full_like(b, identity_bn_var(bn.eps))})
            for name, v in new.items():
                if base + name not in sd:
                    raise PosePafError(f"the network has no {base + name}")
                sd[base + name] = v.to(sd[base + name].dtype)
        return sd
