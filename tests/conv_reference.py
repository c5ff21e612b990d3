"""Ground truth for the fused convolution forms at the shapes the product runs (helper module, not a test file).

A layer key of the kernel-choice table (posepaf/fused_model.py: FConv._fused, forward_up2, forward_dual, forward_mean,
forward_pool, FResidual._cat; the bench geometry's keys are listed in profiles/conv_choice_b128.json) names one convolution
form with its shape.  For it this module builds seeded operands, computes the exact value of chosen output pixels in float64
on the CPU from the same fp16 operands, computes the whole output in fp32 with torch.nn.functional (TF32 / xf32 off), and
compares a kernel's output with either.

Operand recipe: inputs N(0, 1), weights N(0, 1) / sqrt(fan_in), bias N(0, 1), added tensors N(0, 1), SE gains U(0, 1);
all stored as fp16.  Epilogues (include/posepaf.h, extra_mode):
  0  y = act(conv + b)            1  y = act(conv + b + e1)           2  y = act(conv + b) + e1
  3  y = fp16(act(conv + b)) + e1 + e2                                4  y = act(conv + b + e1),  y2 = fp16(y) + e2
  5  y = act(conv + b),  y2 = fp16(y) + e2
act = LeakyReLU(0.01) or none.  SE gains multiply the input in binary16 before the convolution; `cat` convolves [t ; x];
`up2` convolves the x2 nearest upsample of x; `pool` outputs are the 2x2 max-pool of the produced tensor (y2 where it exists).
The published variant's forms: `rmean` is mode 1 with the channel mean of y on the side; `pre` is the 1x1 convolution of
fp16(fp16(x * scale[n]) + pre_add); an `up2` key ending in "nopost" has nothing added behind it (mode 0).

Where the roundings sit (held to the bit by tests/test_gpu_conv_exact.py on exact operands, `expected_exact` below): the
accumulator conv + b (+ e1 in modes 1 and 4) is fp32; the activation is max(t, t * slope) with the product rounded to fp32; every
output is rounded to binary16 once, at the store; the inner binary16 roundings are the SE product, the pre_add sum, and fp16(act) /
fp16(y) in front of the adds of modes 3, 4, 5.  The 2x2 maximum orders -0 below +0 (IEEE 754-2019 `maximum`).  The channel mean is
fp16(sum fp16(y) * fl32(1 / hw)): the fp32 sum of the binary16 outputs TIMES the fp32 reciprocal of the pixel count, the product
rounded to binary16 once (multiply and conversion are one instruction) -- not sum / hw: where hw is no power of two the two differ
at ties (sum / hw exactly between two binary16 numbers: the reciprocal's own rounding error, 2^-25 upwards for hw = 3 * 2^j,
decides the side instead of the even mantissa; measured: 1 of 512 means of a 32 x 48 map).
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass

import torch
import torch.nn.functional as F

LEAK = 0.01
TOL = 2e-3               # |y - ref| <= TOL * max(1, max |ref|): fp32 accumulate, fp16 store
TOL_COLLAPSED = 4e-3     # the collapsed upsample convolution's summed weights are rounded to fp16 once more
TOL_FP32 = 1e-5          # the fp32 reference against float64 at the sampled pixels
TILE_PIXELS = 512        # the halo kernel's output tile (csrc/posepaf_conv_own.hip: halo_geometry)
TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "conv_choice_b128.json")


def table_entries(path: str = TABLE) -> list:
    """[(key tuple, committed choice), ...] of a saved kernel-choice table"""
    from posepaf.fused_model import _key_from_json
    return [(_key_from_json(k), int(v)) for k, v in json.load(open(path))["entries"]]


OFFBENCH = os.path.join(os.path.dirname(TABLE), "conv_keys_offbench.json")


def offbench_rows(path: str = OFFBENCH) -> tuple:
    """the key census of the image geometries off the bench's (tools/offbench_keys.py) -> (rows [{"arch", "image": [h, w], "n"}],
    per entry of table_entries(path) the indices of the rows that look its key up)"""
    doc = json.load(open(path))
    return doc["rows"], doc["lookups"]


def key_id(key) -> str:
    return "-".join(("T" if v else "F") if isinstance(v, bool) else str(v) for v in key)


@dataclass
class Spec:
    key: tuple
    form: str        # plain / up2 / dual / mean / pool / cat / rmean / pre
    n: int
    c: int           # input channels of the convolution (c1 + c2 for cat)
    h: int           # input height / width (half resolution for up2)
    w: int
    k: int
    r: int
    pad: int
    dil: int
    mode: int
    act: bool
    c1: int = 0      # cat: channels of t and of x
    c2: int = 0
    ldx: int = 0     # plain keys: pixel strides of x and y (channel slices of wider tensors when > c / k)
    ldy: int = 0
    up: bool = False
    scaled: bool = False
    pooled: bool = False   # the form also hands over the 2x2 max-pool (of y2 when there is one)
    has_y2: bool = False
    has_mean: bool = False
    pre_add: bool = False  # pre: a tensor is added to the scaled input before the convolution

    @property
    def H(self):
        return 2 * self.h if self.up else self.h + 2 * self.pad - self.dil * (self.r - 1)

    @property
    def W(self):
        return 2 * self.w if self.up else self.w + 2 * self.pad - self.dil * (self.r - 1)

    @property
    def fan_in(self):
        return self.c * self.r * self.r

    def outputs(self):
        return ["y"] + (["y2"] if self.has_y2 else []) + (["pool"] if self.pooled else []) + (["mean"] if self.has_mean else [])


def parse_key(key, n: int | None = None) -> Spec:
    """Spec of a table key; n: run it at another batch size"""
    key = tuple(key)
    if not isinstance(key[0], str):
        nn_, c, h, w, k, r, pad, dil, mode, act = key[:10]
        ldx, ldy = (key[11], key[12]) if len(key) > 10 and key[10] == "slice" else (c, k)
        # (a "pixel stride" below the channel count is torch's stride of a size-1 width -- a 1-wide map keyed as a slice, FConv._fused;
        # there is no next pixel in the row for it to reach: the operands are packed)
        ldx, ldy = max(ldx, c), max(ldy, k)
        s = Spec(key, "plain", nn_, c, h, w, k, r, pad, dil, mode, act, ldx=ldx, ldy=ldy)
    elif key[0] == "up2":
        _, nn_, c, h, w, k, post2, act = key[:8]
        nopost = len(key) > 8 and key[8] == "nopost"
        if len(key) > 8 + nopost or (nopost and post2):
            raise ValueError(f"unknown layer key {key}")
        s = Spec(key, "up2", nn_, c, h, w, k, 3, 1, 1, 0 if nopost else (3 if post2 else 2), act, up=True)
    elif key[0] == "dual":
        _, nn_, c, h, w, k, r, pad, dil, act, scaled, pool_ok = key[:12]
        nores = len(key) > 12 and key[12] == "nores"
        s = Spec(key, "dual", nn_, c, h, w, k, r, pad, dil, 5 if nores else 4, act, scaled=scaled, pooled=pool_ok, has_y2=True)
    elif key[0] == "mean":
        _, nn_, c, h, w, k, act = key
        s = Spec(key, "mean", nn_, c, h, w, k, 3, 1, 1, 0, act, has_mean=True)
    elif key[0] == "rmean":
        _, nn_, c, h, w, k, act = key
        s = Spec(key, "rmean", nn_, c, h, w, k, 3, 1, 1, 1, act, has_mean=True)
    elif key[0] == "pre":
        _, nn_, c, h, w, k, pre_add, act = key
        s = Spec(key, "pre", nn_, c, h, w, k, 1, 0, 1, 0, act, scaled=True, pre_add=pre_add)
    elif key[0] == "pool":
        _, nn_, c, h, w, k, res, act = key
        s = Spec(key, "pool", nn_, c, h, w, k, 1, 0, 1, 1 if res else 0, act, pooled=True)
    elif key[0] == "cat":
        _, nn_, c1, c2, h, w, k, act, pool_ok = key
        s = Spec(key, "cat", nn_, c1 + c2, h, w, k, 1, 0, 1, 0, act, c1=c1, c2=c2, pooled=pool_ok)
    else:
        raise ValueError(f"unknown layer key {key}")
    if n is not None:
        s.n = n
    return s


# ---------------------------------------------------------------- operands
def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def make_operands(spec: Spec, seed: int, device="cpu") -> dict:
    """fp16 operands on `device` from a seeded generator on that device (a CPU generator for CPU runs; at 256 samples the inputs
    are 2^28..2^30 elements each, which a CPU generator takes seconds per tensor to draw).  Tensors are NCHW views of
    channels-last storage; a sliced x is the LAST c channels of an (n, h, w, ldx) tensor."""
    g = torch.Generator(device=device).manual_seed(seed)

    def randn(*shape):
        return torch.randn(shape, generator=g, device=device).half()

    s, ops = spec, {}
    if s.form == "cat":
        ops["t"] = randn(s.n, s.h, s.w, s.c1).permute(0, 3, 1, 2)
        ops["x"] = randn(s.n, s.h, s.w, s.c2).permute(0, 3, 1, 2)
    else:
        ld = s.ldx or s.c
        ops["x"] = randn(s.n, s.h, s.w, ld).permute(0, 3, 1, 2)[:, ld - s.c:]
    ops["w"] = _cl((torch.randn((s.k, s.c, s.r, s.r), generator=g, device=device) / math.sqrt(s.fan_in)).half())
    ops["b"] = randn(s.k)
    if s.mode in (1, 2, 3, 4):
        ops["e1"] = randn(s.n, s.H, s.W, s.k).permute(0, 3, 1, 2)
    if s.mode in (3, 4, 5):
        ops["e2"] = randn(s.n, s.H, s.W, s.k).permute(0, 3, 1, 2)
    if s.scaled:
        ops["scale"] = torch.rand((s.n, s.c), generator=g, device=device).half()
    if s.pre_add:
        ops["pre"] = randn(s.n, s.h, s.w, s.c).permute(0, 3, 1, 2)
    return ops


def conv_input(spec: Spec, ops: dict, i0: int, i1: int) -> torch.Tensor:
    """images i0:i1 of what the convolution reads, in fp16 (SE gains multiplied in binary16, then pre_add added in binary16;
    [t ; x] for cat)"""
    x = ops["x"][i0:i1]
    if spec.form == "cat":
        x = torch.cat([ops["t"][i0:i1], x], dim=1)
    if spec.scaled:
        x = x * ops["scale"][i0:i1, :, None, None]
    if spec.pre_add:
        x = x + ops["pre"][i0:i1]
    return x


# ---------------------------------------------------------------- epilogue (any float dtype, any broadcastable layout)
def epilogue(spec: Spec, acc, e1=None, e2=None) -> dict:
    """acc = conv + bias -> {"y": ..., "y2": ...} per extra_mode (module docstring)"""
    m = spec.mode
    t = acc + e1 if m in (1, 4) else acc
    if spec.act:
        t = F.leaky_relu(t, LEAK)
    if m == 2:
        return {"y": t + e1}
    if m == 3:
        return {"y": t.half().to(t.dtype) + e1 + e2}
    if m in (4, 5):
        return {"y": t, "y2": t.half().to(t.dtype) + e2}
    return {"y": t}


# ---------------------------------------------------------------- whole-tensor fp32 reference
class NoTF32:
    """TF32 / xf32 off for the duration (restored afterwards)"""

    def __enter__(self):
        self.saved = (torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32)
        torch.backends.cudnn.allow_tf32 = False
        torch.backends.cuda.matmul.allow_tf32 = False

    def __exit__(self, *a):
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = self.saved


def acc32(spec: Spec, ops: dict, i0: int, i1: int) -> torch.Tensor:
    """conv + bias of images i0:i1 in fp32 (torch.nn.functional)"""
    x = conv_input(spec, ops, i0, i1).float()
    if spec.up:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(x, ops["w"].float(), ops["b"].float(), 1, spec.pad, spec.dil)


def chunk_images(spec: Spec, budget: int = 1 << 28) -> int:
    """images per chunk of the fp32 reference: a power of two (every chunk of a power-of-two batch has the same shape)"""
    nb = 1
    while nb * 2 <= spec.n and nb * 2 * max(spec.k, spec.c) * spec.H * spec.W <= budget:
        nb *= 2
    return nb


def reference32(spec: Spec, ops: dict, pix=None, chunk: int | None = None) -> tuple:
    """-> (outputs {name: fp32 NCHW}, acc32 at the pixels `pix` (P, k) or None).  Computed in chunks of images with TF32 off."""
    n, nb = spec.n, chunk or chunk_images(spec)
    out = {}
    at = torch.empty((len(pix), spec.k), dtype=torch.float32) if pix is not None else None
    with NoTF32(), torch.no_grad():
        for i0 in range(0, n, nb):
            i1 = min(n, i0 + nb)
            a = acc32(spec, ops, i0, i1)
            if pix is not None:
                sel = ((pix[:, 0] >= i0) & (pix[:, 0] < i1)).nonzero().flatten()
                if len(sel):
                    p = pix[sel].to(a.device)
                    at[sel] = a.permute(0, 2, 3, 1)[p[:, 0] - i0, p[:, 1], p[:, 2]].float().cpu()
            e1 = ops["e1"][i0:i1].float() if "e1" in ops else None
            e2 = ops["e2"][i0:i1].float() if "e2" in ops else None
            o = epilogue(spec, a, e1, e2)
            if spec.pooled:
                o["pool"] = F.max_pool2d(o["y2" if spec.has_y2 else "y"], 2, 2)
            if spec.has_mean:
                o["mean"] = o["y"].mean(dim=(2, 3))
            for name, v in o.items():
                if name not in out:
                    out[name] = torch.empty((n,) + tuple(v.shape[1:]), dtype=torch.float32, device=v.device,
                                            memory_format=torch.channels_last if v.dim() == 4 else torch.contiguous_format)
                out[name][i0:i1] = v
            del a, o
    return out, at


# ---------------------------------------------------------------- float64 at chosen pixels
def halo_tile_width(W: int) -> int:
    """the halo kernel's tile width for a map W wide: the widest power of two up to 128 that divides W; 0 when none >= 16 does"""
    tw = 128
    while tw >= 16 and W % tw:
        tw >>= 1
    return tw if tw >= 16 else 0


def halo_cell(n: int, H: int, W: int, dil: int = 1, up: bool = False, csum: bool = False, mode: int = 0):
    """halo_geometry (csrc/posepaf_conv_own.hip) replayed for a 3x3 / pad = dil convolution whose channel counts the kernel takes,
    on an (n, H, W) OUTPUT map: (tile width, tile height, images stacked in a tile, tiles per image), or None where the launcher
    refuses the shape.  up: the input is read at half resolution; csum: channel sums on the side (their stacked form exists for
    the residual epilogue, mode 1, only)."""
    if dil != 1 and (dil < 3 or dil > 5 or up or csum):
        return None
    tw = halo_tile_width(W)
    if not tw:
        return None
    th = TILE_PIXELS // tw
    if dil > 1:
        if tw < 32:
            return None
        gimg, tiles, nhalo = 1, (W // tw) * dil * -(-(-(-H // dil)) // th), (th + 2) * (tw + 2 * dil)
    elif H % th == 0:
        gimg, tiles, nhalo = 1, (W // tw) * (H // th), (th + 2) * (tw + 2)
    else:
        if tw != W or th % H or H % (128 // tw) or n % (th // H) or (csum and mode != 1):
            return None
        gimg, tiles, nhalo = th // H, 1, (th // H) * (H + 2) * (tw + 2)
    npieces = -(-nhalo // 16)
    if not 32 <= npieces <= (56 if tw == 128 or dil > 1 else 48):
        return None
    return tw, th, gimg, tiles


def tile_geometry(H: int, W: int) -> tuple:
    """(tile height, tile width, tiles per row) of the tiles the halo kernel cuts an H x W map into (halo_geometry, dilation 1):
    512 pixels, TW = the widest power of two up to 128 that divides W, TH = 512 / TW when it divides H.  A map lower than that
    tile whose whole images stack in one (TW = W, H | TH, 128 / TW | H) is one tile per image, H x W.  A map the halo kernel does
    not take runs on kernels that do not tile the image: it is cut in bands of up to 512 pixels, min(W, 128) wide (a map narrower
    than 16 is one band) -- the rule this module had before it followed the kernel on maps that are not square powers of two."""
    tw = halo_tile_width(W)
    if tw:
        th = TILE_PIXELS // tw
        if H % th == 0:
            return th, tw, W // tw
        if tw == W and th % H == 0 and H % (128 // tw) == 0:
            return H, W, 1
    tw = min(W, 128)
    th = max(1, min(TILE_PIXELS // tw, H))
    return th, tw, -(-W // tw)


def truth_pixels(n: int, H: int, W: int, seed: int = 0) -> torch.Tensor:
    """the pixels the float64 truth is computed at: every pixel of every image where n * H * W <= 4096, else sample_pixels"""
    if n * H * W > 4096:
        return sample_pixels(n, H, W, seed)
    i, y, x = torch.meshgrid(torch.arange(n), torch.arange(H), torch.arange(W), indexing="ij")
    return torch.stack([i.flatten(), y.flatten(), x.flatten()], 1)


def tile_of(H, W, y, x) -> int:
    th, tw, tx = tile_geometry(H, W)
    return (y // th) * tx + x // tw


def tile_pixels(H, W, tile) -> torch.Tensor:
    th, tw, tx = tile_geometry(H, W)
    y0, x0 = (tile // tx) * th, (tile % tx) * tw
    ys, xs = torch.meshgrid(torch.arange(y0, min(H, y0 + th)), torch.arange(x0, min(W, x0 + tw)), indexing="ij")
    return torch.stack([ys.flatten(), xs.flatten()], 1)


def sample_pixels(n: int, H: int, W: int, seed: int = 0) -> torch.Tensor:
    """(P, 3) long (image, y, x), unique: 8 random pixels of every image; every border pixel and every tile's first and last pixel
    of images 0, n/2 and n - 1; every pixel of the last tile of image n - 1"""
    g = torch.Generator().manual_seed(seed)
    parts = [torch.stack([torch.arange(n).repeat_interleave(8), torch.randint(0, H, (8 * n,), generator=g),
                          torch.randint(0, W, (8 * n,), generator=g)], 1)]
    th, tw, tx = tile_geometry(H, W)
    ntiles = tx * (-(-H // th))
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    border = ((ys == 0) | (ys == H - 1) | (xs == 0) | (xs == W - 1)).flatten()
    yx = torch.stack([ys.flatten(), xs.flatten()], 1)
    ends = torch.cat([tile_pixels(H, W, t)[[0, -1]] for t in range(ntiles)])
    for img in sorted({0, n // 2, n - 1}):
        for q in (yx[border], ends):
            parts.append(torch.cat([torch.full((len(q), 1), img), q], 1))
    q = tile_pixels(H, W, ntiles - 1)
    parts.append(torch.cat([torch.full((len(q), 1), n - 1), q], 1))
    return torch.unique(torch.cat(parts), dim=0)


def _nhwc_at(t, img, y, x):
    """t (n, c, h, w) view: rows t[img, :, y, x] -> (P, c) on the CPU"""
    dev = t.device
    return t.permute(0, 2, 3, 1)[img.to(dev), y.to(dev), x.to(dev)].cpu()


def acc64_at(spec: Spec, ops: dict, pix: torch.Tensor, drop=None) -> torch.Tensor:
    """conv + bias in float64 at output pixels pix (P, 3): each pixel's receptive field (every tap, zero padding, dilation, the x2
    upsample, channel slices, SE gains in binary16) gathered from the fp16 operands and ONE matmul.
    drop = (channel, tap): leave that input channel's contribution at that tap out (the tolerance test's wrong kernel)."""
    img, oy, ox = pix[:, 0], pix[:, 1], pix[:, 2]
    Hin, Win = (2 * spec.h, 2 * spec.w) if spec.up else (spec.h, spec.w)
    cols = []
    for i in range(spec.r):
        for j in range(spec.r):
            iy, ix = oy - spec.pad + i * spec.dil, ox - spec.pad + j * spec.dil
            ok = (iy >= 0) & (iy < Hin) & (ix >= 0) & (ix < Win)
            sy, sx = iy.clamp(0, Hin - 1), ix.clamp(0, Win - 1)
            if spec.up:
                sy, sx = sy // 2, sx // 2
            v = _nhwc_at(ops["x"], img, sy, sx)
            if spec.form == "cat":
                v = torch.cat([_nhwc_at(ops["t"], img, sy, sx), v], 1)
            if spec.scaled:
                v = v * ops["scale"].cpu()[img]                          # binary16 product, as the kernel's input read
            if spec.pre_add:
                v = v + _nhwc_at(ops["pre"], img, sy, sx)                # binary16 sum of the rounded product
            v = v.double() * ok[:, None].double()
            if drop is not None and drop[1] == i * spec.r + j:
                v[:, drop[0]] = 0
            cols.append(v)
    wm = ops["w"].cpu().double().permute(0, 2, 3, 1).reshape(spec.k, -1)      # (k, r * r * c), taps major like `cols`
    return torch.cat(cols, 1) @ wm.T + ops["b"].cpu().double()


def outputs64_at(spec: Spec, ops: dict, pix: torch.Tensor, drop=None) -> dict:
    """every per-pixel output of the form in float64 at pix (P, 3): {"y": (P, k), "y2": ...}"""
    a = acc64_at(spec, ops, pix, drop)
    e = {n_: _nhwc_at(ops[n_], pix[:, 0], pix[:, 1], pix[:, 2]).double() if n_ in ops else None for n_ in ("e1", "e2")}
    return epilogue(spec, a, e["e1"], e["e2"])


def pooled64_at(spec: Spec, ops: dict, pix: torch.Tensor) -> torch.Tensor:
    """the form's 2x2 max-pool output in float64 at pooled-grid pixels pix (P, 3)"""
    src = torch.cat([torch.stack([pix[:, 0], 2 * pix[:, 1] + dy, 2 * pix[:, 2] + dx], 1) for dy in (0, 1) for dx in (0, 1)])
    o = outputs64_at(spec, ops, src)["y2" if spec.has_y2 else "y"]
    return o.view(4, len(pix), spec.k).amax(0)


def values_at(t: torch.Tensor, pix: torch.Tensor) -> torch.Tensor:
    """(n, k, H, W) -> (P, k) float64 on the CPU"""
    return _nhwc_at(t, pix[:, 0], pix[:, 1], pix[:, 2]).double()


# ---------------------------------------------------------------- the comparison
def mismatch(got, ref, bound: float, label: str, pix=None, img0: int = 0):
    """None when every |got - ref| <= bound (NaN fails), else a message naming the first bad image, its tile and the error.
    Whole tensors: got / ref (nb, k, H, W), images img0 ...; sampled pixels: got / ref (P, k) at pix (P, 3).  (n, k) tensors
    (channel means) are compared as (n, k, 1, 1)."""
    if pix is None and got.dim() == 2:
        got, ref = got[:, :, None, None], ref[:, :, None, None]
    err = (got.to(ref.dtype) - ref).abs()
    bad = ~(err <= bound)
    if pix is None:
        per_img = bad.flatten(1).any(1)
        if not bool(per_img.any()):
            return None
        i = int(per_img.nonzero()[0])
        H, W = got.shape[2:]
        q = int(bad[i].any(0).flatten().nonzero()[0])
        y, x = divmod(q, W)
        e_img = float(err[i].nan_to_num(float("inf")).max())
        n_bad = int(per_img.sum())
        img = img0 + i
    else:
        rows = bad.any(1)
        if not bool(rows.any()):
            return None
        order = torch.argsort(pix[:, 0] * (1 << 40) + pix[:, 1] * (1 << 20) + pix[:, 2])   # first bad in image order
        j = int(order[rows[order].nonzero()[0]])
        img, y, x = (int(v) for v in pix[j])
        H, W = int(pix[:, 1].max()) + 1, int(pix[:, 2].max()) + 1
        e_img = float(err[pix[:, 0] == img].nan_to_num(float("inf")).max())
        n_bad = int(pix[rows, 0].unique().numel())
    return (f"{label}: image {img} (first of {n_bad} bad images), tile {tile_of(H, W, y, x)} at pixel (y {y}, x {x}): "
            f"max |err| {e_img:.4g} in that image > bound {bound:.4g}")


def assert_close(got, ref, bound, label, pix=None, img0=0):
    msg = mismatch(got, ref, bound, label, pix, img0)
    assert msg is None, msg


def bound_for(ref_max: float, tol: float = TOL) -> float:
    return tol * max(1.0, float(ref_max))


# ---------------------------------------------------------------- exact operands, exact expectations
# Operands for which every fp32 partial sum of the convolution is exact IN ANY ORDER: the only roundings left are the ones the
# module docstring names, the expected output is known to the last bit, and a kernel is compared with it as integers
# (tests/test_gpu_conv_exact.py; the house style of test_exact_small_integers in tests/test_gpu_head_wgrad.py).
RECIPES = ("small", "rounding", "subnormal")
SUBNORMAL_UNIT = 2.0 ** -24          # the binary16 subnormal grid
EXACT_LIMIT = 2.0 ** 24              # fp32 holds every integer below it
GAINS = (0.5, 1.0, 1.5, 2.0)


def inner_roundings(spec: Spec) -> list:
    """the binary16 roundings INSIDE the form's contract (the final store is not one): "scale" fp16(x * s), "pre"
    fp16(fp16(x * s) + pre_add), "act" fp16(act) in front of the adds of modes 3, 4, 5"""
    return (["scale"] if spec.scaled else []) + (["pre"] if spec.pre_add else []) + (["act"] if spec.mode in (3, 4, 5) else [])


def recipes_for(spec: Spec) -> list:
    """`rounding` goes to the forms with an inner rounding.  The channel-mean forms are left out of it: their sums are fp32 sums in
    a kernel-chosen order, exact only while sum |fp16(y)| stays below 2^24 grid units, which magnitudes beyond 2048 over a map of
    thousands of pixels do not allow (their only rounding besides the store is the mean's own, which `small` has as well)."""
    return ["small"] + (["rounding"] if inner_roundings(spec) and not spec.has_mean else []) + ["subnormal"]


def make_exact_operands(spec: Spec, seed: int, recipe: str, device="cpu") -> dict:
    """make_operands' dictionary and layouts with operands on a grid (drawn by a CPU generator, then moved to `device`).
    small      x integers in [-3, 3], weights in [-2, 2], bias / e1 / e2 / pre_add in [-8, 8], SE gains from {0.5, 1, 1.5, 2}.
               The channel-mean forms (`mean`, `rmean`) get x and weights from {0, 1} and bias / e1 from [0, 8] instead: the
               product's slope is 0.01, a negative output fp16(0.01 t) sits on a 2^-17 grid, and an fp32 sum of such values over a
               map is not exact in every order; without negative outputs every y is an integer and sum y < 2^24.  (The negative
               branch of their epilogue is reached under `subnormal`, where every binary16 value is on ONE grid.)
    rounding   magnitudes at which the inner roundings are visible.  Scaled forms: two input channels hold odd integers of magnitude
               1025 .. 2047 under a gain of 1.5 or 3 (the product needs more than 11 bits, as in test_exact_product_needs_its_rounding
               of tests/test_gpu_head_wgrad.py), so accumulators reach +-25000 and fp16(y) + e2 differs from y + e2.  Unscaled forms:
               x integers up to +-1500 sqrt(1.5 / fan_in) (accumulators of standard deviation ~1500, many beyond 2048); e1 / e2 in
               [-255, 255].
    subnormal  `small` (mixed signs for every form) with x, bias, e1, e2 and pre_add multiplied by 2^-24: every input value and every
               output is a binary16 subnormal or zero, every accumulator an integer multiple of 2^-24."""
    assert recipe in RECIPES, recipe
    assert recipe != "rounding" or "rounding" in recipes_for(spec), f"{spec.form}: no inner rounding to show"
    g = torch.Generator().manual_seed(seed)
    s, ops = spec, {}
    nonneg = s.has_mean and recipe == "small"
    unit = SUBNORMAL_UNIT if recipe == "subnormal" else 1.0
    xmax, wmax, emax = (1, 1, 8) if nonneg else (3, 2, 8)
    if recipe == "rounding":
        emax = 255
        if not s.scaled:
            xmax = max(3, min(255, int(1500.0 * math.sqrt(1.5 / s.fan_in))))

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()

    def put(t):
        return t.half().to(device)

    lo = 0 if nonneg else -1
    if s.form == "cat":
        xs = {"t": ints(lo * xmax, xmax, s.n, s.h, s.w, s.c1), "x": ints(lo * xmax, xmax, s.n, s.h, s.w, s.c2)}
    else:
        ld = s.ldx or s.c
        xs = {"x": ints(lo * xmax, xmax, s.n, s.h, s.w, ld)}
    if s.scaled:
        scale = torch.tensor(GAINS)[torch.randint(0, len(GAINS), (s.n, s.c), generator=g)]
        if recipe == "rounding":
            big = torch.randperm(s.c, generator=g)[:2]
            mag = 1025 + 2 * torch.randint(0, 512, (s.n, s.h, s.w, 2), generator=g)                      # odd, 1025 .. 2047
            sign = 1 - 2 * torch.randint(0, 2, (s.n, s.h, s.w, 2), generator=g)
            xs["x"][..., big] = (mag * sign).float()
            scale[:, big] = torch.tensor((1.5, 3.0))[torch.randint(0, 2, (s.n, 2), generator=g)]
        ops["scale"] = put(scale)
    for name, v in xs.items():
        v = put(v * unit).permute(0, 3, 1, 2)
        ops[name] = v[:, v.shape[1] - s.c:] if name == "x" and s.form != "cat" else v
    ops["w"] = _cl(put(ints(lo * wmax, wmax, s.k, s.c, s.r, s.r)))
    ops["b"] = put(ints(lo * 8, 8, s.k) * unit)
    if s.mode in (1, 2, 3, 4):
        ops["e1"] = put(ints(lo * emax, emax, s.n, s.H, s.W, s.k) * unit).permute(0, 3, 1, 2)
    if s.mode in (3, 4, 5):
        ops["e2"] = put(ints(lo * emax, emax, s.n, s.H, s.W, s.k) * unit).permute(0, 3, 1, 2)
    if s.pre_add:
        ops["pre"] = put(ints(-8, 8, s.n, s.h, s.w, s.c) * unit).permute(0, 3, 1, 2)
    return ops


def _to_half_once(t64: torch.Tensor) -> torch.Tensor:
    """float64 -> binary16 with ONE rounding (NumPy converts directly; torch's conversion passes through float32)"""
    return torch.from_numpy(t64.contiguous().numpy().astype("float16"))


def exact_input64(spec: Spec, ops: dict, skip=()) -> torch.Tensor:
    """what the convolution reads, (n, c, h, w) float64 on the CPU: x [; t], times the SE gains, rounded to binary16, plus pre_add,
    rounded to binary16.  skip: roundings left out (a WRONG order, for the share of elements that can tell)."""
    x = ops["x"].cpu().double()
    if spec.form == "cat":
        x = torch.cat([ops["t"].cpu().double(), x], dim=1)
    if spec.scaled:
        x = x * ops["scale"].cpu().double()[:, :, None, None]        # 11 x 11 bits: exact in float64 (and in float32)
        if "scale" not in skip:
            x = _to_half_once(x).double()
    if spec.pre_add:
        x = x + ops["pre"].cpu().double()
        if "pre" not in skip:
            x = _to_half_once(x).double()
    return x


def exact_epilogue(spec: Spec, acc64, e1=None, e2=None, skip=()) -> dict:
    """acc64 = conv + bias, exact in float64 -> {"y": fp16, "y2": fp16} per extra_mode, any layout.  The accumulator (with e1 in
    modes 1 and 4) must be a float32 number -- the validity condition; from there the arithmetic is the epilogue's, in float32:
    the activation max(t, t * slope) with the PRODUCT rounded to float32, the adds of modes 2 .. 5 as float32 sums (exact under
    every recipe except mode 2's act + e1 behind a negative t, where the float32 sum is rounded before the store rounds it)."""
    m = spec.mode
    t64 = acc64 + e1.double() if m in (1, 4) else acc64
    t = t64.float()
    assert bool((t.double() == t64).all()), "the case is not exact: an accumulator is no float32 number"
    u = t * torch.tensor(LEAK if spec.act else 1.0, dtype=torch.float32)
    a = torch.maximum(t, u)
    if m == 2:
        return {"y": (a + e1.float()).half()}
    inner = a if "act" in skip else a.half().float()
    if m == 3:
        return {"y": (inner + e1.float() + e2.float()).half()}
    if m in (4, 5):
        return {"y": a.half(), "y2": (inner + e2.float()).half()}
    return {"y": a.half()}


def exact_acc64(spec: Spec, xin64: torch.Tensor, ops: dict) -> torch.Tensor:
    """conv + bias of the whole batch in float64 on the CPU"""
    if spec.up:
        xin64 = F.interpolate(xin64, scale_factor=2, mode="nearest")
    return F.conv2d(xin64.contiguous(), ops["w"].cpu().double().contiguous(), ops["b"].cpu().double(), 1, spec.pad, spec.dil)


def expected_exact(spec: Spec, ops: dict, skip=()) -> dict:
    """every output of the form ("y", "y2", "pool" (n, k, H, W) views; "mean" (n, k)) as the binary16 tensor the contract of the
    module docstring defines, computed in float64 on the CPU from the fp16 operands:
      the SE product x * s, then + pre_add, each rounded to binary16;  the activation max(t, t * slope), product in float32;
      mode 3: fp16(act) + e1 + e2;  modes 4 and 5: y2 = fp16(y) + e2;  pool: the max-pool of the produced binary16 tensor;
      mean: fp16(sum fp16(y) * fl32(1 / hw)), sum and product exact, one rounding."""
    acc = exact_acc64(spec, exact_input64(spec, ops, skip), ops)
    e1 = ops["e1"].cpu() if "e1" in ops else None
    e2 = ops["e2"].cpu() if "e2" in ops else None
    out = exact_epilogue(spec, acc, e1, e2, skip)
    if spec.pooled:
        out["pool"] = max_pool_binary16(out["y2" if spec.has_y2 else "y"])
    if spec.has_mean:
        out["mean"] = mean_binary16(out["y"])
    return out


def max_pool_binary16(t: torch.Tensor) -> torch.Tensor:
    """2x2 max-pool of an fp16 tensor with the maximum of IEEE 754-2019, which orders -0 below +0 (the packed binary16 maximum of
    the kernels does; torch's max_pool2d keeps whichever zero it met first).  Both zeros occur under the `subnormal` recipe."""
    m = F.max_pool2d(t.float(), 2, 2)
    plus = F.max_pool2d((t.contiguous().view(torch.int16) == 0).float(), 2, 2) > 0          # a +0 in the window
    zero = torch.zeros_like(m)
    return torch.where(m == 0, torch.where(plus, zero, -zero), m).half()


def mean_binary16(y: torch.Tensor) -> torch.Tensor:
    """(n, k, H, W) fp16 -> (n, k) fp16 channel means as the kernels form them (csrc/posepaf_epilogue.hip: k_channel_mean_finish,
    k_se_gains): the exact sum TIMES the float32 reciprocal of the pixel count, the exact product rounded to binary16 once"""
    inv = (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(y.shape[2] * y.shape[3]), dtype=torch.float32)).double()
    return _to_half_once(y.double().sum(dim=(2, 3)) * inv)


def _on_grid(t, grid: float) -> bool:
    q = t.double() / grid
    return bool((q == q.round()).all())


def assert_exact_case(spec: Spec, ops: dict, recipe: str, want: dict, label: str) -> dict:
    """The conditions under which bit equality may be asked of ANY summation order, asserted on the reference before anything is
    compared (a case that breaks one is a bug of the test, not a finding):
      per output element  sum |x * w| + |b| + |e1| + |e2| < 2^24  in units of the operands' grid (0.5; 2^-24 under `subnormal`), and
      every conv input and added tensor on that grid: every fp32 partial sum is exact in every order;
      every expected output finite;
      channel sums: every y on a grid (1; 2^-24) with sum |y| < 2^24 grid units per image and channel;
      subnormal: every input value and every expected output is a binary16 subnormal or zero;
      rounding: per inner rounding of the form, the share of elements of the output behind it that differ between the contract's order
      and the order WITHOUT that rounding is > 0, and the share of elements any of them changes is >= 1 %.
    -> {"abs_sum_max": grid units, "shares": {rounding: share, "any": share}}"""
    grid = SUBNORMAL_UNIT if recipe == "subnormal" else 0.5
    xin = exact_input64(spec, ops)
    added = [ops[n_].cpu().double() for n_ in ("e1", "e2") if n_ in ops]
    for t in [xin, ops["b"].cpu()] + added:
        assert _on_grid(t, grid), f"{label} [{recipe}]: an operand is off the grid {grid}"
    s_abs = dict(ops, w=ops["w"].abs(), b=ops["b"].abs())
    a = exact_acc64(spec, xin.abs(), s_abs)
    for t in added:
        a = a + t.abs()
    abs_max = float(a.max()) / grid
    assert abs_max < EXACT_LIMIT, f"{label} [{recipe}]: sum |x w| + |b| + |e| reaches {abs_max:.4g} grid units: fp32 sums are not exact"
    for name, v in want.items():
        assert bool(torch.isfinite(v.float()).all()), f"{label} [{recipe}]: expected {name} is not finite"
    if spec.has_mean:
        ygrid = SUBNORMAL_UNIT if recipe == "subnormal" else 1.0
        y = want["y"].double()
        assert _on_grid(y, ygrid), f"{label} [{recipe}]: outputs off the grid {ygrid}: their fp32 sum depends on the order"
        tot = float(y.abs().sum(dim=(2, 3)).max()) / ygrid
        assert tot < EXACT_LIMIT, f"{label} [{recipe}]: sum |y| reaches {tot:.4g} grid units"
    if recipe == "subnormal":
        lim = 2.0 ** -14
        for name in [n_ for n_ in ("x", "t", "b", "e1", "e2", "pre") if n_ in ops]:
            assert float(ops[name].abs().max()) < lim, f"{label}: operand {name} is not subnormal"
        assert float(xin.abs().max()) < lim
        for name, v in want.items():
            assert float(v.float().abs().max()) < lim, f"{label}: expected {name} leaves the subnormal range"
    shares = {}
    if recipe == "rounding":
        anyd = None
        for r in inner_roundings(spec):
            other = expected_exact(spec, ops, skip=(r,))
            name = "y2" if (r == "act" and spec.has_y2) else "y"
            d = want[name].view(torch.int16) != other[name].view(torch.int16)
            shares[r] = float(d.float().mean())
            anyd = d if anyd is None else (anyd | d)
            assert shares[r] > 0, f"{label}: no element can tell whether the rounding `{r}` happens"
        shares["any"] = float(anyd.float().mean())
        assert shares["any"] >= 0.01, f"{label}: only {shares['any']:.3%} of the elements depend on the rounding order"
    return {"abs_sum_max": abs_max, "shares": shares}


def first_bit_difference(got: torch.Tensor, want: torch.Tensor, label: str):
    """None when two fp16 tensors ((n, k, H, W), or (n, k) channel means) hold the same BITS, else a message naming the first
    differing image, its tile and pixel, the channel and both values"""
    if got.dim() == 2:
        got, want = got[:, :, None, None], want[:, :, None, None]
    g, w = got.contiguous().view(torch.int16), want.to(got.device).contiguous().view(torch.int16)
    bad = g != w
    if not bool(bad.any()):
        return None
    n_bad = int(bad.sum())
    zeros = int((bad & ((g & 0x7FFF) == 0) & ((w & 0x7FFF) != 0)).sum())     # a flush shows as zeros where a value is due
    i, ch, y, x = (int(v) for v in bad.permute(0, 2, 3, 1).nonzero()[0][[0, 3, 1, 2]])
    H, W = got.shape[2:]
    return (f"{label}: {n_bad} of {bad.numel()} elements differ ({zeros} of them are zero where a value is expected, largest "
            f"|difference| {float((got.double() - want.to(got.device).double()).abs().nan_to_num(float('inf')).max()):.6g}); "
            f"first: image {i}, tile {tile_of(H, W, y, x)} at pixel (y {y}, x {x}), "
            f"channel {ch}: got {float(got[i, ch, y, x])!r} (0x{int(g[i, ch, y, x]) & 0xFFFF:04x}), "
            f"expected {float(want[i, ch, y, x])!r} (0x{int(w[i, ch, y, x]) & 0xFFFF:04x})")
