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
