"""The launch side of the per-key kernel sweeps (helper module, not a test file; tests/test_gpu_bench_shapes.py and
tests/test_gpu_offbench_shapes.py): guarded NaN-filled outputs, and per layer key every kernel the tuner could pick for it, each
with its launch on given outputs.  The plain keys run through FConv._fused_launch, the product's own argument marshalling; the
other forms allocate their outputs themselves in posepaf/fused_model.py, so their C entry points are called here."""
import ctypes as C

import torch

import conv_reference as cr

GUARD = 64 * 1024 // 2          # fp16 elements of NaN on each side of an output
NAN16 = 0x7E00                  # the bits torch.full(nan) stores in fp16
REFUSED = (-6, -3)              # PP_ERR_UNSUPPORTED, PP_ERR_TOO_LARGE: the tuner skips the candidate
MIOPEN = -1                     # the tuner's choice -1: MIOpen's convolution, then the k_bias_act pass


class Out:
    """an (n, k, H, W) fp16 output with pixel stride ld at channel offset off inside a NaN-filled buffer with guards"""

    def __init__(self, n, k, H, W, ld=None, off=0):
        ld = ld or k
        self.body = n * H * W * ld
        self.buf = torch.full((GUARD + self.body + GUARD,), float("nan"), dtype=torch.float16, device="cuda")
        self.t = self.buf.as_strided((n, k, H, W), (H * W * ld, 1, W * ld, ld), GUARD + off)
        self.ld, self.off, self.k = ld, off, k

    def intact(self):
        """-> None, or what was overwritten outside the tensor"""
        bits = self.buf.view(torch.int16)
        for name, part in (("guard before", bits[:GUARD]), ("guard after", bits[GUARD + self.body:])):
            if not bool((part == NAN16).all()):
                return name
        if self.ld != self.k:
            rows = bits[GUARD:GUARD + self.body].view(-1, self.ld)
            if not (bool((rows[:, :self.off] == NAN16).all()) and bool((rows[:, self.off + self.k:] == NAN16).all())):
                return "the other channels of the wider tensor"
        return None


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _fconv(spec, ops):
    """the product's layer object holding the test's fp16 weights"""
    from posepaf import fused_model as fm
    conv = torch.nn.Conv2d(spec.c, spec.k, spec.r, 1, spec.pad, spec.dil, bias=True)
    with torch.no_grad():
        conv.weight.copy_(ops["w"].float().cpu())
        conv.bias.copy_(ops["b"].float().cpu())
    f = fm.FConv(conv, None, spec.act).cuda().half()
    f.weight.data = f.weight.data.contiguous(memory_format=torch.channels_last)
    assert torch.equal(f.weight, ops["w"]) and torch.equal(f.bias, ops["b"])
    return f


def _miopen_bias_act(f, x, res=None, post=None):
    """the product's path where no fused kernel takes a shape (FConv.forward: hip_bias_act_(conv_only(x), ...)), with torch's
    convolution pinned to its deterministic algorithms as tests/test_gpu_val_loss.py pins it: MIOpen's default choice for these
    small maps accumulates in an order that changes from call to call (measured on the MI355X: six calls of conv2d
    (1, 128, 16, 16) -> 128, 3x3, gave a first result and five that differ from it by up to 2^-8; with the flag six equal ones),
    which the two-runs comparison would report as a race of this library's kernels"""
    from posepaf import fused_model as fm
    pinned = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        y = f.conv_only(x)
    finally:
        torch.backends.cudnn.deterministic = pinned
    return fm.hip_bias_act_(y, f.bias, res, f.act, post)


def candidates(spec, ops, miopen: bool = False):
    """[(candidate id, tolerance, launch(outs) -> rc, output shapes)] -- the tuner's candidate list for the form
    (posepaf/fused_model.py), each with its launch on given outputs.  miopen: a plain key also gets candidate -1
    (_miopen_bias_act), and an `rmean` key candidate 0, the separate form on the same path (its one-launch form is refused by
    BATCH SIZE where images stack, after the key is made: FConv._res_mean_fused asks for the splits of a batch of 32); both
    allocate their own outputs, which are copied into the given ones."""
    from posepaf import _lib, fused_model as fm
    L = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    s, f = spec, _fconv(spec, ops)
    slope = fm.LEAK if s.act else 1.0
    x, e1, e2 = ops["x"], ops.get("e1"), ops.get("e2")
    n, H, W, k = s.n, s.H, s.W, s.k
    full = {"y": (n, k, H, W)}
    out = []
    if s.form == "plain":
        cfgs = list(range(L.pp_conv_num_configs()))
        cfgs += [c for c in fm.OWN_VARIANTS if L.pp_conv_own_supported(s.c, k, s.r)]
        if s.r == 1 and L.pp_pw_supported(s.c, k):
            cfgs.append(fm.PW_VARIANT)
        for cfg in cfgs:
            out.append((cfg, cr.TOL, lambda o, cfg=cfg: f._fused_launch(cfg, x, e1, s.mode, o["y"]), full))
        if miopen:
            def launch(o):
                o["y"].copy_(_miopen_bias_act(f, x, e1 if s.mode == 1 else None, e1 if s.mode == 2 else None))
                return 0
            out.append((MIOPEN, cr.TOL, launch, full))
    elif s.form == "up2":
        out.append((1, cr.TOL, lambda o: L.pp_conv_own_ex_f16(_p(x), _p(f.weight), _p(f.bias), _p(e1), _p(e2), _p(o["y"]), None, n, H, W,
                                                             s.c, k, 3, 1, 1, s.mode, slope, 512, 1, st), full))
        w4 = f._collapsed_weights()
        for i, bn in enumerate((256, 128, 64, 512)):
            if k % (bn if bn != 512 else 64) == 0:
                out.append((2 + i, cr.TOL_COLLAPSED, lambda o, bn=bn: L.pp_conv_up2_collapsed_f16(
                    _p(x), _p(w4), _p(f.bias), _p(e1), _p(e2), _p(o["y"]), n, s.h, s.w, s.c, k, s.mode, slope, bn, st), full))
    elif s.form == "dual":
        shapes = dict(full, y2=(n, k, H, W), **({"pool": (n, k, H // 2, W // 2)} if s.pooled else {}))
        sc = ops.get("scale")
        for bn in (256, 128, 64, 512, fm.PW_VARIANT):
            if bn != fm.PW_VARIANT and (k % (bn if bn != 512 else 128) or s.mode == 5 or sc is not None):
                continue                 # the tuner does not try it, or the kernel has no such form (FConv.forward_dual.fused)
            if bn == fm.PW_VARIANT:
                if not (s.r == 1 and s.pad == 0 and L.pp_pw_supported(s.c, k)):
                    continue

                def launch(o):
                    if s.pooled:
                        return L.pp_pw_pool_f16(_p(x), _p(sc), _p(f.weight), _p(f.bias), _p(e1), _p(e2), _p(o["y"]), _p(o["y2"]),
                                                _p(o["pool"]), n * H * W, H * W, W, s.c, k, k, s.mode, slope, st)
                    return L.pp_pw_f16(_p(x), _p(sc), _p(f.weight), _p(f.bias), _p(e1), _p(e2), _p(o["y"]), _p(o["y2"]), n * H * W,
                                       H * W, s.c, k, k, s.mode, slope, st)
            else:
                def launch(o, bn=bn):
                    return L.pp_conv_own_ex_f16(_p(x), _p(f.weight), _p(f.bias), _p(e1), _p(e2), _p(o["y"]), _p(o["y2"]), n, s.h, s.w,
                                                s.c, k, s.r, s.pad, s.dil, 4, slope, bn, 0, st)
            if s.pooled and bn != fm.PW_VARIANT:
                def launch(o, inner=launch):   # the product pools y2 with the helper kernel (fm.maxpool2) after the launch
                    rc = inner(o)
                    if rc == 0:
                        rc = L.pp_maxpool2_f16(_p(o["y2"]), _p(o["pool"]), n, H // 2, W // 2, k, st)
                    return rc
            out.append((bn, cr.TOL, launch, shapes))
    elif s.form == "mean":
        splits = L.pp_conv_own_sums_splits(s.h, s.w)

        def launch(o):
            ws = torch.full((n, max(splits, 1), k), float("nan"), dtype=torch.float32, device="cuda")
            rc = L.pp_conv_own_sums_f16(_p(x), _p(f.weight), _p(f.bias), _p(o["y"]), _p(ws), n, s.h, s.w, s.c, k, slope, st)
            if rc == 0:
                rc = L.pp_channel_mean_finish_f16(_p(ws), _p(o["mean"]), n, H * W, k, splits, st)
            return rc
        if splits > 0:
            out.append((1, cr.TOL, launch, dict(full, mean=(n, k))))
    elif s.form == "rmean":
        splits = L.pp_conv_own_res_sums_splits(s.h, s.w)

        def launch(o):
            ws = torch.full((n, max(splits, 1), k), float("nan"), dtype=torch.float32, device="cuda")
            rc = L.pp_conv_own_res_sums_f16(_p(x), _p(f.weight), _p(f.bias), _p(e1), _p(o["y"]), _p(ws), n, s.h, s.w, s.c, k, slope, st)
            if rc == 0:
                rc = L.pp_channel_mean_finish_f16(_p(ws), _p(o["mean"]), n, H * W, k, splits, st)
            return rc
        if splits > 0:       # (0: halo_geometry refuses the map for every batch size, and there is no workspace size to launch with)
            out.append((1, cr.TOL, launch, dict(full, mean=(n, k))))
        if miopen:
            def separate(o):
                y = _miopen_bias_act(f, x, e1)
                o["y"].copy_(y)
                o["mean"].copy_(fm.channel_mean(y))
                return 0
            out.append((0, cr.TOL, separate, dict(full, mean=(n, k))))
    elif s.form == "pre":
        sc, aa = ops["scale"].contiguous(), ops.get("pre")
        out.append((1, cr.TOL, lambda o: L.pp_pw_pre_f16(_p(x), _p(sc), _p(aa), _p(f.weight), _p(f.bias), _p(o["y"]), n * H * W, H * W,
                                                        s.c, k, k, slope, st), full))
    elif s.form == "pool":
        out.append((1, cr.TOL, lambda o: L.pp_pw_pool_f16(_p(x), None, _p(f.weight), _p(f.bias), _p(e1), None, _p(o["y"]), None,
                                                         _p(o["pool"]), n * H * W, H * W, W, s.c, k, k, s.mode, slope, st),
                    dict(full, pool=(n, k, H // 2, W // 2))))
    elif s.form == "cat":
        wcat = f.weight.detach().flatten(1).contiguous()          # (k, c1 + c2): the product's _wcat
        shapes = dict(full, **({"pool": (n, k, H // 2, W // 2)} if s.pooled else {}))
        out.append((1, cr.TOL, lambda o: L.pp_pw_cat_f16(_p(ops["t"]), _p(x), _p(wcat), _p(f.bias), None, _p(o["y"]), _p(o.get("pool")),
                                                        n * H * W, H * W, W if s.pooled else 0, s.c1, s.c2, k, k, 0, slope, st),
                    shapes))
    return out


def cells(spec, cand) -> set:
    """names of the launcher cells a candidate that RAN (rc 0) went through, worked out on the CPU from the launchers' own rules
    (csrc/posepaf_conv_own.hip: conv_own_run, halo_geometry): "<halo form> tw<tile width> x<images stacked in a tile>[ dil]" for the
    halo kernel's instances, "igemm[ ragged]" for k_conv_igemm (ragged: W % 16 != 0), "pwpool W<width>", "pwpre"."""
    s = spec
    halo3 = s.r == 3 and s.pad == s.dil and s.c % 32 == 0 and s.k % 64 == 0

    def halo(name, H, W, **kw):
        g = cr.halo_cell(s.n, H, W, **kw) if halo3 else None
        return {f"{name} tw{g[0]} x{g[2]}" + (" dil" if kw.get("dil", 1) > 1 else "")} if g else set()

    if s.form == "plain":
        if cand in (104, 106):
            return halo(f"halo{cand}", s.H, s.W, dil=s.dil)
        if cand in (101, 102, 103):
            return {"igemm ragged" if s.W % 16 else "igemm"}
    elif s.form == "up2":
        if cand == 1:
            return halo("up", s.H, s.W, up=True)
        if cand == 5:
            return halo("collapsed", s.h, s.w)          # the four phases walk the half-resolution grid
        return {"igemm ragged" if s.w % 16 else "igemm"}
    elif s.form == "mean":
        return halo("sums", s.H, s.W, csum=True, mode=0)
    elif s.form == "rmean":
        return halo("rsums", s.H, s.W, csum=True, mode=1) if cand == 1 else set()
    elif s.form == "dual":
        if cand == 512:
            return halo("dual", s.H, s.W, dil=s.dil)
        if cand == 105:
            return {f"pwpool W{s.W}"} if s.pooled else set()
        return {"igemm ragged" if s.W % 16 else "igemm"}
    elif s.form == "pool":
        return {f"pwpool W{s.W}"}
    elif s.form == "pre":
        return {"pwpre"}
    return set()


def _outputs(spec, shapes):
    o = {}
    for name, shp in shapes.items():
        if name == "y" and spec.ldy != spec.k and spec.form == "plain":
            o[name] = Out(*shp, ld=spec.ldy, off=spec.ldy - spec.k)       # the LAST k channels of the wider tensor
        elif len(shp) == 4:
            o[name] = Out(*shp)
        else:
            o[name] = Out(shp[0], shp[1], 1, 1)
    return o


def _view(spec, name, o):
    return o.t[:, :, 0, 0] if name == "mean" else o.t
