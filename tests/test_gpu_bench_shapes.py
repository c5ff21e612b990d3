"""GPU: every kernel the per-shape tuner could pick, at every layer shape of the bench geometry (512 x 512, 256 samples = 128 images
and their flips; profiles/conv_choice_b128.json) and at the batch-1-with-flip geometry (2 samples), against ground truth over the
WHOLE batch.  Which candidate wins a shape changes from box to box inside the timing noise, so any candidate that takes a shape
can end up in the product.

Per key and candidate: the whole output (and the second / pooled / channel-mean output where the form has one) against an fp32
torch.nn.functional reference that is itself checked against float64 at a stratified pixel sample (tests/conv_reference.py), the
sample against float64 directly, two runs bit-identical, outputs pre-filled with NaN so that an unwritten element fails, and every
output a view into a buffer with a 64 KiB NaN guard on both sides (and, for a channel slice, the other channels of the wider
tensor) that must come back intact.  The plain keys run through FConv._fused_launch, the product's own argument marshalling;
the other forms allocate their outputs themselves in posepaf/fused_model.py, so their C entry points are called here with the
NaN-filled guarded outputs instead -- an element a kernel never writes cannot hold an earlier candidate's value."""
import ctypes as C
import json
import zlib

import pytest
import torch

import conv_reference as cr

pytestmark = pytest.mark.gpu

ENTRIES = cr.table_entries()
GUARD = 64 * 1024 // 2          # fp16 elements of NaN on each side of an output
NAN16 = 0x7E00                  # the bits torch.full(nan) stores in fp16
REFUSED = (-6, -3)              # PP_ERR_UNSUPPORTED, PP_ERR_TOO_LARGE: the tuner skips the candidate


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


def candidates(spec, ops):
    """[(candidate id, tolerance, launch(outs) -> rc, output shapes)] -- the tuner's candidate list for the form
    (posepaf/fused_model.py), each with its launch on given outputs"""
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


def test_the_table_lists_every_shape_of_the_bench_geometry():
    """Census: with the committed table installed, one forward of the bench model (256 x 512 x 512 x 3) tunes no new shape -- the
    sweep below covers every shape the bench runs."""
    from posepaf import fused_model as fm
    saved = (fm._conv_choice, fm._conv_timing, fm._conv_calls)

    class Recording(dict):
        looked_up = set()

        def get(self, key, default=None):
            self.looked_up.add(key)
            return super().get(key, default)

    try:
        fm._conv_choice, fm._conv_timing, fm._conv_calls = Recording(), {}, {}
        fm.install_entries(json.load(open(cr.TABLE))["entries"])   # (the library hash it was tuned on does not matter here)
        before = set(fm._conv_choice)
        model = fm.build_inference_model("cuda")
        x = torch.rand((256, 512, 512, 3), generator=torch.Generator(device="cuda").manual_seed(1), device="cuda").half()
        with torch.no_grad():
            y = model(x)
        torch.cuda.synchronize()
        assert y.shape == (256, 50, 128, 128)
        new = set(fm._conv_choice) - before
        assert not new, (f"the bench geometry tuned {len(new)} shapes the committed table does not list: {sorted(map(str, new))}; "
                         "regenerate profiles/conv_choice_b128.json (bench.py at 128 images, fused_model.save_table)")
        # (keys not looked up here are the inner convolutions of fused forms: the tuner times them on the way, see forward_up2)
        print(f"{len(before - Recording.looked_up)} of {len(before)} table keys are not looked up with every choice installed")
    finally:
        fm._conv_choice, fm._conv_timing, fm._conv_calls = saved


@pytest.mark.parametrize("samples", [256, 2])
@pytest.mark.parametrize("entry", ENTRIES, ids=[cr.key_id(k) for k, _ in ENTRIES])
def test_every_tuner_candidate_at_the_bench_shapes_over_the_whole_batch(entry, samples):
    key, committed = entry
    spec = cr.parse_key(key, n=samples)
    label = f"{cr.key_id(key)} at n = {samples}"
    ops = cr.make_operands(spec, seed=zlib.crc32(label.encode()), device="cuda")
    pix = cr.sample_pixels(spec.n, spec.H, spec.W)
    ref, at32 = cr.reference32(spec, ops, pix)
    # the fp32 reference is proven against float64 before it judges a kernel
    a64 = cr.acc64_at(spec, ops, pix)
    cr.assert_close(at32.double(), a64, cr.TOL_FP32 * max(1.0, float(a64.abs().max())), label + ": fp32 reference", pix)
    o64 = cr.outputs64_at(spec, ops, pix)
    qpix = cr.sample_pixels(spec.n, spec.H // 2, spec.W // 2) if spec.pooled else None
    p64 = cr.pooled64_at(spec, ops, qpix) if spec.pooled else None
    scale = {name: float(v.abs().max()) for name, v in ref.items()}
    nb = cr.chunk_images(spec)

    ran, refused = [], []
    for cand, tol, launch, shapes in candidates(spec, ops):
        runs = []
        for rep in range(2):
            o = _outputs(spec, shapes)
            rc = launch({name: v.t if name != "mean" else v.t[:, :, 0, 0] for name, v in o.items()})
            torch.cuda.synchronize()
            if rc in REFUSED and rep == 0:
                break
            assert rc == 0, f"{label} candidate {cand}: rc {rc}"
            runs.append(o)
        if not runs:
            refused.append(cand)
            continue
        ran.append(cand)
        first, second = runs
        for name in shapes:
            what = f"{label} candidate {cand} output {name}"
            for o in (first[name], second[name]):
                hit = o.intact()
                assert hit is None, f"{what}: a store landed in {hit}"
            got, bound = _view(spec, name, first[name]), cr.bound_for(scale[name], tol)
            for i0 in range(0, spec.n, nb):
                cr.assert_close(got[i0:i0 + nb], ref[name][i0:i0 + nb], bound, what, img0=i0)
            if name in o64:
                cr.assert_close(cr.values_at(got, pix), o64[name], bound, what + " (float64 sample)", pix)
            elif name == "pool":
                cr.assert_close(cr.values_at(got, qpix), p64, bound, what + " (float64 sample)", qpix)
            assert torch.equal(got, _view(spec, name, second[name])), f"{what}: two runs differ (race?)"
        del runs, first, second
    print(f"{label}: {len(ran)} candidates ran {ran}, refused {refused}, committed {committed}")
    assert ran, f"{label}: no candidate ran"
    if spec.form == "plain" or committed != 0:     # 0 of a fused form = its separate path: plain keys of the table
        assert committed in ran, f"{label}: the committed choice {committed} did not run (ran {ran}, refused {refused})"
