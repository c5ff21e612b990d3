"""MI355X-only: the published IMHN variant (models/posenet_final.py) on the fused path -- the two kernels that came with it
(pp_pw_pre_f16, pp_conv_own_res_sums_f16), FusedIMHNFinal against the fp32 module, its switches, and evaluate.py --arch final."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu

vp = C.c_void_p


def _cl(t):
    return t.cuda().half().contiguous(memory_format=torch.channels_last)


def _st():
    return vp(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ pp_pw_pre_f16
def test_streaming_kernel_takes_768_input_channels():
    from posepaf import _lib
    L = _lib.load()
    assert L.pp_pw_supported(768, 256) == 1
    assert L.pp_pw_supported(768, 64) == 1 and L.pp_pw_supported(800, 256) == 0


def test_plain_stream_at_768_input_channels_matches_torch():
    """pp_pw_f16 at the width pp_pw_supported gained, 768 -> 256 without a tensor added (k_pw<24, 1, 0>): against fp32 torch on the
    same fp16 operands, with and without the SE gains, bound 2e-3 of the output scale as for the other widths; the forms that add
    tensors have no 768-channel instance and are refused."""
    import torch.nn.functional as F
    from posepaf import _lib
    L = _lib.load()
    n, h, w, ci, co = 2, 8, 8, 768, 256
    g = torch.Generator(device="cpu").manual_seed(47)
    x = _cl(torch.randn(n, ci, h, w, generator=g))
    wt = _cl(torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5)
    b = torch.randn(co, generator=g).cuda().half()
    sc = (0.2 + torch.rand(n, ci, generator=g)).cuda().half()
    ex = _cl(torch.randn(n, co, h, w, generator=g))
    for use_scale in (False, True):
        xin = x * sc[:, :, None, None] if use_scale else x
        ref = F.leaky_relu(F.conv2d(xin.float(), wt.float(), b.float()), 0.01)
        y = torch.full((n, co, h, w), float("nan"), dtype=torch.float16, device="cuda").contiguous(memory_format=torch.channels_last)
        rc = L.pp_pw_f16(vp(x.data_ptr()), vp(sc.data_ptr()) if use_scale else None, vp(wt.data_ptr()), vp(b.data_ptr()), None, None,
                         vp(y.data_ptr()), None, n * h * w, h * w, ci, co, co, 0, 0.01, _st())
        assert rc == 0, rc
        torch.cuda.synchronize()
        err = (y.float() - ref).abs().max().item()
        assert torch.isfinite(y).all() and err <= 2e-3 * max(1.0, ref.abs().max().item()), (use_scale, err)
    assert L.pp_pw_f16(vp(x.data_ptr()), None, vp(wt.data_ptr()), vp(b.data_ptr()), vp(ex.data_ptr()), None, vp(y.data_ptr()), None,
                       n * h * w, h * w, ci, co, co, 1, 0.01, _st()) == -6


@pytest.mark.parametrize("shape", [
    # n, h, w, c_in, c_out, pre_add
    (2, 8, 8, 768, 256, True), (2, 8, 8, 768, 256, False),      # C_out split over four workgroup columns (96 KB of weights each)
    (2, 8, 8, 640, 256, True), (2, 8, 8, 640, 256, False),      # 16-pixel groups
    (2, 8, 8, 384, 256, True), (2, 8, 8, 384, 256, False),      # 32-pixel groups; hw = 64 is the smallest legal image
    (2, 16, 16, 768, 256, True),                                # 32 groups for 8 waves: a wave walks more than one
])
def test_pre_form_of_the_streaming_convolution_matches_torch(shape):
    """pp_pw_pre_f16: y = act(W (x * scale[n] + pre_add) + b) against fp32 torch on the same fp16 operands, with the two binary16
    roundings restated (the product, then the sum -- the tensors the separate channel_scale pass and the tensor add would have
    written).  Bound: this kernel family's, 2e-3 of the output scale (test_streaming_pointwise_convolution_matches_torch).  A second
    call on the same operands is bit-identical."""
    import torch.nn.functional as F
    from posepaf import _lib
    L = _lib.load()
    n, h, w, ci, co, with_add = shape
    g = torch.Generator(device="cpu").manual_seed(43)
    x = _cl(torch.randn(n, ci, h, w, generator=g))
    wt = _cl(torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5)
    b = torch.randn(co, generator=g).cuda().half()
    sc = (0.2 + torch.rand(n, ci, generator=g)).cuda().half()
    add = _cl(torch.randn(n, ci, h, w, generator=g))
    xin = x * sc[:, :, None, None]                       # binary16 product
    if with_add:
        xin = xin + add                                  # binary16 sum of the rounded product and the cache
    ref = F.leaky_relu(F.conv2d(xin.float(), wt.float(), b.float()), 0.01)
    ys = []
    for _ in range(2):
        y = torch.full((n, co, h, w), float("nan"), dtype=torch.float16, device="cuda").contiguous(memory_format=torch.channels_last)
        rc = L.pp_pw_pre_f16(vp(x.data_ptr()), vp(sc.data_ptr()), vp(add.data_ptr()) if with_add else None, vp(wt.data_ptr()),
                             vp(b.data_ptr()), vp(y.data_ptr()), n * h * w, h * w, ci, co, co, 0.01, _st())
        assert rc == 0, (shape, rc)
        torch.cuda.synchronize()
        ys.append(y)
    assert torch.isfinite(ys[0]).all()
    err = (ys[0].float() - ref).abs().max().item()
    print("pp_pw_pre_f16", shape, "max error", err, "output scale", ref.abs().max().item())
    assert err <= 2e-3 * max(1.0, ref.abs().max().item()), (shape, err)
    assert torch.equal(ys[0], ys[1])
    # refusals: no gains, an image size a group could straddle, an input width without an instance
    args = lambda sc_, hw_, ci_: (vp(x.data_ptr()), sc_, None, vp(wt.data_ptr()), vp(b.data_ptr()), vp(ys[1].data_ptr()), n * h * w, hw_, ci_,
                                  co, co, 0.01, _st())
    assert L.pp_pw_pre_f16(*args(None, h * w, ci)) == -2
    assert L.pp_pw_pre_f16(*args(vp(sc.data_ptr()), 32, ci)) == -6
    assert L.pp_pw_pre_f16(*args(vp(sc.data_ptr()), h * w, 448)) == -6
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1])                     # a refused call writes nothing


# ------------------------------------------------------------------------------------------------ pp_conv_own_res_sums_f16
@pytest.mark.parametrize("shape", [(2, 128, 128, 16, 16),      # whole images in one tile (two 16 x 16 images stacked)
                                   (2, 128, 256, 32, 64)])     # two tiles per row (64-wide tiles of 8 rows)
def test_halo_kernel_emits_the_channel_sums_of_its_residual_mode_output(shape):
    """pp_conv_own_res_sums_f16: y byte for byte pp_conv_own_f16's with the same residual (extra_mode 1), and the SE gains computed
    from its partial sums equal to the gains from channel_mean(y) (pp_se_gains_f16, both inputs) -- within the bound of
    test_halo_kernel_emits_the_channel_sums_of_its_output, 1e-3 of the scale (gains lie in (0, 1): scale 1)."""
    from posepaf import _lib, fused_model as fm
    L = _lib.load()
    n, ci, co, h, w = shape
    g = torch.Generator(device="cpu").manual_seed(59)
    x = _cl(torch.randn(n, ci, h, w, generator=g))
    wt = _cl(torch.randn(co, ci, 3, 3, generator=g) / (ci * 9) ** 0.5)
    b = torch.randn(co, generator=g).cuda().half()
    res = _cl(torch.randn(n, co, h, w, generator=g))
    splits = L.pp_conv_own_res_sums_splits(h, w)
    assert splits == h * w // 128
    y0 = torch.empty((n, co, h, w), dtype=torch.float16, device="cuda").contiguous(memory_format=torch.channels_last)
    assert L.pp_conv_own_f16(vp(x.data_ptr()), vp(wt.data_ptr()), vp(b.data_ptr()), vp(res.data_ptr()), vp(y0.data_ptr()), n, h, w, ci, co,
                             3, 1, 1, 1, 0.01, 512, _st()) == 0
    y1 = torch.full_like(y0, float("nan"), memory_format=torch.channels_last)
    ws = torch.full((n, splits, co), float("nan"), dtype=torch.float32, device="cuda")
    assert L.pp_conv_own_res_sums_f16(vp(x.data_ptr()), vp(wt.data_ptr()), vp(b.data_ptr()), vp(res.data_ptr()), vp(y1.data_ptr()),
                                      vp(ws.data_ptr()), n, h, w, ci, co, 0.01, _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and torch.isfinite(ws).all()
    want_sums = y1.float().sum(dim=(2, 3))
    assert (ws.sum(dim=1) - want_sums).abs().max().item() <= 1e-3 * max(1.0, want_sums.abs().max().item())
    hid = co // 16
    fc1 = torch.nn.Linear(co, hid)
    fc2 = torch.nn.Linear(hid, co)
    with torch.no_grad():
        fc1.weight.copy_(torch.randn(hid, co, generator=g) / co ** 0.5)
        fc2.weight.copy_(torch.randn(co, hid, generator=g) / hid ** 0.5)
    fc1, fc2 = fc1.cuda().half(), fc2.cuda().half()
    mean = fm.channel_mean(y1).contiguous()
    gains = []
    for pws, pmean, hw_, sp in ((vp(ws.data_ptr()), None, h * w, splits), (None, vp(mean.data_ptr()), 0, 0)):
        out = torch.empty((n, co), dtype=torch.float16, device="cuda")
        assert L.pp_se_gains_f16(pws, pmean, vp(fc1.weight.data_ptr()), vp(fc1.bias.data_ptr()), vp(fc2.weight.data_ptr()),
                                 vp(fc2.bias.data_ptr()), vp(out.data_ptr()), n, hw_, co, hid, sp, 0.01, _st()) == 0
        gains.append(out.float())
    torch.cuda.synchronize()
    assert (gains[0] - gains[1]).abs().max().item() <= 1e-3
    assert gains[1].max().item() - gains[1].min().item() > 0.05   # the gains are not degenerate
    if h == 16:   # stacked images: an odd batch has no whole tile -- refused, the caller's separate form runs
        assert L.pp_conv_own_res_sums_f16(vp(x.data_ptr()), vp(wt.data_ptr()), vp(b.data_ptr()), vp(res.data_ptr()), vp(y1.data_ptr()),
                                          vp(ws.data_ptr()), 1, h, w, ci, co, 0.01, _st()) == -6


# ------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def net32():
    """the fp32 final module (4 stages, deterministic init, seed 7) on the host: the tests move copies of it"""
    from posepaf.model_init import build_network
    return build_network("final")[0]


@pytest.fixture(scope="module")
def fused(net32):
    import copy
    from posepaf.fused_model import FusedIMHN, FusedIMHNFinal
    # (a copy: the fused model holds the SE blocks' own Linear modules and converts them with itself)
    m = FusedIMHN.from_network(copy.deepcopy(net32)).eval().cuda().half().to(memory_format=torch.channels_last)
    assert isinstance(m, FusedIMHNFinal)
    return m


@pytest.fixture(scope="module")
def module_outputs(net32):
    """per input size: (x fp32 on the GPU, [fp32 module's scale-0 prediction per stage], [plain fp16 channels-last module's]) --
    computed once"""
    import copy
    out = {}
    with torch.no_grad():
        xs = {size: torch.from_numpy(np.random.default_rng(5).random((2, size, size, 3), dtype=np.float32)).cuda() for size in (128, 256)}
        m32 = copy.deepcopy(net32).cuda()
        ref = {size: [st[0].float() for st in m32(x)] for size, x in xs.items()}
        m16 = m32.half().to(memory_format=torch.channels_last)
        for size, x in xs.items():
            out[size] = (x, ref[size], [st[0].float() for st in m16(x.half())])
    del m32, m16
    torch.cuda.empty_cache()
    return out


@pytest.mark.parametrize("size", [128, 256])
def test_fused_fp16_final_model_against_the_fp32_module(fused, module_outputs, size):
    """Every stage's scale-0 prediction of FusedIMHNFinal (fp16) against the fp32 final module, deterministic_init(seed=7).  The
    bound is not a number fixed in advance: the plain fp16 channels-last nn.Module on PyTorch-ROCm evaluates the same real function
    in the same precision on the same input, the fused model's rewrites only re-associate sums -- so its max and rms error,
    relative to the stage's scale, must be <= 2x the plain fp16 module's."""
    x, ref, plain = module_outputs[size]
    with torch.no_grad():
        fused(x.half())                                  # tunes the shapes of this geometry
        got = [g.float() for g in fused(x.half(), stage_preds=True)]
        last = fused(x.half()).float()
    assert len(got) == len(ref) == 4 and torch.equal(last, got[-1])
    report = []
    for t in range(4):
        assert got[t].shape == ref[t].shape == (2, 50, size // 4, size // 4) and torch.isfinite(got[t]).all()
        scale = ref[t].abs().max().item()
        err = lambda a: ((a - ref[t]).abs().max().item() / scale, (a - ref[t]).pow(2).mean().sqrt().item() / scale)
        report.append((t, err(got[t]), err(plain[t])))
    print(f"final model {size} x {size}: stage, fused (max, rms), plain fp16 module (max, rms), relative to the stage's scale:", report)
    for t, (f_max, f_rms), (p_max, p_rms) in report:
        assert f_max <= 2 * p_max and f_rms <= 2 * p_rms, report


def _people(post, out, scenes):
    """records of the scenes with the network's own ripple added (scaled by the caller)"""
    return [post.process((scene + out.view(2, 50, 64, 64)).half().contiguous()[None], 256)[0] for scene in scenes]


def _same_people(a, b):
    assert a["status"] == 0 and b["status"] == 0
    n = int(a["n_humans"])
    assert n == int(b["n_humans"]) and n >= 3
    ha, hb = a["humans"][:n], b["humans"][:n]
    assert np.array_equal(ha["peak_id"] >= 0, hb["peak_id"] >= 0)
    m = ha["peak_id"] >= 0
    assert (np.abs(ha["x"][m] - hb["x"][m]) <= 4).all() and (np.abs(ha["y"][m] - hb["y"][m]) <= 4).all()
    return n


SWITCHES = ["USE_PW", "USE_FUSED_CONV", "USE_OWN_CONV", "USE_SUM_FUSION", "USE_COLLAPSED_UP2", "USE_CAT_SKIP", "USE_SE_KERNEL",
            "USE_POOL_FUSION", "USE_RES_SUM_FUSION", "USE_PRE_FUSION", "USE_FOLDED_MERGE"]


def test_every_switch_off_finds_the_same_people_as_on(fused, net32):
    """One synthetic scene set through the fused final model with each switch of posepaf/fused_model.py off, against all on: the
    network's output scaled to an amplitude of 0.05 (below the peak threshold) and added to the same clean scenes, then the full
    HIP post-processing, as test_fp16_fused_forward_and_fp32_module_find_the_same_people does: equal counts, equal part sets, joint
    coordinates within one feature-map cell (4 px).  USE_FOLDED_MERGE acts at load time: a second fused model is built for it."""
    from posepaf import fused_model as fm, synth
    from posepaf.api import PosePostProcessor
    from posepaf.pipeline import preprocess_batch
    img = torch.from_numpy(np.random.default_rng(21).integers(0, 256, (1, 256, 256, 3), dtype=np.uint8)).cuda()
    x = preprocess_batch(img, True, torch.float16)
    scenes = [torch.from_numpy(synth.make_net_output(5, 800 + seed, h=64, w=64, noise=0.0, dtype=np.float32)).cuda() for seed in (1, 2)]
    post = PosePostProcessor(max_batch=1, max_h=64, max_w=64, max_peaks_per_part=64)
    try:
        with torch.no_grad():
            on = fused(x).float()
            k = 0.05 / on.abs().max().item()
            want = _people(post, on * k, scenes)
            for name in SWITCHES:
                assert getattr(fm, name) is True, name
                setattr(fm, name, False)
                try:
                    model = fused
                    if name == "USE_FOLDED_MERGE":
                        import copy
                        model = fm.FusedIMHN.from_network(copy.deepcopy(net32)).eval().cuda().half().to(memory_format=torch.channels_last)
                        assert not model.folded_merge
                    off = model(x).float()
                finally:
                    setattr(fm, name, True)
                assert torch.isfinite(off).all(), name
                print(name, "off: max difference / amplitude", ((off - on).abs().max() / on.abs().max()).item())
                people = sum(_same_people(a, b) for a, b in zip(want, _people(post, off * k, scenes)))
                assert people >= 6, name
    finally:
        post.close()


def test_new_forms_join_the_choice_table(fused):
    """after the tuning passes above the table holds the final variant's keys: the residual-mode sums (rmean), the compress
    convolution's input form (pre) and hg[i][3] without a tensor added behind it (up2 ... nopost), each with a choice from its
    candidate list"""
    from posepaf import fused_model as fm
    x = torch.from_numpy(np.random.default_rng(5).random((2, 256, 256, 3), dtype=np.float32)).cuda().half()
    with torch.no_grad():
        fused(x)
    table = fm.conv_choices()
    rmean = {k: v for k, v in table.items() if k[0] == "rmean"}
    pre = {k: v for k, v in table.items() if k[0] == "pre"}
    nopost = {k: v for k, v in table.items() if k[0] == "up2" and k[-1] == "nopost"}
    assert rmean and pre and nopost
    assert all(v in (0, 1) for v in rmean.values()) and all(v in (0, 1) for v in pre.values())
    assert {k[2] for k in pre} >= {256, 384, 512, 640}          # scales 0..3 at 256 x 256 (scale 4 is a 4 x 4 map: hw % 64 != 0)
    assert all(0 <= v <= 5 for v in nopost.values())
    assert not any(k[0] in ("rmean", "pre") and k[1] != 2 for k in table)


def test_evaluate_script_runs_the_final_variant(tmp_path):
    """evaluate.py --arch final --run_refactor --run_cpp as a child process: exit 0, status_or 0; a second run on the kernel-choice
    table the first one saved gives the identical dump."""
    cache = tmp_path / "cache"
    cache.mkdir()
    dumps = []
    for name in ("first", "second"):
        dump = tmp_path / f"{name}.json"
        env = dict(os.environ, POSEPAF_CACHE_DIR=str(cache))
        r = subprocess.run([sys.executable, os.path.join(PKG, "evaluate.py"), "--arch", "final", "--run_refactor", "--run_cpp",
                            "--synthetic", "4", "--batch", "2", "--sizes", "256x256", "--dump_name", str(dump)],
                           capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        summary = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert summary["images"] == 4 and summary["status_or"] == 0
        dumps.append(json.load(open(dump)))
    assert len(dumps[0]) > 0 and dumps[0] == dumps[1]


def test_demo_and_speed_scripts_take_the_final_variant(tmp_path):
    """demo_image.py --arch final draws the injected people (exit 0, a canvas is written); inference_speed.py --arch final runs the
    forward-only loop and its JSON line names the architecture and the class that ran."""
    out = tmp_path / "canvas.npy"
    r = subprocess.run([sys.executable, os.path.join(PKG, "demo_image.py"), "--arch", "final", "--run_refactor", "--run_cpp",
                        "--synthetic", "3", "--output", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    import re
    found = int(re.search(r"(\d+) people", r.stdout).group(1))
    assert 2 <= found <= 4 and np.load(out).shape == (512, 512, 3), r.stdout      # three injected; random weights add only ripple
    r = subprocess.run([sys.executable, os.path.join(PKG, "inference_speed.py"), "--arch", "final", "--batch", "2", "--size", "128", "128",
                        "--iters", "3", "--json"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert sum(ln.startswith("==================>Test: [") and "Speed" in ln for ln in lines) == 3
    line = json.loads(lines[-1])
    assert line["arch"] == "final" and line["model"] == "FusedIMHNFinal" and line["value"] > 0 and line["batch"] == 2
