"""CPU: the run-time test configuration of the batched Python-rule paths -- packing / validation of cfg dicts, evaluate.py's
options, the INI reader, the C ABI's new symbols, and the order of NumPy's mean() for 1..128 samples that the general
kernels restate."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_merge_and_pack_defaults_and_moves():
    from posepaf import skeleton as sk
    assert sk.pack_test_cfg() == (0.1, 0.8, 16.0, 0.7, 20, 2, 0)
    assert sk.pack_test_cfg({}) == sk.pack_test_cfg(sk.default_test_cfg())      # a full reference `param` dict passes
    c = sk.merge_test_cfg({"thre2": 0.05, "mid_num": 40, "remove_recon": 1, "len_rate": 8, "offset_radius": np.int64(3)})
    assert (c["thre2"], c["mid_num"], c["remove_recon"], c["len_rate"], c["offset_radius"]) == (0.05, 40, 1, 8.0, 3)
    assert isinstance(c["len_rate"], float) and isinstance(c["offset_radius"], int)
    assert c["connect_ration"] == 0.8 and c["thre1"] == 0.1                      # untouched keys keep the INI values
    assert sk.pack_test_cfg(c) == (0.05, 0.8, 8.0, 0.7, 40, 3, 1)
    assert sk.default_test_cfg()["mid_num"] == 20                                # merge never edits the defaults


@pytest.mark.parametrize("bad", [{"mid_num": 0}, {"mid_num": 129}, {"mid_num": 20.5}, {"offset_radius": -1}, {"offset_radius": 8},
                                 {"remove_recon": 2}, {"remove_recon": -1}, {"thre2": float("nan")}, {"thre2": -0.1},
                                 {"connect_ration": float("inf")}, {"len_rate": -1.0}, {"connection_tole": "0.7"},
                                 {"thre2": True}, {"crop_ratio": 3.0}, {"scale_search": [1.0]}, {"no_such_key": 1}])
def test_merge_refuses(bad):
    from posepaf import skeleton as sk
    with pytest.raises(ValueError):
        sk.merge_test_cfg(bad)


def test_mid_num_and_radius_limits_accepted():
    from posepaf import skeleton as sk
    for m in (1, 7, 8, 128):
        assert sk.merge_test_cfg({"mid_num": m})["mid_num"] == m
    for r in (0, 7):
        assert sk.merge_test_cfg({"offset_radius": r})["offset_radius"] == r


def test_ctypes_struct_matches_header():
    """posepaf._lib.TestCfg against sizeof / offsetof of pp_test_cfg compiled from include/posepaf.h"""
    import subprocess
    import tempfile
    from posepaf import _lib
    fields = [n for n, _ in _lib.TestCfg._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "posepaf.h"\nint main(){printf("%zu", sizeof(pp_test_cfg));' + \
          "".join(f'printf(" %zu", offsetof(pp_test_cfg, {n}));' for n in fields) + \
          'printf(" %u\\n", PP_ST_RECON_UNDEFINED);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")],
                       check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.TestCfg)
    assert out[1:-1] == [getattr(_lib.TestCfg, n).offset for n in fields]
    assert out[-1] == _lib.ST_RECON_UNDEFINED == 128
    assert _lib.ST_DEFINED_MASK & _lib.ST_RECON_UNDEFINED


def test_new_symbols_declared_exported_and_default_values():
    from posepaf import _lib
    hdr = open(os.path.join(ROOT, "include", "posepaf.h")).read()
    declared = re.findall(r"^PP_API\s+[\w\s\*]+?\b(\w+)\(", hdr, flags=re.M)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pp_set_test_cfg", "pp_get_test_cfg", "pp_default_test_cfg"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    assert "typedef struct" in hdr and "} pp_test_cfg;" in hdr
    L = _lib.load()
    c = _lib.TestCfg()
    assert L.pp_default_test_cfg(ctypes.byref(c)) == 0           # host-only call: no device needed
    from posepaf import skeleton as sk
    assert (c.thre2, c.connect_ration, c.len_rate, c.connection_tole, c.mid_num, c.offset_radius, c.remove_recon) == \
        sk.pack_test_cfg()
    assert L.pp_default_test_cfg(None) == -2                      # PP_ERR_BAD_ARG
    assert L.pp_set_test_cfg(None, ctypes.byref(c)) == -2 and L.pp_get_test_cfg(None, ctypes.byref(c)) == -2


def test_evaluate_parse_test_cfg_and_config_file(tmp_path):
    import evaluate
    a = evaluate.parse(["--synthetic", "4"])
    assert a.test_cfg_dict is None
    a = evaluate.parse(["--synthetic", "4", "--test_cfg", "thre2=0.05", "mid_num=40", "remove_recon=1", "thre1=0.2"])
    assert (a.test_cfg_dict["thre2"], a.test_cfg_dict["mid_num"], a.test_cfg_dict["remove_recon"], a.test_cfg_dict["thre1"]) == \
        (0.05, 40, 1, 0.2)
    assert a.test_cfg_dict["connect_ration"] == 0.8
    ini = tmp_path / "config"
    ini.write_text("[param]\n# CPU mode or GPU mode\nuse_gpu = 1\nscale_search =    0.5, 1, 1.5\nthre1 = 0.12  # keypoint threshold\n"
                   "thre2 = 0.05 # limb threshold\n\nconnect_ration = 0.7 # comment\nmid_num = 30  # samples\nlen_rate = 12\n"
                   "connection_tole = 0.6\ncrop_ratio = 2.5\noffset_radius = 3  #7\nremove_recon = 1  # 0 or 1\n\n[models]\n"
                   "[[1]]\nmid_num = 99\nboxsize = 512\n[other]\nthre2 = 0.9\n", encoding="utf-8")
    from posepaf import skeleton as sk
    got = sk.read_config_file(str(ini))
    assert got == {"thre1": 0.12, "thre2": 0.05, "connect_ration": 0.7, "mid_num": 30, "len_rate": 12.0, "connection_tole": 0.6,
                   "offset_radius": 3, "remove_recon": 1}
    a = evaluate.parse(["--synthetic", "4", "--config_file", str(ini), "--test_cfg", "mid_num=64"])
    assert a.test_cfg_dict["mid_num"] == 64 and a.test_cfg_dict["thre2"] == 0.05 and a.test_cfg_dict["offset_radius"] == 3
    for bad in (["--test_cfg", "mid_num=200"], ["--test_cfg", "mid_num"], ["--test_cfg", "scale_search=1"],
                ["--test_cfg", "mid_num=4.5"], ["--test_cfg", "thre2=abc"], ["--config_file", str(tmp_path / "missing")]):
        with pytest.raises(SystemExit):
            evaluate.parse(["--synthetic", "4"] + bad)
    bad_ini = tmp_path / "bad"
    bad_ini.write_text("[param]\nmid_num = many\n")
    with pytest.raises(ValueError):
        sk.read_config_file(str(bad_ini))


def test_evaluate_refuses_test_cfg_with_cpp_rules_and_refactored_path():
    """like --rotation_search: refused before anything touches the GPU"""
    import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--run_refactor", "--run_cpp", "--synthetic", "4", "--test_cfg", "thre2=0.05"])
    assert "run_cpp" in str(e.value) and "compiled in" in str(e.value)
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--run_refactor", "--synthetic", "4", "--test_cfg", "thre2=0.05"])
    assert "original path only" in str(e.value)


def mean_in_kernel_order(x):
    """The order the general kernels form limb_response.mean() in, in the array's dtype: n < 8: plain loop from 0; otherwise
    eight running sums over the full blocks of 8, the tree add, then the tail one by one; then / n."""
    t, n = x.dtype.type, len(x)
    if n < 8:
        s = t(0)
        for v in x:
            s = t(s + v)
    else:
        r = [x[k] for k in range(8)]
        full = n - (n % 8)
        for i in range(8, full, 8):
            for k in range(8):
                r[k] = t(r[k] + x[i + k])
        s = t(t(t(r[0] + r[1]) + t(r[2] + r[3])) + t(t(r[4] + r[5]) + t(r[6] + r[7])))
        for i in range(full, n):
            s = t(s + x[i])
    return t(s / t(n))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mean_order_matches_numpy_for_every_n_up_to_128(dtype):
    rng = np.random.default_rng(5)
    for n in range(1, 129):
        for rep in range(6):
            x = (rng.random(n) * (10.0 ** rng.integers(-3, 3, n)) - 0.3).astype(dtype)
            got, want = mean_in_kernel_order(x), x.mean()
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (dtype.__name__, n, rep)
    # what the gather score_mid[ys, xs] returns is contiguous, like x above; beyond 128 NumPy recurses and this order stops
    # holding -- the reason for the cap
    x = (rng.random(129 * 50) - 0.3).astype(np.float32).reshape(50, 129)
    assert any(mean_in_kernel_order(row).tobytes() != row.mean().tobytes() for row in x)
