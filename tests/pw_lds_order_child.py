"""Child process of tests/test_gpu_conv_exact.py (a plain script, not a test file): the streaming 1x1 kernel pp_pw_f16 at 256 input
channels, m = 2 * 8 * 8 pixels, called at two output widths in the order given -- 64 channels (32 KiB of weights in LDS) and 256
(128 KiB), both through the SAME k_pw instance, whose dynamic-LDS limit the launcher raises once, at the first call.  Each output
is compared with conv_reference.expected_exact under the `small` recipe as bit patterns.

usage: pw_lds_order_child.py small-first|large-first [mode]      (mode 0: EX = 0; mode 1: EX = 1, a residual before the activation)
prints one JSON line: {"order": ..., "mode": ..., "c_out": [..], "rc": [..], "equal": [..], "intact": [..]}"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "improved-body-parts_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import conv_reference as cr  # noqa: E402
from conv_candidates import Out, _p  # noqa: E402


def main(order: str, mode: int) -> dict:
    from posepaf import _lib, fused_model as fm
    L = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    widths = {"small-first": [64, 256], "large-first": [256, 64]}[order]
    res = {"order": order, "mode": mode, "c_out": widths, "rc": [], "equal": [], "intact": []}
    for k in widths:
        spec = cr.parse_key((2, 256, 8, 8, k, 1, 0, 1, mode, True))
        ops = cr.make_exact_operands(spec, 1000 + k + mode, "small", device="cuda")
        want = cr.expected_exact(spec, ops)
        cr.assert_exact_case(spec, ops, "small", want, f"pw {k}")
        o = Out(spec.n, k, spec.H, spec.W)
        rc = L.pp_pw_f16(_p(ops["x"]), None, _p(ops["w"]), _p(ops["b"]), _p(ops.get("e1")), None, _p(o.t), None, spec.n * spec.H * spec.W,
                         spec.H * spec.W, spec.c, k, k, mode, fm.LEAK, st)
        torch.cuda.synchronize()
        res["rc"].append(int(rc))
        res["equal"].append(rc == 0 and cr.first_bit_difference(o.t, want["y"], "y") is None)
        res["intact"].append(o.intact() is None)
    return res


if __name__ == "__main__":
    print(json.dumps(main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 0)))
