"""The layer keys of the exact-operand sweep (helper module, not a test file; tests/test_gpu_conv_exact.py runs them,
tests/test_conv_exact_reference_cpu.py checks the selection and the expectations on the CPU).

The keys are recorded, not typed: they are selected from profiles/conv_keys_offbench.json among the rows with n <= 4.  Keys are
grouped by everything that sends a launch down another path --
  form, kernel size, dilation;  epilogue mode, activation;  scaled / pooled / pre-add / sliced;
  for 1x1 keys the input channel count (each is its own k_pw instance);
  the set of launcher cells conv_candidates.cells names over the form's candidate ids
-- and of each group the key with the fewest multiply-adds n H W k fan_in stays (ties: the smaller key id).
The stem is not in the key file (it is no tuner form): its two images are listed by hand."""
import zlib

import torch
import torch.nn.functional as F

import conv_reference as cr
from conv_candidates import cells

MAX_KEYS = 160                 # the selection's key count stays below this
MAX_KEY_MACS = 8.0e9           # one key: its float64 expectation is computed on the CPU in about a second
MAX_TOTAL_MACS = 1.0e11        # the whole selection
MAX_N = 4

# the candidate ids conv_candidates.candidates can hand out per form (posepaf/fused_model.py: OWN_VARIANTS, PW_VARIANT; the library
# templates of a plain key name no launcher cell)
CANDIDATE_IDS = {"plain": (101, 102, 103, 104, 105, 106), "up2": (1, 2, 3, 4, 5), "dual": (256, 128, 64, 512, 105), "mean": (1,),
                 "rmean": (1,), "pre": (1,), "pool": (1,), "cat": (1,)}


def macs(spec) -> int:
    return spec.n * spec.H * spec.W * spec.k * spec.fan_in


def group_of(spec) -> tuple:
    cs = set()
    for cand in CANDIDATE_IDS[spec.form]:
        cs |= cells(spec, cand)
    sliced = spec.form == "plain" and (spec.ldx != spec.c or spec.ldy != spec.k)
    return (spec.form, spec.r, spec.dil, spec.mode, spec.act, spec.scaled, spec.pooled, spec.pre_add, sliced,
            spec.c if spec.r == 1 else 0, tuple(sorted(cs)))


def select(entries=None) -> list:
    """[(key, Spec)] of the sweep, in key-id order"""
    best = {}
    for key, _ in entries if entries is not None else cr.table_entries(cr.OFFBENCH):
        spec = cr.parse_key(key)
        if spec.n > MAX_N:
            continue
        g, rank = group_of(spec), (macs(spec), cr.key_id(key))
        if g not in best or rank < best[g][0]:
            best[g] = (rank, key, spec)
    return sorted(((k, s) for _, k, s in best.values()), key=lambda ks: cr.key_id(ks[0]))


def seed_of(label: str, recipe: str) -> int:
    return zlib.crc32(f"{label}/{recipe}".encode())


def selected_cells(selection) -> set:
    out = set()
    for _, spec in selection:
        for cand in CANDIDATE_IDS[spec.form]:
            out |= cells(spec, cand)
    return out


# ---------------------------------------------------------------- the stem (pp_stem7x7_f16): 7x7, stride 2, padding 3, 3 -> 64, LeakyReLU
STEM_IMAGES = [(2, 64, 64), (1, 128, 192)]          # (n, h, w): one tile column / three, two workgroup rows and more
STEM_FAN_IN = 3 * 7 * 7


def stem_operands(shape, seed: int, recipe: str) -> dict:
    """x (n, h, w, 3) NHWC, w (64, 3, 7, 7), b (64,) in fp16 on the CPU.  The stem's contract has no inner rounding: its `rounding`
    recipe is x up to +-255 (an image's range), which puts most accumulators beyond 2048, where the one store rounding shows."""
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    unit = cr.SUBNORMAL_UNIT if recipe == "subnormal" else 1.0
    xmax = 255 if recipe == "rounding" else 3

    def ints(lo, hi, *shp):
        return torch.randint(lo, hi + 1, shp, generator=g).float()

    return {"x": (ints(-xmax, xmax, n, h, w, 3) * unit).half(), "w": ints(-2, 2, 64, 3, 7, 7).half(), "b": (ints(-8, 8, 64) * unit).half()}


STEM_SPEC = cr.Spec(("stem",), "plain", 0, 3, 0, 0, 64, 7, 3, 1, 0, True)      # mode 0, activation: all exact_epilogue reads


def stem_expected(ops: dict, recipe: str, label: str) -> torch.Tensor:
    """(n, 64, h / 2, w / 2) fp16, after the validity conditions of conv_reference.assert_exact_case that apply to the stem"""
    grid = cr.SUBNORMAL_UNIT if recipe == "subnormal" else 1.0
    x, w, b = ops["x"].double().permute(0, 3, 1, 2).contiguous(), ops["w"].double(), ops["b"].double()
    bound = float((F.conv2d(x.abs(), w.abs(), b.abs(), 2, 3)).max()) / grid
    assert bound < cr.EXACT_LIMIT, f"{label} [{recipe}]: sum |x w| + |b| reaches {bound:.4g} grid units"
    y = cr.exact_epilogue(STEM_SPEC, F.conv2d(x, w, b, 2, 3))["y"]
    assert bool(torch.isfinite(y.float()).all()), f"{label} [{recipe}]: the expected output is not finite"
    if recipe == "subnormal":
        assert float(ops["x"].abs().max()) < 2.0 ** -14 and float(y.float().abs().max()) < 2.0 ** -14
    if recipe == "rounding":
        assert float((y.float().abs() > 2048).float().mean()) > 0.01, f"{label}: hardly an accumulator beyond 2048"
    return y
