"""The cases of tests/test_gpu_head_wgrad_paths.py: operands for pp_head_wgrad_f16 (include/posepaf.h) whose float32 result is exact
in ANY order of the additions, a classifier that says which code of csrc/posepaf_headgrad.hip a case reaches, and the list itself.
Pure NumPy; nothing here imports the package.  tests/test_head_wgrad_cases_cpu.py proves, without a GPU, that every case is what
it claims (exact, and in its class) and that the `wide` recipe makes every output element depend on every term of the kernel's
bfloat16 split.

The kernel as restated here (its opening comment and the header): chunks of P pixels; min(G, chunks) workgroups, workgroup b takes
chunks b, b + grid, ...; g is loaded in 16-byte groups of 8 channels where its rows are 16-byte aligned and element by element
elsewhere; the 16-byte groups of an x row are dealt to 256 threads in order, so a thread's groups sit at one channel offset iff
256 % (c_in / 8) == 0; a second launch adds the workgroups' partials in four interleaved runs."""
import functools
from dataclasses import dataclass, field

import numpy as np

import head_wgrad_reference as ref

P_DEFAULT, G_DEFAULT = 64, 256      # pp_head_wgrad_chunk_pixels(), pp_head_wgrad_max_workgroups(): the GPU file asserts both
KP = 64                             # output channels of the kernel's tile
THREADS = 256
WIDE_MAX_M = 8192                   # db of `wide` is exact while m * 2047 < 2^24
WIDE_R = 2                          # non-zero pixels per input channel


# ---------------------------------------------------------------------------------------------------------------- operand recipes

def _g_buffer(m, ldg):
    return np.full((m, ldg), np.nan, np.float16)


def small(rng, m, c_in, c_out, ldg, n_img=None, g_max=3, x_max=15, gains=(0.5, 1.0, 1.5, 3.0)):
    """integers |g| <= g_max, |x| <= x_max, gains in {0.5, 1, 1.5, 3}: the recipe of tests/test_gpu_head_wgrad.py"""
    g = _g_buffer(m, ldg)
    g[:, :c_out] = rng.integers(-g_max, g_max + 1, (m, c_out)).astype(np.float16)
    x = rng.integers(-x_max, x_max + 1, (m, c_in)).astype(np.float16)
    scale = None if n_img is None else rng.choice(np.asarray(gains, np.float16), (n_img, c_in))
    return g, x, scale


def _odd11(rng, shape):
    """odd integers in [1025, 2047] with a random sign: all 11 significand bits of a binary16 value, the lowest one set"""
    return (1025 + 2 * rng.integers(0, 512, shape)) * rng.choice((-1, 1), shape)


def wide(rng, m, c_in, c_out, ldg, n_img=None):
    """every non-zero value is an odd 11-bit integer (times a gain in {1, -1, 0.5}), so each has a non-zero low part in the
    bfloat16 split and each product needs all 22 bits; x has WIDE_R non-zero pixels per channel, so an element of dw is the sum of
    at most two products below 2^22 units and every partial sum is exact"""
    assert m <= WIDE_MAX_M
    g = _g_buffer(m, ldg)
    g[:, :c_out] = _odd11(rng, (m, c_out)).astype(np.float16)
    x = np.zeros((m, c_in), np.float16)
    ch = np.arange(c_in)
    first = rng.integers(0, m, c_in)
    x[first, ch] = _odd11(rng, c_in).astype(np.float16)
    if m >= WIDE_R:
        second = (first + rng.integers(1, m, c_in)) % m
        x[second, ch] = _odd11(rng, c_in).astype(np.float16)
    scale = None if n_img is None else rng.choice(np.asarray((1.0, -1.0, 0.5), np.float16), (n_img, c_in))
    return g, x, scale


def reals(rng, m, c_in, c_out, ldg, n_img=None):
    """real-valued operands (make_reals of tests/test_gpu_head_wgrad.py): judged by the rounding bound, never bit for bit"""
    g = _g_buffer(m, ldg)
    g[:, :c_out] = (rng.standard_normal((m, c_out)) * 2.0 ** -3).astype(np.float16)
    x = rng.standard_normal((m, c_in)).astype(np.float16)
    scale = None if n_img is None else rng.uniform(0.5, 1.5, (n_img, c_in)).astype(np.float16)
    return g, x, scale


RECIPES = {"small": small, "wide": wide, "reals": reals}


# ---------------------------------------------------------------------------------------------------------------- the classifier

def paths(m, hw, c_in, c_out, ldg, g_byte_offset, scaled, P=P_DEFAULT, G=G_DEFAULT):
    """which code of the kernel a call reaches, from its arguments alone"""
    assert c_in % 64 == 0 and 64 <= c_in <= 256 and 1 <= c_out <= KP and ldg >= c_out and g_byte_offset % 2 == 0
    assert not scaled or (hw % 64 == 0 and m % hw == 0)
    vpp = c_in // 8
    n_chunks = -(-m // P)
    grid = min(G, n_chunks)
    if c_out == KP:
        straddle = "none"                   # every 16-byte group of the tile is real
    elif c_out % 8 == 0:
        straddle = "behind"                 # no group is cut, some lie wholly at or behind c_out and are not loaded
    else:
        straddle = "odd" if c_out % 2 else "even"     # odd: c_out cuts a 32-bit pair of the straddling group in half
    changes = False
    if scaled:
        for b in range(grid):
            img = [(c * P) // hw for c in range(b, n_chunks, grid)]
            changes = changes or any(i != j for i, j in zip(img, img[1:]))
    return dict(load="vector" if g_byte_offset % 16 == 0 and ldg % 8 == 0 else "element",
                same_offset=THREADS % vpp == 0,
                straddle=straddle,
                groups_behind=(KP - 8 * -(-c_out // 8)) // 8,
                row_padding=ldg - c_out,    # > 0: the element path's `c < c_out` guard differs from `c < ldg`
                second_row_tile_empty=c_out <= 32,
                n_chunks=n_chunks, grid=grid, max_passes=-(-n_chunks // grid),
                ragged_tail=m % P != 0,
                gain_row_changes=changes,
                finish_runs=min(4, grid))


# ---------------------------------------------------------------------------------------------------------------- cases

@dataclass(frozen=True)
class Case:
    group: str              # A, B or C of the list below
    recipe: str
    m: int
    hw: int
    c_in: int
    c_out: int
    ldg: int
    g_byte_offset: int
    scaled: bool
    seed: int
    kw: tuple = field(default=())        # extra arguments of the recipe, as sorted (name, value) pairs

    @property
    def n_img(self):
        return self.m // self.hw if self.scaled else None

    @property
    def name(self):
        extra = "".join(f"-{k}{v}" for k, v in self.kw)
        return (f"{self.group}-{self.recipe}-cin{self.c_in}-cout{self.c_out}-ldg{self.ldg}-off{self.g_byte_offset}-"
                f"{'gains' if self.scaled else 'plain'}-m{self.m}-hw{self.hw}{extra}")

    def paths(self, P=P_DEFAULT, G=G_DEFAULT):
        return paths(self.m, self.hw, self.c_in, self.c_out, self.ldg, self.g_byte_offset, self.scaled, P, G)

    def operands(self):
        return _operands(self)


@functools.lru_cache(maxsize=None)
def _operands(case):
    out = RECIPES[case.recipe](np.random.default_rng(case.seed), case.m, case.c_in, case.c_out, case.ldg, case.n_img, **dict(case.kw))
    for a in out:
        if a is not None:
            a.setflags(write=False)         # shared among the tests: never changed
    return out


@functools.lru_cache(maxsize=None)
def expected(case):
    """(dw, db) of the float64 restatement, computed once per case"""
    g, x, scale = case.operands()
    want = ref.head_wgrad(g, x, case.c_out, scale, case.hw)
    for a in want:
        a.setflags(write=False)
    return want


def unit(*arrays):
    """the largest power of two that divides every (finite, non-zero) value of the arrays"""
    vals = np.unique(np.concatenate([np.abs(a.astype(np.float64)).ravel() for a in arrays]))
    vals = vals[(vals > 0) & np.isfinite(vals)]
    u = 2.0 ** 15
    while vals.size and not np.array_equal(vals / u, np.round(vals / u)):
        u /= 2.0
    return u


def assert_exact(case):
    """the validity condition of a bit-exact case: with u the unit of g and xs, sum_m |g| |xs| / u < 2^24 per element of dw and of
    db, so every float32 partial sum -- of the products or of the terms of their bfloat16 split, which are multiples of u and add
    up to the product in absolute value -- is an integer below 2^24 units and exact in any order.  -> the largest sum / u"""
    assert case.recipe in ("small", "wide")
    g, x, scale = case.operands()
    assert np.isnan(g[:, case.c_out:]).all(), "every element of g at or behind c_out is NaN"
    xs = ref.scaled_input(x, scale, case.hw)
    assert np.isfinite(g[:, :case.c_out]).all() and np.isfinite(xs).all()
    u = unit(g[:, :case.c_out], xs)
    assert u in (1.0, 0.5), u
    adw, adb = ref.abs_products(g, x, case.c_out, scale, case.hw)
    worst = max(adw.max(), adb.max()) / u
    assert worst < 2.0 ** 24, (case.name, worst)
    want_dw, want_db = expected(case)
    assert np.array_equal(want_dw, want_dw.astype(np.float32)) and np.array_equal(want_db, want_db.astype(np.float32))
    return worst


C_INS = (64, 128, 192, 256)
C_OUTS = (1, 2, 7, 8, 9, 31, 32, 33, 49, 50, 63, 64)
G_OFFSETS = (2, 4, 8)


def pixel_counts(P=P_DEFAULT, G=G_DEFAULT):
    return (1, 2, P - 1, P, P + 1, 4 * P, 5 * P + 1, G * P, G * P + 1)


def gain_row_case(P=P_DEFAULT, G=G_DEFAULT):
    """171 images of 3 chunks, 2 G + 1 chunks: workgroup b takes chunks b and b + G (and 0 a third), which lie in different images"""
    return Case("C", "small", (2 * G + 1) * P, 3 * P, 256, 50, 64, 0, True, 3999, (("g_max", 1),))


def exact_cases(P=P_DEFAULT, G=G_DEFAULT):
    out, seed = [], 1000

    def add(*a, **kw):
        nonlocal seed
        seed += 1
        out.append(Case(*a, seed=seed, **kw))

    # A: every c_in x load path x gains, small and wide.  c_out = 50 (an even straddle and a group behind); three chunks, the
    # last one ragged without gains.  Element path: a packed-but-one row (ldg 51) or a 16-byte-aligned pitch from a base 2 bytes off.
    for c_in in C_INS:
        for vector in (True, False):
            ldg, off = (64, 0) if vector else ((51, 0) if c_in in (128, 256) else (64, 2))
            for scaled in (False, True):
                m, hw = (3 * P, P) if scaled else (2 * P + 17, 2 * P + 17)
                for recipe in ("small", "wide"):
                    add("A", recipe, m, hw, c_in, 50, ldg, off, scaled)

    # B: every c_out class on both load paths, with c_in 256 (small, no gains, P + 1 pixels) and c_in 192 (wide, gains, 2 images)
    for c_out in C_OUTS:
        up8 = 8 * -(-c_out // 8)
        add("B", "small", P + 1, P + 1, 256, c_out, up8, 0, False)
        add("B", "wide", 2 * P, P, 192, c_out, up8, 0, True)
        add("B", "small", P + 1, P + 1, 256, c_out, c_out, 2 if c_out % 8 == 0 else 0, False)                 # packed
        add("B", "wide", 2 * P, P, 192, c_out, c_out + 1, 4 if (c_out + 1) % 8 == 0 else 0, True)            # one element of padding
    for c_out, c_in in ((50, 256), (63, 192), (64, 128)):
        add("B", "small", P + 1, P + 1, c_in, c_out, 72, 0, False)                # vector, a pitch that is no power of two
    add("B", "wide", 2 * P, P, 192, 50, 64, 16, True)                             # vector, g 16 bytes off a 128-byte line
    for c_out, c_in in ((33, 256), (49, 192), (50, 64)):
        add("B", "small", P + 1, P + 1, c_in, c_out, 57, 0, False)                # element, an odd pitch
    for off in G_OFFSETS:
        add("B", "small", P + 1, P + 1, 256, 50, 64, off, False)                  # element only because of the base
        add("B", "wide", 2 * P, P, 192, 49, 64, off, True)
    add("B", "small", P + 1, P + 1, 128, 64, 64, 2, False)

    # C: every pixel-count class.  small at all of them, wide where it is valid and has two pixels to use.
    for i, m in enumerate(pixel_counts(P, G)):
        c_in = C_INS[3 - i % 4]
        vector = i % 3 != 2
        add("C", "small", m, m, c_in, 50, 64, 0 if vector else 2, False)
        if WIDE_R <= m <= WIDE_MAX_M:
            add("C", "wide", m, m, C_INS[i % 4], 50, 64 if vector else 50, 0, False)
    out.append(gain_row_case(P, G))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


# the real-valued shapes of the alignment, rounding-bound and non-finite tests: (m, hw, scaled) at P
def real_shape(scaled, P=P_DEFAULT):
    return (3 * P, P, True) if scaled else (2 * P + 17, P, False)


@functools.lru_cache(maxsize=None)
def real_case(c_in, scaled, P=P_DEFAULT):
    """reals at c_out = 50, ldg = 64 -> dict(g, x, scale, m, hw, want, absprod); read-only, shared"""
    m, hw, _ = real_shape(scaled, P)
    g, x, scale = reals(np.random.default_rng(5000 + c_in + int(scaled)), m, c_in, 50, 64, m // hw if scaled else None)
    want, absprod = ref.head_wgrad(g, x, 50, scale, hw), ref.abs_products(g, x, 50, scale, hw)
    for a in (g, x, scale) + want + absprod:
        if a is not None:
            a.setflags(write=False)
    return dict(g=g, x=x, scale=scale, m=m, hw=hw, c_in=c_in, c_out=50, want=want, absprod=absprod)


def relayout(g, c_out, ldg):
    """the same channels 0 .. c_out - 1 in rows of ldg elements, NaN behind them"""
    out = _g_buffer(g.shape[0], ldg)
    out[:, :c_out] = g[:, :c_out]
    return out


# ---------------------------------------------------------------------------------------------------------------- the bf16 split

def split_bf16(a):
    """binary16 -> (hi, lo) float64 with a = hi + lo: hi keeps 8 significant bits (the float32 form cut to bfloat16), lo the low 3"""
    a = np.ascontiguousarray(a, np.float16)
    normal = np.abs(a.astype(np.float64)) >= 2.0 ** -14
    assert (normal | (a == 0)).all(), "the 3-bit cut below is written for normal values"
    hi = (a.view(np.uint16) & np.uint16(0xFFF8)).view(np.float16).astype(np.float64)
    return hi, a.astype(np.float64) - hi
