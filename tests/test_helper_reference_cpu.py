"""CPU: tests/helper_reference.py against the plain torch formulation of every helper entry, the validity of its exact recipes (every
float32 partial sum exact in any order), the distance of the SE recipe's sigmoid values from the binary16 rounding boundaries, and the
shape lists of tests/test_gpu_helper_kernels.py against the launchers' arithmetic (csrc/posepaf_epilogue.hip), restated here."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helper_reference as ref

NOISE = 1e-12


def rand16(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float16)


def t64(a):
    return torch.from_numpy(np.asarray(a).astype(np.float64))


def close(got, want, tol=NOISE):
    want = want.numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max())


# ------------------------------------------------------------------------------------------------ against torch on random data

@pytest.mark.parametrize("res,act,post", [(r, a, p) for r in (0, 1) for a in (0, 1) for p in (0, 1)])
def test_bias_act_against_torch(res, act, post):
    rng = np.random.default_rng(1)
    y, r, p, b = rand16(rng, (37, 24)), rand16(rng, (37, 24)), rand16(rng, (37, 24)), rand16(rng, (24,))
    want = t64(y) + t64(b)
    want = want + t64(r) if res else want
    want = F.leaky_relu(want, float(ref.LEAK)) if act else want
    want = want + t64(p) if post else want
    close(ref.bias_act(y, b, r if res else None, p if post else None, act, ref.LEAK), want)


def test_add3_scale_mean_against_torch():
    rng = np.random.default_rng(2)
    a, b, c = (rand16(rng, (2, 45, 16)) for _ in range(3))
    close(ref.add3(a, b, c), t64(a) + t64(b) + t64(c))
    close(ref.add3(a, b), t64(a) + t64(b))
    s = rand16(rng, (2, 16))
    close(ref.channel_scale(a, s), t64(a) * t64(s)[:, None, :])
    close(ref.channel_mean_real(a), t64(a).mean(dim=1))
    ints = rng.integers(-4, 5, (2, 45, 16)).astype(np.float16)
    close(ref.mean_of_sums(ref.channel_sums(ints), 45), t64(ints).mean(dim=1), 2.0 ** -22)      # two float32 roundings
    with pytest.raises(AssertionError):
        ref.mean_of_sums(np.array([2.0 ** 24 + 1.0]), 4)


def test_se_gains_against_torch():
    rng = np.random.default_rng(3)
    n, c, hid = 3, 40, 6
    mean, w1, b1 = rand16(rng, (n, c)), rand16(rng, (hid, c), c ** -0.5), rand16(rng, (hid,))
    w2, b2 = rand16(rng, (c, hid)), rand16(rng, (c,))
    r16 = lambda t: t.half().double()
    h = r16(F.linear(t64(mean), t64(w1), t64(b1)))
    h = r16(F.leaky_relu(h, float(ref.LEAK)))
    z = r16(F.linear(h, t64(w2), t64(b2)))
    got = ref.se_gains(mean, w1, b1, w2, b2, ref.LEAK)
    close(got["z"], z)
    close(got["gain"], torch.sigmoid(z))


def test_pool_upsample_planes_against_torch():
    rng = np.random.default_rng(4)
    x = rand16(rng, (2, 6, 10, 8))
    nchw = torch.from_numpy(x).permute(0, 3, 1, 2).float()
    close(ref.pool_max(x), F.max_pool2d(nchw, 2, 2).permute(0, 2, 3, 1).double())
    close(ref.f64(ref.upsample2(x)), F.interpolate(nchw, scale_factor=2, mode="nearest").permute(0, 2, 3, 1).double())
    p = rand16(rng, (2, 72, 64))
    close(ref.f64(ref.nhwc64_to_planes(p, 50)), torch.from_numpy(p).permute(0, 2, 1)[:, :50].double())


def test_pool_rule_on_nan_and_zeros():
    """the rule of include/posepaf.h: the maximum of the non-NaN elements, NaN only when all four are, +0 above -0 -- where torch's
    max_pool2d (the fallback of fused_model.maxpool2) propagates NaN instead"""
    w = lambda *v: np.array(v, np.float16).reshape(1, 2, 2, 1)
    bits = lambda x: ref.to_half(ref.pool_max(x)).view(np.uint16).item()
    nan = np.nan
    assert bits(w(nan, 1, 2, -3)) == 0x4000 and bits(w(nan, nan, nan, -3)) == 0xC200 and bits(w(nan, nan, nan, nan)) & 0x7FFF > 0x7C00
    assert bits(w(-0.0, 0.0, -0.0, -0.0)) == 0x0000 and bits(w(-0.0, -0.0, -0.0, -0.0)) == 0x8000 and bits(w(-0.0, nan, nan, -1)) == 0x8000
    assert bits(w(-np.inf, nan, -np.inf, -np.inf)) == 0xFC00 and bits(w(np.inf, nan, 1, -np.inf)) == 0x7C00
    nchw = torch.tensor([[[[nan, 1.0], [2.0, -3.0]]]])
    assert torch.isnan(F.max_pool2d(nchw, 2, 2)).all()
    x = ref.pool_windows(8)
    got = ref.to_half(ref.pool_max(x))
    assert got.shape == (1, 8, 4, 8) and np.isnan(got).any() and (got.view(np.uint16) == 0x8000).any() and np.isinf(got).any()
    win = x.reshape(1, 8, 2, 4, 2, 8).transpose(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    for pos in range(4):                                           # NaN alone in every position; +0 alone among -0 in every position
        others = np.delete(win, pos, axis=1)
        assert (np.isnan(win[:, pos]) & ~np.isnan(others).any(axis=1)).any()
        z = (win == 0) & ~np.isnan(win)
        assert (z.all(axis=1) & ~np.signbit(win[:, pos]) & np.signbit(others).all(axis=1)).any()


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_flip_average_against_the_references_formula(dtype, flip):
    """utils/parse_skeletons.py:82-93 of the reference on one image: (out + out_flip[:, ::-1, :][:, :, ord]) / 2 in the input's type"""
    rng = np.random.default_rng(5)
    b, h, w = 2, 3, 5
    net = rng.standard_normal((b * (2 if flip else 1), 50, h, w)).astype(dtype)
    heat, paf = ref.flip_average(net, flip)
    assert heat.shape == (b, h, w, 20) and paf.shape == (b, h, w, 30)
    for i in range(b):
        hwc = net[i * (2 if flip else 1)].transpose(1, 2, 0)
        o_paf, o_heat = hwc[:, :, :30], hwc[:, :, 30:]
        if flip:
            f = net[2 * i + 1].transpose(1, 2, 0)
            o_paf = (o_paf + f[:, :, :30][:, ::-1, :][:, :, ref.FLIP_PAF]) / 2
            o_heat = (o_heat + f[:, :, 30:][:, ::-1, :][:, :, ref.FLIP_HEAT]) / 2
            assert o_paf.dtype == dtype
        tol = 2.0 ** -10 if dtype == np.float16 else 0.0             # NumPy's binary16 division rounds once, the entry twice
        assert np.abs(paf[i] - o_paf.astype(np.float64)).max() <= tol * 4 and np.abs(heat[i] - o_heat.astype(np.float64)).max() <= tol * 4
    assert sorted(ref.FLIP_PAF) == list(range(30)) and sorted(ref.FLIP_HEAT) == list(range(20))
    assert all(ref.FLIP_CH[ref.FLIP_CH[c]] == c for c in range(50))   # a mirror: applying it twice is the identity


def test_flip_average_binary16_rounds_twice():
    net = np.zeros((2, 50, 1, 1), np.float16)
    net[0, 0], net[1, 0] = 60000.0, 60000.0                          # the sum overflows before it is halved
    net[0, 30], net[1, 30] = 3 * ref.SUB, 2 * ref.SUB                # 5 * 2^-24 halved: a tie on the subnormal grid, to even
    net[0, 3], net[1, 4] = 2050.0, 1.0                               # channel 3's partner is 4: 2051 -> 2052 -> 1026, not 1025.5
    heat, paf = ref.flip_average(net, 1)
    assert np.isinf(paf[0, 0, 0, 0]) and heat[0, 0, 0, 0] == 2 * ref.SUB and paf[0, 0, 0, 3] == 1026.0


@pytest.mark.parametrize("flip", [0, 1])
def test_preprocess_against_numpy(flip):
    """utils/util.py:44-65 padRightDownCorner + / 255 + the mirror of the padded image (utils/parse_skeletons.py:52-73)"""
    rng = np.random.default_rng(6)
    b, h, w, pad_to, pad_value = 2, 5, 7, 4, 128
    img = rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
    hp, wp = -(-h // pad_to) * pad_to, -(-w // pad_to) * pad_to
    slots = np.full((b, hp, wp, 3), 0xFF, np.uint8)
    slots[:, :h, :w] = img
    got = ref.preprocess(slots, ([h] * b, [w] * b), pad_value, flip)
    padded = torch.full((b, hp, wp, 3), float(pad_value))
    padded[:, :h, :w] = torch.from_numpy(img).float()
    want = padded / 255
    if flip:
        want = torch.stack([want, want.flip(2)], dim=1).reshape(2 * b, hp, wp, 3)
    assert np.array_equal(got, want.double().numpy())
    ragged = ref.preprocess(slots, ([h, 3], [w, 8]), pad_value, flip)
    assert np.array_equal(ragged[0], got[0]) and (ragged[1 + flip, 3:] == got[0, -1, -1, 0]).all() and ragged[1 + flip, 2, 7, 0] == 1.0


# ------------------------------------------------------------------------------------------------ the exact recipes are exact

@pytest.mark.parametrize("recipe", ["small", "rounding", "subnormal"])
def test_elementwise_recipes_are_exact(recipe):
    (y, r, p), b = ref.tensor_operands(recipe, 343, 24, 3, 0)
    grid = ref.recipe_grid(recipe)
    units = ref.assert_exact([y, r, p, b], ref.bias_act_abs_terms(y, b, r, p), grid, recipe)
    print(f"{recipe}: sum |terms| = {units:.0f} grid units")
    want = ref.bias_act(y, b, r, p, True, ref.SLOPE)
    if recipe == "rounding":
        fin = np.isfinite(ref.to_half(want))
        assert (~fin).mean() > 0.01 and (ref.f64(ref.to_half(want))[fin] != want[fin]).mean() > 0.25    # the store's rounding shows
    if recipe == "subnormal":
        assert (np.abs(want) < 2.0 ** -14).all() and (ref.f64(ref.to_half(want)) != want).mean() > 0.1   # ties and eighths of a step
    x, s = ref.scale_operands(recipe, 2, 37, 24, 0)
    prod = ref.channel_scale(x, s)
    assert np.array_equal(prod.astype(np.float32).astype(np.float64)[np.isfinite(prod)], prod[np.isfinite(prod)])   # exact in float32
    if recipe != "small":
        assert (ref.f64(ref.to_half(prod)) != prod).mean() > 0.1


def test_special_recipe_places_every_combination():
    (y, r, p), b = ref.tensor_operands("special", 343, 8, 3, 0)
    code = lambda a: np.select([np.isnan(a)] + [a.view(np.uint16) == s for s in ref.SPECIALS.view(np.uint16)[1:]], range(7), 7)
    seen = {(i, j, k, l) for i, j, k, l in zip(code(y).ravel(), np.broadcast_to(code(b), y.shape).ravel(), code(r).ravel(), code(p).ravel())}
    assert {(i, j, k, l) for i in range(7) for j in range(7) for k in range(7) for l in range(7)} <= seen
    x, s = ref.scale_operands("special", 1, 7, 8, 0)
    assert {(i, j) for i in range(7) for j in range(7)} <= set(zip(code(x[0]).ravel(), np.broadcast_to(code(s[0]), x[0].shape).ravel()))


@pytest.mark.parametrize("case", ref.MEAN_CASES, ids=str)
def test_mean_cases_are_exact(case):
    n, hw, c, _ = case
    x = ref.mean_operands(case)
    assert x.shape == (n, hw, c)
    ref.assert_exact([x], np.abs(ref.f64(x)).sum(axis=1), 1.0, str(case))
    ref.mean_of_sums(ref.channel_sums(x), hw)                        # asserts that the sums are float32 values


@pytest.mark.parametrize("slope", ref.SE_SLOPES)
@pytest.mark.parametrize("case", ref.SE_CASES, ids=str)
def test_se_recipe_is_exact_and_clear_of_the_boundaries(case, slope):
    o = ref.se_operands(case, slope)
    r = ref.se_gains(o["mean"], o["w1"], o["b1"], o["w2"], o["b2"], slope)
    assert float(np.float32(slope)) == slope and np.array_equal(ref.f64(ref.to_half(r["hidden_sum"])) * slope * 2.0 ** 12 % 1, 0 * r["hidden_sum"])
    m, w1, w2 = ref.f64(o["mean"]), ref.f64(o["w1"]), ref.f64(o["w2"])
    ref.assert_exact([w1, o["b1"]], np.abs(m) @ np.abs(w1).T + np.abs(ref.f64(o["b1"])), o["grid1"], "W1 m + b1")
    ref.assert_exact([r["hidden"][:, None, :] * w2[None], o["b2"]], np.abs(r["hidden"]) @ np.abs(w2).T + np.abs(ref.f64(o["b2"])), o["grid2"],
                     "W2 h + b2")
    assert np.array_equal(o["partial"].astype(np.float64).sum(axis=1), m * o["hw"])
    ref.assert_exact([o["partial"]], np.abs(o["partial"]).astype(np.float64).sum(axis=1), 1.0, "the partial sums")
    assert np.array_equal(ref.to_half(ref.mean_of_sums(o["partial"].astype(np.float64).sum(axis=1), o["hw"])).view(np.uint16),
                          o["mean"].view(np.uint16))
    z = ref.se_z_values(case, slope)
    dist = ref.half_boundary_distance(ref.sigmoid(z))
    print(f"{case}: {z.size} values of z in [{z.min()}, {z.max()}], nearest boundary {dist.min() / 2.0 ** -18:.2f} x 2^-18 away")
    assert (dist >= ref.SE_Z_CLEARANCE).all()
    if case[2] > 1:                                                  # the hidden vector's rounding is not a no-op
        assert (ref.f64(ref.to_half(r["hidden_sum"])) != r["hidden_sum"]).mean() > 0.1
        assert np.unique(ref.to_half(r["gain"])).size > 100
        unrounded = ref.se_gains(o["mean"], o["w1"], o["b1"], o["w2"], o["b2"], slope, round_hidden_sum=False)
        changed = (ref.to_half(unrounded["gain"]).view(np.uint16) != ref.to_half(r["gain"]).view(np.uint16)).mean()
        print(f"without the hidden vector's first rounding {changed:.3f} of the gains change")
        assert changed == 0.0 if slope == ref.SLOPE else changed > 0.01    # a power of two cannot see that rounding, 3/8 can


def test_boundary_distance():
    d = ref.half_boundary_distance(np.array([1.0 + 2.0 ** -11, 1.0, 2.0 ** -25, 0.75 * 2.0 ** -24]))
    assert d[0] == 0.0 and d[2] == 0.0 and abs(d[1] - 2.0 ** -11) < 1e-15 and abs(d[3] - 1 / 3) < 1e-12


# ------------------------------------------------------------------------------------------------ the shapes reach what they claim

def grid_for(items):                                                 # csrc/posepaf_epilogue.hip grid_for
    return min((items + 255) // 256, 8192)


def reaches_second_pass(items):
    return items > grid_for(items) * 256 and items > 8192 * 256 and items % 256 != 0


def test_second_pass_cases_reach_the_second_pass():
    assert reaches_second_pass(ref.SECOND_PASS_VECTORS)
    n, ho, wo, c = ref.POOL_SECOND_PASS
    assert reaches_second_pass(n * ho * wo * (c // 8)) and wo % 2 == 1
    n, hi, wi, c = ref.UPSAMPLE_SECOND_PASS
    assert reaches_second_pass(n * hi * wi * (c // 8))
    p = ref.PREPROCESS_LARGE
    hp, wp = -(-p["h"] // p["pad_to"]) * p["pad_to"], -(-p["w"] // p["pad_to"]) * p["pad_to"]
    assert reaches_second_pass(p["batch"] * hp * wp) and hp > p["h"] and wp > p["w"]
    r = ref.RAGGED_LARGE
    assert reaches_second_pass(r["batch"] * r["hp"] * r["wp"]) and len(set(r["sizes"])) == 2
    assert all(h <= r["hp"] and w <= r["wp"] for h, w in r["sizes"]) and any(h < r["hp"] and w < r["wp"] for h, w in r["sizes"])
    b, h, w = ref.FLIP_SHAPES[-1]
    assert reaches_second_pass(b * h * w * ref.NUM_CH) and not any(reaches_second_pass(b * h * w * 50) for b, h, w in ref.FLIP_SHAPES[:-1])
    assert (1, 1, 1) in [s[:3] for s in ref.POOL_SHAPES] and any(s[2] % 2 for s in ref.POOL_SHAPES)
    assert {s[3] for s in ref.POOL_SHAPES} == {8, 24}


def test_mean_cases_reach_every_path_of_the_sum_kernel():
    """k_channel_sum: per = ceil(hw / splits) pixels per split, split s takes [s per, min((s + 1) per, hw)), plan = 256 / cvec lanes"""
    seen = set()
    for n, hw, c, splits in ref.MEAN_CASES:
        cvec = c // 8
        plan, per = 256 // cvec, -(-hw // splits)
        sizes = [max(0, min((s + 1) * per, hw) - s * per) for s in range(splits)]
        assert sum(sizes) == hw
        seen |= {"empty" for s in sizes if s == 0} | {"ragged" for s in sizes if 0 < s < per}
        seen |= {"idle threads"} if 256 % cvec else set()
        seen |= {"one lane"} if cvec == 256 else set()
        seen |= {"lane loop"} if per > plan > 1 else set()
        seen |= {"one pixel"} if splits == hw else set()
        seen |= {"hw a power of two"} if hw & (hw - 1) == 0 else {"hw no power of two"}
    assert seen == {"empty", "ragged", "idle threads", "one lane", "lane loop", "one pixel", "hw a power of two", "hw no power of two"}
    n, hw, c, splits = ref.MEAN_CASES[0]
    assert -(-hw // splits) * (splits - 1) >= hw                     # the first case's last split is the empty one


def test_scale_and_layout_cases():
    n, hw, c = ref.SCALE_CAPPED
    per_block = 256 // (c // 8)
    assert (hw + per_block * 8 - 1) // (per_block * 8) > 4096 and hw % per_block != 0      # capped grid, a ragged last step
    assert {256 % (c // 8) == 0 for c in ref.SCALE_CHANNELS} == {True, False}
    kinds = {("vector rows" if hw % 8 == 0 else "element rows", "partial tile" if hw % 64 else "whole tiles") for hw in ref.PLANES_HW}
    assert kinds == {("vector rows", "partial tile"), ("vector rows", "whole tiles"), ("element rows", "partial tile")}
    assert any(hw % 8 == 0 and hw % 64 != 0 and hw > 64 for hw in ref.PLANES_HW)           # whole tile, then a partial one, 16-byte rows
    assert any(hw % 8 == 0 and hw < 64 for hw in ref.PLANES_HW) and any(hw % 8 and hw > 64 for hw in ref.PLANES_HW)
    assert min(ref.PLANES_C_OUT) == 1 and max(ref.PLANES_C_OUT) == 64 and 50 in ref.PLANES_C_OUT
