"""CPU: the cases of tests/head_wgrad_cases.py are what tests/test_gpu_head_wgrad_paths.py takes them for -- exact in every order
of the float32 additions, and in the class (load path, channel offset, straddle, chunks, gain row) they are listed under -- shown
through the float64 restatement and the classifier, never through the kernel.  Each test prints what it measured (pytest -s).
"""
import types

import numpy as np
import pytest

import head_wgrad_cases as hc
import head_wgrad_reference as ref

P, G = hc.P_DEFAULT, hc.G_DEFAULT
CASES = hc.exact_cases(P, G)


def test_every_case_is_exact_in_any_order():
    worst = {}
    for case in CASES:
        w = hc.assert_exact(case)
        key = (case.group, case.recipe)
        if w > worst.get(key, (0.0, None))[0]:
            worst[key] = (w, case.name)
    print(f"\n{len(CASES)} exact cases; the largest sum |g| |xs| / u per class, against 2^24 = {2 ** 24}:")
    for key in sorted(worst):
        w, name = worst[key]
        print(f"  {key[0]} {key[1]:5s}  {w:12.1f} = 2^{np.log2(w):5.2f}   {name}")
    assert max(w for w, _ in worst.values()) < 2.0 ** 24


def test_the_gain_row_case_is_exact_and_changes_image_in_every_workgroup():
    case = hc.gain_row_case(P, G)
    assert case in CASES and dict(case.kw) == {"g_max": 1}
    w = hc.assert_exact(case)
    p = case.paths(P, G)
    print(f"\n{case.name}: sum |g| |xs| / u = {w:.0f} (2^24 = {2 ** 24}); {case.n_img} images, {p['n_chunks']} chunks, grid {p['grid']}")
    assert case.n_img == 171 and p["n_chunks"] == 2 * G + 1 and p["grid"] == G and p["max_passes"] == 3 and p["gain_row_changes"]
    for b in range(G):      # EVERY workgroup, not just one
        img = [(c * P) // case.hw for c in range(b, p["n_chunks"], G)]
        assert len(img) >= 2 and all(i != j for i, j in zip(img, img[1:])), b
    # with the recipe's default |g| <= 3 the condition would still hold here; with g_max = 1 the margin is printed above


def _table():
    """required class -> predicate over (case, paths)"""
    req = {}
    for c_in in hc.C_INS:
        for load in ("vector", "element"):
            for scaled in (False, True):
                for recipe in ("small", "wide"):
                    req[f"A c_in {c_in} {load} {'gains' if scaled else 'plain'} {recipe}"] = (
                        lambda c, p, c_in=c_in, load=load, scaled=scaled, recipe=recipe:
                        c.c_in == c_in and p["load"] == load and c.scaled == scaled and c.recipe == recipe)
    for c_out in hc.C_OUTS:
        for load in ("vector", "element"):
            for c_in in (192, 256):
                req[f"B c_out {c_out} {load} c_in {c_in}"] = (lambda c, p, c_out=c_out, load=load, c_in=c_in:
                                                             c.c_out == c_out and p["load"] == load and c.c_in == c_in)
        req[f"B c_out {c_out} vector, ldg the next multiple of 8"] = (
            lambda c, p, c_out=c_out: c.c_out == c_out and p["load"] == "vector" and c.ldg == 8 * -(-c_out // 8))
        req[f"B c_out {c_out} element, packed"] = lambda c, p, c_out=c_out: c.c_out == c_out and p["load"] == "element" and c.ldg == c_out
        req[f"B c_out {c_out} element, ldg = c_out + 1"] = (
            lambda c, p, c_out=c_out: c.c_out == c_out and p["load"] == "element" and c.ldg == c_out + 1)
    req["B vector ldg 72"] = lambda c, p: p["load"] == "vector" and c.ldg == 72
    req["B element ldg 57"] = lambda c, p: p["load"] == "element" and c.ldg == 57
    for off in hc.G_OFFSETS:
        req[f"B element ldg 64 at g + {off} bytes"] = lambda c, p, off=off: p["load"] == "element" and c.ldg == 64 and c.g_byte_offset == off
    for s in ("none", "even", "odd", "behind"):
        for load in ("vector", "element"):
            req[f"straddle {s} {load}"] = lambda c, p, s=s, load=load: p["straddle"] == s and p["load"] == load
    req["odd straddle with a group behind it, vector"] = lambda c, p: p["straddle"] == "odd" and p["groups_behind"] > 0 and p["load"] == "vector"
    req["odd straddle in the last group, vector"] = lambda c, p: p["straddle"] == "odd" and p["groups_behind"] == 0 and p["load"] == "vector"
    req["c_out < 8, vector"] = lambda c, p: c.c_out < 8 and p["load"] == "vector"
    for load in ("vector", "element"):
        req[f"second row tile empty, {load}"] = lambda c, p, load=load: p["second_row_tile_empty"] and p["load"] == load
        req[f"second row tile holds one row (c_out 33), {load}"] = lambda c, p, load=load: c.c_out == 33 and p["load"] == load
    req["element path with padding in the row, c_in 192"] = lambda c, p: p["load"] == "element" and p["row_padding"] > 0 and c.c_in == 192
    req["element path with padding in the row, c_in 256"] = lambda c, p: p["load"] == "element" and p["row_padding"] > 0 and c.c_in == 256
    for m in hc.pixel_counts(P, G):
        req[f"C m = {m}"] = lambda c, p, m=m: c.m == m
    req["C more chunks than workgroups, ragged tail"] = lambda c, p: p["max_passes"] == 2 and p["ragged_tail"] and p["grid"] == G
    req["C gains, every workgroup changes image"] = lambda c, p: p["gain_row_changes"] and c.m == (2 * G + 1) * P and c.hw == 3 * P
    for c_in in (128, 192):
        req[f"gains with c_in {c_in}"] = lambda c, p, c_in=c_in: c.scaled and c.c_in == c_in
    req["gains where a thread's groups sit at different channel offsets, wide"] = (
        lambda c, p: c.scaled and not p["same_offset"] and c.recipe == "wide")
    for n in (1, 2, 3, 4):
        req[f"finish: {n} non-empty runs"] = lambda c, p, n=n: p["finish_runs"] == n
    return req


def test_every_class_is_hit():
    classified = [(c, c.paths(P, G)) for c in CASES]
    missing = []
    print()
    for name, pred in _table().items():
        hits = [c.name for c, p in classified if pred(c, p)]
        print(f"  {name:70s} {len(hits):3d}  {hits[0] if hits else '-'}")
        if not hits:
            missing.append(name)
    assert not missing, missing
    biggest = max(CASES, key=lambda c: c.m * c.c_in)
    assert biggest.m * biggest.c_in * 2 <= 17.5e6, "the largest case stays near 33 000 pixels x 256 channels"
    assert all(c.recipe != "wide" or c.m <= hc.WIDE_MAX_M for c in CASES)


def test_classifier_on_hand_checked_calls():
    p = hc.paths(192, 64, 256, 50, 64, 0, True, P, G)
    assert (p["load"], p["same_offset"], p["straddle"], p["groups_behind"], p["n_chunks"], p["grid"], p["max_passes"]) == \
        ("vector", True, "even", 1, 3, 3, 1) and not p["gain_row_changes"] and p["finish_runs"] == 3
    p = hc.paths(1, 1, 192, 49, 49, 0, False, P, G)
    assert (p["load"], p["same_offset"], p["straddle"], p["groups_behind"], p["finish_runs"]) == ("element", False, "odd", 1, 1)
    assert hc.paths(65, 65, 64, 64, 64, 2, False, P, G)["load"] == "element" and hc.paths(65, 65, 64, 64, 72, 16, False, P, G)["load"] == "vector"
    assert hc.paths(65, 65, 64, 32, 32, 0, False, P, G)["straddle"] == "behind" and hc.paths(65, 65, 64, 32, 32, 0, False, P, G)["second_row_tile_empty"]
    # 2 G chunks in images of G chunks: workgroup b takes chunk b of image 0 and chunk b of image 1
    assert hc.paths(2 * G * P, G * P, 64, 50, 64, 0, True, P, G)["gain_row_changes"]
    assert not hc.paths(2 * G * P, G * P, 64, 50, 64, 0, False, P, G)["gain_row_changes"]
    assert not hc.paths(2 * G * P, 2 * G * P, 64, 50, 64, 0, True, P, G)["gain_row_changes"]


def test_the_existing_suite_misses_these_classes():
    """the written proof of the gap: what exact_shapes of tests/test_gpu_head_wgrad.py (and its two other exact tests) classify as"""
    import test_gpu_head_wgrad as old
    fake = types.SimpleNamespace(pp_head_wgrad_chunk_pixels=lambda: P, pp_head_wgrad_max_workgroups=lambda: G)
    shapes, big = old.exact_shapes(fake)
    shapes = shapes + [big, (192, 64, 256, 50, 64, True)]            # + test_exact_product_needs_its_rounding
    seen = [hc.paths(m, hw, c_in, c_out, ldg, 0, scaled, P, G) for m, hw, c_in, c_out, ldg, scaled in shapes]
    print("\nthe existing exact shapes:")
    for s, p in zip(shapes, seen):
        print(f"  {s}: {p}")
    assert {s[2] for s in shapes} == {64, 128, 256}
    assert all(p["same_offset"] for p in seen)
    assert all(p["straddle"] != "odd" for p in seen) and {p["straddle"] for p in seen} == {"even", "none"}
    assert not any(p["gain_row_changes"] for p in seen)
    assert {s[3] for s in shapes} == {50, 64}
    element = [(s, p) for s, p in zip(shapes, seen) if p["load"] == "element"]
    assert element and all(p["row_padding"] == 0 and s[2] == 256 and not s[5] for s, p in element)
    assert all(p["n_chunks"] <= p["grid"] for s, p in zip(shapes, seen) if s[5])


WIDE = [c for c in CASES if c.recipe == "wide"]


def test_wide_makes_every_term_of_the_split_count():
    """every value of a wide case has a non-zero low part, so every PRODUCT has non-zero hi*lo, lo*hi and lo*lo terms; an
    element of dw is the sum of at most two products.  Cutting g (or x) to its high part changes every element that has a product;
    dropping only lo*lo changes every element except those whose two lo*lo terms cancel (equal magnitude among the products of two
    odd numbers in 1 .. 7 -- 28 of 256 pairs -- and opposite sign: 5.5 % expected), which are counted and printed."""
    assert len(WIDE) >= 16
    print()
    for case in WIDE:
        g, x, scale = case.operands()
        xs = ref.scaled_input(x, scale, case.hw)
        gv = g[:, :case.c_out]
        g_hi, g_lo = hc.split_bf16(gv)
        x_hi, x_lo = hc.split_bf16(xs)
        assert (g_lo != 0).all() and ((x_lo != 0) == (xs != 0)).all()
        per_channel = (xs != 0).sum(axis=0)
        assert (per_channel == min(hc.WIDE_R, case.m)).all()
        full = hc.expected(case)[0]
        assert np.array_equal(full, g_hi.T @ x_hi + g_hi.T @ x_lo + g_lo.T @ x_hi + g_lo.T @ x_lo)      # all four exact in float64
        has_product = np.ones_like(full, bool)          # every g is non-zero and every channel has a pixel
        no_g_lo, no_x_lo, no_lolo = g_hi.T @ xs.astype(np.float64), gv.astype(np.float64).T @ x_hi, full - g_lo.T @ x_lo
        # the terms of every single product are non-zero
        assert (np.abs(g_lo).T @ np.abs(x_lo) > 0).all()
        changed = [float((d != full)[has_product].mean()) for d in (no_g_lo, no_x_lo, no_lolo)]
        print(f"  {case.name:75s} changed by g -> g_hi {changed[0]:.4f}, x -> x_hi {changed[1]:.4f}, without lo*lo {changed[2]:.4f}")
        if case.m == 1 or case.c_out * case.c_in < 4096:
            assert min(changed) > 0.5            # one product, or too few elements for a rate: most of them at the least
        else:
            assert changed[0] > 0.98 and changed[1] > 0.98 and changed[2] > 0.9
        # a float32 accumulation of the three remaining terms is still exact, so the damage would be visible bit for bit
        assert np.array_equal(no_lolo, no_lolo.astype(np.float32))


def test_recipes_fill_the_padding_with_nan_and_reals_are_shared_read_only():
    for case in CASES[:8]:
        g, x, scale = case.operands()
        assert g.shape == (case.m, case.ldg) and x.shape == (case.m, case.c_in) and np.isnan(g[:, case.c_out:]).all()
        assert not g.flags.writeable and not x.flags.writeable
        assert (scale is None) == (not case.scaled)
    r = hc.real_case(192, True, P)
    assert r["m"] == 3 * P and r["hw"] == P and r["scale"].shape == (3, 192) and not r["x"].flags.writeable
    g51 = hc.relayout(r["g"], 50, 51)
    assert g51.shape == (3 * P, 51) and np.array_equal(g51[:, :50], r["g"][:, :50]) and np.isnan(g51[:, 50]).all()
    with pytest.raises(ValueError):
        r["x"][0, 0] = 1
