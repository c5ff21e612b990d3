"""CPU: the restated loss-scale state machine (tests/head_step_reference.py) against a table written out by hand, and the refusals of
pp_head_wgrad_multi_f16 and pp_head_update_f32 in their documented order -- every call here is refused before a device is needed
(pointers are made-up addresses that nothing dereferences), so the file gives the same answers with and without a GPU."""
import ctypes as C

import numpy as np
import pytest

import head_step_reference as hs

OK, NO_DEVICE, BAD_ARG, TOO_LARGE, UNSUPPORTED = 0, -1, -2, -3, -6


# ---------------------------------------------------------------------------------------------------- the state machine, by hand
# (scale, good_steps, skipped) after each outcome; F = a finite step, X = a gradient that is not finite
F, X = True, False
TABLE = [
    # halving, down to the floor and no further
    (dict(scale=4.0, growth_interval=2000, min_scale=1.0), [X, X, X, F],
     [(2.0, 0, 1), (1.0, 0, 2), (1.0, 0, 3), (1.0, 1, 3)]),
    # doubling, up to the cap and no further; the count starts again after each growth
    (dict(scale=4.0, growth_interval=1, max_scale=16.0), [F, F, F, F],
     [(8.0, 0, 0), (16.0, 0, 0), (16.0, 0, 0), (16.0, 0, 0)]),
    # growth_interval 0: static, whatever happens; skipped still counts
    (dict(scale=8.0, growth_interval=0), [F, X, F, X, X],
     [(8.0, 0, 0), (8.0, 0, 1), (8.0, 0, 1), (8.0, 0, 2), (8.0, 0, 3)]),
    # growth_interval 3: the third finite step in a row doubles
    (dict(scale=2.0, growth_interval=3), [F, F, F, F, F, F],
     [(2.0, 1, 0), (2.0, 2, 0), (4.0, 0, 0), (4.0, 1, 0), (4.0, 2, 0), (8.0, 0, 0)]),
    # an overflow on the very step that would have grown the scale: halved instead, and the count starts again
    (dict(scale=2.0, growth_interval=3), [F, F, X, F, F, F],
     [(2.0, 1, 0), (2.0, 2, 0), (1.0, 0, 1), (1.0, 1, 1), (1.0, 2, 1), (2.0, 0, 1)]),
    # the default range: 2^24 is the cap, 2^-24 the floor
    (dict(scale=2.0 ** 24, growth_interval=1), [F, X], [(2.0 ** 24, 0, 0), (2.0 ** 23, 0, 1)]),
    (dict(scale=2.0 ** -24, growth_interval=1), [X, F], [(2.0 ** -24, 0, 1), (2.0 ** -23, 0, 1)]),
]


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_state_machine_against_the_hand_written_table(row):
    start, outcomes, want = TABLE[row]
    states = hs.run(hs.new_state(**start), outcomes)
    assert len(states) == len(want)
    for i, (s, (scale, good, skipped)) in enumerate(zip(states, want)):
        assert (float(s["scale"]), s["good_steps"], s["skipped"]) == (scale, good, skipped), (row, i)
        assert float(s["inv_scale"]) == 1.0 / scale and s["inv_scale"].dtype == np.float32       # a power of two: exact
        assert s["growth_interval"] == start["growth_interval"]


def test_state_block_layout():
    from posepaf import _lib
    dt = _lib.HEAD_UPDATE_STATE_DTYPE
    assert tuple(dt.names) == hs.FIELDS and dt.itemsize == 32
    assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 20, 24]
    assert C.sizeof(_lib.HeadUpdateDesc) == 64 and C.sizeof(_lib.HeadWgradDesc) == 72


# ---------------------------------------------------------------------------------------------------- refusals

@pytest.fixture(scope="module")
def lib():
    from posepaf import _lib
    return _lib.load()


A = 0x10000          # a made-up address on a 64-KiB boundary: no refused call reads or writes through it


def desc(**over):
    from posepaf import _lib
    d = dict(g=A, ldg=64, x=A, scale=None, m=64, hw=64, c_in=256, c_out=50, dw=A, db=A)
    d.update(over)
    return _lib.HeadWgradDesc(**d)


def table(*descs):
    from posepaf import _lib
    return (_lib.HeadWgradDesc * len(descs))(*descs)


def multi(lib, t, n=None, inv=1.0, inv_dev=None, ws=A, ws_bytes=1 << 40):
    return lib.pp_head_wgrad_multi_f16(len(t) if n is None else n, t, inv, C.c_void_p(inv_dev), C.c_void_p(ws), ws_bytes, None)


def test_multi_refusals_in_their_order(lib):
    assert lib.pp_head_wgrad_multi_max_heads() == 40
    good = desc()
    bad_arg, unsupported, too_large = desc(g=None), desc(c_in=100), desc(m=2 ** 31)
    # the table itself
    assert lib.pp_head_wgrad_multi_f16(1, None, 1.0, None, C.c_void_p(A), 1 << 40, None) == BAD_ARG
    assert multi(lib, table(good), n=0) == BAD_ARG and multi(lib, table(good), n=-3) == BAD_ARG
    # too many heads comes before anything about a head, the workspace or the factor
    assert multi(lib, table(*[bad_arg] * 41), ws=None, inv=0.0) == UNSUPPORTED
    assert multi(lib, table(*[good] * 40), ws=None) == BAD_ARG          # 40 are taken: the next refusal answers
    # the first head that fails one answers, with the single entry's order inside a head
    assert multi(lib, table(good, unsupported, bad_arg)) == UNSUPPORTED
    assert multi(lib, table(good, bad_arg, unsupported)) == BAD_ARG
    assert multi(lib, table(too_large, bad_arg)) == TOO_LARGE
    assert multi(lib, table(desc(c_in=100, ldg=10))) == BAD_ARG           # ldg < c_out before unsupported
    assert multi(lib, table(desc(c_in=100, x=A + 8))) == BAD_ARG          # alignment before unsupported
    assert multi(lib, table(desc(c_in=100, m=2 ** 31))) == UNSUPPORTED    # unsupported before too large
    for over in (dict(x=None), dict(dw=None), dict(db=None), dict(m=0), dict(hw=0), dict(scale=A, m=100, hw=64), dict(ldg=49),
                 dict(g=A + 1), dict(scale=A + 8), dict(dw=A + 2), dict(db=A + 1)):
        assert multi(lib, table(good, desc(**over))) == BAD_ARG, over
    for over in (dict(c_out=65, ldg=72), dict(c_out=0, ldg=0), dict(c_in=320), dict(scale=A, m=96, hw=32)):
        assert multi(lib, table(good, desc(**over))) == UNSUPPORTED, over
    # a head's refusal before the workspace and the factor
    assert multi(lib, table(too_large), ws=None, inv=float("nan")) == TOO_LARGE
    # the workspace: the sum of the single entry's sizes
    two = table(good, desc(m=64 * 300 + 1, c_in=64, c_out=7, ldg=7))
    need = lib.pp_head_wgrad_multi_workspace_bytes(2, two)
    assert need == lib.pp_head_wgrad_workspace_bytes(64, 256, 50) + lib.pp_head_wgrad_workspace_bytes(64 * 300 + 1, 64, 7) > 0
    assert need % 4 == 0 and lib.pp_head_wgrad_workspace_bytes(64, 256, 50) % 4 == 0
    assert lib.pp_head_wgrad_multi_workspace_bytes(2, table(good, unsupported)) == UNSUPPORTED
    assert lib.pp_head_wgrad_multi_workspace_bytes(0, two) == BAD_ARG
    assert multi(lib, two, ws=None) == BAD_ARG and multi(lib, two, ws=A + 2) == BAD_ARG
    assert multi(lib, two, ws_bytes=need - 1) == BAD_ARG
    # the factor: a device pointer off a 4-byte boundary; without one, a host value that is not finite and positive
    assert multi(lib, two, ws_bytes=need, inv_dev=A + 2) == BAD_ARG
    for inv in (0.0, -1.0, float("inf"), float("nan")):
        assert multi(lib, two, ws_bytes=need, inv=inv) == BAD_ARG
    if not lib.pp_device_available():           # only then does a complete call end without launching
        assert multi(lib, two, ws_bytes=need) == NO_DEVICE
        assert multi(lib, two, ws_bytes=need, inv=float("nan"), inv_dev=A) == NO_DEVICE       # the host value is ignored


def update(lib, masters=A, grads=A, momentum=A, n=1000, table=A, n_heads=3, hyper=A, state=A, ws=A):
    p = C.c_void_p
    return lib.pp_head_update_f32(p(masters), p(grads), p(momentum), n, p(table), n_heads, p(hyper), p(state), p(ws), None)


def test_update_refusals_in_their_order(lib):
    for name in ("masters", "grads", "momentum", "table", "hyper", "state", "ws"):
        assert update(lib, **{name: None}) == BAD_ARG, name
    assert update(lib, n=0) == BAD_ARG and update(lib, n=-5) == BAD_ARG and update(lib, n_heads=-1) == BAD_ARG
    for name, off in (("masters", 2), ("grads", 1), ("momentum", 2), ("hyper", 2), ("ws", 2), ("table", 4), ("state", 4)):
        assert update(lib, **{name: A + off}) == BAD_ARG, name
        assert update(lib, n_heads=41, **{name: A + off}) == BAD_ARG, name          # alignment before the number of heads
    assert update(lib, n_heads=41) == UNSUPPORTED
    assert update(lib, n_heads=41, n=2 ** 31) == UNSUPPORTED
    assert update(lib, n=2 ** 31) == TOO_LARGE
    assert lib.pp_head_update_workspace_bytes(0) == BAD_ARG and lib.pp_head_update_workspace_bytes(2 ** 31) == TOO_LARGE
    assert lib.pp_head_update_workspace_bytes(1) == 4 and lib.pp_head_update_workspace_bytes(10 ** 7) == 4 * 256
    if not lib.pp_device_available():
        assert update(lib) == NO_DEVICE and update(lib, n_heads=40) == NO_DEVICE
