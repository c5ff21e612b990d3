"""GPU: pp_layer_update_f32 (csrc/posepaf_headopt.hip) -- pp_head_update_f32's chain with a table of single segments.  On a table both
entries can express the two give the same bits (masters, momentum, binary16 copies, state block) and both equal torch.optim.SGD; a
240-segment table, the skipped step and the refusals are checked on the new entry alone.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import head_step_reference as hs
from test_gpu_head_step import DEV, N, SHAPES, Update, bits, same

pytestmark = pytest.mark.gpu

BAD_ARG, TOO_LARGE, UNSUPPORTED = -2, -3, -6


@pytest.fixture(scope="module")
def lib():
    from posepaf import _lib
    return _lib.load()


def segment_table(entries):
    """a device pp_update_segment array from (off, len, dst tensor, dst2 tensor)"""
    from posepaf import _lib
    table = (_lib.UpdateSegment * max(1, len(entries)))()
    for d, (off, n, dst, dst2) in zip(table, entries):
        d.off, d.len, d.dst, d.dst2 = off, n, dst.data_ptr(), dst2.data_ptr()
    return torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).to(DEV)


class LayerUpdate(Update):
    """the three heads of test_gpu_head_step.Update as six segments: (weight, wpad) and (bias, bpad) of each"""

    def __init__(self, lib, *args, **kw):
        super().__init__(lib, *args, **kw)
        entries = []
        for (w_off, w_len, b_off, b_len), (w, b, wpad, bpad) in zip(self.ranges, self.fp16):
            entries += [(w_off, w_len, w, wpad), (b_off, b_len, b, bpad)]
        self.segments, self.n_segments = segment_table(entries), len(entries)

    def step(self):
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = self.lib.pp_layer_update_f32(p(self.masters), p(self.grads), p(self.momentum), N, p(self.segments), self.n_segments, p(self.hyper),
                                          p(self.state), p(self.ws), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0


@pytest.mark.parametrize("weight_decay", [1e-4, 0.0])
@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_both_entries_and_torch_sgd_bit_for_bit(lib, momentum, weight_decay):
    """three consecutive steps, the learning rate changes after the first"""
    lr = 1e-2
    new, old = LayerUpdate(lib, lr, momentum, weight_decay), Update(lib, lr, momentum, weight_decay)
    p = torch.nn.Parameter(new.masters.clone())
    p.grad = torch.zeros_like(p)
    opt = torch.optim.SGD([p], lr=lr, momentum=momentum, weight_decay=weight_decay)
    if momentum:
        opt.state[p]["momentum_buffer"] = torch.zeros_like(p)
    for step in range(3):
        for u in (new, old):
            u.new_grads(100 + step)
            u.step()
        p.grad.copy_(new.grads)
        opt.step()
        for a, b in zip(new.snapshot(), old.snapshot()):
            assert np.array_equal(a, b), step
        assert new.read_state() == old.read_state()
        assert same(new.masters, p), (step, int((new.masters != p.detach()).sum()))
        if momentum:
            assert same(new.momentum, opt.state[p]["momentum_buffer"]) and bool(new.momentum.any()), step
        else:
            assert not new.momentum.any()
        new.assert_copies()
        if step == 0:
            for u in (new, old):
                u.hyper[0] = 3e-3
            opt.param_groups[0]["lr"] = 3e-3
    assert new.read_state() == hs.as_tuple(new.state0)


@pytest.mark.parametrize("where", ["inf in the last element", "nan in the first element"])
def test_nonfinite_gradient_skips_and_halves_a_dynamic_scale(lib, where):
    u = LayerUpdate(lib, 1e-2, 0.9, 1e-4, scale=2.0 ** 10, growth_interval=2, max_scale=2.0 ** 11)
    u.new_grads(200)
    u.step()
    state = hs.advance(u.state0, True)
    before = u.snapshot()
    u.new_grads(201)
    if where == "inf in the last element":
        u.grads[N - 1] = float("inf")
    else:
        u.grads[0] = float("nan")
    u.step()
    state = hs.advance(state, False)
    for a, b in zip(before, u.snapshot()):
        assert np.array_equal(a, b)
    assert u.read_state() == hs.as_tuple(state) and state["skipped"] == 1 and float(state["scale"]) == 2.0 ** 9
    u.new_grads(202)
    u.step()
    assert u.read_state() == hs.as_tuple(hs.advance(state, True)) and not np.array_equal(before[0], bits(u.masters))
    u.assert_copies()


def test_240_segments(lib):
    """8 stacks x 5 scales x 3 layers x (weight, bias): ragged lengths, gaps between some segments, dst2 == dst on every second one"""
    from posepaf import _lib
    n_seg = 240
    assert n_seg <= lib.pp_layer_update_max_segments()
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 90, n_seg)
    gaps = np.where(np.arange(n_seg) % 7 == 3, rng.integers(1, 5, n_seg), 0)
    offs = np.cumsum(np.concatenate([[2], lens[:-1] + gaps[:-1]]))
    n = int(offs[-1] + lens[-1] + 3)
    masters = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)
    grads = torch.from_numpy((rng.standard_normal(n) * 1e-2).astype(np.float32)).to(DEV)
    momentum = torch.zeros(n, dtype=torch.float32, device=DEV)
    entries, copies = [], []
    for i in range(n_seg):
        a = torch.full((int(lens[i]) + 8,), 7.0, dtype=torch.float16, device=DEV)
        b = a if i % 2 else torch.full((int(lens[i]) + 8,), 7.0, dtype=torch.float16, device=DEV)
        entries.append((int(offs[i]), int(lens[i]), a, b))
        copies.append((a, b))
    table = segment_table(entries)
    hyper = torch.tensor([1e-2, 0.9, 1e-4], dtype=torch.float32, device=DEV)
    st = np.zeros(1, _lib.HEAD_UPDATE_STATE_DTYPE)
    state0 = hs.new_state(2.0 ** 10, 0)
    for k in hs.FIELDS:
        st[k] = state0[k]
    state = torch.from_numpy(st.view(np.uint8).copy()).to(DEV)
    ws = torch.empty(int(lib.pp_head_update_workspace_bytes(n)), dtype=torch.uint8, device=DEV).fill_(0xFF)
    p = torch.nn.Parameter(masters.clone())
    p.grad = grads.clone()
    opt = torch.optim.SGD([p], lr=1e-2, momentum=0.9, weight_decay=1e-4)
    opt.state[p]["momentum_buffer"] = torch.zeros_like(p)
    opt.step()
    q = lambda t: C.c_void_p(t.data_ptr())
    assert lib.pp_layer_update_f32(q(masters), q(grads), q(momentum), n, q(table), n_seg, q(hyper), q(state), q(ws),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    assert same(masters, p) and same(momentum, opt.state[p]["momentum_buffer"])
    h = masters.half()
    for (off, ln, _, _), (a, b) in zip(entries, copies):
        for t in (a, b):
            assert same(t[:ln], h[off:off + ln]) and bool((t[ln:] == 7.0).all())      # nothing behind a segment's length is written


def test_refusals(lib):
    u = LayerUpdate(lib, 1e-2, 0.9, 1e-4)
    u.new_grads(300)
    before, state = u.snapshot(), u.read_state()
    names = ("masters", "grads", "momentum", "n", "segments", "n_segments", "hyper", "state", "workspace")
    base = dict(masters=u.masters.data_ptr(), grads=u.grads.data_ptr(), momentum=u.momentum.data_ptr(), n=N, segments=u.segments.data_ptr(),
                n_segments=u.n_segments, hyper=u.hyper.data_ptr(), state=u.state.data_ptr(), workspace=u.ws.data_ptr())

    def call(**over):
        v = dict(base)
        v.update(over)
        args = [v[k] if k in ("n", "n_segments") else C.c_void_p(v[k]) for k in names]
        return lib.pp_layer_update_f32(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for k in names:
        if k not in ("n", "n_segments"):
            assert call(**{k: None, "n": 0}) == BAD_ARG, k
    assert call(n=0, n_segments=300) == BAD_ARG and call(n=-1, n_segments=300) == BAD_ARG
    assert call(n_segments=-1, masters=base["masters"] + 2) == BAD_ARG
    for k, off in (("masters", 2), ("grads", 1), ("momentum", 2), ("hyper", 2), ("workspace", 2), ("segments", 4), ("state", 4)):
        assert call(**{k: base[k] + off, "n_segments": 300}) == BAD_ARG, k
    assert call(n_segments=lib.pp_layer_update_max_segments() + 1, n=2 ** 31) == UNSUPPORTED
    assert call(n=2 ** 31) == TOO_LARGE
    torch.cuda.synchronize()
    for a, b in zip(before, u.snapshot()):
        assert np.array_equal(a, b)
    assert u.read_state() == state
    assert len(SHAPES) * 2 == u.n_segments
