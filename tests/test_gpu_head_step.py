"""GPU: the captured head-training step -- pp_head_wgrad_multi_f16 against pp_head_wgrad_f16 bit for bit,
pp_head_update_f32 against torch.optim.SGD bit for bit and its loss-scale state against tests/head_step_reference.py, and
HeadTrainer(update="device", graph=True) against the same trainer eager and against today's path, step for step.

The network is the one of tests/test_gpu_head_train.py (2 stages, 2 x 64 x 64).  Nothing here has a tolerance: every comparison is of
bits.  The largest number of halvings test 6 has seen from 2^24 on this data is printed by the test.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import head_step_reference as hs
import head_wgrad_cases as hc
import head_wgrad_reference as ref
from conftest import PKG
from test_gpu_head_wgrad import DEV, Call

pytestmark = pytest.mark.gpu

BAD_ARG, TOO_LARGE, UNSUPPORTED = -2, -3, -6
P, G = hc.P_DEFAULT, hc.G_DEFAULT
T0 = time.perf_counter()


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().contiguous().cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def lib():
    from posepaf import _lib
    lib = _lib.load()
    assert lib.pp_head_wgrad_chunk_pixels() == P and lib.pp_head_wgrad_max_workgroups() == G
    yield lib
    torch.cuda.synchronize()
    print(f"\ntest_gpu_head_step.py: {time.perf_counter() - T0:.1f} s from import to the last test")


# ================================================================================================ 1, 2: multi against single

BIG = P * G + 17          # every workgroup of the head takes two chunks, the last chunk is ragged
INV = 2.0 ** -3           # a power of two: the small-integer results stay exact


def mixed_heads():
    """(recipe, m, hw, c_in, c_out, ldg, scaled): both c_in, three c_out, both pitches, gains and none, in one table; the
    (c_in, load) pairs are (256, 16-byte), (64, element), (64, 16-byte) and (256, element)"""
    return [("small", 1, 1, 256, 50, 64, False), ("small", P - 1, P - 1, 64, 1, 50, False), ("small", P, P, 256, 64, 64, True),
            ("small", P + 1, P + 1, 64, 50, 64, False), ("small", BIG, BIG, 256, 50, 50, False), ("small", 2 * P, P, 64, 50, 64, True),
            ("reals", 2 * P + 17, 2 * P + 17, 256, 50, 64, False), ("small", BIG, BIG, 64, 64, 64, False),
            ("small", P + 1, P + 1, 256, 1, 64, False)]


@pytest.fixture(scope="module")
def heads(lib):
    """[(spec, (g, x, scale) NumPy, Call, single (dw, db))]: the operands and pp_head_wgrad_f16's own result, computed once"""
    out = []
    for i, spec in enumerate(mixed_heads()):
        recipe, m, hw, c_in, c_out, ldg, scaled = spec
        g, x, scale = hc.RECIPES[recipe](np.random.default_rng(7000 + i), m, c_in, c_out, ldg, m // hw if scaled else None)
        assert np.isnan(g[:, c_out:]).all()                       # NaN in every padding channel of g
        call = Call(lib, g, x, scale, hw, c_out)
        out.append((spec, (g, x, scale), call, call.run(inv=INV)))
    return out


class Multi:
    """a table over Calls: their inputs and their guarded dw / db, one workspace filled with 0xFF before every launch"""

    def __init__(self, lib, calls):
        from posepaf import _lib
        self.lib, self.calls = lib, calls
        self.table = (_lib.HeadWgradDesc * len(calls))()
        for d, c in zip(self.table, calls):
            d.g, d.ldg, d.x, d.scale = c.g.data_ptr(), c.ldg, c.x.data_ptr(), None if c.scale is None else c.scale.data_ptr()
            d.m, d.hw, d.c_in, d.c_out, d.dw, d.db = c.m, c.hw, c.c_in, c.c_out, c.dw.data_ptr(), c.db.data_ptr()
        self.need = int(lib.pp_head_wgrad_multi_workspace_bytes(len(calls), self.table))
        assert self.need == sum(c.ws_bytes for c in calls)
        self.ws = torch.empty(self.need + 64, dtype=torch.uint8, device=DEV)

    def poison(self):
        self.ws.fill_(0xFF)
        for c in self.calls:
            c.poison()

    def launch(self, inv=INV, inv_dev=None, n=None, ws_bytes=None, ws_offset=0):
        return self.lib.pp_head_wgrad_multi_f16(len(self.calls) if n is None else n, self.table, inv, C.c_void_p(inv_dev),
                                                C.c_void_p(self.ws.data_ptr() + ws_offset), self.need if ws_bytes is None else ws_bytes,
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def run(self, **kw):
        self.poison()
        assert self.launch(**kw) == 0
        out = [c.results() for c in self.calls]                   # asserts the guards behind every dw / db
        assert bool((self.ws[self.need:] == 0xFF).all()), "bytes behind the workspace were written"
        return out

    def untouched(self):
        return all(c.untouched() for c in self.calls) and bool((self.ws == 0xFF).all())


@pytest.mark.parametrize("factor", ["host", "device"])
def test_multi_equals_single_bit_for_bit(lib, heads, factor):
    multi = Multi(lib, [h[2] for h in heads])
    pairs = {(c.c_in, c.g.data_ptr() % 16 == 0 and c.ldg % 8 == 0) for c in multi.calls}
    assert len(pairs) == 4                                        # every (c_in, load form) of the table is there: four accumulate launches
    if factor == "host":
        got = multi.run(inv=INV)
    else:
        inv_dev = torch.tensor([INV], dtype=torch.float32, device=DEV)
        got = multi.run(inv=-1.0, inv_dev=inv_dev.data_ptr())     # the host value is ignored
    for (spec, (g, x, scale), call, single), (dw, db) in zip(heads, got):
        assert same(dw, single[0]) and same(db, single[1]), spec
        if spec[0] == "small":
            want_dw, want_db = ref.head_wgrad(g, x, call.c_out, scale, call.hw, INV)
            assert same(dw, want_dw.astype(np.float32)) and same(db, want_db.astype(np.float32)), spec
        else:
            assert np.isfinite(dw).all() and np.abs(dw).max() > 0


def test_multi_one_head_and_forty_heads(lib, heads):
    spec, _, call, single = heads[4]                              # the two-chunks-per-workgroup head alone
    (dw, db), = Multi(lib, [call]).run()
    assert same(dw, single[0]) and same(db, single[1])
    assert lib.pp_head_wgrad_multi_max_heads() == 40
    _, x, _ = hc.small(np.random.default_rng(7100), 1, 64, 1, 1)  # the smallest shape: one pixel, one output channel
    g = np.ones((1, 1), np.float16)
    calls = [Call(lib, g * (1 + i % 3), x, None, 1, 1) for i in range(40)]
    singles = [c.run(inv=INV) for c in calls]
    for (dw, db), single in zip(Multi(lib, calls).run(), singles):
        assert same(dw, single[0]) and same(db, single[1])
    assert not same(singles[0][0], singles[1][0])


def test_multi_refusals_write_nothing(lib, heads):
    calls = [heads[0][2], heads[3][2]]
    multi = Multi(lib, calls)

    def refused(code, edit=None, **kw):
        keep = bytes(multi.table)
        if edit:
            edit(multi.table)
        multi.poison()
        rc = multi.launch(**kw)
        C.memmove(multi.table, keep, len(keep))
        torch.cuda.synchronize()
        assert rc == code and multi.untouched(), (code, rc, kw)

    refused(BAD_ARG, n=0)
    refused(UNSUPPORTED, n=41)
    refused(BAD_ARG, lambda t: setattr(t[1], "ldg", 49))
    refused(BAD_ARG, lambda t: setattr(t[1], "db", t[1].db + 2))
    refused(UNSUPPORTED, lambda t: setattr(t[1], "c_in", 100))
    refused(UNSUPPORTED, lambda t: setattr(t[0], "c_out", 0))
    refused(TOO_LARGE, lambda t: setattr(t[1], "m", 2 ** 31))
    refused(BAD_ARG, ws_bytes=multi.need - 1)
    refused(BAD_ARG, ws_offset=2)
    refused(BAD_ARG, inv=0.0)
    refused(BAD_ARG, inv=float("nan"))
    inv_dev = torch.tensor([INV, INV], dtype=torch.float32, device=DEV)
    refused(BAD_ARG, inv_dev=inv_dev.data_ptr() + 2)
    assert lib.pp_head_wgrad_multi_f16(2, None, INV, None, C.c_void_p(multi.ws.data_ptr()), multi.need, None) == BAD_ARG
    got = multi.run()                                             # and the untouched table still runs
    assert same(got[0][0], heads[0][3][0]) and same(got[1][1], heads[3][3][1])


# ================================================================================================ 3, 4: the update

SHAPES = [(1, 64), (50, 256), (7, 64)]        # (c_out, c_in) of three heads: 65 + 12850 + 455 = 13370 masters, 58 over a multiple of 64
N = sum(k * c + k for k, c in SHAPES)


class Update:
    """three heads' flat masters / gradients / momentum, their fp16 tensors (zero-padded 64-row copies included) and the blocks of
    pp_head_update_f32, filled from a seed"""

    def __init__(self, lib, lr, momentum, weight_decay, scale=2.0 ** 10, growth_interval=0, max_scale=hs.MAX_SCALE):
        from posepaf import _lib
        assert N % 64 == 58
        self.lib = lib
        rng = np.random.default_rng(11)
        self.masters = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).to(DEV)
        self.momentum = torch.zeros(N, dtype=torch.float32, device=DEV)
        self.grads = torch.zeros(N, dtype=torch.float32, device=DEV)
        self.hyper = torch.tensor([lr, momentum, weight_decay], dtype=torch.float32, device=DEV)
        self.state0 = hs.new_state(scale, growth_interval, max_scale=max_scale)
        st = np.zeros(1, _lib.HEAD_UPDATE_STATE_DTYPE)
        for k in hs.FIELDS:
            st[k] = self.state0[k]
        self.state = torch.from_numpy(st.view(np.uint8).copy()).to(DEV)
        self.ws = torch.empty(int(lib.pp_head_update_workspace_bytes(N)), dtype=torch.uint8, device=DEV).fill_(0xFF)
        table = (_lib.HeadUpdateDesc * len(SHAPES))()
        self.ranges, self.fp16, at = [], [], 0
        for d, (k, c) in zip(table, SHAPES):
            w = torch.full((k, c), 7.0, dtype=torch.float16, device=DEV)
            b = torch.full((k,), 7.0, dtype=torch.float16, device=DEV)
            wpad, bpad = torch.zeros((64, c), dtype=torch.float16, device=DEV), torch.zeros(64, dtype=torch.float16, device=DEV)
            wpad[:k], bpad[:k] = 7.0, 7.0
            d.w_off, d.w_len, d.b_off, d.b_len = at, k * c, at + k * c, k
            d.weight, d.bias, d.wpad, d.bpad = w.data_ptr(), b.data_ptr(), wpad.data_ptr(), bpad.data_ptr()
            self.ranges.append((at, k * c, at + k * c, k))
            self.fp16.append((w, b, wpad, bpad))
            at += k * c + k
        self.table = torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).to(DEV)
        self.ptrs = self.pointers()

    def pointers(self):
        return [t.data_ptr() for quad in self.fp16 for t in quad] + [self.masters.data_ptr(), self.momentum.data_ptr(), self.grads.data_ptr()]

    def new_grads(self, seed):
        """normal gradients with +0, -0 and subnormals of both signs among them"""
        rng = np.random.default_rng(seed)
        g = (rng.standard_normal(N) * 1e-2).astype(np.float32)
        special = np.array([0.0, -0.0, 1e-40, -1e-42, 1.4e-45, -1.4e-45], np.float32)
        where = rng.choice(N, 600, replace=False)
        g[where] = special[np.arange(600) % len(special)]
        self.grads.copy_(torch.from_numpy(g))

    def step(self):
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = self.lib.pp_head_update_f32(p(self.masters), p(self.grads), p(self.momentum), N, p(self.table), len(SHAPES), p(self.hyper),
                                         p(self.state), p(self.ws), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0

    def read_state(self):
        from posepaf import _lib
        st = self.state.cpu().numpy().view(_lib.HEAD_UPDATE_STATE_DTYPE)[0]
        return tuple(st[k].item() for k in hs.FIELDS)

    def snapshot(self):
        return [bits(self.masters), bits(self.momentum)] + [bits(t) for quad in self.fp16 for t in quad]

    def assert_copies(self):
        m = self.masters
        for (w_off, w_len, b_off, b_len), (w, b, wpad, bpad), (k, c) in zip(self.ranges, self.fp16, SHAPES):
            w16, b16 = m[w_off:w_off + w_len].half().view(k, c), m[b_off:b_off + b_len].half()
            assert same(w, w16) and same(b, b16) and same(wpad[:k], w16) and same(bpad[:k], b16)
            assert not wpad[k:].any() and not bpad[k:].any()      # the pad rows are never touched
        assert self.pointers() == self.ptrs


@pytest.mark.parametrize("weight_decay", [1e-4, 0.0])
@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_update_is_torch_sgd_bit_for_bit(lib, momentum, weight_decay):
    """three consecutive steps, so the momentum buffers are non-zero; the learning rate changes after the first.  The torch side is
    HeadTrainer's own arrangement: one SGD over views of flat tensors, the momentum buffers preset to zeros"""
    lr = 1e-2
    u = Update(lib, lr, momentum, weight_decay)
    p = torch.nn.Parameter(u.masters.clone())
    p.grad = torch.zeros_like(p)
    opt = torch.optim.SGD([p], lr=lr, momentum=momentum, weight_decay=weight_decay)
    if momentum:
        opt.state[p]["momentum_buffer"] = torch.zeros_like(p)
    for step in range(3):
        u.new_grads(100 + step)
        p.grad.copy_(u.grads)
        opt.step()
        u.step()
        assert same(u.masters, p), (step, int((u.masters != p.detach()).sum()))
        if momentum:
            assert same(u.momentum, opt.state[p]["momentum_buffer"]), step
            assert bool(u.momentum.any())
        else:
            assert not u.momentum.any()                           # torch's no-buffer form: never written
        u.assert_copies()
        if step == 0:                                             # what HeadTrainer.set_lr does
            u.hyper[0] = 3e-3
            opt.param_groups[0]["lr"] = 3e-3
    assert u.read_state() == hs.as_tuple(u.state0)                # static, nothing skipped: the block is as it was


@pytest.mark.parametrize("where", ["inf in the last db", "nan in the first dw"])
def test_nonfinite_gradient_skips_and_the_scale_follows_the_restatement(lib, where):
    u = Update(lib, 1e-2, 0.9, 1e-4, scale=2.0 ** 10, growth_interval=2, max_scale=2.0 ** 11)
    u.new_grads(200)
    u.step()                                                      # a finite step first: non-zero momentum
    state = hs.advance(u.state0, True)
    before = u.snapshot()
    u.new_grads(201)
    if where == "inf in the last db":
        u.grads[N - 1] = float("inf")
    else:
        u.grads[0] = float("nan")
    u.step()
    state = hs.advance(state, False)
    for a, b in zip(before, u.snapshot()):
        assert np.array_equal(a, b)                               # masters, momentum and every fp16 copy keep their bits
    assert u.read_state() == hs.as_tuple(state) and state["skipped"] == 1 and float(state["scale"]) == 2.0 ** 9
    scales = []
    for step in range(6):                                         # finite steps: doubles after every second one, stops at max_scale
        u.new_grads(210 + step)
        u.step()
        state = hs.advance(state, True)
        assert u.read_state() == hs.as_tuple(state), step
        scales.append(float(state["scale"]))
        u.assert_copies()
    assert scales == [2.0 ** 9, 2.0 ** 10, 2.0 ** 10, 2.0 ** 11, 2.0 ** 11, 2.0 ** 11]
    assert not np.array_equal(before[0], bits(u.masters))


# ================================================================================================ 5, 6, 8: the trainer

STAGES, B, H, W = 2, 2, 64, 64
LR = 1e-2


@pytest.fixture(scope="module")
def data():
    """the network and two batches (tests/test_gpu_head_train.py::data explains the flag); one forward of a throw-away trainer times
    the kernel candidates of these shapes, so that every trainer below runs the same kernels from its first step"""
    from posepaf import head_train, synth, synth_device
    from posepaf.model_init import build_network
    keep = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    net, _ = build_network("posenet", None, 7, nstack=STAGES)
    batches = []
    for j in range(2):
        rng = np.random.default_rng(1 + j)
        x = torch.from_numpy(rng.uniform(0.0, 1.0, (B, H, W, 3)).astype(np.float16)).to(DEV)
        people = [synth.random_people(1 + i + j, np.random.default_rng(20 + 10 * j + i), img_h=H, img_w=W) for i in range(B)]
        joints, n_people = synth_device.pack_joints(people, 4)
        target = synth_device.render_scenes(torch.from_numpy(joints).to(DEV), torch.from_numpy(n_people).to(DEV), H // 4, W // 4,
                                            dtype=torch.float16, flip=False, noise=0.0, reverse_kp=True)
        batches.append((x, target))
    head_train.HeadTrainer(net, DEV, lr=LR).gradients(*batches[0])
    yield dict(net=net, batches=batches)
    torch.backends.cudnn.deterministic = keep


def trainer_bits(tr):
    out = [bits(tr._flat), bits(tr._flat_buf)]
    for h in tr.heads.values():
        out += [bits(h.weight), bits(h.bias), bits(h.wpad), bits(h.bpad)]
    return out


def head_pointers(tr):
    return [(h.weight.data_ptr(), h.bias.data_ptr(), h.wpad.data_ptr(), h.bpad.data_ptr()) for h in tr.heads.values()]


def six_steps(tr, batches):
    """six steps over two alternating batches, set_lr after the third -> per step (tensor bits, loss bits, skipped_steps)"""
    out, ptrs = [], head_pointers(tr)           # from construction on
    for step in range(6):
        loss = tr.step(*batches[step % 2])
        assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.is_cuda
        out.append((trainer_bits(tr), bits(loss), int(tr.skipped_steps)))
        assert head_pointers(tr) == ptrs, step
        if step == 2:
            tr.set_lr(LR / 2)
    return out


@pytest.fixture(scope="module")
def todays_path(data):
    from posepaf import head_train
    return six_steps(head_train.HeadTrainer(data["net"], DEV, lr=LR, update="torch", wgrad="device"), data["batches"])


@pytest.mark.parametrize("wgrad", ["multi", "device"])
def test_graph_equals_eager_equals_todays_path(data, todays_path, wgrad):
    from posepaf import head_train
    eager = head_train.HeadTrainer(data["net"], DEV, lr=LR, update="device", wgrad=wgrad)
    graphed = head_train.HeadTrainer(data["net"], DEV, lr=LR, update="device", wgrad=wgrad, graph=True)
    want, got = six_steps(eager, data["batches"]), six_steps(graphed, data["batches"])
    assert graphed.graph_replays >= 4 and eager.graph_replays == 0
    for step in range(6):
        for name, other in (("graph", got), ("today's path", todays_path)):
            assert other[step][2] == want[step][2] == 0, (name, step)
            assert np.array_equal(other[step][1], want[step][1]), (name, step, "loss")
            assert len(other[step][0]) == len(want[step][0]) == 2 + 4 * 5 * STAGES
            for i, (a, b) in enumerate(zip(other[step][0], want[step][0])):
                assert np.array_equal(a, b), (name, step, i)
    assert not np.array_equal(want[0][0][0], want[5][0][0]) and not np.array_equal(want[4][1], want[5][1])
    g2, ldg, x2, scale = graphed.last_inputs[(0, 0)]              # the graph's own tensors
    assert x2.shape == (B * 16 * 16, 256)


def test_replay_after_the_eager_entries_took_a_larger_workspace(data):
    """a captured graph holds the ADDRESS of the weight gradients' workspace.  The entries that stay eager next to the graph need a
    larger one -- gradients_from_last("multi") on a wgrad="device" trainer (the sum of the heads' sizes against their maximum) and
    gradients() on twice the batch -- and replace it; the graph's own must stay alive, or the next replay writes every head's partial
    sums into memory the allocator has handed to someone else.  Tensors of the old workspace's size are allocated in between and
    must keep their fill; the steps after must equal the eager trainer's bit for bit"""
    from posepaf import head_train
    b0, b1 = data["batches"]
    big = (torch.cat([b0[0], b1[0]]), torch.cat([b0[1], b1[1]]))
    eager = head_train.HeadTrainer(data["net"], DEV, lr=LR, update="device", wgrad="device")
    graphed = head_train.HeadTrainer(data["net"], DEV, lr=LR, update="device", wgrad="device", graph=True)
    for tr in (eager, graphed):
        tr.step(*b0), tr.step(*b1)                # graphed: eager, then capture + replay
    assert graphed.graph_replays == 1
    captured = graphed._workspace
    size, address = captured.numel(), captured.data_ptr()
    graphed.gradients_from_last("multi")
    assert graphed._workspace.numel() > size and graphed._workspace.data_ptr() != address
    middle = graphed._workspace.numel()
    graphed.gradients(*big)                       # another shape on the eager entry, between the replays
    assert graphed._workspace.numel() >= middle
    del captured
    others = [torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV) for n in (size, size, size // 2, size // 2, middle, 4 * size)]
    assert address not in [t.data_ptr() for t in others]          # the graph's workspace was not handed out again
    for step in range(4):
        a, b = eager.step(*data["batches"][step % 2]), graphed.step(*data["batches"][step % 2])
        assert np.array_equal(bits(a), bits(b)), step
        for i, (u, v) in enumerate(zip(trainer_bits(eager), trainer_bits(graphed))):
            assert np.array_equal(u, v), (step, i)
    assert graphed.graph_replays == 5
    torch.cuda.synchronize()
    assert all(bool((t == 0x5A).all()) for t in others)
    # a second, larger signature gets its own graph (and its own pinned workspace); the first one still replays the same bits
    for _ in range(2):
        eager.step(*big), graphed.step(*big)
    a, b = eager.step(*b0), graphed.step(*b0)
    assert graphed.graph_replays == 7 and len(graphed._graphs) == 2 and np.array_equal(bits(a), bits(b))
    for i, (u, v) in enumerate(zip(trainer_bits(eager), trainer_bits(graphed))):
        assert np.array_equal(u, v), i


def test_dynamic_scale_from_the_first_batch_with_the_torch_gradient(data):
    """loss_scale="dynamic" without init_scale starts at auto_loss_scale of the first batch, and wgrad="torch" multiplies by the device
    factor: one step equals the static trainer's with the same formulation, bit for bit"""
    from posepaf import head_train
    x, target = data["batches"][0]
    dyn = head_train.HeadTrainer(data["net"], DEV, lr=LR, update="device", wgrad="torch", loss_scale="dynamic")
    from posepaf._lib import PosePafError
    with pytest.raises(PosePafError):
        dyn.loss_scale_now()                      # no batch yet
    static = head_train.HeadTrainer(data["net"], DEV, lr=LR, wgrad="torch")
    a, b = dyn.step(x, target), static.step(x, target)
    assert float(dyn.loss_scale_now()) == static.loss_scale_for(B) == ref.auto_loss_scale(B, STAGES)
    assert int(dyn.skipped_steps) == 0 and np.array_equal(bits(a), bits(b))
    for i, (u, v) in enumerate(zip(trainer_bits(dyn), trainer_bits(static))):
        assert np.array_equal(u, v), i


def test_dynamic_scale_inside_the_graph(data):
    from posepaf import head_train
    x, target = data["batches"][0]
    tr = head_train.HeadTrainer(data["net"], DEV, lr=LR, update="device", wgrad="multi", loss_scale="dynamic", init_scale=2 ** 24, graph=True)
    assert float(tr.loss_scale_now()) == 2.0 ** 24
    start = trainer_bits(tr)
    k = None
    for step in range(30):
        before = int(tr.skipped_steps)
        tr.step(x, target)
        if int(tr.skipped_steps) == before:
            k = before
            break
        for a, b in zip(start, trainer_bits(tr)):
            assert np.array_equal(a, b), step                     # a skipped step leaves everything
    print(f"2^24 was halved k = {k} times before the first step that was not skipped; graph_replays = {tr.graph_replays}")
    assert k is not None and k >= 1
    assert float(tr.loss_scale_now()) == 2.0 ** 24 / 2.0 ** k
    assert tr.graph_replays == k                                  # k + 1 steps, all but the eager first one were replays
    fresh = head_train.HeadTrainer(data["net"], DEV, lr=LR, loss_scale=2.0 ** 24 / 2.0 ** k)
    fresh.step(x, target)
    assert int(fresh.skipped_steps) == 0
    for i, (a, b) in enumerate(zip(trainer_bits(tr), trainer_bits(fresh))):
        assert np.array_equal(a, b), i
    assert not np.array_equal(start[0], bits(tr._flat))


def test_refused_combinations_and_bad_arguments(data):
    from posepaf import head_train
    from posepaf._lib import PosePafError
    for kw in (dict(graph=True, update="torch"), dict(graph=True), dict(loss_scale="dynamic", wgrad="device", update="device"),
               dict(loss_scale="dynamic", update="torch", wgrad="multi"), dict(loss_scale="dynamic"),
               dict(growth_interval=-1), dict(growth_interval=1.5), dict(init_scale=3), dict(init_scale=0), dict(update="hip"),
               dict(wgrad="many")):
        with pytest.raises(PosePafError):
            head_train.HeadTrainer(data["net"], DEV, **kw)
    tr = head_train.HeadTrainer(data["net"], DEV, update="device", wgrad="multi", loss_scale="dynamic")
    with pytest.raises(PosePafError):
        tr.loss_scale_for(B)
    with pytest.raises(PosePafError):
        tr.set_lr(0.0)


# ================================================================================================ 7: finetune.py

FINETUNE = ["--model", "fused", "--train", "heads", "--update", "device", "--synthetic", "4", "--batch", "2", "--sizes", "64x64", "--stages", "2",
            "--steps", "6", "--lr", "5e-3"]


def run_finetune(cache, *extra):
    env = dict(os.environ, POSEPAF_CACHE_DIR=str(cache))
    r = subprocess.run([sys.executable, os.path.join(PKG, "finetune.py"), *FINETUNE, *extra], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_finetune_with_and_without_graph(tmp_path):
    cache = tmp_path / "cache"
    eager = run_finetune(cache)
    graphed = run_finetune(cache, "--graph")
    print("eager  ", eager["losses"], eager["steps_per_s"])
    print("graphed", graphed["losses"], graphed["steps_per_s"])
    assert eager["losses"] == graphed["losses"] and len(eager["losses"]) == 6 and all(np.isfinite(v) for v in eager["losses"])
    assert graphed["graph"] is True and graphed["graph_replays"] >= 4 and graphed["update"] == "device"
    assert eager["graph"] is False and eager["graph_replays"] == 0 and eager["update"] == "device"
    for res in (eager, graphed):
        assert res["skipped_steps"] == 0 and res["loss_scale_last"] == res["loss_scale"] == ref.auto_loss_scale(2, 2)
        assert res["steps_per_s"] > 0 and res["loss_last"] < res["loss_first"]
