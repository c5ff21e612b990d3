"""CPU: the per-shape tuning protocol of posepaf/fused_model.py -- the chooser of the five fused forms (_choose), the form
methods that call it (key tuples, choice encodings, fall-back to the separate form) and FConv._tune's own selection rule.
Nothing here touches a device: fm._timed is replaced by a scripted clock, fm._capturing by a constant, and the kernels of a
form by stubs; the separate forms run for real on host tensors (the torch path of the module)."""
import types

import pytest
import torch

from posepaf import fused_model as fm


class Clock:
    """Stands in for fm._timed.  It runs the thunk once and charges the milliseconds scripted for the stub that ran; a thunk
    that reaches no stub is the separate form of a layer.  log: ("run", name) per stub call, ("timed", name) per timing."""

    def __init__(self, ms=None):
        self.ms, self.log, self.last = dict(ms or {}), [], None

    def ran(self, name):
        self.log.append(("run", name))
        self.last = name

    def thunk(self, name, result=True):
        def fn():
            self.ran(name)
            return name if result is True else result
        return fn

    def __call__(self, fn):
        self.last = "separate"
        fn()
        self.log.append(("timed", self.last))
        return self.ms[self.last]

    @property
    def timed(self):
        return [name for kind, name in self.log if kind == "timed"]

    def runs(self, name):
        return self.log.count(("run", name))


@pytest.fixture
def tuner(monkeypatch):
    """fresh tables, a scripted clock, no capture, the progress lines collected"""
    t = types.SimpleNamespace(clock=Clock(), notes=[], capturing=False)
    monkeypatch.setattr(fm, "_conv_choice", {})
    monkeypatch.setattr(fm, "_conv_timing", {})
    monkeypatch.setattr(fm, "_conv_calls", {})
    monkeypatch.setattr(fm, "_timed", t.clock)
    monkeypatch.setattr(fm, "_capturing", lambda: t.capturing)
    monkeypatch.setattr(fm, "_progress", t.notes.append)
    return t


def _candidates(clock, *names, refuse=()):
    return [(i, name, clock.thunk(name, None if name in refuse else True)) for i, name in enumerate(names)]


# ---------------------------------------------------------------------------------------------------- the chooser
def test_chooser_keeps_the_strictly_fastest_and_a_tie_keeps_the_earlier(tuner):
    tuner.clock.ms = {"separate": 2.0, "a": 1.0, "b": 1.0, "c": 1.5}
    assert fm._choose(("k", 1), True, _candidates(tuner.clock, "separate", "a", "b", "c")) == 1
    assert fm._conv_choice == {("k", 1): 1}
    assert fm._conv_timing == {("k", 1): {"separate": 2.0, "a": 1.0, "b": 1.0, "c": 1.5}}
    tuner.clock.ms = {"separate": 1.0, "a": 1.0}
    assert fm._choose(("k", 2), True, _candidates(tuner.clock, "separate", "a")) == 0
    tuner.clock.ms = {"separate": 1.0, "a": 2.0, "b": 0.5}
    assert fm._choose(("k", 3), True, _candidates(tuner.clock, "separate", "a", "b")) == 2
    assert len(tuner.notes) == 3 and all(f"('k', {i + 1})" in line for i, line in enumerate(tuner.notes))


def test_chooser_neither_times_nor_chooses_a_candidate_that_refuses(tuner):
    tuner.clock.ms = {"separate": 2.0, "a": 0.1, "b": 1.0}
    assert fm._choose(("k",), True, _candidates(tuner.clock, "separate", "a", "b", refuse=("a",))) == 2
    assert tuner.clock.timed == ["separate", "b"] and tuner.clock.runs("a") == 1      # the probe call alone
    assert "a" not in fm._conv_timing[("k",)]
    tuner.clock.ms = {"separate": 2.0}
    assert fm._choose(("only",), True, _candidates(tuner.clock, "separate", "a", refuse=("a",))) == 0
    assert fm._conv_choice[("only",)] == 0 and fm._conv_timing.get(("only",), {}).keys() <= {"separate"}


def test_chooser_runs_the_separate_form_once_before_the_first_timing(tuner):
    tuner.clock.ms = {"separate": 1.0, "a": 2.0}
    fm._choose(("k",), True, _candidates(tuner.clock, "separate", "a"))
    first = [kind for kind, _ in tuner.clock.log].index("timed")
    before = tuner.clock.log[:first]                     # the untimed run, then the clock's own call of the thunk it times
    assert before[0] == ("run", "separate") and before.count(("run", "separate")) == 1 + (tuner.clock.timed[0] == "separate")
    assert all(name == "separate" for _, name in before)


def test_chooser_table_hit_capture_and_ineligible_shapes(tuner):
    cands = _candidates(tuner.clock, "separate", "a")
    fm._conv_choice[("hit",)] = 7
    assert fm._choose(("hit",), True, cands) == 7
    assert tuner.clock.log == [] and fm._conv_timing == {} and tuner.notes == []       # a table hit times and runs nothing
    tuner.capturing = True
    assert fm._choose(("cap",), True, cands) == 0                                       # the caller then runs the separate form
    assert tuner.clock.log == [] and ("cap",) not in fm._conv_choice and ("cap",) not in fm._conv_timing
    tuner.capturing = False

    class Untouchable(dict):
        def get(self, *a):
            raise AssertionError("an ineligible shape must not be looked up")
    fm._conv_choice = Untouchable()
    assert fm._choose(("no",), False, cands) == 0
    assert tuner.clock.log == [] and len(fm._conv_choice) == 0 and fm._conv_timing == {} and tuner.notes == []


def test_chooser_writes_into_the_tables_bound_at_call_time(tuner):
    saved = (fm._conv_choice, fm._conv_timing)
    tuner.clock.ms = {"separate": 2.0, "a": 1.0}
    try:
        fm._conv_choice, fm._conv_timing = {}, {}
        fresh = (fm._conv_choice, fm._conv_timing)
        assert fm._choose(("k",), True, _candidates(tuner.clock, "separate", "a")) == 1
        assert fresh[0] == {("k",): 1} and ("k",) in fresh[1] and saved == ({}, {})
    finally:
        fm._conv_choice, fm._conv_timing = saved
    assert len(tuner.notes) == 1


def test_table_entries_install_back_exactly_with_or_without_json(tuner):
    import json
    table = {("up2", 2, 8, 4, 4, 8, False, True): 3, (2, 8, 4, 4, 8, 3, 1, 1, 0, True, "slice", 16, 8): -1,
             ("dual", 2, 8, 4, 4, 8, 1, 0, 1, False, True, True, "nores"): fm.PW_VARIANT}
    fm._conv_choice.update(table)
    entries = fm.table_entries()
    for form in (entries, json.loads(json.dumps(entries))):        # as broadcast between ranks, and as saved to a file
        fm._conv_choice = {}
        assert fm.install_entries(form) == len(table) and fm._conv_choice == table
        assert fm.install_entries(form) == 0                        # existing keys keep their choice
        assert all(type(v) is type(w) for k in fm._conv_choice for v, w in zip(k, next(t for t in table if t == k)))


# ---------------------------------------------------------------------------------------------------- the five forms
def _conv(cin, cout, r, act=True, seed=0):
    torch.manual_seed(seed)
    return fm.FConv(torch.nn.Conv2d(cin, cout, r, 1, r // 2, bias=True), None, act)


def _same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return len(a) == len(b) and all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def test_up2_key_encoding_and_fallback(tuner):
    f = _conv(8, 8, 3)
    low, post = torch.randn(1, 8, 4, 4), torch.randn(1, 8, 8, 8)
    want = f(fm.upsample2(low), post=post)
    names = {1: "fused", 2: "collapsed256", 3: "collapsed128", 4: "collapsed64", 5: "collapsed512"}
    refuse = set()

    def run(choice):
        tuner.clock.ran(names[choice])
        return None if choice in refuse else names[choice]
    f._up2_fused = lambda low, post, post2: run
    key = ("up2", 1, 8, 4, 4, 8, False, True)
    tuner.clock.ms = {"separate": 3.0, "fused": 2.0, "collapsed256": 2.5, "collapsed128": 1.0, "collapsed64": 1.0, "collapsed512": 4.0}
    assert f.forward_up2(low, post) == "collapsed128"
    assert fm._conv_choice == {key: 3}                                   # 2 + the index into (256, 128, 64, 512)
    assert list(fm._conv_timing[key]) == ["separate", "fused", "collapsed256", "collapsed128", "collapsed64", "collapsed512"]
    fm._conv_choice[key] = 1
    assert f.forward_up2(low, post) == "fused"
    for choice in (1, 3):                                                # an installed choice whose kernel refuses the shape
        fm._conv_choice[key] = choice
        refuse.add(choice)
        assert _same(f.forward_up2(low, post), want)
    fm._conv_choice.clear()
    tuner.capturing, before = True, len(tuner.clock.log)                 # a new shape inside a capture: the separate form, untimed
    assert _same(f.forward_up2(low, post), want) and fm._conv_choice == {} and len(tuner.clock.log) == before
    tuner.capturing = False
    f._up2_fused = lambda low, post, post2: None                         # not eligible: nothing looked up or recorded
    assert _same(f.forward_up2(low, post), want) and fm._conv_choice == {} and len(tuner.notes) == 1


def test_dual_key_encoding_and_fallback(tuner):
    f = _conv(8, 128, 1, act=False)
    x, res, other = torch.randn(1, 8, 4, 4), torch.randn(1, 128, 4, 4), torch.randn(1, 128, 4, 4)
    y = f(x, res)
    want = (y, y + other)
    refuse = {256}

    def run(bn):
        tuner.clock.ran(bn)
        return None if bn in refuse else bn
    f._dual_fused = lambda *a: run
    key = ("dual", 1, 8, 4, 4, 128, 1, 0, 1, False, False, False)
    tuner.clock.ms = {"separate": 3.0, 128: 2.0, 64: 2.0, 512: 2.5, fm.PW_VARIANT: 2.0}
    assert f.forward_dual(x, res, other) == 128                          # 256 does not divide 128 channels: never tried
    assert fm._conv_choice == {key: 128} and tuner.clock.runs(256) == 0
    assert list(fm._conv_timing[key]) == ["separate", 128, 64, 512, fm.PW_VARIANT]
    tuner.clock.ms[fm.PW_VARIANT] = 1.0
    assert f.forward_dual(x, None, other) == fm.PW_VARIANT               # the key without a residual is another shape
    assert fm._conv_choice[key + ("nores",)] == fm.PW_VARIANT
    fm._conv_choice[key] = 256
    assert _same(f.forward_dual(x, res, other), want) and tuner.clock.runs(256) == 1
    fm._conv_choice[key] = 0
    assert _same(f.forward_dual(x, res, other), want) and tuner.clock.runs(256) == 1
    assert len(tuner.notes) == 2


@pytest.mark.parametrize("form", ["mean", "pool"])
def test_mean_and_pool_key_encoding_and_fallback(tuner, form):
    f = _conv(8, 16, 3 if form == "mean" else 1)
    x = torch.randn(1, 8, 4, 4)
    y = f(x)
    if form == "mean":
        key, want, call, hook = ("mean", 1, 8, 4, 4, 16, True), (y, y.mean(dim=(2, 3))), lambda: f.forward_mean(x, partial=True), "_mean_fused"
    else:
        key, want, call, hook = ("pool", 1, 8, 4, 4, 16, False, True), (y, torch.nn.functional.max_pool2d(y, 2, 2)), lambda: f.forward_pool(x), "_pool_fused"
    seen, refuse = [], []

    def run(*args):
        tuner.clock.ran("fused")
        seen.append(args)
        return None if refuse else "fused"
    setattr(f, hook, lambda *a: run)
    tuner.clock.ms = {"separate": 2.0, "fused": 1.0}
    assert call() == "fused" and fm._conv_choice == {key: 1}
    assert fm._conv_timing[key] == {"separate": 2.0, "fused": 1.0}
    if form == "mean":   # the timing runs the whole fused form (the mean finished); the dispatch hands the partial sums over
        assert seen[-1] == (True,) and all(a in ((), (False,)) for a in seen[:-1])
    refuse.append(True)
    assert _same(call(), want)                                           # installed 1, the kernel refuses
    fm._conv_choice.clear()
    tuner.clock.ms = {"separate": 2.0, "fused": 2.0}
    refuse.clear()
    assert _same(call(), want) and fm._conv_choice == {key: 0}            # a tie keeps the separate form
    assert len(tuner.notes) == 2


def test_cat_key_encoding_and_fallback(tuner):
    from models.layers_transposed import Residual
    torch.manual_seed(1)
    r = fm.FResidual(Residual(32, 64).eval())
    x = torch.randn(1, 32, 4, 4)
    want = r.c3(r.c2(r.c1(x)), r.skip.conv_only(x))
    refuse = []

    def run():
        tuner.clock.ran("fused")
        return None if refuse else ("fused", None)
    r._cat_fused = lambda *a: run
    key = ("cat", 1, 32, 32, 4, 4, 64, True, False)
    tuner.clock.ms = {"separate": 2.0, "fused": 1.0}
    assert r(x) == "fused" and fm._conv_choice == {key: 1}
    assert fm._conv_timing[key] == {"separate": 2.0, "fused": 1.0}
    refuse.append(True)
    assert _same(r(x), want)                                             # installed 1, the kernel refuses: the block's own path
    tuner.capturing = True
    fm._conv_choice.clear()
    assert _same(r(x), want) and fm._conv_choice == {}                    # no timing inside a capture, nothing recorded
    tuner.capturing = False
    r._cat_fused = lambda *a: None                                       # preconditions fail: no key exists
    assert _same(r(x), want) and fm._conv_choice == {} and len(tuner.notes) == 1


# ---------------------------------------------------------------------------------------------------- FConv._tune
def _tune(tuner, monkeypatch, ms, runs, templates=2, tune_miopen=False):
    """FConv._tune of a 1x1 layer whose library has `templates` template configurations and every hand-written kernel;
    `runs`: the configuration ids that accept the shape.  -> (choice, timing labels in the order they were taken)"""
    from posepaf import _lib
    f = _conv(8, 16, 1)
    f._fused_launch = lambda cfg, x, extra, mode, y: (tuner.clock.ran(cfg), 0 if cfg in runs else -6)[1]
    monkeypatch.setattr(_lib, "load", lambda: types.SimpleNamespace(
        pp_conv_num_configs=lambda: templates, pp_conv_own_supported=lambda c, k, r: 1, pp_pw_supported=lambda c, k: 1))
    monkeypatch.setattr(fm, "hip_bias_act_", lambda y, *a: (tuner.clock.ran("miopen"), y)[1])
    monkeypatch.setattr(fm, "TUNE_MIOPEN", tune_miopen)
    tuner.clock.ms, tuner.clock.log = ms, []
    x = torch.zeros(1, 8, 4, 4)
    key = ("plain", len(fm._conv_choice))
    choice = f._tune(key, x, None, 0, torch.zeros(1, 16, 4, 4), None, None)
    assert fm._conv_choice[key] == choice and list(fm._conv_timing[key]) == tuner.clock.timed
    assert tuner.notes[-1].endswith(f"-> {choice}")
    return choice, tuner.clock.timed


def test_tune_prefers_a_hand_written_kernel_inside_the_margin_of_the_best_template(tuner, monkeypatch):
    assert fm.OWN_MARGIN == 0.03
    choice, timed = _tune(tuner, monkeypatch, {0: 1.00, 1: 1.10, 101: 1.02}, {0, 1, 101})
    assert choice == 101 and timed == [0, 1, 101]                        # templates first, then the ids >= 100; no MIOpen timing
    assert _tune(tuner, monkeypatch, {0: 1.00, 1: 1.10, 101: 1.04}, {0, 1, 101})[0] == 0        # beyond the margin
    assert _tune(tuner, monkeypatch, {0: 1.10, 1: 1.00, 105: 1.02}, {0, 1, 105})[0] == fm.PW_VARIANT
    assert len(tuner.notes) == 3


def test_tune_between_two_hand_written_kernels_only_the_strictly_faster_wins(tuner, monkeypatch):
    assert _tune(tuner, monkeypatch, {0: 2.0, 101: 1.00, 102: 1.00}, {0, 101, 102})[0] == 101
    assert _tune(tuner, monkeypatch, {0: 2.0, 101: 1.00, 102: 1.02}, {0, 101, 102})[0] == 101   # no margin among themselves
    assert _tune(tuner, monkeypatch, {0: 2.0, 101: 1.00, 102: 0.99}, {0, 101, 102})[0] == 102
    assert _tune(tuner, monkeypatch, {0: 1.00, 1: 1.00}, {0, 1})[0] == 0                         # nor among the templates


def test_tune_times_miopen_only_when_nothing_ran_or_on_request(tuner, monkeypatch):
    choice, timed = _tune(tuner, monkeypatch, {"miopen": 5.0}, set())
    assert choice == -1 and timed == ["miopen"]                          # nothing else took the shape
    assert tuner.clock.runs(0) == 1 and tuner.clock.runs(104) == 1       # every candidate was asked once
    choice, timed = _tune(tuner, monkeypatch, {0: 1.0, "miopen": 0.5}, {0})
    assert choice == 0 and "miopen" not in timed
    choice, timed = _tune(tuner, monkeypatch, {0: 1.0, "miopen": 0.5}, {0}, tune_miopen=True)
    assert choice == -1 and timed == [0, "miopen"]                       # -1 is stored when it wins
    choice, timed = _tune(tuner, monkeypatch, {0: 1.0, "miopen": 1.0}, {0}, tune_miopen=True)
    assert choice == 0 and timed == [0, "miopen"]
