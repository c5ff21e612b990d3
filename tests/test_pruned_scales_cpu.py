"""CPU, float32: the coarse scales s = 1..4 of a stage feed only their own heads and the next stage's coarse scales
(models/posenet.py:115-119: only `s == 0` reaches x), so with fused_model.USE_PRUNED_SCALES the default forward and
stage_preds=True compute feat / mfeat / the cache add for scale 0 alone, in every stage; all_preds=True runs everything.

Both architectures at the sizes of tests/test_loss_reference_cpu.py (`_small`), input 2 x 64 x 128 x 3; the development variant also
with THREE stages, so that the default path reaches a middle stage -- the one whose `hg[s] + caches[s]` adds disappear."""
import pytest
import torch


def _net(arch, stages):
    from posepaf.model_init import deterministic_init
    if arch == "final":
        from models.posenet_final import PoseNet
        body = PoseNet(stages, 32, 50, bn=True, increase=16, init_weights=False)
    else:   # (the backbone of models/posenet.py is 256 wide)
        from models.posenet import PoseNet
        body = PoseNet(stages, 256, 50, bn=True, increase=32, init_weights=False)

    class Wrap(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.posenet = body

        def forward(self, x):
            return self.posenet(x)

    net = Wrap().eval()
    deterministic_init(net, seed=11)
    return net


class Calls:
    """forward hooks on feat[t][s] and mfeat[t][s] for s > 0: how often each was called since reset()"""

    def __init__(self, fused):
        self.n = {}
        for name, grid in (("feat", fused.feat), ("mfeat", fused.mfeat)):
            for t, row in enumerate(grid):
                for s, m in enumerate(row):
                    if s > 0:
                        self.n[(name, t, s)] = 0
                        m.register_forward_hook(lambda *_a, key=(name, t, s): self.n.__setitem__(key, self.n[key] + 1))

    def reset(self):
        for k in self.n:
            self.n[k] = 0


CASES = [("posenet", 2), ("posenet", 3), ("final", 3)]


@pytest.mark.parametrize("arch,stages", CASES, ids=[f"{a}-{s}stages" for a, s in CASES])
def test_default_and_stage_preds_skip_the_coarse_scales_and_keep_their_bits(arch, stages, monkeypatch):
    from posepaf import fused_model as fm
    assert fm.USE_PRUNED_SCALES
    net = _net(arch, stages)
    fused = fm.FusedIMHN.from_network(net).eval()
    assert isinstance(fused, fm.FusedIMHNFinal) == (arch == "final") and fused.folded_merge and fused.S == stages and fused.K == 5
    calls = Calls(fused)
    assert {k[0] for k in calls.n} == {"feat", "mfeat"} and len([k for k in calls.n if k[0] == "feat"]) == stages * 4
    x = torch.rand(2, 64, 128, 3, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        calls.reset()
        out = fused(x)
        assert not any(calls.n.values()), f"fused(x) ran coarse modules: {[k for k, v in calls.n.items() if v]}"
        calls.reset()
        stage = fused(x, stage_preds=True)
        assert not any(calls.n.values()), f"stage_preds ran coarse modules: {[k for k, v in calls.n.items() if v]}"
        calls.reset()
        every = fused(x, all_preds=True)
        # (the last stage has no successor: its merge convolutions never run, in the reference either)
        want_calls = {k: (0 if k[0] == "mfeat" and k[1] == stages - 1 else 1) for k in calls.n}
        assert calls.n == want_calls, {k: v for k, v in calls.n.items() if v != want_calls[k]}
        # the unpruned form: what the forward computed before the switch existed
        monkeypatch.setattr(fm, "USE_PRUNED_SCALES", False)
        calls.reset()
        out_full = fused(x)
        assert sum(calls.n.values()) == (stages - 1) * 8, "the unpruned default path runs the coarse scales of every stage but the last"
        stage_full = fused(x, stage_preds=True)
        every_full = fused(x, all_preds=True)
        want = net.posenet(x)
    assert torch.equal(out, out_full)
    assert len(stage) == len(stage_full) == stages and all(torch.equal(a, b) for a, b in zip(stage, stage_full))
    assert all(torch.isfinite(t).all() for t in stage)
    assert torch.equal(out, stage[-1]) and torch.equal(out, every[-1][0])
    # all_preds runs exactly what it ran: equal with and without the switch, and within the bound of
    # tests/test_loss_reference_cpu.py (1e-5 of each prediction's scale) of the reference module
    worst = 0.0
    for t in range(stages):
        assert len(every[t]) == 5
        for s in range(5):
            assert torch.equal(every[t][s], every_full[t][s])
            scale = want[t][s].abs().max().item()
            assert scale > 1e-3
            err = (every[t][s] - want[t][s]).abs().max().item() / scale
            worst = max(worst, err)
            assert err <= 1e-5, (t, s, err)
    print(f"{arch}, {stages} stages: largest error of the {stages * 5} predictions, relative to each one's scale: {worst:.3e}")
