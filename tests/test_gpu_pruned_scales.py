"""GPU: when the forward prunes the coarse scales (fused_model.USE_PRUNED_SCALES).  The first eager forward of a model on a device
input of a new shape runs every scale -- it is the pass that tunes the layer shapes, and the table it leaves must serve all_preds
too (tests/test_gpu_model.py pins that key set) -- every later one, and every stream capture, computes scale 0 only.  The bits are
the same either way (tests/test_pruned_scales_cpu.py; test_tuning_pass_table_hits_and_graph_capture_run_the_same_kernels)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("arch", ["posenet", "final"])
def test_first_eager_pass_of_a_shape_runs_every_scale_later_ones_and_captures_prune(arch, monkeypatch):
    from posepaf import fused_model as fm
    model = fm.build_inference_model("cuda", arch=arch)
    a = torch.zeros((2, 64, 64, 3), dtype=torch.float16, device="cuda")
    b = torch.zeros((2, 64, 128, 3), dtype=torch.float16, device="cuda")
    assert model._prune_scales(a, True) is False and model._prune_scales(a, True) is False     # all_preds: never, and not remembered
    assert model._prune_scales(a, False) is False                                               # the tuning pass of this shape
    assert model._prune_scales(a, False) is True and model._prune_scales(a, False) is True
    assert model._prune_scales(b, False) is False and model._prune_scales(b, False) is True     # another shape: its own tuning pass
    assert model._prune_scales(a.float(), False) is False                                       # another dtype: other kernels
    assert model._prune_scales(a.cpu(), False) is True                                          # host tensors tune nothing
    c = torch.zeros((2, 128, 64, 3), dtype=torch.float16, device="cuda")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        c.add_(1)
        inside = model._prune_scales(c, False)
    assert inside is True                                                                       # nothing is tuned inside a capture
    assert model._prune_scales(c, False) is False                                               # ... and the capture did not count
    monkeypatch.setattr(fm, "USE_PRUNED_SCALES", False)
    assert model._prune_scales(a, False) is False
