"""Deterministic, name-seeded initialisation for the IMHN (no pretrained weights are available offline).

Every tensor of the state_dict is filled from a generator seeded by CRC32(key) ^ seed, so two
implementations with the same keys get bit-identical weights.  Used for the model golden vector
(tests/golden/make_golden.py applies it to the REFERENCE module, tests apply it to ours) and for the
benchmark's random-init weights.  Scales (unit-gain fan-in) are chosen so that activations neither vanish nor explode
through 4 stages (the reference's own N(0, 0.001) init drives every output to ~0)."""
import math
import zlib

import torch


@torch.no_grad()
def deterministic_init(model: torch.nn.Module, seed: int = 0) -> None:
    sd = model.state_dict()
    for key, t in sd.items():
        g = torch.Generator().manual_seed((zlib.crc32(key.encode()) ^ seed) & 0x7FFFFFFF)
        if key.endswith("num_batches_tracked"):
            t.fill_(1)
        elif key.endswith("running_var"):
            t.copy_(0.6 + 0.8 * torch.rand(t.shape, generator=g))
        elif key.endswith("running_mean"):
            t.copy_(0.1 * torch.randn(t.shape, generator=g))
        elif t.dim() == 4:  # conv weight
            fan_in = t.shape[1] * t.shape[2] * t.shape[3]
            t.copy_(torch.randn(t.shape, generator=g) * math.sqrt(1.0 / fan_in))
        elif t.dim() == 2:  # linear weight
            t.copy_(torch.randn(t.shape, generator=g) * math.sqrt(1.0 / t.shape[1]))
        elif key.endswith("bn.weight") or ".bn1.weight" in key or (key.endswith(".weight") and t.dim() == 1):
            t.copy_(0.9 + 0.2 * torch.rand(t.shape, generator=g))
        else:  # biases
            t.copy_(0.05 * torch.randn(t.shape, generator=g))


ARCHS = ("posenet", "final")


def _without_module_prefix(state_dict: dict) -> dict:
    """the keys as the bare module has them: a checkpoint saved from a DataParallel wrapper carries `module.` in front of every key"""
    if state_dict and all(k.startswith("module.") for k in state_dict):
        return {k[len("module."):]: v for k, v in state_dict.items()}
    return state_dict


def arch_of_state_dict(state_dict) -> tuple:
    """-> (architecture, nstack) of a checkpoint's weights, from its keys alone (a mapping, or any iterable of key names).
    `posenet.channel_attention.*` exists only in the published variant (models/posenet_final.py -> "final"),
    `posenet.pre.dilation.*` only in the development one (models/posenet.py -> "posenet"); nstack is the number of
    `posenet.hourglass.N` entries.  Keys that show neither, or both, are no IMHN checkpoint: ValueError."""
    keys = list(_without_module_prefix(dict.fromkeys(state_dict)))
    final = any(k.startswith("posenet.channel_attention.") for k in keys)
    dev = any(k.startswith("posenet.pre.dilation.") for k in keys)
    if final == dev:
        raise ValueError("not an IMHN state dict: " + ("both" if final else "neither") +
                         " of posenet.channel_attention.* (final) and posenet.pre.dilation.* (posenet) are present")
    stages = {int(k.split(".")[2]) for k in keys if k.startswith("posenet.hourglass.") and k.split(".")[2].isdigit()}
    if not stages or stages != set(range(len(stages))):
        raise ValueError(f"not an IMHN state dict: posenet.hourglass.N entries {sorted(stages)}")
    return ("final" if final else "posenet"), len(stages)


def network_class(arch: str):
    """the checkpoint-compatible NetworkEval of an architecture name"""
    if arch == "final":
        from models.posenet_final import NetworkEval
    elif arch == "posenet":
        from models.posenet import NetworkEval
    else:
        raise ValueError(f"unknown architecture {arch!r}: one of {ARCHS}")
    return NetworkEval


def load_weights(model: torch.nn.Module, state_dict, arch: str) -> None:
    """strict load (a DataParallel `module.` prefix on every key is taken off first, as arch_of_state_dict does); on a mismatch the
    error names the architecture the keys belong to and the flag that selects it"""
    state_dict = _without_module_prefix(state_dict)
    try:
        model.load_state_dict(state_dict, strict=True)
    except RuntimeError as e:
        try:
            found, nstack = arch_of_state_dict(state_dict)
            hint = f"the checkpoint's keys are those of --arch {found} with nstack {nstack}"
        except ValueError as ve:
            hint = str(ve)
        raise RuntimeError(f"checkpoint does not fit --arch {arch}: {hint} (or pass --arch auto)\n{str(e)[:2000]}") from None


def build_network(arch: str = "posenet", checkpoint_path=None, seed: int = 7, nstack=None):
    """-> (NetworkEval in eval mode, architecture name): the weights of a reference checkpoint (.pth with a 'weights' entry, loaded
    strictly) or, without one, the deterministic initialisation.  arch "auto" reads architecture and nstack off the checkpoint's
    keys (arch_of_state_dict); "posenet" / "final" take nstack from the argument or the configuration."""
    from config.config import GetConfig, TrainingOpt
    weights = None
    if checkpoint_path:
        weights = torch.load(checkpoint_path, map_location="cpu", weights_only=True)["weights"]
    if arch == "auto":
        if weights is None:
            raise ValueError("--arch auto decides from a checkpoint's keys: pass --checkpoint_path, or name the architecture")
        arch, nstack = arch_of_state_dict(weights)
    opt = TrainingOpt()
    if nstack is not None:
        opt.nstack = nstack
    net = network_class(arch)(opt, GetConfig(TrainingOpt.config_name), bn=True).eval()
    if weights is not None:
        load_weights(net, weights, arch)
    else:
        deterministic_init(net, seed)
    return net, arch
