"""PoseNet / NetworkEval of the published 3- and 4-stage IMHN: the reference's models/posenet_final.py (:50-132, :190-208),
the network its config/config_final.py checkpoint (`PoseNet_102_epoch.pth`) belongs to.

Same constructor signature, forward contract (NHWC float image batch in [0,1] -> list[stage][scale] of
(N, 50, H/2^(2+s), W/2^(2+s))) and state_dict keys as the reference (1236 entries at nstack = 4, from
`posenet.pre.conv1.weight` to `posenet.merge_preds.2.4.conv.bn.num_batches_tracked`).  Against models/posenet.py: the
squeeze-and-excitation sits on the hourglass outputs (`channel_attention[t][s]`), not at the end of `before_regress`, and
`before_regress[s]` starts with a 1x1 convolution that compresses 256 + 128 s channels to 256.  Inference only."""
import torch
from torch import nn

from models.layers_transposed_final import Backbone, Conv, Hourglass, SELayer


class Merge(nn.Module):
    """1x1 conv (no activation) that changes the channel count (:13-21)."""

    def __init__(self, x_dim, y_dim, bn=False):
        super().__init__()
        self.conv = Conv(x_dim, y_dim, 1, relu=False, bn=bn)

    def forward(self, x):
        return self.conv(x)


class Features(nn.Module):
    """Per scale: 1x1 conv (inp_dim + s * increase -> inp_dim) -> 3x3 conv -> 3x3 conv; no SE at the end (:24-47)."""

    def __init__(self, inp_dim, increase=128, bn=False):
        super().__init__()
        self.before_regress = nn.ModuleList([
            nn.Sequential(Conv(inp_dim + i * increase, inp_dim, 1, bn=bn), Conv(inp_dim, inp_dim, 3, bn=bn),
                          Conv(inp_dim, inp_dim, 3, bn=bn)) for i in range(5)])

    def forward(self, fms):
        assert len(fms) == 5
        return [blk(f) for blk, f in zip(self.before_regress, fms)]


class PoseNet(nn.Module):
    def __init__(self, nstack, inp_dim, oup_dim, bn=False, increase=128, init_weights=True, **kwargs):
        super().__init__()
        self.pre = Backbone(nFeat=inp_dim)
        self.hourglass = nn.ModuleList([Hourglass(4, inp_dim, increase, bn=bn) for _ in range(nstack)])
        self.features = nn.ModuleList([Features(inp_dim, increase=increase, bn=bn) for _ in range(nstack)])
        self.outs = nn.ModuleList([nn.ModuleList([Conv(inp_dim, oup_dim, 1, relu=False, bn=False) for _ in range(5)])
                                   for _ in range(nstack)])
        self.channel_attention = nn.ModuleList([nn.ModuleList([SELayer(inp_dim + j * increase) for j in range(5)])
                                                for _ in range(nstack)])
        self.merge_features = nn.ModuleList([nn.ModuleList([Merge(inp_dim, inp_dim + j * increase, bn=bn) for j in range(5)])
                                             for _ in range(nstack - 1)])
        self.merge_preds = nn.ModuleList([nn.ModuleList([Merge(oup_dim, inp_dim + j * increase, bn=bn) for j in range(5)])
                                          for _ in range(nstack - 1)])
        self.nstack = nstack
        self.num_stages, self.num_scales = nstack, 5
        if init_weights:
            self._initialize_weights()

    def forward(self, imgs):
        x = self.pre(imgs.permute(0, 3, 1, 2))
        preds, caches = [], None
        for t in range(self.nstack):
            hg = self.hourglass[t](x)
            hg = [se(h) for se, h in zip(self.channel_attention[t], hg)]   # :104-113: SE first, then the cache of the stage before
            if caches is not None:
                hg = [a + c for a, c in zip(hg, caches)]
            feats = self.features[t](hg)
            stage_preds = [head(f) for head, f in zip(self.outs[t], feats)]
            if t != self.nstack - 1:
                caches = [self.merge_preds[t][s](stage_preds[s]) + self.merge_features[t][s](feats[s])
                          for s in range(self.num_scales)]
                x = x + caches[0]
            preds.append(stage_preds)
        return preds

    def _initialize_weights(self):  # :134-154
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.data.normal_(0, 0.001)
                if m.bias is not None:
                    m.bias.data.zero_()
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
            elif isinstance(m, nn.Linear):
                torch.nn.init.normal_(m.weight.data, 0, 0.01)
                m.bias.data.zero_()


class NetworkEval(nn.Module):
    """Inference wrapper (:190-208): `opt` supplies nstack / hourglass_inp_dim / increase, `config` supplies num_layers (50)."""

    def __init__(self, opt, config, bn=False):
        super().__init__()
        self.posenet = PoseNet(opt.nstack, opt.hourglass_inp_dim, config.num_layers, bn=bn, init_weights=False,
                               increase=opt.increase)

    def forward(self, inp_imgs):
        if self.training:
            raise ValueError("\nOnly eval mode is available!!")
        return self.posenet(inp_imgs)
