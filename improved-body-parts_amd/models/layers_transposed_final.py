"""Building blocks of the published 3- and 4-stage IMHN (the reference's models/layers_transposed_final.py), inference-only.

Module/attribute names follow the reference so that its checkpoint (`PoseNet_102_epoch.pth`, config/config_final.py) loads
with strict=True: Residual (:15-46), Conv (:49-79), Backbone (:82-107), Hourglass (:110-198), SELayer (:201-222).  This is a
different network from models/layers_transposed.py, not a flag of it: the backbone has no dilated stack, every hourglass block
is a plain 3x3 Conv + BN, and the residual add of a level comes BEFORE its activation.  See posepaf/fused_model.py
(FusedIMHNFinal) for the BN-folded, channels-last fp16 form."""
from torch import nn

from models.layers_transposed import SELayer, _act  # SELayer (:201-222) is the development variant's, name for name

__all__ = ["Residual", "Conv", "Backbone", "Hourglass", "SELayer"]


class Residual(nn.Module):
    """1x1 -> 3x3 -> 1x1 bottleneck (mid = outs // 2) with BN after every conv, optional 1x1+BN skip, LeakyReLU after the add
    (:15-46; the backbone's only user)."""

    def __init__(self, ins, outs):
        super().__init__()
        mid = outs // 2
        self.convBlock = nn.Sequential(
            nn.Conv2d(ins, mid, 1, bias=False), nn.BatchNorm2d(mid), _act(),
            nn.Conv2d(mid, mid, 3, 1, 1, bias=False), nn.BatchNorm2d(mid), _act(),
            nn.Conv2d(mid, outs, 1, bias=False), nn.BatchNorm2d(outs))
        if ins != outs:
            self.skipConv = nn.Sequential(nn.Conv2d(ins, outs, 1, bias=False), nn.BatchNorm2d(outs))
        self.relu = _act()
        self.ins, self.outs = ins, outs
        self.relu_flag = True

    def forward(self, x):
        y = self.convBlock(x)
        y = y + (self.skipConv(x) if self.ins != self.outs else x)
        return self.relu(y)


class Conv(nn.Module):
    """conv(k, 'same' padding) [+ BN] [+ LeakyReLU]; bias only when there is no BN (:49-79; dropout is off at inference)."""

    def __init__(self, inp_dim, out_dim, kernel_size=3, stride=1, bn=False, relu=True, dropout=False):
        super().__init__()
        self.inp_dim = inp_dim
        self.conv = nn.Conv2d(inp_dim, out_dim, kernel_size, stride, padding=(kernel_size - 1) // 2, bias=not bn)
        self.bn = nn.BatchNorm2d(out_dim) if bn else None
        self.relu = _act() if relu else None

    def forward(self, x):
        x = self.conv(x)
        if self.bn is not None:
            x = self.bn(x)
        if self.relu is not None:
            x = self.relu(x)
        return x


class Backbone(nn.Module):
    """7x7/2 stem -> Residual(64,128) -> maxpool -> Residual(128,128) -> Residual(128,nFeat): nFeat channels at 1/4
    resolution (:82-107).  No dilated stack, no concatenation."""

    def __init__(self, nFeat=256, inplanes=3, resBlock=Residual):
        super().__init__()
        self.nFeat = nFeat
        self.conv1 = nn.Conv2d(inplanes, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = _act()
        self.res1 = resBlock(64, 128)
        self.pool = nn.MaxPool2d(2, 2)
        self.res2 = resBlock(128, 128)
        self.res3 = resBlock(128, nFeat)

    def forward(self, x):
        x = self.relu(self.bn1(self.conv1(x)))
        return self.res3(self.res2(self.pool(self.res1(x))))


class Hourglass(nn.Module):
    """Order-`depth` hourglass of plain 3x3 Conv + BN blocks whose channel count grows by `increase` per level (:110-198).
    Per level: [0] the skip path (no activation), [1] / [2] the way down / up (+- increase channels), [3] on the x2 nearest
    upsample of [2]'s output, [4] without activation, [5] the LeakyReLU that follows `up1 += deconv2`; the innermost level
    adds [6].  Returns the full-resolution output followed by the four coarser maps it passes through (5 scales)."""

    def __init__(self, depth, nFeat, increase=128, bn=False, resBlock=Conv):
        super().__init__()
        self.depth = depth
        levels = []
        for i in range(depth):
            c, cn = nFeat + increase * i, nFeat + increase * (i + 1)
            mods = [resBlock(c, c, bn=bn, relu=False), resBlock(c, cn, bn=bn), resBlock(cn, c, bn=bn), resBlock(c, c, bn=bn),
                    resBlock(c, c, bn=bn, relu=False), _act()]
            if i == depth - 1:
                mods.append(resBlock(cn, cn, bn=bn))
            levels.append(nn.ModuleList(mods))
        self.hg = nn.ModuleList(levels)
        self.downsample = nn.MaxPool2d(2, 2)
        self.upsample = nn.Upsample(scale_factor=2, mode="nearest")

    def _level(self, i, x, coarse):
        lv = self.hg[i]
        up1 = lv[0](x)
        low = lv[1](self.downsample(x))
        low = lv[6](low) if i == self.depth - 1 else self._level(i + 1, low, coarse)
        coarse.append(low)
        return lv[5](up1 + lv[4](lv[3](self.upsample(lv[2](low)))))

    def forward(self, x):
        coarse = []
        top = self._level(0, x, coarse)
        return [top] + coarse[::-1]
