"""torch-core restatement of torchvision's FeaturePyramidNetwork + LastLevelMaxPool (torchvision is not installed:
parity is unpinned by the reference; the restatement itself is pinned by test_fpn_ref_cpu.py).  Works in any float dtype:
the GPU tests call it in float64."""
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn


class FeaturePyramidNetwork(nn.Module):
    def __init__(self, in_channels_list, out_channels, pool=True):
        super(FeaturePyramidNetwork, self).__init__()
        self.inner_blocks = nn.ModuleList(nn.Conv2d(c, out_channels, 1) for c in in_channels_list)
        self.layer_blocks = nn.ModuleList(nn.Conv2d(out_channels, out_channels, 3, padding=1) for _ in in_channels_list)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=1)
                nn.init.constant_(m.bias, 0)
        self.pool = pool

    def forward(self, x, return_inner=False):
        names, x = list(x.keys()), list(x.values())
        last_inner = inner_step(x[-1], self.inner_blocks[-1].weight, self.inner_blocks[-1].bias, None)
        inners = [last_inner]
        results = [output_step(last_inner, self.layer_blocks[-1].weight, self.layer_blocks[-1].bias)]
        for idx in range(len(x) - 2, -1, -1):
            last_inner = inner_step(x[idx], self.inner_blocks[idx].weight, self.inner_blocks[idx].bias, last_inner)
            inners.insert(0, last_inner)
            results.insert(0, output_step(last_inner, self.layer_blocks[idx].weight, self.layer_blocks[idx].bias))
        if self.pool:
            names.append('pool')
            results.append(last_level_max_pool(results[-1]))
        out = OrderedDict(zip(names, results))
        return (out, inners) if return_inner else out


def inner_step(x, weight, bias, top):
    """inner_blocks[i](x) + F.interpolate(top, size=x.shape[-2:], mode='nearest'); NCHW."""
    lateral = F.conv2d(x, weight.to(x.dtype), None if bias is None else bias.to(x.dtype))
    if top is None:
        return lateral
    return lateral + F.interpolate(top, size=lateral.shape[-2:], mode='nearest')


def output_step(inner, weight, bias):
    return F.conv2d(inner, weight.to(inner.dtype), bias.to(inner.dtype), padding=1)


def last_level_max_pool(x):
    return F.max_pool2d(x, 1, 2, 0)


def nchw(flat, B, h, w):
    """channels-last [B h w, C] -> [B, C, h, w]."""
    return flat.reshape(B, h, w, -1).permute(0, 3, 1, 2)


def nhwc(x):
    """[B, C, h, w] -> [B h w, C]."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])
