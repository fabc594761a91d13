"""torch-core restatement of torchvision's resnet50 body (IntermediateLayerGetter over layer1..layer4, Bottleneck v1.5:
the stride on conv2) and of its FrozenBatchNorm2d (torchvision is not installed: parity is unpinned by the reference; the
restatement itself is pinned by test_body_ref_cpu.py).  The package never imports it.  Works in any float dtype: the GPU
tests call it in float64."""
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn

LAYERS = (3, 4, 6, 3)
PLANES = (64, 128, 256, 512)


def frozen_bn(x, weight, bias, running_mean, running_var, eps=0.0):
    """torchvision's FrozenBatchNorm2d.forward, in x's dtype: scale = w * rsqrt(rv + eps); x * scale + (b - rm * scale)."""
    w, b = weight.to(x.dtype).reshape(1, -1, 1, 1), bias.to(x.dtype).reshape(1, -1, 1, 1)
    rv, rm = running_var.to(x.dtype).reshape(1, -1, 1, 1), running_mean.to(x.dtype).reshape(1, -1, 1, 1)
    scale = w * (rv + eps).rsqrt()
    return x * scale + (b - rm * scale)


def out_side(n, stride=2):
    return (n - 1) // stride + 1


def expected_state():
    """name -> shape of the `backbone.body.*` slice: 53 conv weights and 53 x 4 norm buffers."""
    want = OrderedDict()

    def bn(prefix, c):
        for n in ('weight', 'bias', 'running_mean', 'running_var'):
            want['%s.%s' % (prefix, n)] = (c,)

    want['conv1.weight'] = (64, 3, 7, 7)
    bn('bn1', 64)
    inplanes = 64
    for li, (planes, n) in enumerate(zip(PLANES, LAYERS)):
        for bi in range(n):
            p = 'layer%d.%d' % (li + 1, bi)
            want[p + '.conv1.weight'] = (planes, inplanes, 1, 1)
            bn(p + '.bn1', planes)
            want[p + '.conv2.weight'] = (planes, planes, 3, 3)
            bn(p + '.bn2', planes)
            want[p + '.conv3.weight'] = (planes * 4, planes, 1, 1)
            bn(p + '.bn3', planes * 4)
            if bi == 0:
                want[p + '.downsample.0.weight'] = (planes * 4, inplanes, 1, 1)
                bn(p + '.downsample.1', planes * 4)
            inplanes = planes * 4
    return want


def conv_shapes(hw):
    """The 52 bottleneck convs of a frame whose pooled stem output has sides hw: (name, h, w, c_in, c_out, taps, stride)."""
    out = []
    inplanes = 64
    for li, (planes, n) in enumerate(zip(PLANES, LAYERS)):
        for bi in range(n):
            s = 2 if (li > 0 and bi == 0) else 1
            p = 'layer%d.%d.' % (li + 1, bi)
            if bi == 0:
                out.append((p + 'downsample', hw[0], hw[1], inplanes, planes * 4, 1, s))
            out.append((p + 'conv1', hw[0], hw[1], inplanes, planes, 1, 1))
            out.append((p + 'conv2', hw[0], hw[1], planes, planes, 9, s))
            hw = (out_side(hw[0], s), out_side(hw[1], s))
            out.append((p + 'conv3', hw[0], hw[1], planes, planes * 4, 1, 1))
            inplanes = planes * 4
    return out


def random_state(seed, var_range=(0.5, 2.0)):
    """A full state dict with fan-in-scaled conv weights and frozen-norm buffers that keep activations of order one."""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for k, s in expected_state().items():
        if k.endswith('running_var'):
            sd[k] = var_range[0] + (var_range[1] - var_range[0]) * torch.rand(s, generator=g)
        elif k.endswith('running_mean'):
            sd[k] = 0.2 * torch.randn(s, generator=g)
        elif len(s) == 1 and k.endswith('.weight'):
            sd[k] = 0.5 + 0.5 * torch.rand(s, generator=g)
        elif k.endswith('.bias'):
            sd[k] = 0.2 * torch.randn(s, generator=g)
        else:
            sd[k] = torch.randn(s, generator=g) * (1.0 / (s[1] * s[2] * s[3])) ** 0.5
    return sd


class ResNetBody(nn.Module):
    """Functional over a state dict (names of expected_state()); forward in the dtype of x."""

    def __init__(self, state, eps=0.0):
        super(ResNetBody, self).__init__()
        self.state, self.eps = state, eps

    def _bn(self, x, p):
        s = self.state
        return frozen_bn(x, s[p + '.weight'], s[p + '.bias'], s[p + '.running_mean'], s[p + '.running_var'], self.eps)

    def _conv(self, x, name, stride=1, padding=0):
        return F.conv2d(x, self.state[name + '.weight'].to(x.dtype), None, stride, padding)

    def forward(self, x):
        x = F.relu(self._bn(self._conv(x, 'conv1', 2, 3), 'bn1'))
        x = F.max_pool2d(x, 3, 2, 1)
        out = OrderedDict()
        for li, n in enumerate(LAYERS):
            for bi in range(n):
                p = 'layer%d.%d' % (li + 1, bi)
                s = 2 if (li > 0 and bi == 0) else 1
                identity = x
                o = F.relu(self._bn(self._conv(x, p + '.conv1'), p + '.bn1'))
                o = F.relu(self._bn(self._conv(o, p + '.conv2', s, 1), p + '.bn2'))
                o = self._bn(self._conv(o, p + '.conv3'), p + '.bn3')
                if bi == 0:
                    identity = self._bn(self._conv(x, p + '.downsample.0', s), p + '.downsample.1')
                x = F.relu(o + identity)
            out[str(li)] = x
        return out


def nchw(flat, B, h, w):
    """channels-last [B h w, C] -> [B, C, h, w]."""
    return flat.reshape(B, h, w, -1).permute(0, 3, 1, 2)


def nhwc(x):
    """[B, C, h, w] -> [B h w, C]."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])
