"""The ResNet-50 body of the reference's backbone (code/helpers/model.py:204, `maskrcnn_model.backbone(...)`: the
`body` half of torchvision's BackboneWithFPN) on libsfvos kernels: the normalised image tensor -> C2..C5, and with
BackboneWithFPN on to the packed pyramid.  The transform in front of it (normalise, resize, batch) is transform.py's; its
batched tensor is what the stem reads.

The reference freezes the backbone (model.py:176-177) and runs it under no_grad (:324), so this is inference only:
every BatchNorm is a FrozenBatchNorm2d, a per-channel affine in the conv's epilogue.  torchvision is third-party, not
vendored and absent in this build's environment: the classes mirror its published module structure
(`IntermediateLayerGetter(resnet50, {'layer1': '0', ..., 'layer4': '3'})`; same attribute names and state-dict keys, so
the `backbone.body.*` slice of a reference checkpoint loads with strict=True) and their results are checked against a
torch-core restatement (tests/body_ref.py) -- PARITY UNPINNED BY THE REFERENCE.  No CPU fallback.

Per frame: one sfvos_body_stem launch (conv1 + bn1 + ReLU straight from the planar fp32 image), one
sfvos_maxpool3x3s2, then one sfvos_conv2d launch per conv of the 16 bottlenecks (52; a K-split shape adds its combine
launch), each with its frozen norm, the residual and the ReLU in the epilogue; activations stay channels-last in the
compute dtype from the stem to C5.

Out of scope: the transform (transform.py), any backward, trainable or train-mode BatchNorm, other block types, e4m3."""
from collections import OrderedDict

import torch
from torch import nn
from torch.nn import functional as F

from . import _lib
from ._heads import _check_precision
from ._lib import _DT, _check_gpu, _ptr, _stream
from .fpn import FeaturePyramidNetwork

STEM_K = 176   # conv1's K as sfvos_body_stem reads it: (3 x 7 rows + 1 row of zeros) x 8


class FrozenBatchNorm2d(nn.Module):
    """torchvision's FrozenBatchNorm2d: four buffers, no statistics update, no gradient.  `num_batches_tracked` of a
    checkpoint is dropped on load, as torchvision's does."""

    def __init__(self, num_features, eps=0.0):
        super(FrozenBatchNorm2d, self).__init__()
        self.eps = float(eps)
        self.register_buffer('weight', torch.ones(num_features))
        self.register_buffer('bias', torch.zeros(num_features))
        self.register_buffer('running_mean', torch.zeros(num_features))
        self.register_buffer('running_var', torch.ones(num_features))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kw):
        state_dict.pop(prefix + 'num_batches_tracked', None)
        super(FrozenBatchNorm2d, self)._load_from_state_dict(state_dict, prefix, *args, **kw)

    def coefficients(self):
        """(scale, shift) fp32 [C], in torchvision's order of operations."""
        w, b = self.weight.float(), self.bias.float()
        scale = w * (self.running_var.float() + self.eps).rsqrt()
        return scale.contiguous(), (b - self.running_mean.float() * scale).contiguous()

    def extra_repr(self):
        return '%d, eps=%g' % (self.weight.shape[0], self.eps)


class Bottleneck(nn.Module):
    """torchvision's Bottleneck (v1.5: the stride sits on conv2), expansion 4; a holder of parameters -- ResNetBody runs it."""
    expansion = 4

    def __init__(self, inplanes, planes, stride, downsample, eps):
        super(Bottleneck, self).__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = FrozenBatchNorm2d(planes, eps)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = FrozenBatchNorm2d(planes, eps)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = FrozenBatchNorm2d(planes * 4, eps)
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False),
                                            FrozenBatchNorm2d(planes * 4, eps))
        else:
            self.downsample = None
        self.stride = stride


class ResNetBody(nn.Module):
    """torchvision's IntermediateLayerGetter(resnet50(norm_layer=FrozenBatchNorm2d), {'layer1': '0', 'layer2': '1',
    'layer3': '2', 'layer4': '3'}) without a backward, under its names: conv1, bn1, layerN.i.conv{1,2,3},
    layerN.i.bn{1,2,3}, layerN.0.downsample.{0,1}; no fc.

    eps defaults to 0.0: the reference builds the model with pretrained=True, for which torchvision sets the frozen
    norms' eps to 0 (its older releases had no eps at all); torchvision's own default for a fresh FrozenBatchNorm2d is
    1e-5.  scale = weight * rsqrt(running_var + eps), shift = bias - running_mean * scale, in fp32.
    Inference only: it raises when a gradient would be needed."""

    def __init__(self, layers=(3, 4, 6, 3), precision='fp32', eps=0.0):
        super(ResNetBody, self).__init__()
        self.precision = _check_precision(precision)
        layers = tuple(int(n) for n in layers)
        if len(layers) != 4 or min(layers) < 1:
            raise ValueError('ResNetBody: four layers of at least one block each, got %r' % (layers,))
        self.eps = float(eps)
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = FrozenBatchNorm2d(64, eps)
        inplanes = 64
        for i, (planes, n) in enumerate(zip((64, 128, 256, 512), layers)):
            stride = 1 if i == 0 else 2
            blocks = [Bottleneck(inplanes, planes, stride, True, eps)]
            inplanes = planes * 4
            blocks += [Bottleneck(inplanes, planes, 1, False, eps) for _ in range(1, n)]
            setattr(self, 'layer%d' % (i + 1), nn.Sequential(*blocks))
        for m in self.modules():   # torchvision's init
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
        self.out_channels_list = (256, 512, 1024, 2048)
        self._images = _lib.WeightImages()

    # ---- host-side checks ----
    def _check_inference(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise RuntimeError('ResNetBody is inference only (the reference freezes the backbone): call it under '
                               'torch.no_grad() or freeze its parameters')

    def _images_in(self, images):
        self._check_inference(images)
        _check_gpu(images, 'ResNetBody')
        if images.dim() != 4 or images.shape[1] != 3 or min(images.shape) < 1:
            raise RuntimeError('ResNetBody: expected [B, 3, H, W] images, got %s' % (tuple(images.shape),))
        if self.conv1.weight.device != images.device:
            raise RuntimeError('ResNetBody: the images are on %s, the parameters on %s' % (images.device,
                                                                                       self.conv1.weight.device))
        x = images.detach()
        if x.dtype != torch.float32:
            x = x.float()
        if x.stride(3) != 1 or min(x.stride()) < 0:
            x = x.contiguous()
        return x

    @staticmethod
    def level_shapes(hw):
        """(H, W) of C2..C5 for an image of hw: each stride-2 op gives (n - 1) // 2 + 1."""
        def half(s):
            return ((s[0] - 1) // 2 + 1, (s[1] - 1) // 2 + 1)
        c2 = half(half(tuple(int(v) for v in hw)))
        c3 = half(c2)
        c4 = half(c3)
        return [c2, c3, c4, half(c4)]

    # ---- weight images and coefficients, cached on the tensors' versions ----
    def _affine(self, key, bn):
        return self._images.get(('affine', key), (bn.weight, bn.bias, bn.running_mean, bn.running_var), bn.coefficients)

    def _weight(self, key, conv):
        """[c_out][taps][c_in] in the compute dtype: the layout sfvos_conv2d reads."""
        dt_id, tdt = _DT[self.precision]
        wt = conv.weight
        return self._images.get(('w', key, dt_id), (wt,), lambda: wt.detach().float().permute(0, 2, 3, 1).reshape(
            wt.shape[0], -1).to(tdt).contiguous())

    def _stem_weight(self):
        dt_id, tdt = _DT[self.precision]
        wt = self.conv1.weight
        return self._images.get(('w', 'conv1', dt_id), (wt,), lambda: F.pad(F.pad(
            wt.detach().float(), (0, 1)).reshape(64, 168), (0, STEM_K - 168)).to(tdt).contiguous())

    # ---- launches ----
    def _conv(self, key, conv, bn, x, B, hw, residual, relu, stages):
        """conv + bn (+ residual) (+ ReLU) of x [B h w, c_in] -> ([B oh ow, c_out], (oh, ow)).  One launch (two with a K split)."""
        dt_id, tdt = _DT[self.precision]
        c_in, c_out, s = conv.in_channels, conv.out_channels, conv.stride[0]
        taps = conv.kernel_size[0] * conv.kernel_size[1]
        oh, ow = (hw[0] - 1) // s + 1, (hw[1] - 1) // s + 1
        scale, shift = self._affine(key, bn)
        y = torch.empty((B * oh * ow, c_out), dtype=tdt, device=x.device)
        nbytes = _lib.load().sfvos_conv2d_workspace_bytes(dt_id, B, hw[0], hw[1], c_in, c_out, taps, s)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
        _lib.call('sfvos_conv2d', _ptr(x), c_in, _ptr(self._weight(key, conv)), _ptr(scale), _ptr(shift), _ptr(residual),
                  c_out, _ptr(y), c_out, B, hw[0], hw[1], c_in, c_out, taps, s, int(relu), dt_id, _ptr(ws), _stream())
        if stages is not None:
            stages.append(dict(name=key, kind='conv', x=x, y=y, residual=residual, relu=bool(relu), in_hw=tuple(hw),
                               out_hw=(oh, ow), stride=s, conv=conv, bn=bn))
        return y, (oh, ow)

    def _stem(self, x, stages=None):
        """conv1 + bn1 + ReLU of the images x [B, 3, H, W] -> ([B h1 w1, 64], (h1, w1)).  One launch."""
        dt_id, tdt = _DT[self.precision]
        B, _, H, W = x.shape
        h1, w1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        scale, shift = self._affine('bn1', self.bn1)
        stem = torch.empty((B * h1 * w1, 64), dtype=tdt, device=x.device)
        _lib.call('sfvos_body_stem', _ptr(x), x.stride(0), x.stride(1), x.stride(2), x.stride(3), B, H, W,
                  _ptr(self._stem_weight()), _ptr(scale), _ptr(shift), _ptr(stem), 64, dt_id, _stream())
        if stages is not None:
            stages.append(dict(name='conv1', kind='stem', x=x, y=stem, in_hw=(H, W), out_hw=(h1, w1)))
        return stem, (h1, w1)

    def _pool(self, stem, B, hw, stages=None):
        """max_pool2d(3, 2, 1) of the stem's output.  One launch."""
        dt_id, tdt = _DT[self.precision]
        h2, w2 = (hw[0] - 1) // 2 + 1, (hw[1] - 1) // 2 + 1
        out = torch.empty((B * h2 * w2, 64), dtype=tdt, device=stem.device)
        _lib.call('sfvos_maxpool3x3s2', _ptr(stem), 64, _ptr(out), 64, B, hw[0], hw[1], 64, dt_id, _stream())
        if stages is not None:
            stages.append(dict(name='maxpool', kind='pool', x=stem, y=out, in_hw=tuple(hw), out_hw=(h2, w2)))
        return out, (h2, w2)

    def _layer(self, li, cur, B, hw, stages=None):
        """layer<li> of cur [B h w, C] -> (its output, its sides)."""
        for bi, blk in enumerate(getattr(self, 'layer%d' % li)):
            key = 'layer%d.%d.' % (li, bi)
            identity = cur
            if blk.downsample is not None:
                identity, _ = self._conv(key + 'downsample', blk.downsample[0], blk.downsample[1], cur, B, hw, None, False,
                                         stages)
            o, _ = self._conv(key + 'conv1', blk.conv1, blk.bn1, cur, B, hw, None, True, stages)
            o, ohw = self._conv(key + 'conv2', blk.conv2, blk.bn2, o, B, hw, None, True, stages)
            cur, hw = self._conv(key + 'conv3', blk.conv3, blk.bn3, o, B, ohw, identity, True, stages)
        return cur, hw

    def forward_channels_last(self, images, return_stages=False):
        """images: fp32 [B, 3, H, W] -> (the four maps C2..C5 as [B h w, C] in the compute dtype, their (h, w)).
        return_stages=True: also a list of dicts, one per launch in order -- the stem ('conv1'), the pool ('maxpool') and
        every conv ('layerN.i.convK', 'layerN.0.downsample') -- with its input `x`, output `y`, `residual`, `relu`, the
        sides `in_hw` / `out_hw` and, for convs, `conv`, `bn` and `stride`."""
        x = self._images_in(images)
        B = x.shape[0]
        stages = [] if return_stages else None
        maps, shapes = [], []
        with torch.no_grad():
            cur, hw = self._stem(x, stages)
            cur, hw = self._pool(cur, B, hw, stages)
            for li in range(1, 5):
                cur, hw = self._layer(li, cur, B, hw, stages)
                maps.append(cur)
                shapes.append(hw)
        return (maps, shapes, stages) if return_stages else (maps, shapes)

    def _unpack(self, maps, shapes, B):
        dt_id, _ = _DT[self.precision]
        outs = []
        for m, (h, w) in zip(maps, shapes):
            C = m.shape[1]
            out = torch.empty((B, C, h, w), dtype=torch.float32, device=m.device)
            _lib.call('sfvos_ndhwc_to_frames', _ptr(m), dt_id, _ptr(out), out.stride(0), out.stride(1), out.stride(2),
                      out.stride(3), B, C, h, w, C, 0, _stream())
            outs.append(out)
        return outs

    def forward(self, images):
        """The drop-in for `backbone.body`: fp32 [B, 3, H, W] -> ordered dict '0'..'3' of fp32 NCHW maps (C2..C5).  With
        precision='bf16' the values are bf16-rounded (computed and stored in bf16, then widened)."""
        maps, shapes = self.forward_channels_last(images)
        return OrderedDict(zip(('0', '1', '2', '3'), self._unpack(maps, shapes, images.shape[0])))


class BackboneWithFPN(nn.Module):
    """torchvision's BackboneWithFPN over resnet50: `body` (ResNetBody) and `fpn` (FeaturePyramidNetwork with
    LastLevelMaxPool), out_channels 256.  The `backbone.*` slice of a reference checkpoint loads with strict=True.
    The FPN's lateral step reads the body's maps as the planar fp32 tensors `body.forward` returns."""

    def __init__(self, precision='fp32', eps=0.0):
        super(BackboneWithFPN, self).__init__()
        self.body = ResNetBody(precision=precision, eps=eps)
        self.fpn = FeaturePyramidNetwork(self.body.out_channels_list, 256, precision=precision)
        self.out_channels = 256
        self.precision = self.body.precision

    def forward(self, images):
        """The drop-in for `maskrcnn_model.backbone` (model.py:204): images -> ordered dict '0'..'3', 'pool' of fp32
        NCHW maps of 256 channels."""
        return self.fpn(self.body(images))

    def write_frames(self, images, seq, first_frame):
        """images: N consecutive frames of ONE video -> frames first_frame .. first_frame + N - 1 of the resident
        PackedClip seq (FeaturePyramidNetwork.write_frames)."""
        return self.fpn.write_frames(self.body(images), seq, first_frame)
