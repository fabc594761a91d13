"""The feature pyramid network of the reference's backbone (code/helpers/model.py:204, `maskrcnn_model.backbone(...)`:
the `fpn` half of torchvision's BackboneWithFPN), on libsfvos kernels: the body's C2..C5 maps -> the packed pyramid that
RegionProposalNetwork.propose_packed and SlowFastWindows read in place.

The reference freezes the backbone (model.py:176-177), so this is inference only.  torchvision is third-party, not
vendored and absent in this build's environment: the class mirrors its published module structure
(`FeaturePyramidNetwork` with `LastLevelMaxPool`; same attribute names and state-dict keys, so the `backbone.fpn.*`
slice of a reference checkpoint loads with strict=True) and its results are checked against a torch-core restatement
(tests/fpn_ref.py) -- PARITY UNPINNED BY THE REFERENCE.  No CPU fallback.

Per level, coarsest first: one sfvos_fpn_lateral launch (1x1 conv straight from the planar fp32 map + bias + the
nearest-upsampled coarser inner map -> channels-last inner map), then one sfvos_conv3d launch (3x3, kt = 1) that writes
the level's region of the pyramid buffer; `pool` is one sfvos_fpn_pool launch.  Between the body and the detections no
layout pass remains.

Out of scope: the ResNet body (body.py), the transform (transform.py), any backward, the frame-major ring of SlowFastStream, e4m3 output, and
B > 1 in `write_frames`."""
import ctypes
from collections import OrderedDict

import torch
from torch import nn

from . import _lib
from ._heads import _check_precision, _pack
from ._lib import _DT, _check_gpu, _conv_desc, _f32, _ptr, _stream


class FeaturePyramidNetwork(nn.Module):
    """torchvision's FeaturePyramidNetwork(in_channels_list, out_channels, extra_blocks=LastLevelMaxPool()) without a
    backward: `inner_blocks` (1x1) and `layer_blocks` (3x3) under torchvision's parameter names; the newer
    `inner_blocks.i.0.*` / `layer_blocks.i.0.*` spelling loads too.  pool=False leaves the extra level out.
    Limits: channels multiples of 32, out_channels <= 256, at most 7 input levels with the pool level (8 levels per
    pyramid); each level's sides must be 2 n or 2 n - 1 of the next coarser one (what a stride-2 body gives).
    Inference only: it raises when a gradient would be needed."""

    def __init__(self, in_channels_list=(256, 512, 1024, 2048), out_channels=256, pool=True, precision='fp32'):
        super(FeaturePyramidNetwork, self).__init__()
        self.precision = _check_precision(precision)
        in_channels_list = [int(c) for c in in_channels_list]
        if not in_channels_list or len(in_channels_list) + bool(pool) > _lib.MAX_LEVELS:
            raise ValueError('FeaturePyramidNetwork: 1..%d levels with the pool level' % _lib.MAX_LEVELS)
        if any(c <= 0 or c % 32 for c in in_channels_list) or out_channels % 32 or not 0 < out_channels <= 256:
            raise ValueError('FeaturePyramidNetwork: channels must be multiples of 32, out_channels <= 256')
        self.out_channels, self.pool = int(out_channels), bool(pool)
        self.inner_blocks, self.layer_blocks = nn.ModuleList(), nn.ModuleList()
        for c in in_channels_list:
            self.inner_blocks.append(nn.Conv2d(c, out_channels, 1))
            self.layer_blocks.append(nn.Conv2d(out_channels, out_channels, 3, padding=1))
        for m in self.modules():   # torchvision's init
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=1)
                nn.init.constant_(m.bias, 0)
        self._images = _lib.WeightImages()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kw):
        for block in ('inner_blocks', 'layer_blocks'):
            for i in range(len(self.inner_blocks)):
                for name in ('weight', 'bias'):
                    new = '%s%s.%d.0.%s' % (prefix, block, i, name)
                    if new in state_dict:
                        state_dict['%s%s.%d.%s' % (prefix, block, i, name)] = state_dict.pop(new)
        super(FeaturePyramidNetwork, self)._load_from_state_dict(state_dict, prefix, *args, **kw)

    def _check_inference(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise RuntimeError('FeaturePyramidNetwork is inference only (the reference freezes the backbone): call it '
                               'under torch.no_grad() or freeze its parameters')

    def level_shapes(self, shapes):
        """(H, W) of the output levels for input levels `shapes`: the same, plus the pool level's."""
        shapes = [tuple(int(v) for v in s) for s in shapes]
        if self.pool:
            shapes.append(((shapes[-1][0] - 1) // 2 + 1, (shapes[-1][1] - 1) // 2 + 1))
        return shapes

    def _maps(self, x):
        maps = list(x.values()) if isinstance(x, dict) else list(x)
        if len(maps) != len(self.inner_blocks):
            raise RuntimeError('FeaturePyramidNetwork: %d maps for %d levels' % (len(maps), len(self.inner_blocks)))
        for m in maps:
            self._check_inference(m)
        _check_gpu(maps[0], 'FeaturePyramidNetwork')
        out = []
        for m, conv in zip(maps, self.inner_blocks):
            if m.dim() != 4 or m.shape[1] != conv.in_channels or m.shape[0] != maps[0].shape[0]:
                raise RuntimeError('FeaturePyramidNetwork: expected [%d, %d, H, W] maps, got %s'
                                   % (maps[0].shape[0], conv.in_channels, tuple(m.shape)))
            m = m.detach()
            if m.dtype != torch.float32:
                m = m.float()
            if m.stride(3) != 1 or min(m.stride()) < 0:
                m = m.contiguous()
            out.append(m)
        return out

    def _lateral(self, l, m, top, top_hw, out):
        """Level l's inner map into out [B h w, C]: m [B, c_l, h, w] fp32, top = the coarser inner map (or None) of
        top_hw.  One launch."""
        dt_id, tdt = _DT[self.precision]
        conv, C = self.inner_blocks[l], self.out_channels
        wt = conv.weight
        image = self._images.get(('inner', l, dt_id), (wt,),
                                 lambda: wt.detach().reshape(C, conv.in_channels).to(tdt).contiguous())
        _lib.call('sfvos_fpn_lateral', _ptr(m), m.stride(0), m.stride(1), m.stride(2), m.stride(3), m.shape[0],
                  conv.in_channels, m.shape[2], m.shape[3], _ptr(image), _ptr(_f32(conv.bias)), C, _ptr(top),
                  top_hw[0], top_hw[1], C, _ptr(out), C, dt_id, _stream())

    def _layer(self, l, inner, B, hw, dst, pos):
        """Level l's 3x3 conv of inner [B h w, C] into dst [*, C] from position pos on.  One launch."""
        dt_id, tdt = _DT[self.precision]
        conv, C = self.layer_blocks[l], self.out_channels
        wt = conv.weight
        packed = self._images.get(('layer', l, dt_id), (wt,), _pack, 'sfvos_pack_weights_fwd', wt, dt_id, tdt, C, C, 1, 9)
        d = _conv_desc(dt_id, B, _lib.make_pyramid([hw]), 1, 9, C, C, 1, inner, C)
        _lib.call('sfvos_conv3d', ctypes.byref(d), _ptr(inner), _ptr(packed), _ptr(_f32(conv.bias)), _ptr(dst, pos * C),
                  None, _stream())

    def _subsample(self, B, hw, dst, src_pos, dst_pos):
        """LastLevelMaxPool of the level at src_pos of dst into dst_pos.  One launch."""
        dt_id, C = _DT[self.precision][0], self.out_channels
        _lib.call('sfvos_fpn_pool', _ptr(dst, src_pos * C), C, _ptr(dst, dst_pos * C), C, B, hw[0], hw[1], C, dt_id,
                  _stream())

    def _inner(self, maps):
        """The inner maps, the coarsest computed first: list (finest first) of [B H W, C] in the compute dtype."""
        tdt = _DT[self.precision][1]
        inner = [None] * len(maps)
        for l in reversed(range(len(maps))):
            m = maps[l]
            inner[l] = torch.empty((m.shape[0] * m.shape[2] * m.shape[3], self.out_channels), dtype=tdt, device=m.device)
            top = inner[l + 1] if l + 1 < len(maps) else None
            self._lateral(l, m, top, tuple(maps[l + 1].shape[2:]) if top is not None else (0, 0), inner[l])
        return inner

    def _outputs(self, inner, shapes, B, dst, level_pos):
        """The 3x3 convs and the pool into dst [*, C]: level l (of B images) at position level_pos[l]."""
        for l in range(len(inner)):
            self._layer(l, inner[l], B, shapes[l], dst, level_pos[l])
        if self.pool:
            self._subsample(B, shapes[len(inner) - 1], dst, level_pos[len(inner) - 1], level_pos[len(inner)])

    def forward_pyramid(self, x, return_inner=False):
        """x: ordered dict (or list) of fp32 [B, c_l, H_l, W_l] maps, finest first -> (flat [P, out_channels] in the
        compute dtype, level-major with B images per level: the pyramid buffer RPNHead.conv_pyramid reads; shapes of its
        levels, the pool level last).  return_inner=True: also the list of inner maps [B H_l W_l, out_channels]."""
        maps = self._maps(x)
        _, tdt = _DT[self.precision]
        B, C = maps[0].shape[0], self.out_channels
        shapes = self.level_shapes([m.shape[2:] for m in maps])
        level_pos, P = [], 0
        for h, w in shapes:
            level_pos.append(P)
            P += B * h * w
        with torch.no_grad():
            inner = self._inner(maps)
            flat = torch.empty((P, C), dtype=tdt, device=maps[0].device)
            self._outputs(inner, shapes, B, flat, level_pos)
        return (flat, shapes, inner) if return_inner else (flat, shapes)

    def forward(self, x):
        """The drop-in for `backbone.fpn`: ordered dict of fp32 NCHW maps, finest first -> ordered dict with the same
        keys plus 'pool' (with pool=True) of fp32 NCHW maps.  With precision='bf16' the values are bf16-rounded (the
        pyramid is computed and stored in bf16, then widened)."""
        from .module import _planar_levels
        keys = list(x.keys()) if isinstance(x, dict) else [str(i) for i in range(len(x))]
        flat, shapes = self.forward_pyramid(x)
        dt_id, _ = _DT[self.precision]
        C = self.out_channels
        B = flat.shape[0] // sum(h * w for h, w in shapes)
        outs = [torch.empty((B, C, h, w), dtype=torch.float32, device=flat.device) for h, w in shapes]
        _lib.call('sfvos_pyramid_to_frames', _ptr(flat), dt_id, _planar_levels(outs), len(outs), B, C, C, 0, _stream())
        if self.pool:
            keys = keys + ['pool']
        return OrderedDict(zip(keys, outs))

    def write_frames(self, x, seq, first_frame):
        """x: maps of N consecutive frames of ONE video (the batch dimension counts frames); seq: the resident
        PackedClip of that video (batch 1, layout 'ndhwc', out_channels channels in the compute dtype, every frame
        stored: pad (0, 0), the level shapes of `level_shapes`).  Frames first_frame .. first_frame + N - 1 of every
        level are contiguous positions there, so each level's conv (and the pool) writes them in place: no staging copy.
        Bumps seq.data._version, so a SlowFastWindows on the sequence recomputes its first-layer frames."""
        maps = self._maps(x)
        _, tdt = _DT[self.precision]
        N, C = maps[0].shape[0], self.out_channels
        shapes = self.level_shapes([m.shape[2:] for m in maps])
        d = seq.data
        if seq.layout != 'ndhwc':
            raise RuntimeError("write_frames writes 'ndhwc' clips, not the layout %r" % seq.layout)
        if seq.batch != 1 or seq.pad != (0, 0):
            raise RuntimeError('write_frames takes one video (B = 1) with every frame stored, got B=%d pad=%s'
                               % (seq.batch, seq.pad))
        if seq.channels != C or d.dtype != tdt or not d.is_contiguous() or d.device != maps[0].device:
            raise RuntimeError('write_frames: the sequence must hold %d channels of contiguous %s on the device of the '
                               'maps, got %s x %d' % (C, tdt, d.dtype, seq.channels))
        if [tuple(s) for s in seq.shapes] != shapes:
            raise RuntimeError('write_frames: the sequence has levels %s, these maps give %s' % (seq.shapes, shapes))
        first_frame = int(first_frame)
        if first_frame < 0 or first_frame + N > seq.frames:
            raise RuntimeError('write_frames: frames [%d, %d) outside the sequence [0, %d)'
                               % (first_frame, first_frame + N, seq.frames))
        if d.requires_grad:
            raise RuntimeError('write_frames: the sequence must not require grad')
        level_pos, P = [], 0
        for h, w in shapes:   # position(l, 0, first_frame, 0, 0) of include/sfvos.h with B = 1
            level_pos.append(seq.frames * P + first_frame * h * w)
            P += h * w
        with torch.no_grad():
            self._outputs(self._inner(maps), shapes, N, d, level_pos)
            d[:0].zero_()   # an in-place op on an empty slice: the values are the kernels', the version counter moves
        return seq
