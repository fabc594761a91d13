"""The region proposal network of the reference's Mask R-CNN (code/helpers/model.py:236-240, called at :329-335), on
libsfvos kernels: raw FPN maps -> proposals for `roi_heads` (`RoIHeadsInference`, `BoxBranch`).

The reference freezes the RPN (model.py:178-179) and runs it under `no_grad`, so this is inference only.  torchvision is
third-party, not vendored and absent in this build's environment: these classes mirror its published module structure
(`RPNHead`, `AnchorGenerator`, `RegionProposalNetwork`; same attribute names and state-dict keys, so the `rpn.head.*`
slice of a reference checkpoint loads with strict=True) and their results are checked against a torch-core restatement
(tests/rpn_ref.py) -- PARITY UNPINNED BY THE REFERENCE.  No CPU fallback.

Order of the proposals, everywhere: objectness logit descending, ties by (level, anchor index) ascending; values compare
as floats (-0 == +0, +-inf ordinary).  A NaN logit ranks below every number (torch.topk ranks it above); it can never
become a proposal, because its score fails the score threshold.  Where torchvision's order is unspecified (ties,
saturated sigmoids) this rule is the contract.

Out of scope: `loss_objectness` / `loss_rpn_box_reg` (the IoU matcher and the balanced sampler draw with torch's RNG; the
RPN is frozen, the reference only logs them): `forward` returns `{}` for the losses.  The backbone, the transform and any
backward are out of scope too."""
import ctypes
import math

import torch
from torch import nn

from . import _lib
from ._heads import _check_precision, _pack
from ._lib import _DT, _check_gpu, _conv_desc, _f32, _ptr, _stream

BBOX_XFORM_CLIP = math.log(1000.0 / 16)
MAX_PRE_NMS = 4096
MAX_ANCHORS = 8


class AnchorGenerator(object):
    """torchvision's AnchorGenerator(sizes, aspect_ratios): one tuple of sizes and one of ratios per level, the same
    number of anchors A per position on every level.  `base_anchors()` is the [L, A, 4] fp32 table the kernel reads (made
    once with torch on the CPU: round half to even, as torch.round); the anchors themselves are never materialised on
    the hot path, `grid_anchors` builds them as tensors for tests and callers."""

    def __init__(self, sizes=((32,), (64,), (128,), (256,), (512,)), aspect_ratios=((0.5, 1.0, 2.0),) * 5):
        if not isinstance(sizes[0], (list, tuple)):
            sizes = tuple((s,) for s in sizes)
        if not isinstance(aspect_ratios[0], (list, tuple)):
            aspect_ratios = (tuple(aspect_ratios),) * len(sizes)
        if len(sizes) != len(aspect_ratios):
            raise ValueError('AnchorGenerator: one tuple of sizes and one of aspect ratios per level')
        self.sizes = tuple(tuple(s) for s in sizes)
        self.aspect_ratios = tuple(tuple(a) for a in aspect_ratios)
        counts = set(len(s) * len(a) for s, a in zip(self.sizes, self.aspect_ratios))
        if len(counts) != 1:
            raise ValueError('AnchorGenerator: every level must have the same number of anchors per position')
        self._device_tables = {}

    def num_anchors_per_location(self):
        return [len(s) * len(a) for s, a in zip(self.sizes, self.aspect_ratios)]

    def base_anchors(self):
        """[L, A, 4] fp32 on the CPU: round([-w_r s, -h_r s, w_r s, h_r s] / 2), h_r = sqrt(ratio), w_r = 1 / h_r."""
        rows = []
        for sizes, ratios in zip(self.sizes, self.aspect_ratios):
            scales = torch.as_tensor(sizes, dtype=torch.float32)
            ar = torch.as_tensor(ratios, dtype=torch.float32)
            h_r = torch.sqrt(ar)
            w_r = 1 / h_r
            ws = (w_r[:, None] * scales[None, :]).view(-1)
            hs = (h_r[:, None] * scales[None, :]).view(-1)
            rows.append((torch.stack([-ws, -hs, ws, hs], dim=1) / 2).round())
        return torch.stack(rows)

    def device_table(self, device):
        key = str(device)
        if key not in self._device_tables:
            self._device_tables[key] = self.base_anchors().to(device).contiguous()
        return self._device_tables[key]

    def grid_anchors(self, shapes, tensor_size):
        """Anchors of every level as [H_l W_l A, 4] fp32 CPU tensors in (h, w, a) order; strides = tensor_size // shape
        (the padded batch tensor's size)."""
        base = self.base_anchors()
        out = []
        for l, (H, W) in enumerate(shapes):
            sh, sw = int(tensor_size[0]) // int(H), int(tensor_size[1]) // int(W)
            ys = torch.arange(0, H, dtype=torch.int32) * sh
            xs = torch.arange(0, W, dtype=torch.int32) * sw
            sy, sx = torch.meshgrid(ys, xs, indexing='ij')
            shifts = torch.stack([sx.reshape(-1), sy.reshape(-1), sx.reshape(-1), sy.reshape(-1)], dim=1).float()
            out.append((shifts.view(-1, 1, 4) + base[l].view(1, -1, 4)).reshape(-1, 4))
        return out


def _levels_of(anchor_generator, n):
    if len(anchor_generator.sizes) != n:
        raise RuntimeError('the anchor generator has %d levels, the features %d' % (len(anchor_generator.sizes), n))


class RPNHead(nn.Module):
    """torchvision's RPNHead(in_channels, num_anchors): conv (3x3 + ReLU), cls_logits (1x1 -> A), bbox_pred (1x1 -> 4A)
    under torchvision's parameter names; the newer `conv.0.0.*` spelling of the first conv loads too.  The conv is one
    sfvos_conv3d launch over the whole pyramid (kt = 1), the two 1x1 heads one sfvos_box_predictor launch.  Inference
    only: it raises when a gradient would be needed."""

    def __init__(self, in_channels=256, num_anchors=3, precision='fp32'):
        super(RPNHead, self).__init__()
        self.precision = _check_precision(precision)
        if not 1 <= num_anchors <= MAX_ANCHORS:
            raise ValueError('RPNHead: 1..%d anchors per position are implemented' % MAX_ANCHORS)
        if in_channels % 32 != 0:
            raise ValueError('RPNHead: in_channels must be a multiple of 32')
        self.conv = nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1)
        self.cls_logits = nn.Conv2d(in_channels, num_anchors, kernel_size=1, stride=1)
        self.bbox_pred = nn.Conv2d(in_channels, num_anchors * 4, kernel_size=1, stride=1)
        for layer in (self.conv, self.cls_logits, self.bbox_pred):   # torchvision's init
            nn.init.normal_(layer.weight, std=0.01)
            nn.init.constant_(layer.bias, 0)
        self._images = _lib.WeightImages()

    @property
    def num_anchors(self):
        return self.cls_logits.out_channels

    def _load_from_state_dict(self, state_dict, prefix, *args, **kw):
        for name in ('weight', 'bias'):
            new = prefix + 'conv.0.0.' + name
            if new in state_dict:
                state_dict[prefix + 'conv.' + name] = state_dict.pop(new)
        super(RPNHead, self)._load_from_state_dict(state_dict, prefix, *args, **kw)

    def _check_inference(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise RuntimeError('RPNHead is inference only (the reference freezes the RPN): call it under '
                               'torch.no_grad() or freeze its parameters')

    def conv_pyramid(self, x, shapes, batch, t_alloc=1, t_offset=0):
        """relu(conv3x3(x)) over the whole pyramid in one launch.  x: a pyramid buffer in the compute dtype ([M, C], or
        channel groups [C/32, M, 32]) with t_alloc frames per image, of which frame t_offset is read -> [P, C] in the
        compute dtype, P = batch * sum H W positions in level-major order."""
        dt_id, tdt = _DT[self.precision]
        C = self.conv.in_channels
        P = batch * sum(h * w for h, w in shapes)
        d = _conv_desc(dt_id, batch, _lib.make_pyramid(shapes), 1, 9, C, C, 1, x, C, t_alloc, t_offset, relu=1)
        w = self.conv.weight
        packed = self._images.get(('conv', dt_id), (w,), _pack, 'sfvos_pack_weights_fwd', w, dt_id, tdt, C, C, 1, 9)
        t = torch.empty((P, C), dtype=tdt, device=x.device)
        _lib.call('sfvos_conv3d', ctypes.byref(d), _ptr(x), _ptr(packed), _ptr(_f32(self.conv.bias)), _ptr(t), None,
                  _stream())
        return t

    def predict(self, t):
        """cls_logits and bbox_pred on t [P, C] -> (objectness [P, A], deltas [P, 4A]) fp32, one launch; the weights are
        read as fp32 masters."""
        dt_id, _ = _DT[self.precision]
        (P, C), A = t.shape, self.num_anchors
        objectness = torch.empty((P, A), dtype=torch.float32, device=t.device)
        deltas = torch.empty((P, 4 * A), dtype=torch.float32, device=t.device)
        wc, bc = _f32(self.cls_logits.weight).view(A, C), _f32(self.cls_logits.bias)
        wb, bb = _f32(self.bbox_pred.weight).view(4 * A, C), _f32(self.bbox_pred.bias)
        _lib.call('sfvos_box_predictor', _ptr(t), dt_id, _ptr(wc), _ptr(bc), _ptr(wb), _ptr(bb), P, C, A, _ptr(objectness),
                  _ptr(deltas), _stream())
        return objectness, deltas

    def forward_pyramid(self, x, shapes, batch, t_alloc=1, t_offset=0):
        """conv_pyramid + predict."""
        return self.predict(self.conv_pyramid(x, shapes, batch, t_alloc, t_offset))

    def maps_to_pyramid(self, maps):
        """list of [B, C, H, W] fp32 maps -> the pyramid buffer [P, C] in the compute dtype (one launch)."""
        from .module import _planar_levels
        dt_id, tdt = _DT[self.precision]
        B, C = maps[0].shape[0], maps[0].shape[1]
        maps = [m.detach() if m.dtype == torch.float32 else m.detach().float() for m in maps]
        flat = torch.empty((B * sum(m.shape[2] * m.shape[3] for m in maps), C), dtype=tdt, device=maps[0].device)
        _lib.call('sfvos_frames_to_pyramid', _planar_levels(maps), len(maps), _ptr(flat), dt_id, B, C, C, _stream())
        return flat

    def forward(self, x):
        """list of [B, C, H, W] maps -> (list of objectness [B, A, H, W], list of deltas [B, 4A, H, W]) fp32 (views of
        the channels-last results)."""
        x = list(x)
        _check_gpu(x[0], 'RPNHead')
        self._check_inference(x[0])
        if len(x) > _lib.MAX_LEVELS:
            raise RuntimeError('at most %d pyramid levels per call' % _lib.MAX_LEVELS)
        B = x[0].shape[0]
        shapes = [tuple(m.shape[2:]) for m in x]
        obj, dl = self.forward_pyramid(self.maps_to_pyramid(x), shapes, B)
        logits, deltas, off = [], [], 0
        for H, W in shapes:
            n = B * H * W
            logits.append(obj[off:off + n].view(B, H, W, -1).permute(0, 3, 1, 2))
            deltas.append(dl[off:off + n].view(B, H, W, -1).permute(0, 3, 1, 2))
            off += n
        return logits, deltas


class RegionProposalNetwork(nn.Module):
    """torchvision's RegionProposalNetwork in inference: head, anchors, per-level top-k, decode, clip, small-box and
    score filter, per-level NMS, the best post_nms_top_n per image.  `self.training` picks the top-n, as in torchvision.
    Limits: pre_nms_top_n <= 4096 per level, 8 anchors per position, 8 levels."""

    def __init__(self, anchor_generator=None, head=None, pre_nms_top_n=None, post_nms_top_n=None, nms_thresh=0.7,
                 score_thresh=0.0, min_size=1e-3, precision='fp32'):
        super(RegionProposalNetwork, self).__init__()
        self.anchor_generator = anchor_generator if anchor_generator is not None else AnchorGenerator()
        A = self.anchor_generator.num_anchors_per_location()[0]
        self.head = head if head is not None else RPNHead(256, A, precision)
        if self.head.num_anchors != A:
            raise ValueError('the head predicts %d anchors per position, the generator makes %d'
                             % (self.head.num_anchors, A))
        self._pre_nms_top_n = dict(pre_nms_top_n or dict(training=2000, testing=1000))
        self._post_nms_top_n = dict(post_nms_top_n or dict(training=2000, testing=1000))
        self.nms_thresh, self.score_thresh, self.min_size = float(nms_thresh), float(score_thresh), float(min_size)
        self._size_tables = {}

    def pre_nms_top_n(self):
        return int(self._pre_nms_top_n['training' if self.training else 'testing'])

    def post_nms_top_n(self):
        return int(self._post_nms_top_n['training' if self.training else 'testing'])

    def _sizes_on(self, image_sizes, device):
        """image sizes (height, width) as a device table [B, 2] fp32, made once per distinct list (a host-to-device
        copy: outside a graph capture the first time)."""
        key = (str(device), tuple((float(h), float(w)) for h, w in image_sizes))
        if key not in self._size_tables:
            if len(self._size_tables) > 64:
                self._size_tables.clear()
            self._size_tables[key] = torch.tensor(key[1], dtype=torch.float32).to(device)
        return self._size_tables[key]

    @torch.no_grad()
    def filter_proposals(self, objectness, deltas, shapes, batch, image_sizes, tensor_size):
        """objectness [P, A], deltas [P, 4A] fp32 in level-major order -> (boxes [B, post, 4], scores [B, post],
        count [B] int32, index [B, post] int32), zeros / -1 behind the count.  index = level * pre_nms_top_n + rank of the
        proposal in its level's selection; `self.last_selection` keeps (counts, anchor index) of that selection."""
        _check_gpu(objectness, 'RegionProposalNetwork')
        lib = _lib.load()
        _levels_of(self.anchor_generator, len(shapes))
        if len(image_sizes) != batch:
            raise RuntimeError('one image size per image expected')
        dev = objectness.device
        A, k, post = self.head.num_anchors, self.pre_nms_top_n(), self.post_nms_top_n()
        if not 1 <= k <= MAX_PRE_NMS:
            raise RuntimeError('pre_nms_top_n %d out of [1, %d]' % (k, MAX_PRE_NMS))
        pyr = _lib.make_pyramid(shapes)
        S = len(shapes) * batch
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        counts, index = torch.empty(S, **i32), torch.empty((S, k), **i32)
        obj, dl = _f32(objectness), _f32(deltas)
        st = _stream()
        _lib.call('sfvos_rpn_select', _ptr(obj), ctypes.byref(pyr), batch, A, k, _ptr(counts), _ptr(index), st)
        boxes, logits = torch.empty((S, k, 4), **f32), torch.empty((S, k), **f32)
        scores, valid = torch.empty((S, k), **f32), torch.empty((S, k), **i32)
        _lib.call('sfvos_rpn_decode', _ptr(obj), _ptr(dl), _ptr(counts), _ptr(index), ctypes.byref(pyr), batch, A, k,
                  _ptr(self.anchor_generator.device_table(dev)), int(tensor_size[0]), int(tensor_size[1]),
                  _ptr(self._sizes_on(image_sizes, dev)), BBOX_XFORM_CLIP, self.min_size, self.score_thresh, _ptr(boxes),
                  _ptr(logits), _ptr(scores), _ptr(valid), st)
        ws = torch.empty(lib.sfvos_rpn_workspace_bytes(len(shapes), batch, k), dtype=torch.uint8, device=dev)
        ob, osc = torch.empty((batch, post, 4), **f32), torch.empty((batch, post), **f32)
        oi, cnt = torch.empty((batch, post), **i32), torch.empty(batch, **i32)
        _lib.call('sfvos_rpn_nms', _ptr(boxes), _ptr(logits), _ptr(scores), _ptr(valid), _ptr(counts), len(shapes), batch,
                  k, self.nms_thresh, post, _ptr(ws), _ptr(ob), _ptr(osc), _ptr(oi), _ptr(cnt), st)
        self.last_selection = (counts, index)
        return ob, osc, cnt, oi

    def _maps(self, features):
        maps = list(features.values()) if isinstance(features, dict) else list(features)
        _check_gpu(maps[0], 'RegionProposalNetwork')
        self.head._check_inference(maps[0])
        if len(maps) > _lib.MAX_LEVELS:
            raise RuntimeError('at most %d pyramid levels per call' % _lib.MAX_LEVELS)
        return maps

    def head_outputs(self, features):
        """(objectness [P, A], deltas [P, 4A], shapes, batch) of an ordered dict of [B, C, H, W] fp32 maps."""
        maps = self._maps(features)
        shapes, B = [tuple(m.shape[2:]) for m in maps], maps[0].shape[0]
        with torch.no_grad():
            obj, dl = self.head.forward_pyramid(self.head.maps_to_pyramid(maps), shapes, B)
        return obj, dl, shapes, B

    def propose_padded(self, features, image_sizes, tensor_size):
        """features: ordered dict of fp32 [B, C, H, W] maps; image_sizes: list of (height, width) per image (unpadded);
        tensor_size: (height, width) of the padded batch tensor -> (boxes [B, post, 4], scores [B, post], count [B]) on
        the device, no host synchronisation: capturable in a graph."""
        obj, dl, shapes, B = self.head_outputs(features)
        return self.filter_proposals(obj, dl, shapes, B, image_sizes, tensor_size)[:3]

    def propose(self, features, image_sizes, tensor_size):
        """-> list of [n_b, 4] proposals per image (one synchronisation, for the counts)."""
        boxes, _, count = self.propose_padded(features, image_sizes, tensor_size)
        return [boxes[b, :n] for b, n in enumerate(count.tolist())]

    def propose_packed(self, clip, frame=None, image_sizes=None, tensor_size=None):
        """Proposals from one frame of a resident PackedClip ('ndhwc' or 'grouped'), read in place through the conv
        descriptor (no layout pass, no copy) -> as propose_padded.  frame: index among the STORED frames; default the
        centre of the fast window, clip.window // 2 - clip.pad[0]."""
        _check_gpu(clip.data, 'RegionProposalNetwork')
        self.head._check_inference(clip.data)
        _, tdt = _DT[self.head.precision]
        if clip.layout == 'grouped8':
            raise RuntimeError("propose_packed reads 'ndhwc' or 'grouped' clips, not the e4m3 layout 'grouped8'")
        if clip.data.dtype != tdt or not clip.data.is_contiguous() or clip.channels != self.head.conv.in_channels:
            raise RuntimeError('propose_packed: the clip must hold %d channels of contiguous %s'
                               % (self.head.conv.in_channels, tdt))
        if frame is None:
            frame = clip.window // 2 - clip.pad[0]
        if not 0 <= frame < clip.frames:
            raise RuntimeError('propose_packed: frame %d is a zero-padding frame of the window (stored frames: [0, %d))'
                               % (frame, clip.frames))
        if image_sizes is None or tensor_size is None:
            raise RuntimeError('propose_packed: image_sizes and tensor_size are required')
        if len(clip.shapes) > _lib.MAX_LEVELS:
            raise RuntimeError('at most %d pyramid levels per call' % _lib.MAX_LEVELS)
        with torch.no_grad():
            obj, dl = self.head.forward_pyramid(clip.data, clip.shapes, clip.batch, clip.frames, int(frame))
        return self.filter_proposals(obj, dl, clip.shapes, clip.batch, image_sizes, tensor_size)[:3]

    def forward(self, images, features, targets=None):
        """torchvision's call (model.py:237-238): images has `.tensors` (the padded batch) and `.image_sizes` ->
        (list of [n_b, 4] proposals, {}): the RPN losses are out of scope."""
        tensor_size = tuple(int(v) for v in images.tensors.shape[-2:])
        return self.propose(features, list(images.image_sizes), tensor_size), {}
