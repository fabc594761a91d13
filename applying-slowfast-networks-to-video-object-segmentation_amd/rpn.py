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

Training call (model.py:329-335 passes the targets; the two RPN losses enter the logged total_loss at :361-368): in
training mode with targets, `forward` also returns `loss_objectness` and `loss_rpn_box_reg`, computed by
csrc/rpn_targets.hip -- the IoU matcher with torchvision's low-quality rule, the balanced sampler, BoxCoder(1, 1, 1,
1).encode, BCE-with-logits and smooth-L1.  The sampler draws nothing itself: the caller's key per anchor decides (the
smallest (key, index) pairs of a class are its sample); without keys they come from `torch.rand`, which is torchvision's
randperm draw in distribution, not its random stream.  The losses carry no gradient (the RPN is frozen).

Out of scope: the backbone (body.py, fpn.py), the transform (transform.py; its ImageList is what `forward` takes) and any
backward."""
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
    """torchvision's RegionProposalNetwork without a backward: head, anchors, per-level top-k, decode, clip, small-box
    and score filter, per-level NMS, the best post_nms_top_n per image; in training mode with targets also the two RPN
    losses (anchor targets, balanced sampler, BCE and smooth-L1 with `smooth_l1_beta`; 0 is the plain L1 of newer
    torchvision releases).  `self.training` picks the top-n, as in torchvision.
    Limits: pre_nms_top_n <= 4096 per level, 8 anchors per position, 8 levels; for the losses 1024 ground-truth boxes per
    image, batch_size_per_image <= 4096 and fewer than 2^24 anchors per image."""

    def __init__(self, anchor_generator=None, head=None, pre_nms_top_n=None, post_nms_top_n=None, nms_thresh=0.7,
                 score_thresh=0.0, min_size=1e-3, precision='fp32', fg_iou_thresh=0.7, bg_iou_thresh=0.3,
                 batch_size_per_image=256, positive_fraction=0.5, smooth_l1_beta=1.0 / 9):
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
        self.fg_iou_thresh, self.bg_iou_thresh = float(fg_iou_thresh), float(bg_iou_thresh)
        self.batch_size_per_image, self.positive_fraction = int(batch_size_per_image), float(positive_fraction)
        self.smooth_l1_beta = float(smooth_l1_beta)

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

    def _anchor_args(self, shapes, tensor_size, dev):
        """(pyramid, A, anchors per image, the C arguments `pyr, A, base_anchors, tensor_h, tensor_w`)."""
        _levels_of(self.anchor_generator, len(shapes))
        pyr, A = _lib.make_pyramid(shapes), self.head.num_anchors
        N = A * sum(int(h) * int(w) for h, w in shapes)
        return pyr, A, N, (ctypes.byref(pyr), A, _ptr(self.anchor_generator.device_table(dev)), int(tensor_size[0]),
                           int(tensor_size[1]))

    def _targets_workspace(self, pyr, A, G, dev):
        nbytes = _lib.load().sfvos_rpn_targets_workspace_bytes(ctypes.byref(pyr), A, G, self.batch_size_per_image)
        if nbytes == 0:
            _lib.check(-1, 'sfvos_rpn_targets_workspace_bytes')
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def _match(self, anchor_args, gt, ws, N):
        labels = torch.empty(N, dtype=torch.int32, device=gt.device)
        matched = torch.empty(N, dtype=torch.int32, device=gt.device)
        G = gt.shape[0]
        _lib.call('sfvos_rpn_match', *anchor_args, _ptr(gt) if G else None, G, self.fg_iou_thresh, self.bg_iou_thresh, 1,
                  _ptr(ws), _ptr(matched), _ptr(labels), None, _stream())
        return labels, matched

    @staticmethod
    def _gt_boxes(boxes):
        _check_gpu(boxes, 'RegionProposalNetwork')
        return _f32(boxes).reshape(-1, 4)

    @torch.no_grad()
    def anchor_targets(self, shapes, tensor_size, gt_boxes):
        """assign_targets_to_anchors of one image: gt_boxes [G, 4] on the device -> (labels int32 [N]: 1 positive, 0
        background, -1 ignored; matched int32 [N]: the ground-truth index of a positive, 0 elsewhere), N = the anchors of
        an image in torchvision's order (level, h, w, a).  Matcher(fg_iou_thresh, bg_iou_thresh,
        allow_low_quality_matches=True); an empty gt_boxes labels everything background."""
        gt = self._gt_boxes(gt_boxes)
        pyr, A, N, args = self._anchor_args(shapes, tensor_size, gt.device)
        return self._match(args, gt, self._targets_workspace(pyr, A, gt.shape[0], gt.device), N)

    @torch.no_grad()
    def compute_loss(self, objectness, deltas, shapes, batch, tensor_size, targets, keys=None):
        """objectness [P, A], deltas [P, 4A] fp32 in level-major order (head_outputs), targets: one dict with 'boxes'
        [G_b, 4] per image -> {'loss_objectness', 'loss_rpn_box_reg'}: 0-dim fp32 device tensors without a gradient.
        keys: one [N] tensor per image, the sampler's order (the smallest keys of a class are sampled); None draws them
        with torch.rand.  One branch, no host synchronisation: capturable in a graph when keys are passed.
        `self.last_sample` keeps (counts [B, 2] = (sampled, positives), index [B, batch_size_per_image])."""
        _check_gpu(objectness, 'RegionProposalNetwork')
        if len(targets) != batch or (keys is not None and len(keys) != batch):
            raise RuntimeError('one target dict (and one key tensor) per image expected')
        dev = objectness.device
        pyr, A, N, args = self._anchor_args(shapes, tensor_size, dev)
        obj, dl = _f32(objectness), _f32(deltas)
        if obj.numel() != batch * N or dl.numel() != 4 * batch * N:
            raise RuntimeError('objectness / deltas do not hold %d images of %d anchors' % (batch, N))
        bs = self.batch_size_per_image
        counts = torch.empty((batch, 2), dtype=torch.int32, device=dev)
        index = torch.empty((batch, bs), dtype=torch.int32, device=dev)
        reg = torch.empty((batch, bs, 4), dtype=torch.float32, device=dev)
        st = _stream()
        for b, t in enumerate(targets):
            gt = self._gt_boxes(t['boxes'])
            G = gt.shape[0]
            ws = self._targets_workspace(pyr, A, G, dev)
            labels, matched = self._match(args, gt, ws, N)
            k = torch.rand(N, dtype=torch.float32, device=dev) if keys is None else _f32(keys[b])
            if k.device != dev or k.numel() != N:
                raise RuntimeError('keys: one value per anchor (%d) on the device expected' % N)
            _lib.call('sfvos_rpn_sample', _ptr(labels), _ptr(matched), _ptr(k), N, *args, _ptr(gt) if G else None, G, bs,
                      self.positive_fraction, _ptr(ws), _ptr(counts[b]), _ptr(index[b]), _ptr(reg[b]), st)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.call('sfvos_rpn_loss', _ptr(obj), _ptr(dl), ctypes.byref(pyr), batch, A, _ptr(index), _ptr(counts), _ptr(reg),
                  bs, self.smooth_l1_beta, None, _ptr(out), st)
        self.last_sample = (counts, index)
        return {'loss_objectness': out[0], 'loss_rpn_box_reg': out[1]}

    def forward(self, images, features, targets=None, keys=None):
        """torchvision's call (model.py:237-238, :329-335): images has `.tensors` (the padded batch) and `.image_sizes`
        -> (list of [n_b, 4] proposals, losses).  losses = compute_loss on the same head outputs when the module is in
        training mode and targets are given (keys: see compute_loss), {} otherwise."""
        tensor_size = tuple(int(v) for v in images.tensors.shape[-2:])
        obj, dl, shapes, B = self.head_outputs(features)
        boxes, _, count, _ = self.filter_proposals(obj, dl, shapes, B, list(images.image_sizes), tensor_size)
        losses = {}
        if self.training and targets is not None:
            losses = self.compute_loss(obj, dl, shapes, B, tensor_size, targets, keys)
        return [boxes[b, :n] for b, n in enumerate(count.tolist())], losses
