"""`roi_heads` as the reference trains it (code/helpers/model.py:346 with targets, `losses.backward()` at :369), on
libsfvos kernels: the step from proposals + ground truth to the arguments of the losses, and the module that holds both
branches under torchvision's names.

torchvision's `RoIHeads.forward` in training is `select_training_samples` (append the ground-truth boxes to the proposals,
`Matcher(0.5, 0.5)` on the IoU, `BalancedPositiveNegativeSampler(512, 0.25)`, `BoxCoder(10, 10, 5, 5).encode`), the box
branch + `fastrcnn_loss`, and the mask branch on the positive samples + `maskrcnn_loss`, whose targets are
`project_masks_on_boxes`: the RoIAlign (adaptive sampling grid) of each positive's ground-truth mask onto its box, 28 x 28.
Both steps run in csrc/roi_targets.hip; the branches and losses are box_head.py's and mask_head.py's.

torchvision is third-party, not vendored and absent in this build's environment: the arithmetic restates its published
sources and is checked against tests/roi_targets_ref.py -- PARITY UNPINNED BY THE REFERENCE.  No CPU fallback.

One deviation: the sampler's only random input is a tensor of keys, one per candidate; the n
candidates of a class with the smallest (key, index) pairs are its sample.  With independent uniform keys that is a
uniformly random subset without replacement, which is what torchvision's `randperm` draws -- the same distribution, not
the same stream of random numbers."""
import torch
from torch import nn

from . import _lib
from ._lib import _check_gpu, _f32, _ptr, _stream
from .box_head import BOX_WEIGHTS, BoxBranch, detect_with_masks, fastrcnn_loss
from .mask_head import MaskBranch, maskrcnn_loss
from .roi_align import MultiScaleRoIAlign

MASK_TARGET_SIZE = 28


def check_targets(targets, need_masks=False):
    """torchvision's RoIHeads.check_targets and the dtype checks of RoIHeads.forward."""
    if targets is None:
        raise ValueError('targets should not be None')
    if not all('boxes' in t for t in targets):
        raise ValueError('Every element of targets should have a boxes key')
    if not all('labels' in t for t in targets):
        raise ValueError('Every element of targets should have a labels key')
    if need_masks and not all('masks' in t for t in targets):
        raise ValueError('Every element of targets should have a masks key')
    for t in targets:
        if t['boxes'].dtype not in (torch.float, torch.double, torch.half):
            raise TypeError('target boxes must of float type, instead got %s' % t['boxes'].dtype)
        if t['labels'].dtype != torch.int64:
            raise TypeError('target labels must of int64 type, instead got %s' % t['labels'].dtype)


def _sample(proposals, targets, keys, generator, batch_size_per_image, positive_fraction, fg_iou_thresh, bg_iou_thresh):
    """-> per image (boxes [S,4], matched [S] int32, labels [S] int64, regression_targets [S,4], pos_slot [P] int32).
    Everything stays on the device; the (S, P) counts of all images come back in one copy."""
    check_targets(targets)
    if len(proposals) != len(targets) or (keys is not None and len(keys) != len(proposals)):
        raise ValueError('select_training_samples: one target (and one key tensor) per image expected')
    if not proposals:
        return []
    _check_gpu(proposals[0], 'select_training_samples')
    dev = proposals[0].device
    lib = _lib.load()
    B, batch = len(proposals), int(batch_size_per_image)
    i32 = dict(dtype=torch.int32, device=dev)
    counts = torch.zeros((B, 2), **i32)
    rows = []
    for b, (props, t) in enumerate(zip(proposals, targets)):
        p = _f32(props, dev)
        gt = _f32(t['boxes'], dev).reshape(-1, 4)
        gl = t['labels'].to(dev).contiguous()
        n_p, G = p.shape[0], gt.shape[0]
        N = n_p + G
        if gl.numel() != G:
            raise ValueError('select_training_samples: %d boxes but %d labels in image %d' % (G, gl.numel(), b))
        if keys is None:
            k = torch.rand(N, dtype=torch.float32, device=dev, generator=generator)
        else:
            k = _f32(keys[b], dev)
            if k.numel() != N:
                raise ValueError('select_training_samples: %d keys for %d proposals + %d ground-truth boxes in image %d'
                                 % (k.numel(), n_p, G, b))
        matched = torch.empty(N, **i32)
        labels = torch.empty(N, dtype=torch.int64, device=dev)
        _lib.call('sfvos_roi_match', _ptr(p) if n_p else None, n_p, _ptr(gt) if G else None, _ptr(gl) if G else None, G,
                  float(fg_iou_thresh), float(bg_iou_thresh), _ptr(matched), _ptr(labels), None, _stream())
        nbytes = lib.sfvos_roi_sample_workspace_bytes(N)
        if not nbytes:
            raise RuntimeError('select_training_samples: %d candidates in image %d, the kernels take 8192' % (N, b))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = (torch.empty(batch, **i32), torch.empty((batch, 4), dtype=torch.float32, device=dev),
               torch.empty(batch, dtype=torch.int64, device=dev), torch.empty(batch, **i32),
               torch.empty((batch, 4), dtype=torch.float32, device=dev), torch.empty(batch, **i32))
        _lib.call('sfvos_roi_sample', _ptr(labels) if N else None, _ptr(matched) if N else None, _ptr(k) if N else None,
                  _ptr(p) if n_p else None, n_p, _ptr(gt) if G else None, G, batch, float(positive_fraction),
                  *(tuple(float(w) for w in BOX_WEIGHTS) + (_ptr(ws), _ptr(counts, 2 * b)) +
                    tuple(_ptr(o) for o in out) + (_stream(),)))
        rows.append(out)
    host = counts.cpu()      # the one synchronisation of the call
    res = []
    for b, (index, boxes, labels, matched, targets_, pos_slot) in enumerate(rows):
        S, P = int(host[b, 0]), int(host[b, 1])
        res.append((boxes[:S], matched[:S], labels[:S], targets_[:S], pos_slot[:P]))
    return res


def select_training_samples(proposals, targets, keys=None, generator=None, batch_size_per_image=512,
                            positive_fraction=0.25, fg_iou_thresh=0.5, bg_iou_thresh=0.5):
    """torchvision's RoIHeads.select_training_samples: proposals (list of [n_i,4]) and targets (list of dicts with 'boxes'
    [G_i,4] and 'labels' [G_i] int64) -> (proposals, matched_idxs, labels, regression_targets), lists per image of the
    sampled rows in ascending candidate index (candidates = the proposals followed by the ground-truth boxes).

    keys: a list of fp32 device tensors of n_i + G_i keys each -- the sampler's only random input (module docstring) --
    or None: they are drawn with torch.rand(..., generator=generator) on the device."""
    res = _sample(proposals, targets, keys, generator, batch_size_per_image, positive_fraction, fg_iou_thresh,
                  bg_iou_thresh)
    return ([r[0] for r in res], [r[1].long() for r in res], [r[2] for r in res], [r[3] for r in res])


def project_masks_on_boxes(gt_masks, boxes, matched_idxs, M):
    """torchvision's roi_heads.project_masks_on_boxes: gt_masks [G,H,W] (uint8, bool or floating), boxes [P,4],
    matched_idxs [P] -> [P,M,M] fp32, the RoIAlign (adaptive grid, aligned=False) of mask matched_idxs[i] onto boxes[i].
    uint8 masks are read as they are (bool is viewed as uint8), other floating types are converted to fp32."""
    _check_gpu(boxes, 'project_masks_on_boxes')
    dev = boxes.device
    b = _f32(boxes, dev).reshape(-1, 4)
    P, M = b.shape[0], int(M)
    out = torch.empty((P, M, M), dtype=torch.float32, device=dev)
    if gt_masks.dim() != 3:
        raise ValueError('project_masks_on_boxes: masks [G,H,W] expected, got %s' % (tuple(gt_masks.shape),))
    m = gt_masks.detach().to(dev)
    if m.dtype == torch.bool:
        m = m.contiguous().view(torch.uint8)
    elif m.dtype != torch.uint8:
        m = m.to(torch.float32)
    m = m.contiguous()
    idx = matched_idxs.detach().to(device=dev, dtype=torch.int32).contiguous()
    if idx.numel() != P:
        raise ValueError('project_masks_on_boxes: one matched index per box expected')
    G, H, W = m.shape
    _lib.call('sfvos_mask_targets', _ptr(m) if G else None, int(m.dtype == torch.uint8), G, H, W,
              _ptr(b) if P else None, _ptr(idx) if P else None, P, M, _ptr(out) if P else None, _stream())
    return out


class RoIHeads(nn.Module):
    """torchvision's RoIHeads for the reference's configuration, with its modules under torchvision's names
    (`box_roi_pool`, `box_head`, `box_predictor`, `mask_roi_pool`, `mask_head`, `mask_predictor`): the `roi_heads.*` slice
    of a reference checkpoint loads with strict=True.  The modules are those of a BoxBranch and a MaskBranch, which this
    class holds outside the module registry and whose code it runs.

    forward(features, proposals, image_shapes, targets=None, keys=None) -> (detections, losses):
      training: ([], {'loss_classifier', 'loss_box_reg', 'loss_mask'}); targets: per image 'boxes', 'labels', 'masks'
                [G,H,W]; keys: select_training_samples' (None: drawn with torch.rand);
      eval    : (what RoIHeadsInference returns with the same weights, {}); with `paste_masks = False` (MaskRCNN sets it)
                'masks' are the [D,1,28,28] probabilities torchvision's roi_heads returns, for transform.postprocess.
    `score_thresh`, `nms_thresh` and `detections_per_img` are read at call time (model.py:187 sets the last one after
    construction)."""

    def __init__(self, num_classes=2, precision='fp32', box_score_thresh=0.05, box_nms_thresh=0.5,
                 box_detections_per_img=100, box_batch_size_per_image=512, box_positive_fraction=0.25,
                 box_fg_iou_thresh=0.5, box_bg_iou_thresh=0.5):
        super(RoIHeads, self).__init__()
        box = BoxBranch(num_classes, precision, box_score_thresh, box_nms_thresh, box_detections_per_img)
        mask = MaskBranch(256, num_classes, precision)
        self.box_roi_pool, self.box_head, self.box_predictor = box.box_roi_pool, box.box_head, box.box_predictor
        self.mask_roi_pool = MultiScaleRoIAlign(['0', '1', '2', '3'], 14, 2)
        self.mask_head, self.mask_predictor = mask.mask_head, mask.mask_predictor
        # The two branches stay outside the module registry, so that the key set is torchvision's.  That rests on an
        # assumption: a BoxBranch / MaskBranch owns no parameter, no buffer and no training-dependent state beside its
        # registered children (shared with this module, which .to(), .train() and .eval() therefore reach), and never
        # reads its own `self.training`.  tests/test_roi_targets_entry_points_cpu.py pins the first half.
        self.__dict__['_box'], self.__dict__['_mask'] = box, mask
        self.score_thresh, self.nms_thresh = float(box_score_thresh), float(box_nms_thresh)
        self.detections_per_img = int(box_detections_per_img)
        self.batch_size_per_image, self.positive_fraction = int(box_batch_size_per_image), float(box_positive_fraction)
        self.fg_iou_thresh, self.bg_iou_thresh = float(box_fg_iou_thresh), float(box_bg_iou_thresh)
        self.paste_masks = True     # False (MaskRCNN): 'masks' stay [D,1,28,28] for transform.postprocess, as in torchvision

    def _branches(self):
        box, mask = self._box, self._mask
        box.score_thresh, box.nms_thresh = float(self.score_thresh), float(self.nms_thresh)
        box.detections_per_img = int(self.detections_per_img)
        return box, mask

    def forward(self, features, proposals, image_shapes, targets=None, keys=None):
        box, mask = self._branches()
        if not self.training:
            return detect_with_masks(box, self.mask_roi_pool, mask, features, proposals, image_shapes,
                                     paste=self.paste_masks), {}
        check_targets(targets, need_masks=True)
        res = _sample(proposals, targets, keys, None, self.batch_size_per_image, self.positive_fraction,
                      self.fg_iou_thresh, self.bg_iou_thresh)
        boxes = [r[0] for r in res]
        labels = [r[2] for r in res]
        logits, deltas = box(features, boxes, image_shapes)
        loss_classifier, loss_box_reg = fastrcnn_loss(logits, deltas, labels, [r[3] for r in res])
        pos = [r[4].long() for r in res]
        mask_boxes = [bx[p] for bx, p in zip(boxes, pos)]
        mask_labels = torch.cat([lb[p] for lb, p in zip(labels, pos)], 0)
        mask_logits = mask(self.mask_roi_pool(features, mask_boxes, image_shapes))
        M = mask_logits.shape[-1]
        mask_targets = torch.cat([project_masks_on_boxes(t['masks'], bx, r[1][p], M)
                                  for t, bx, r, p in zip(targets, mask_boxes, res, pos)], 0)
        loss_mask = maskrcnn_loss(mask_logits, mask_labels, mask_targets)
        if mask_logits.shape[0] == 0 and torch.is_grad_enabled():
            # no positive sample: the zero stays on the graph of the mask parameters (with or without a gradient of the maps)
            loss_mask = loss_mask + sum(p.sum() for p in mask.parameters() if p.requires_grad) * 0
        return [], {'loss_classifier': loss_classifier, 'loss_box_reg': loss_box_reg, 'loss_mask': loss_mask}
