"""The transform of the reference's Mask R-CNN (code/helpers/model.py:283 on every frame of a sequence, :298 on the frames
with targets, `transform.postprocess` at :347) on libsfvos kernels, and `MaskRCNN`, the object the reference builds with
`get_model_instance_segmentation` (:172-173): the transform, `BackboneWithFPN`, `RegionProposalNetwork` and `RoIHeads`
under torchvision's attribute names, so that the whole of `maskrcnn_model.pth` loads with strict=True.

torchvision is third-party, not vendored and absent in this build's environment: `GeneralizedRCNNTransform`, `ImageList`
and `MaskRCNN` mirror its published classes and are checked against a torch-core restatement (tests/transform_ref.py,
whose core is torch's own F.interpolate on the CPU in float64) -- PARITY UNPINNED BY THE REFERENCE.  No CPU fallback.

Which rule: the resize is `F.interpolate(image[None], scale_factor=s, mode='bilinear', recompute_scale_factor=True,
align_corners=False)` -- the output size is floor(in * s) and the kernel's scale is in / out, what torchvision has done
since it passes recompute_scale_factor=True.  The older behaviour (the scale factor itself in the kernel) is not
implemented.  s = min(min_size / min(h, w), max_size / max(h, w)) is evaluated in Python floats, as torchvision 0.7 / 0.8
did; that takes the reference's 480 x 854 frames to 749 x 1333.  Later torchvision releases
evaluate s on float32 tensors, where 854 * float32(1333 / 854) = 1332.99992 floors to 1332: for about half of all sizes
one side is a pixel shorter there.  The kernels take oh and ow as arguments, so either rule can drive them.

One sfvos_transform_image launch per call on a single tensor, or per image of a list, normalises, resizes and zero-pads
straight into the batched tensor `ResNetBody` reads; target masks take one sfvos_transform_masks launch per image, boxes
the existing `resize_boxes`.

Out of scope: any backward (the reference's images never require grad), bf16 or channels-last output, images of
different sizes in one launch, torchvision's random stream for a tuple of training sizes (the draw is the same in
distribution), keypoints, and the dataset's ToTensor on PIL images (a uint8 [N, h, w, 3] tensor is read in place)."""
import math

import torch
from torch import nn

from . import _lib
from ._lib import _check_gpu, _ptr, _stream
from .body import BackboneWithFPN
from .box_head import resize_boxes
from .mask_head import paste_masks_in_image
from .roi_heads import RoIHeads
from .rpn import RegionProposalNetwork


class ImageList(object):
    """torchvision's ImageList: `tensors` [N, 3, Hp, Wp] (the padded batch) and `image_sizes`, the (height, width) of
    each image inside it before the pad."""

    def __init__(self, tensors, image_sizes):
        self.tensors = tensors
        self.image_sizes = [tuple(int(v) for v in s) for s in image_sizes]

    def to(self, device):
        return ImageList(self.tensors.to(device), self.image_sizes)


def resize_masks(masks, size):
    """F.interpolate(masks[:, None].float(), size=size)[:, 0].byte() of masks [G, h, w] (uint8 or bool) -> uint8
    [G, oh, ow]: the nearest resize of torchvision's transform, one launch, dense as sfvos_mask_targets reads it."""
    _check_gpu(masks, 'resize_masks')
    if masks.dim() != 3 or masks.dtype not in (torch.uint8, torch.bool):
        raise RuntimeError('resize_masks: uint8 or bool masks [G, h, w] expected, got %s %s' % (masks.dtype,
                                                                                               tuple(masks.shape)))
    m = masks.detach().contiguous()
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    G, h, w = m.shape
    oh, ow = int(size[0]), int(size[1])
    out = torch.empty((G, oh, ow), dtype=torch.uint8, device=m.device)
    _lib.call('sfvos_transform_masks', _ptr(m) if G else None, G, h, w, _ptr(out) if G else None, oh, ow, _stream())
    return out


class GeneralizedRCNNTransform(nn.Module):
    """torchvision's GeneralizedRCNNTransform(min_size, max_size, image_mean, image_std, size_divisible=32): normalize,
    resize (the rule of the module docstring) and batch_images in one launch per image tensor; no parameters.

    forward(images, targets=None) -> (ImageList, targets).  images: a list of float [3, h, w] tensors (one launch each,
    all into one batch tensor sized to the largest resized image, rounded up to size_divisible), or ONE tensor for
    frames of one size -- float [N, 3, h, w], or uint8 [N, h, w, 3] (decoded frames, scaled by 1 / 255 in the kernel
    as ToTensor does) -- which takes one launch for all N.  Inputs are never written.  targets: per image a dict, copied
    shallowly; 'boxes' go through resize_boxes, 'masks' (uint8 or bool [G, h, w]) through the nearest resize, other
    keys are passed on; a target without 'boxes' (the reference's `{}` of a frame without objects) is passed on as it is.
    min_size may be a tuple: evaluation takes the last entry, training draws one with torch's generator."""

    def __init__(self, min_size=800, max_size=1333, image_mean=(0.485, 0.456, 0.406), image_std=(0.229, 0.224, 0.225),
                 size_divisible=32):
        super(GeneralizedRCNNTransform, self).__init__()
        if not isinstance(min_size, (list, tuple)):
            min_size = (min_size,)
        self.min_size = tuple(min_size)
        self.max_size = max_size
        self.image_mean = tuple(float(v) for v in image_mean)
        self.image_std = tuple(float(v) for v in image_std)
        self.size_divisible = int(size_divisible)
        if len(self.image_mean) != 3 or len(self.image_std) != 3:
            raise ValueError('GeneralizedRCNNTransform: image_mean and image_std of 3 channels expected')
        if min(self.image_std) <= 0:
            raise ValueError('GeneralizedRCNNTransform: image_std must be positive, got %r' % (self.image_std,))
        if len(self.min_size) < 1 or min(self.min_size) <= 0 or max_size <= 0 or self.size_divisible < 1:
            raise ValueError('GeneralizedRCNNTransform: min_size, max_size and size_divisible must be positive')

    # ---- the size rule: host only ----
    @staticmethod
    def resize_size(size, min_size=800, max_size=1333):
        """(h, w) -> (oh, ow) of torchvision's resize: scale = min(min_size / min(h, w), max_size / max(h, w)), then
        floor(h * scale), floor(w * scale) (F.interpolate's recomputed output size), all in Python floats (module
        docstring): (480, 854) -> (749, 1333)."""
        h, w = int(size[0]), int(size[1])
        scale = min(float(min_size) / float(min(h, w)), float(max_size) / float(max(h, w)))
        return (int(math.floor(float(h) * scale)), int(math.floor(float(w) * scale)))

    @staticmethod
    def batch_shape(sizes, size_divisible=32):
        """(Hp, Wp) of batch_images: the largest height and the largest width, each rounded up to size_divisible."""
        stride = float(size_divisible)
        return tuple(int(math.ceil(float(max(int(s[i]) for s in sizes)) / stride) * stride) for i in (0, 1))

    def torch_choice(self, k):
        """torchvision's torch_choice: one entry of k, drawn with torch's global generator."""
        return k[int(torch.empty(1).uniform_(0., float(len(k))).item())]

    # ---- launches ----
    def _launch(self, src, u8, sizes, batch, out, out_hw):
        """src: [N, 3, h, w] float32 or [N, h, w, 3] uint8, viewed through its strides -> out [N, 3, Hp, Wp]."""
        if u8:
            sb, sh, sw, sc = src.stride()
        else:
            sb, sc, sh, sw = src.stride()
        h, w = sizes
        _lib.call('sfvos_transform_image', _ptr(src), _lib.U8 if u8 else _lib.F32, sb, sc, sh, sw, batch, h, w,
                  *(self.image_mean + self.image_std + (_ptr(out), out.stride(0), out.stride(1), out.stride(2), out_hw[0],
                                                        out_hw[1], out.shape[2], out.shape[3], _stream())))

    @staticmethod
    def _source(img, what):
        """The image as the kernel reads it (a copy only where its dtype or strides demand one; never written)."""
        if img.requires_grad:
            raise RuntimeError('GeneralizedRCNNTransform has no backward: %s requires grad' % what)
        _check_gpu(img, 'GeneralizedRCNNTransform')
        x = img.detach()
        if x.dtype == torch.uint8:
            return x if min(x.stride()) >= 0 else x.contiguous()
        if not x.is_floating_point():
            raise RuntimeError('GeneralizedRCNNTransform: %s must be a floating-point or uint8 tensor, got %s'
                               % (what, x.dtype))
        if x.dtype != torch.float32:
            x = x.float()
        if x.stride(-1) != 1 or min(x.stride()) < 0:
            x = x.contiguous()
        return x

    @staticmethod
    def _check_targets(targets, n):
        if targets is not None and len(targets) != n:
            raise RuntimeError('GeneralizedRCNNTransform: %d images but %d targets' % (n, len(targets)))

    def _resize_target(self, t, size, new_size):
        if t is None or 'boxes' not in t:
            return t
        t = dict(t)
        t['boxes'] = resize_boxes(t['boxes'], size, new_size)
        if 'masks' in t:
            t['masks'] = resize_masks(t['masks'], new_size)
        return t

    def forward(self, images, targets=None):
        if self.training:
            min_size = float(self.torch_choice(self.min_size))
        else:
            min_size = float(self.min_size[-1])
        single = torch.is_tensor(images)
        if single:
            if images.dim() != 4:
                raise RuntimeError('GeneralizedRCNNTransform: one tensor of images must be float [N, 3, h, w] or uint8 '
                                   '[N, h, w, 3], got %s' % (tuple(images.shape),))
            u8 = images.dtype == torch.uint8
            if images.shape[3 if u8 else 1] != 3 or min(images.shape) < 1:
                raise RuntimeError('GeneralizedRCNNTransform: one tensor of images must be float [N, 3, h, w] or uint8 '
                                   '[N, h, w, 3], got %s %s' % (images.dtype, tuple(images.shape)))
            n = images.shape[0]
            self._check_targets(targets, n)
            srcs = [self._source(images, 'images')]
            sizes = [tuple(images.shape[1:3] if u8 else images.shape[2:4])] * n
        else:
            images = list(images)
            if not images:
                raise RuntimeError('GeneralizedRCNNTransform: no images')
            for i, img in enumerate(images):
                if not torch.is_tensor(img) or img.dim() != 3 or img.shape[0] != 3 or min(img.shape) < 1 or \
                        not img.is_floating_point():
                    raise RuntimeError('GeneralizedRCNNTransform: images is expected to be a list of float tensors of '
                                       'shape [3, h, w], got %s at %d' % (tuple(img.shape) if torch.is_tensor(img)
                                                                         else type(img), i))
            n = len(images)
            self._check_targets(targets, n)
            srcs = [self._source(img, 'image %d' % i) for i, img in enumerate(images)]
            sizes = [tuple(img.shape[1:]) for img in images]
        new_sizes = [self.resize_size(s, min_size, self.max_size) for s in sizes]
        Hp, Wp = self.batch_shape(new_sizes, self.size_divisible)
        out = torch.empty((n, 3, Hp, Wp), dtype=torch.float32, device=srcs[0].device)
        if single:
            self._launch(srcs[0], srcs[0].dtype == torch.uint8, sizes[0], n, out, new_sizes[0])
        else:
            for i, src in enumerate(srcs):
                if src.device != out.device:
                    raise RuntimeError('GeneralizedRCNNTransform: the images are on different devices')
                self._launch(src.unsqueeze(0), False, sizes[i], 1, out[i:i + 1], new_sizes[i])
        if targets is not None:
            targets = [self._resize_target(t, s, ns) for t, s, ns in zip(targets, sizes, new_sizes)]
        return ImageList(out, new_sizes), targets

    def postprocess(self, result, image_shapes, original_image_sizes):
        """torchvision's postprocess: in training mode `result` as it is; otherwise per image the boxes resized to the
        original size (resize_boxes) and the [D, 1, M, M] mask probabilities pasted into the original image
        (paste_masks_in_image) -> the same list, its dicts updated."""
        if self.training:
            return result
        for i, (pred, im_s, o_im_s) in enumerate(zip(result, image_shapes, original_image_sizes)):
            boxes = resize_boxes(pred['boxes'], im_s, o_im_s)
            result[i]['boxes'] = boxes
            if 'masks' in pred:
                result[i]['masks'] = paste_masks_in_image(pred['masks'], boxes, o_im_s)
        return result

    def extra_repr(self):
        return 'Normalize(mean=%r, std=%r), Resize(min_size=%r, max_size=%r, mode=bilinear), size_divisible=%d' % (
            self.image_mean, self.image_std, self.min_size, self.max_size, self.size_divisible)


def _original_sizes(images):
    if torch.is_tensor(images):
        if images.dim() != 4:
            raise RuntimeError('MaskRCNN: one tensor of images must be float [N, 3, h, w] or uint8 [N, h, w, 3]')
        hw = images.shape[1:3] if images.dtype == torch.uint8 else images.shape[2:4]
        return [(int(hw[0]), int(hw[1]))] * images.shape[0]
    return [(int(img.shape[-2]), int(img.shape[-1])) for img in images]


class MaskRCNN(nn.Module):
    """torchvision's MaskRCNN over resnet50 + FPN as the reference builds it (model.py:11-27, num_classes = 2), holding
    the modules of this package under torchvision's names: `transform` (GeneralizedRCNNTransform), `backbone`
    (BackboneWithFPN), `rpn` (RegionProposalNetwork), `roi_heads` (RoIHeads).  No kernel and no arithmetic of its own.
    A full checkpoint (`backbone.body.*`, `backbone.fpn.*`, `rpn.head.*`, `roi_heads.*`; the `num_batches_tracked`
    entries of the norms are dropped) loads with strict=True; `roi_heads.detections_per_img = 10` (model.py:187) works.

    Keyword arguments, torchvision's names and defaults: min_size, max_size, image_mean, image_std; rpn_pre_nms_top_n_train /
    _test, rpn_post_nms_top_n_train / _test, rpn_nms_thresh, rpn_fg_iou_thresh, rpn_bg_iou_thresh,
    rpn_batch_size_per_image, rpn_positive_fraction, rpn_score_thresh; box_score_thresh, box_nms_thresh,
    box_detections_per_img, box_fg_iou_thresh, box_bg_iou_thresh, box_batch_size_per_image, box_positive_fraction; and
    eps, the frozen norms' (ResNetBody).

    As in torchvision, `roi_heads` returns the detections' [D, 1, 28, 28] mask probabilities in evaluation and
    `transform.postprocess` pastes them at the original size: this class clears `roi_heads.paste_masks`, which a
    stand-alone RoIHeads leaves set (it then pastes at the resized image itself).

    The backbone and the RPN stay inference only: freeze them (model.py:176-179) before a training call, or their own
    errors come through."""

    def __init__(self, num_classes=2, precision='fp32', **kw):
        super(MaskRCNN, self).__init__()
        take = kw.pop
        self.transform = GeneralizedRCNNTransform(take('min_size', 800), take('max_size', 1333),
                                                  take('image_mean', (0.485, 0.456, 0.406)),
                                                  take('image_std', (0.229, 0.224, 0.225)))
        self.backbone = BackboneWithFPN(precision=precision, eps=take('eps', 0.0))
        self.rpn = RegionProposalNetwork(
            pre_nms_top_n=dict(training=take('rpn_pre_nms_top_n_train', 2000), testing=take('rpn_pre_nms_top_n_test', 1000)),
            post_nms_top_n=dict(training=take('rpn_post_nms_top_n_train', 2000),
                                testing=take('rpn_post_nms_top_n_test', 1000)),
            nms_thresh=take('rpn_nms_thresh', 0.7), score_thresh=take('rpn_score_thresh', 0.0), precision=precision,
            fg_iou_thresh=take('rpn_fg_iou_thresh', 0.7), bg_iou_thresh=take('rpn_bg_iou_thresh', 0.3),
            batch_size_per_image=take('rpn_batch_size_per_image', 256),
            positive_fraction=take('rpn_positive_fraction', 0.5))
        self.roi_heads = RoIHeads(num_classes, precision, take('box_score_thresh', 0.05), take('box_nms_thresh', 0.5),
                                  take('box_detections_per_img', 100), take('box_batch_size_per_image', 512),
                                  take('box_positive_fraction', 0.25), take('box_fg_iou_thresh', 0.5),
                                  take('box_bg_iou_thresh', 0.5))
        self.roi_heads.paste_masks = False
        if kw:
            raise TypeError('MaskRCNN: unexpected keyword arguments %s' % sorted(kw))
        self.precision = self.backbone.precision

    def forward(self, images, targets=None, rpn_keys=None, roi_keys=None):
        """torchvision's GeneralizedRCNN.forward: images (what the transform takes) and, in training, targets -> the
        merged loss dict ('loss_classifier', 'loss_box_reg', 'loss_mask', 'loss_objectness', 'loss_rpn_box_reg') in
        training mode, the detections (per image 'boxes', 'labels', 'scores', 'masks' [D, 1, h, w] at the original size)
        in evaluation.  rpn_keys / roi_keys: the samplers' keys (RegionProposalNetwork.compute_loss,
        select_training_samples); None draws them."""
        if self.training and targets is None:
            raise ValueError('In training mode, targets should be passed')
        original_image_sizes = _original_sizes(images)
        images, targets = self.transform(images, targets)
        features = self.backbone(images.tensors)
        proposals, proposal_losses = self.rpn(images, features, targets, keys=rpn_keys)
        detections, detector_losses = self.roi_heads(features, proposals, images.image_sizes, targets, keys=roi_keys)
        detections = self.transform.postprocess(detections, images.image_sizes, original_image_sizes)
        losses = {}
        losses.update(detector_losses)
        losses.update(proposal_losses)
        return losses if self.training else detections
