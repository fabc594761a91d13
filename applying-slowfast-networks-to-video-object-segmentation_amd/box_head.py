"""The box branch of the Mask R-CNN `roi_heads` the reference runs on the fused maps, on libsfvos kernels.

The reference hands the maps `SlowFastLayers` returns to torchvision's `roi_heads` (code/helpers/model.py:346) and
trains it with them (only backbone and RPN are frozen, model.py:176-179; two classes, model.py:172;
`detections_per_img = 10`, model.py:187).  Its box branch is `box_roi_pool = MultiScaleRoIAlign(['0'..'3'], 7, 2)` ->
`box_head = TwoMLPHead(12544, 1024)` -> `box_predictor = FastRCNNPredictor(1024, num_classes)`, then `fastrcnn_loss`
(training) or `postprocess_detections` (evaluation), and `transform.postprocess` (model.py:347) resizes the boxes.

torchvision is third-party, not vendored and absent in this build's environment, so these classes mirror its published
module structure (same attribute names and state-dict keys: the slices `roi_heads.box_head.*` /
`roi_heads.box_predictor.*` of a reference checkpoint load with strict=True) and their results are checked against a
torch-core restatement (tests/box_branch_ref.py) -- PARITY UNPINNED BY THE REFERENCE.  No CPU fallback.

Out of scope: `select_training_samples` (the IoU matcher and the balanced sampler draw with torch's RNG and are host-side
bookkeeping): the caller passes the sampled proposals, `labels` and `regression_targets`, the arguments torchvision's own
`fastrcnn_loss` takes."""
import math

import torch
from torch import nn

from . import _lib
from ._heads import _check_precision, _pack, _project_bwd, _relu_bwd, _to_nchw, _to_nhwc
from ._lib import _DT, _check_gpu, _f32, _ptr, _stream
from .mask_head import MaskBranch
from .roi_align import MultiScaleRoIAlign

BOX_WEIGHTS = (10.0, 10.0, 5.0, 5.0)          # roi_heads' BoxCoder
BBOX_XFORM_CLIP = math.log(1000.0 / 16)
SMOOTH_L1_BETA = 1.0 / 9
MIN_BOX_SIZE = 1e-2


def _inference_only(module, x):
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters())):
        raise RuntimeError('%s.forward on its own is inference only (call it under torch.no_grad()); '
                           'BoxBranch.forward is the differentiable path' % type(module).__name__)


def _dense(x, image, bias, dt_id, tdt, n, relu):
    """act(x [M,K] . image^T + bias) -> [M,n] in the compute dtype."""
    M, K = x.shape
    y = torch.empty((M, n), dtype=tdt, device=x.device)
    nbytes = _lib.load().sfvos_dense_workspace_bytes(dt_id, M, n, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    _lib.call('sfvos_dense', _ptr(x), _ptr(image), _ptr(bias), _ptr(y), dt_id, M, n, K, int(relu), _ptr(ws), _stream())
    return y


class TwoMLPHead(nn.Module):
    """torchvision's TwoMLPHead(in_channels, representation_size): fc6, fc7, each followed by ReLU, on the flattened RoI
    features.  forward(x [N,C,H,W] fp32) -> [N,representation_size] fp32.  The kernels read the features channels-last;
    the packed image of fc6 carries the permutation to torchvision's NCHW flatten.  Called on its own, forward is
    inference only (it raises when a gradient would be needed): the differentiable path is BoxBranch."""

    def __init__(self, in_channels=12544, representation_size=1024, precision='fp32'):
        super(TwoMLPHead, self).__init__()
        self.precision = _check_precision(precision)
        self.fc6 = nn.Linear(in_channels, representation_size)
        self.fc7 = nn.Linear(representation_size, representation_size)
        self._images = _lib.WeightImages()

    def _packed(self, fc, dt_id, tdt, positions, dgrad=False):
        fn = 'sfvos_pack_dense_dgrad' if dgrad else 'sfvos_pack_dense_fwd'
        return self._images.get((id(fc), fn, dt_id, positions), (fc.weight,), _pack, fn, fc.weight, dt_id, tdt,
                                fc.out_features, fc.in_features, positions)

    def forward_rows(self, x):
        """x [N,C,H,W] -> (x rows [N,H*W*C] channels-last, h6, h7), all in the compute dtype."""
        _check_gpu(x, 'TwoMLPHead')
        dt_id, tdt = _DT[self.precision]
        if x.dim() == 2:
            x = x[:, :, None, None]
        N, C, H, W = x.shape
        if C * H * W != self.fc6.in_features:
            raise RuntimeError('TwoMLPHead: %d features per RoI, fc6 takes %d' % (C * H * W, self.fc6.in_features))
        rows = _to_nhwc(x.detach(), dt_id, tdt).view(N, H * W * C)
        h6 = _dense(rows, self._packed(self.fc6, dt_id, tdt, H * W), _f32(self.fc6.bias), dt_id, tdt,
                    self.fc6.out_features, True)
        h7 = _dense(h6, self._packed(self.fc7, dt_id, tdt, 1), _f32(self.fc7.bias), dt_id, tdt,
                    self.fc7.out_features, True)
        return rows, h6, h7

    def forward(self, x):
        _inference_only(self, x)
        if x.shape[0] == 0:
            return x.new_zeros((0, self.fc7.out_features))
        return self.forward_rows(x)[2].float()


class FastRCNNPredictor(nn.Module):
    """torchvision's FastRCNNPredictor(in_channels, num_classes): cls_score, bbox_pred.
    forward(x [N,in_channels]) -> (scores [N,num_classes], bbox_deltas [N,4 num_classes]) fp32.  Called on its own,
    forward is inference only (it raises when a gradient would be needed): the differentiable path is BoxBranch."""

    def __init__(self, in_channels=1024, num_classes=2, precision='fp32'):
        super(FastRCNNPredictor, self).__init__()
        self.precision = _check_precision(precision)
        if not 1 <= num_classes <= 8:
            raise ValueError('FastRCNNPredictor: 1..8 classes are implemented')
        self.cls_score = nn.Linear(in_channels, num_classes)
        self.bbox_pred = nn.Linear(in_channels, num_classes * 4)

    def forward_rows(self, h):
        """h [N,in_channels] in the compute dtype.  The weights are read as fp32 masters: nothing is packed."""
        dt_id, _ = _DT[self.precision]
        N, C = h.shape
        K = self.cls_score.out_features
        logits = torch.empty((N, K), dtype=torch.float32, device=h.device)
        deltas = torch.empty((N, 4 * K), dtype=torch.float32, device=h.device)
        wc, bc = _f32(self.cls_score.weight), _f32(self.cls_score.bias)     # held until the launch is enqueued
        wb, bb = _f32(self.bbox_pred.weight), _f32(self.bbox_pred.bias)
        _lib.call('sfvos_box_predictor', _ptr(h), dt_id, _ptr(wc), _ptr(bc), _ptr(wb), _ptr(bb), N, C, K, _ptr(logits),
                  _ptr(deltas), _stream())
        return logits, deltas

    def forward(self, x):
        _inference_only(self, x)
        _check_gpu(x, 'FastRCNNPredictor')
        _, tdt = _DT[self.precision]
        return self.forward_rows(x.detach().flatten(1).to(tdt).contiguous())


class _BoxBranchFn(torch.autograd.Function):
    """RoI features [N,256,7,7] -> (class_logits, box_regression).  Parameter order: fc6.(weight, bias),
    fc7.(weight, bias), cls_score.(weight, bias), bbox_pred.(weight, bias)."""

    @staticmethod
    def forward(ctx, branch, x, *params):
        rows, h6, h7 = branch.box_head.forward_rows(x)
        logits, deltas = branch.box_predictor.forward_rows(h7)
        ctx.branch, ctx.acts, ctx.shape = branch, (rows, h6, h7), tuple(x.shape)
        return logits, deltas

    @staticmethod
    def backward(ctx, dlogits, ddeltas):
        branch = ctx.branch
        rows, h6, h7 = ctx.acts
        head, pred = branch.box_head, branch.box_predictor
        dt_id, tdt = _DT[head.precision]
        lib = _lib.load()
        dev = rows.device
        N, C, H, W = ctx.shape
        f32 = dict(dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad     # (branch, x, *params)
        K = pred.cls_score.out_features
        R = head.fc7.out_features
        dl = _f32(dlogits) if dlogits is not None else torch.zeros((N, K), **f32)
        dd = _f32(ddeltas) if ddeltas is not None else torch.zeros((N, 4 * K), **f32)
        # ---- cls_score + bbox_pred and fc7's ReLU
        dz7, g_w, g_b, g_b7 = _project_bwd('sfvos_box_predictor_bwd', h7, dt_id,
                                           (dl, dd, _f32(pred.cls_score.weight), _f32(pred.bbox_pred.weight)),
                                           (N, R, K), lib.sfvos_box_predictor_bwd_rows(N), 5 * K)
        # ---- fc7
        R6 = head.fc6.out_features
        g_w7 = None
        if need[4]:     # a frozen weight skips its weight-gradient kernel
            g_w7 = torch.empty((R, R6), **f32)
            _lib.call('sfvos_dense_wgrad', _ptr(h6), _ptr(dz7), dt_id, N, R, R6, 1, _ptr(g_w7), 0, _stream())
        dz6 = _dense(dz7, head._packed(head.fc7, dt_id, tdt, 1, dgrad=True), None, dt_id, tdt, R6, False)
        g_b6 = _relu_bwd(dz6, h6, dt_id)
        # ---- fc6
        Kin = head.fc6.in_features
        g_w6 = None
        if need[2]:
            g_w6 = torch.empty((R6, Kin), **f32)
            _lib.call('sfvos_dense_wgrad', _ptr(rows), _ptr(dz6), dt_id, N, R6, Kin, H * W, _ptr(g_w6), 0, _stream())
        dx = None
        if need[1]:
            drows = _dense(dz6, head._packed(head.fc6, dt_id, tdt, H * W, dgrad=True), None, dt_id, tdt, Kin, False)
            dx = _to_nchw(drows.view(N, H, W, C), dt_id)
        grads = [g_w6, g_b6, g_w7, g_b7, g_w[:K], g_b[:K], g_w[K:], g_b[K:]]
        return (None, dx) + tuple(g if n else None for g, n in zip(grads, need[2:]))


class _FastRCNNLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, deltas, labels, targets):
        N, K = logits.shape
        lg, dl = _f32(logits), _f32(deltas)
        lab = labels.to(device=lg.device, dtype=torch.int64).contiguous()
        tg = _f32(targets, lg.device)
        if lab.numel() != N or tuple(tg.shape) != (N, 4) or tuple(dl.shape) != (N, 4 * K):
            raise RuntimeError('fastrcnn_loss: one label and one [4] target per RoI expected')
        losses = torch.empty(2, dtype=torch.float32, device=lg.device)
        _lib.call('sfvos_fastrcnn_loss', _ptr(lg), _ptr(dl), _ptr(lab), _ptr(tg), N, K, SMOOTH_L1_BETA, _ptr(losses),
                  _stream())
        ctx.save_for_backward(lg, dl, lab, tg)
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, up_cls, up_box):
        lg, dl, lab, tg = ctx.saved_tensors
        N, K = lg.shape
        up = torch.stack([up_cls.detach().float().reshape(()), up_box.detach().float().reshape(())]).contiguous()
        g_l, g_d = torch.empty_like(lg), torch.empty_like(dl)
        _lib.call('sfvos_fastrcnn_loss_grad', _ptr(lg), _ptr(dl), _ptr(lab), _ptr(tg), _ptr(up), N, K, SMOOTH_L1_BETA,
                  _ptr(g_l), _ptr(g_d), _stream())
        return g_l, g_d, None, None


def fastrcnn_loss(class_logits, box_regression, labels, regression_targets):
    """torchvision roi_heads.fastrcnn_loss: labels / regression_targets are lists per image (or already concatenated
    tensors) -> (loss_classifier, loss_box_reg).  No sampled RoI: zeros on the graph."""
    labels = torch.cat(list(labels), 0) if isinstance(labels, (list, tuple)) else labels
    regression_targets = torch.cat(list(regression_targets), 0) if isinstance(regression_targets, (list, tuple)) \
        else regression_targets
    if class_logits.shape[0] == 0:
        return class_logits.sum() * 0, box_regression.sum() * 0
    _check_gpu(class_logits, 'fastrcnn_loss')
    return _FastRCNNLossFn.apply(class_logits, box_regression, labels, regression_targets)


def encode_boxes(reference_boxes, proposals, weights=BOX_WEIGHTS):
    """BoxCoder.encode_single: regression targets [N,4] of `reference_boxes` against `proposals`."""
    _check_gpu(proposals, 'encode_boxes')
    p, r = _f32(proposals), _f32(reference_boxes, proposals.device)
    out = torch.empty_like(p)
    if p.shape[0]:
        _lib.call('sfvos_box_encode', _ptr(r), _ptr(p), p.shape[0], *(tuple(float(w) for w in weights) +
                                                                      (_ptr(out), _stream())))
    return out


def decode_boxes(rel_codes, boxes, weights=BOX_WEIGHTS, bbox_xform_clip=BBOX_XFORM_CLIP):
    """BoxCoder.decode_single: rel_codes [N,4K], boxes [N,4] -> [N,K,4]."""
    _check_gpu(boxes, 'decode_boxes')
    b, d = _f32(boxes), _f32(rel_codes, boxes.device)
    N, K = b.shape[0], d.shape[1] // 4
    out = torch.empty((N, K, 4), dtype=torch.float32, device=b.device)
    if N:
        _lib.call('sfvos_box_decode', None, _ptr(d), _ptr(b), N, K, 0, *(tuple(float(w) for w in weights) + (
            float(bbox_xform_clip), 0.0, 0.0, _ptr(out), None, None, _stream())))
    return out


class BoxBranch(nn.Module):
    """box_roi_pool + box_head + box_predictor as the reference's roi_heads holds them (attribute names =
    torchvision's, so `load_state_dict` takes the `roi_heads.` slice of a reference checkpoint)."""

    def __init__(self, num_classes=2, precision='fp32', box_score_thresh=0.05, box_nms_thresh=0.5,
                 box_detections_per_img=100):
        super(BoxBranch, self).__init__()
        self.box_roi_pool = MultiScaleRoIAlign(['0', '1', '2', '3'], 7, 2)
        self.box_head = TwoMLPHead(256 * 7 * 7, 1024, precision)
        self.box_predictor = FastRCNNPredictor(1024, num_classes, precision)
        self.score_thresh, self.nms_thresh = float(box_score_thresh), float(box_nms_thresh)
        self.detections_per_img = int(box_detections_per_img)

    def _ordered_params(self):
        h, p = self.box_head, self.box_predictor
        return [h.fc6.weight, h.fc6.bias, h.fc7.weight, h.fc7.bias, p.cls_score.weight, p.cls_score.bias,
                p.bbox_pred.weight, p.bbox_pred.bias]

    def forward_features(self, roi_features):
        """RoIAligned features [N,256,7,7] -> (class_logits [N,K], box_regression [N,4K]) fp32; differentiable w.r.t.
        the features and the 8 parameters (backward on libsfvos kernels)."""
        ps = self._ordered_params()
        K = self.box_predictor.cls_score.out_features
        if roi_features.shape[0] == 0:
            zero = roi_features.sum() * 0
            if torch.is_grad_enabled():
                zero = zero + sum(p.sum() for p in ps) * 0
            return roi_features.new_zeros((0, K)) + zero, roi_features.new_zeros((0, 4 * K)) + zero
        _check_gpu(roi_features, 'BoxBranch')
        if torch.is_grad_enabled() and (roi_features.requires_grad or any(p.requires_grad for p in ps)):
            return _BoxBranchFn.apply(self, roi_features, *ps)
        return self.box_predictor.forward_rows(self.box_head.forward_rows(roi_features)[2])

    def forward(self, features, proposals, image_shapes):
        """features: OrderedDict of the fused maps; proposals: list of [L_i,4] per image; image_shapes: list of (H, W)."""
        return self.forward_features(self.box_roi_pool(features, proposals, image_shapes))

    @torch.no_grad()
    def candidates(self, class_logits, box_regression, proposals, image_shape):
        """One image: decode + softmax + clip, class 0 dropped -> (boxes [M(K-1),4], scores, labels) in torchvision's
        order (candidate i (K-1) + k-1)."""
        K = class_logits.shape[1]
        M = proposals.shape[0]
        dev = class_logits.device
        boxes = torch.empty((M * (K - 1), 4), dtype=torch.float32, device=dev)
        scores = torch.empty(M * (K - 1), dtype=torch.float32, device=dev)
        labels = torch.empty(M * (K - 1), dtype=torch.int64, device=dev)
        if M and K > 1:
            _lib.call('sfvos_box_decode', _ptr(_f32(class_logits)), _ptr(_f32(box_regression)),
                      _ptr(_f32(proposals, dev)), M, K, 1, *(BOX_WEIGHTS + (BBOX_XFORM_CLIP, float(image_shape[0]),
                                                                            float(image_shape[1]), _ptr(boxes),
                                                                            _ptr(scores), _ptr(labels), _stream())))
        return boxes, scores, labels

    @torch.no_grad()
    def select(self, boxes, scores, labels, classes_per_roi=1, ratios=(1.0, 1.0)):
        """Score threshold, small boxes, class-wise NMS, the best detections_per_img -> dict with 'boxes' (scaled by
        ratios = (height, width): resize_boxes), 'labels', 'scores', and 'index' / 'roi' (candidate and RoI they came
        from).  Everything runs on the device; only the count is read back, to slice the fixed-size outputs."""
        n, D, dev = boxes.shape[0], self.detections_per_img, boxes.device
        ob = torch.empty((D, 4), dtype=torch.float32, device=dev)
        osc = torch.empty(D, dtype=torch.float32, device=dev)
        ol = torch.empty(D, dtype=torch.int64, device=dev)
        oi = torch.empty(D, dtype=torch.int32, device=dev)
        orr = torch.empty(D, dtype=torch.int32, device=dev)
        d = 0
        if n:
            ws = torch.empty(_lib.load().sfvos_detections_workspace_bytes(n), dtype=torch.uint8, device=dev)
            cnt = torch.empty(1, dtype=torch.int32, device=dev)
            _lib.call('sfvos_detections', _ptr(boxes), _ptr(scores), _ptr(labels), n, int(classes_per_roi),
                      self.score_thresh, MIN_BOX_SIZE, self.nms_thresh, D, float(ratios[0]), float(ratios[1]), _ptr(ws),
                      _ptr(cnt), _ptr(ob), _ptr(osc), _ptr(ol), _ptr(oi), _ptr(orr), _stream())
            d = int(cnt.item())
        return {'boxes': ob[:d], 'labels': ol[:d], 'scores': osc[:d], 'index': oi[:d], 'roi': orr[:d]}

    @torch.no_grad()
    def detect(self, features, proposals, image_shapes, original_image_sizes=None):
        """roi_heads.postprocess_detections (+ transform.postprocess's resize_boxes when original_image_sizes is given)
        -> per image {'boxes', 'labels', 'scores'} (+ 'index', 'roi')."""
        logits, deltas = self.forward(features, proposals, image_shapes)
        K = logits.shape[1]
        out, lo = [], 0
        for i, (props, shape) in enumerate(zip(proposals, image_shapes)):
            hi = lo + props.shape[0]
            boxes, scores, labels = self.candidates(logits[lo:hi], deltas[lo:hi], props, shape)
            ratios = (1.0, 1.0)
            if original_image_sizes is not None:
                # resize_boxes: ratio = float32(original) / float32(resized), as torchvision computes it
                o = original_image_sizes[i]
                ratios = tuple(float(torch.tensor(float(a), dtype=torch.float32) /
                                     torch.tensor(float(b), dtype=torch.float32)) for a, b in zip(o, shape))
            out.append(self.select(boxes, scores, labels, max(K - 1, 1), ratios))
            lo = hi
        return out


class RoIHeadsInference(nn.Module):
    """roi_heads in evaluation + transform.postprocess (model.py:346-347): fused maps + RPN proposals -> detections with
    their masks pasted into the image, ready for `union_mask`.  Holds a BoxBranch (`box`), the mask RoIAlign
    (`mask_roi_pool`, output 14) and a MaskBranch (`mask`)."""

    def __init__(self, num_classes=2, precision='fp32', box_score_thresh=0.05, box_nms_thresh=0.5,
                 box_detections_per_img=100):
        super(RoIHeadsInference, self).__init__()
        self.box = BoxBranch(num_classes, precision, box_score_thresh, box_nms_thresh, box_detections_per_img)
        self.mask_roi_pool = MultiScaleRoIAlign(['0', '1', '2', '3'], 14, 2)
        self.mask = MaskBranch(256, num_classes, precision)

    @torch.no_grad()
    def forward(self, features, proposals, image_shapes, original_image_sizes=None):
        """-> per image {'boxes', 'labels', 'scores', 'masks' [D,1,H,W] fp32 probabilities}; with original_image_sizes the
        boxes are resized and the masks pasted at that size (transform.postprocess)."""
        return detect_with_masks(self.box, self.mask_roi_pool, self.mask, features, proposals, image_shapes,
                                 original_image_sizes)


@torch.no_grad()
def detect_with_masks(box, mask_roi_pool, mask, features, proposals, image_shapes, original_image_sizes=None, paste=True):
    """roi_heads in evaluation (+ transform.postprocess) on a BoxBranch, the mask RoIAlign and a MaskBranch: the body
    RoIHeadsInference and roi_heads.RoIHeads share.  paste=False leaves 'masks' as the [D,1,28,28] probabilities
    (torchvision's roi_heads; transform.postprocess pastes them)."""
    dets = box.detect(features, proposals, image_shapes)
    roi = mask_roi_pool(features, [d['boxes'] for d in dets], image_shapes)
    lo = 0
    for i, d in enumerate(dets):
        hi = lo + d['boxes'].shape[0]
        size = image_shapes[i]
        if original_image_sizes is not None:
            size = original_image_sizes[i]
            d['boxes'] = resize_boxes(d['boxes'], image_shapes[i], size)
        d['masks'] = mask.predict(roi[lo:hi], d['labels'], d['boxes'], size, paste)
        lo = hi
    return dets


def resize_boxes(boxes, original_size, new_size):
    """transform.resize_boxes: x scaled by new width / original width, y by the heights (sizes are (H, W)); the ratios
    are fp32 quotients as torchvision computes them, the multiply is one libsfvos launch."""
    _check_gpu(boxes, 'resize_boxes')
    rh, rw = (float(torch.tensor(float(n), dtype=torch.float32) / torch.tensor(float(o), dtype=torch.float32))
              for n, o in zip(new_size, original_size))
    b = _f32(boxes)
    out = torch.empty_like(b)
    if b.shape[0]:
        _lib.call('sfvos_box_scale', _ptr(b), b.shape[0], rh, rw, _ptr(out), _stream())
    return out
