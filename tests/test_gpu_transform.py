"""GPU: sfvos_amd.transform -- GeneralizedRCNNTransform against tests/transform_ref.py (the float64 F.interpolate
reference under the per-element bound of test_gpu_transform_kernels.py; boxes, masks, sizes, the pad, untouched inputs), its
three input forms against each other bit for bit, postprocess against the composition of its two parts, and the wiring of
MaskRCNN: the detections in evaluation and the five losses in training equal, bit for bit, what the same submodule objects
give when they are called one after the other by hand.  The arithmetic of the parts is covered by their own tests; nothing
here compares the whole chain with the chain of CPU restatements (top-k and NMS decisions would make that fragile and it
would prove nothing more).  Worst error / bound of the transform observed on an MI355X: 0.145 and 0.098 (the list of two
images), 0.167 (byte frames)."""
import pytest
import torch

import body_ref
import transform_ref as R
from kernel_util import check_abs

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)


def bits(t):
    return t.contiguous().view(torch.int32)


def scene():
    """Two images of different sizes (landscape, portrait) with targets, on the CPU."""
    g = torch.Generator().manual_seed(23)
    images = [torch.rand((3, 31, 47), generator=g), torch.rand((3, 40, 33), generator=g)]
    targets = []
    for i, img in enumerate(images):
        h, w = img.shape[1:]
        G = 2 + i
        xy = torch.rand((G, 2), generator=g) * torch.tensor([w / 2.0, h / 2.0])
        wh = 2.0 + torch.rand((G, 2), generator=g) * torch.tensor([w / 2.0 - 2, h / 2.0 - 2])
        targets.append({'boxes': torch.cat([xy, xy + wh], 1), 'labels': torch.ones(G, dtype=torch.int64),
                        'masks': R.random_masks(31 + i, G, h, w), 'image_id': torch.tensor([i])})
    return images, targets


def to_dev(targets):
    return [{k: v.to(DEV) for k, v in t.items()} for t in targets]


def test_transform_on_a_list_with_targets():
    from sfvos_amd import GeneralizedRCNNTransform, ImageList, resize_boxes
    t = GeneralizedRCNNTransform(min_size=48, max_size=80).eval()
    images, targets = scene()
    sizes = [(48, 72), (58, 48)]
    assert [t.resize_size(img.shape[1:], 48, 80) for img in images] == sizes
    xd, td = [img.to(DEV) for img in images], to_dev(targets)
    keep = [x.clone() for x in xd]
    keep_t = [dict(d) for d in td]
    out, new_t = t(xd, td)
    torch.cuda.synchronize()
    assert isinstance(out, ImageList) and out.image_sizes == sizes
    assert tuple(out.tensors.shape) == (2, 3, 64, 96) and out.tensors.dtype == torch.float32
    got = out.tensors.cpu()
    for i, (img, size) in enumerate(zip(images, sizes)):
        ref = R.reference_image(img[None], size, (64, 96))
        _, mag, dh, dw, _ = R.formula_image(img[None], size, (64, 96))
        check_abs('transform image %d %s -> %s' % (i, tuple(img.shape[1:]), size), got[i:i + 1], ref,
                  R.bound(mag, dh, dw, *img.shape[1:]))
        assert bool((bits(got[i, :, size[0]:]) == 0).all()) and bool((bits(got[i, :, :, size[1]:]) == 0).all())
        # the targets: boxes through resize_boxes, masks through the nearest resize, the rest passed on
        assert set(new_t[i].keys()) == set(targets[i].keys())
        assert torch.equal(new_t[i]['boxes'], resize_boxes(td[i]['boxes'], img.shape[1:], size))
        scale = torch.tensor([size[1] / img.shape[2], size[0] / img.shape[1]] * 2, dtype=torch.float64)
        assert torch.allclose(new_t[i]['boxes'].cpu().double(), targets[i]['boxes'].double() * scale, rtol=1e-6)
        assert new_t[i]['masks'].dtype == torch.uint8
        assert torch.equal(new_t[i]['masks'].cpu(), R.reference_masks(targets[i]['masks'], size))
        assert new_t[i]['labels'] is td[i]['labels'] and new_t[i]['image_id'] is td[i]['image_id']
        # nothing the caller passed was written or replaced
        assert torch.equal(xd[i], keep[i])
        assert all(td[i][k] is keep_t[i][k] for k in keep_t[i]) and new_t[i] is not td[i]
        assert torch.equal(td[i]['boxes'].cpu(), targets[i]['boxes'])
        assert torch.equal(td[i]['masks'].cpu(), targets[i]['masks'])
    # bool masks, no masks, no boxes, no objects
    mixed = [{'boxes': td[0]['boxes'], 'masks': td[0]['masks'] != 0}, {}]
    _, res = t(xd, mixed)
    assert res[0]['masks'].dtype == torch.uint8
    assert torch.equal(res[0]['masks'].cpu(), R.reference_masks((targets[0]['masks'] != 0).to(torch.uint8), sizes[0]))
    assert res[1] == {} and mixed[1] == {}
    empty = {'boxes': torch.zeros((0, 4), device=DEV), 'masks': torch.zeros((0, 40, 33), dtype=torch.uint8, device=DEV)}
    _, res = t(xd, [{'boxes': td[0]['boxes']}, empty])
    assert set(res[0].keys()) == {'boxes'} and tuple(res[1]['boxes'].shape) == (0, 4)
    assert tuple(res[1]['masks'].shape) == (0, 58, 48)
    assert t(xd)[1] is None
    # float64 and non-contiguous images are read as their fp32 values
    wide = torch.zeros((3, 31, 60), device=DEV)
    wide[:, :, :47] = xd[0]
    again, _ = t([wide[:, :, :47], xd[1].double()])
    assert torch.equal(bits(again.tensors), bits(out.tensors))


def test_single_tensor_calls_equal_the_list_call():
    from sfvos_amd import GeneralizedRCNNTransform
    t = GeneralizedRCNNTransform(min_size=48, max_size=80).eval()
    g = torch.Generator().manual_seed(29)
    u = torch.randint(0, 256, (3, 31, 47, 3), generator=g, dtype=torch.uint8).to(DEV)
    x = (u.float() / torch.tensor(255.0, device=DEV)).permute(0, 3, 1, 2).contiguous()
    listed, _ = t([x[0], x[1], x[2]])
    whole, _ = t(x)
    frames, _ = t(u)
    torch.cuda.synchronize()
    assert listed.image_sizes == whole.image_sizes == frames.image_sizes == [(48, 72)] * 3
    assert tuple(listed.tensors.shape) == (3, 3, 64, 96)
    assert torch.equal(bits(whole.tensors), bits(listed.tensors))
    assert torch.equal(bits(frames.tensors), bits(listed.tensors))
    ref = R.reference_image(x.cpu(), (48, 72), (64, 96))
    _, mag, dh, dw, _ = R.formula_image(x.cpu(), (48, 72), (64, 96))
    check_abs('transform [N, h, w, 3] bytes', frames.tensors.cpu(), ref, R.bound(mag, dh, dw, 31, 47))
    # a channels-last view of float frames is read through its strides' copy, same values
    nhwc = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert torch.equal(bits(t(nhwc)[0].tensors), bits(listed.tensors))
    # a training-mode draw from a tuple of sizes
    tt = GeneralizedRCNNTransform(min_size=(32, 48), max_size=80).train()
    torch.manual_seed(1)
    seen = {tt(x)[0].image_sizes[0] for _ in range(16)}
    assert seen == {(32, 48), (48, 72)}
    assert tt.eval()(x)[0].image_sizes[0] == (48, 72)


def test_postprocess_is_resize_boxes_and_paste():
    from sfvos_amd import GeneralizedRCNNTransform, paste_masks_in_image, resize_boxes
    t = GeneralizedRCNNTransform(min_size=48, max_size=80)
    g = torch.Generator().manual_seed(31)
    shapes, originals = [(48, 72), (58, 48)], [(31, 47), (40, 33)]
    result = []
    for (h, w), D in zip(shapes, (3, 0)):
        xy = torch.rand((D, 2), generator=g) * torch.tensor([w / 2.0, h / 2.0])
        wh = 4.0 + torch.rand((D, 2), generator=g) * torch.tensor([w / 2.0 - 4, h / 2.0 - 4])
        result.append({'boxes': torch.cat([xy, xy + wh], 1).to(DEV), 'scores': torch.rand(D, generator=g).to(DEV),
                       'labels': torch.ones(D, dtype=torch.int64, device=DEV),
                       'masks': torch.rand((D, 1, 28, 28), generator=g).to(DEV)})
    before = [dict(r) for r in result]
    assert t.train().postprocess(result, shapes, originals) is result
    assert all(result[i][k] is before[i][k] for i in (0, 1) for k in before[i])
    out = t.eval().postprocess([dict(r) for r in result], shapes, originals)
    for i, (r, s, o) in enumerate(zip(before, shapes, originals)):
        boxes = resize_boxes(r['boxes'], s, o)
        assert torch.equal(out[i]['boxes'], boxes)
        masks = paste_masks_in_image(r['masks'], boxes, o)
        assert tuple(out[i]['masks'].shape) == (r['boxes'].shape[0], 1) + o
        assert torch.equal(out[i]['masks'], masks)
        assert out[i]['scores'] is r['scores'] and out[i]['labels'] is r['labels']


@pytest.fixture(scope='module')
def model():
    from sfvos_amd import MaskRCNN
    torch.manual_seed(41)
    m = MaskRCNN(precision='fp32', min_size=64, max_size=96, rpn_pre_nms_top_n_test=200, rpn_post_nms_top_n_test=50,
                 rpn_pre_nms_top_n_train=200, rpn_post_nms_top_n_train=60, box_detections_per_img=8,
                 rpn_batch_size_per_image=64, box_batch_size_per_image=32)
    assert len(m.backbone.body.layer3) == 6                       # `layers` at their default
    m.backbone.body.load_state_dict(body_ref.random_state(43), strict=True)
    for p in list(m.backbone.parameters()) + list(m.rpn.parameters()):
        p.requires_grad_(False)                                   # model.py:176-179
    return m.to(DEV)


def wiring_scene():
    g = torch.Generator().manual_seed(47)
    image = torch.rand((3, 64, 96), generator=g).to(DEV)
    boxes = torch.tensor([[10.0, 8.0, 50.0, 40.0], [40.0, 20.0, 90.0, 60.0]])
    yy, xx = torch.meshgrid(torch.arange(64.0), torch.arange(96.0), indexing='ij')
    masks = torch.stack([((xx >= b[0]) & (xx < b[2]) & (yy >= b[1]) & (yy < b[3])).to(torch.uint8) for b in boxes])
    target = {'boxes': boxes.to(DEV), 'labels': torch.ones(2, dtype=torch.int64, device=DEV), 'masks': masks.to(DEV)}
    return image, target


def test_maskrcnn_evaluation_is_the_chain_of_its_parts(model):
    m = model.eval()
    image, _ = wiring_scene()
    with torch.no_grad():
        images, _ = m.transform([image])
        assert images.image_sizes == [(64, 96)] and tuple(images.tensors.shape) == (1, 3, 64, 96)
        features = m.backbone(images.tensors)
        proposals, losses = m.rpn(images, features)
        assert losses == {} and proposals[0].shape[0] > 0
        dets, losses = m.roi_heads(features, proposals, images.image_sizes)
        assert losses == {} and tuple(dets[0]['masks'].shape[1:]) == (1, 28, 28)
        want = m.transform.postprocess(dets, images.image_sizes, [(64, 96)])
        got = m([image])
        torch.cuda.synchronize()
    assert len(got) == 1 and {'boxes', 'labels', 'scores', 'masks'} <= set(got[0].keys())
    D = got[0]['boxes'].shape[0]
    assert 0 < D <= 8, 'no detection: the comparison would be empty'
    assert tuple(got[0]['masks'].shape) == (D, 1, 64, 96)
    for k in ('boxes', 'labels', 'scores', 'masks'):
        assert got[0][k].dtype == want[0][k].dtype and got[0][k].shape == want[0][k].shape, k
        assert torch.equal(got[0][k].view(torch.int32 if got[0][k].dtype == torch.float32 else got[0][k].dtype),
                           want[0][k].view(torch.int32 if want[0][k].dtype == torch.float32 else want[0][k].dtype)), k
    # the single-tensor forms give the same detections
    again = m(image[None])
    assert torch.equal(again[0]['boxes'], got[0]['boxes']) and torch.equal(again[0]['masks'], got[0]['masks'])
    m.roi_heads.detections_per_img = 1            # read at call time, as model.py:187 needs
    assert m([image])[0]['boxes'].shape[0] == 1
    m.roi_heads.detections_per_img = 8


def test_maskrcnn_training_losses_are_the_chain_of_its_parts(model):
    m = model.train()
    image, target = wiring_scene()
    g = torch.Generator().manual_seed(53)
    images, targets = m.transform([image], [target])
    features = m.backbone(images.tensors)
    n_anchors = 3 * sum(f.shape[2] * f.shape[3] for f in features.values())
    rpn_keys = [torch.rand(n_anchors, generator=g).to(DEV)]
    proposals, rpn_losses = m.rpn(images, features, targets, keys=rpn_keys)
    roi_keys = [torch.rand(proposals[0].shape[0] + 2, generator=g).to(DEV)]
    dets, roi_losses = m.roi_heads(features, proposals, images.image_sizes, targets, keys=roi_keys)
    assert m.transform.postprocess(dets, images.image_sizes, [(64, 96)]) is dets
    want = dict(roi_losses, **rpn_losses)
    got = m([image], [target], rpn_keys=rpn_keys, roi_keys=roi_keys)
    torch.cuda.synchronize()
    assert list(got.keys()) == ['loss_classifier', 'loss_box_reg', 'loss_mask', 'loss_objectness', 'loss_rpn_box_reg']
    for k, v in got.items():
        assert v.dim() == 0 and bool(torch.isfinite(v)), k
        assert torch.equal(v.detach(), want[k].detach()), (k, float(v), float(want[k]))
    assert got['loss_mask'].requires_grad and not got['loss_objectness'].requires_grad
    with pytest.raises(ValueError, match='targets should be passed'):
        m([image])
    # a backbone that is not frozen is refused by the backbone itself
    p = m.backbone.body.conv1.weight
    p.requires_grad_(True)
    try:
        with pytest.raises(RuntimeError, match='inference only'):
            m([image], [target], rpn_keys=rpn_keys, roi_keys=roi_keys)
    finally:
        p.requires_grad_(False)
        m.eval()
