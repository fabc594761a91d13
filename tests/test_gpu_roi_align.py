"""GPU: MultiScaleRoIAlign (csrc/roialign.hip, sfvos_amd.roi_align) -- the step between SlowFastLayers' fused maps and the
mask branch (reference code/helpers/model.py:346: roi_heads' mask_roi_pool) -- against the torch-core restatement of
torchvision's published arithmetic in oracle/roi_align_ref.py, and the whole chain fused maps -> RoIAlign -> MaskBranch ->
loss / paste -> union with gradients flowing back into SlowFastLayers.

PARITY UNPINNED BY THE REFERENCE: torchvision is third-party, not vendored and not installed here; no reference fixture
covers this step.  Tolerances: 1e-5 of the tensor scale for RoIAlign itself (fp32 both sides; the device compiler may
fuse a multiply-add in the sample coordinates, the weights are continuous in them)."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from kernel_util import relmax
from oracle.roi_align_ref import OracleMultiScaleRoIAlign
from oracle.roi_align_ref import roi_align as ref_roi_align

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


ROIS = torch.tensor([[0, 10.3, 20.7, 110.2, 90.5],       # ordinary
                     [1, -15.0, -8.0, 40.0, 30.0],       # sticks out at the top left
                     [0, 100.0, 70.0, 140.0, 100.0],     # reaches beyond the bottom right (the map is 124 x 92 px)
                     [1, 60.0, 40.0, 60.4, 40.3],        # smaller than a feature pixel: extent forced to 1
                     [0, 30.5, 50.2, 30.5, 50.2],        # degenerate (zero area)
                     [1, 0.0, 0.0, 123.0, 91.0],         # the whole image
                     [0, 300.0, 300.0, 340.0, 350.0],    # entirely outside: every sample contributes 0
                     [1, 20.9, 5.1, 33.3, 88.8]])        # tall


def test_roi_align_matches_the_oracle_forward_and_backward():
    from sfvos_amd import roi_align
    g = torch.Generator().manual_seed(4)
    feat = torch.randn(2, 19, 23, 31, generator=g)
    scale = 0.25
    fr = feat.clone().requires_grad_(True)
    ref = ref_roi_align(fr, ROIS, 14, scale, 2)
    up = torch.randn(ref.shape, generator=g)
    (ref * up).sum().backward()
    fg = feat.to(DEV).requires_grad_(True)
    got = roi_align(fg, ROIS.to(DEV), 14, scale, 2)
    assert tuple(got.shape) == (8, 19, 14, 14) and got.dtype == torch.float32
    (got * up.to(DEV)).sum().backward()
    e_f, e_b = relmax(got.detach().cpu(), ref.detach()), relmax(fg.grad.cpu(), fr.grad)
    print('roi_align: forward max err / scale %.2e, backward %.2e' % (e_f, e_b))
    assert e_f < 1e-5 and e_b < 1e-5
    assert float(got[6].abs().max()) == 0.0, 'a RoI outside the map pools zeros'
    # deterministic backward (a gather in fixed order; torchvision scatters with atomics)
    fg2 = feat.to(DEV).requires_grad_(True)
    (roi_align(fg2, ROIS.to(DEV), 14, scale, 2) * up.to(DEV)).sum().backward()
    assert torch.equal(fg.grad, fg2.grad)
    # list-of-boxes form and other output sizes / sampling ratios
    boxes = [ROIS[ROIS[:, 0] == i][:, 1:] for i in range(2)]
    order = torch.cat([torch.where(ROIS[:, 0] == i)[0] for i in range(2)])
    got_l = roi_align(feat.to(DEV), [b.to(DEV) for b in boxes], (7, 7), scale, 4)
    ref_l = ref_roi_align(feat, ROIS[order], 7, scale, 4)
    assert relmax(got_l.cpu(), ref_l) < 1e-5
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        roi_align(feat, ROIS, 14, scale, 2)
    with pytest.raises(NotImplementedError):
        roi_align(feat.to(DEV), ROIS.to(DEV), 14, scale, 0)


@pytest.mark.parametrize('seed', range(6))
def test_roi_align_random_boxes_and_geometries(seed):
    """Random maps (1-3 images, 8-72 channels, 5-60 px), scales, square output sizes 1-14, sampling ratios 1-4 and 1-40 boxes that
    may stick out of the map, lie outside it or have no area: forward and backward against the restatement."""
    import random
    from sfvos_amd import roi_align
    rng = random.Random(77 + seed)
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = rng.randint(1, 3), 8 * rng.randint(1, 9), rng.randint(5, 60), rng.randint(5, 60)
    scale = rng.choice([1.0, 0.5, 0.25, 0.125, 1.0 / 3.0])
    out = rng.randint(1, 14)   # (the restatement is square-only)
    ratio = rng.randint(1, 4)
    K = rng.randint(1, 40)
    ih, iw = H / scale, W / scale
    rois = []
    for _ in range(K):
        x0, y0 = rng.uniform(-0.2 * iw, 1.1 * iw), rng.uniform(-0.2 * ih, 1.1 * ih)
        w, h = rng.choice([0.0, rng.uniform(0, 0.3 / scale), rng.uniform(0, iw)]), rng.choice([0.0, rng.uniform(0, ih)])
        rois.append([rng.randrange(N), x0, y0, x0 + w, y0 + h])
    rois = torch.tensor(rois, dtype=torch.float32)
    feat = torch.randn(N, C, H, W, generator=g)
    fr = feat.clone().requires_grad_(True)
    ref = ref_roi_align(fr, rois, out, scale, ratio)
    up = torch.randn(ref.shape, generator=g)
    (ref * up).sum().backward()
    fg = feat.to(DEV).requires_grad_(True)
    got = roi_align(fg, rois.to(DEV), out, scale, ratio)
    (got * up.to(DEV)).sum().backward()
    assert got.shape == ref.shape
    scale_f, scale_b = float(ref.abs().max()), float(fr.grad.abs().max())
    e_f = float((got.detach().cpu() - ref.detach()).abs().max()) / max(scale_f, 1e-6)
    e_b = float((fg.grad.cpu() - fr.grad).abs().max()) / max(scale_b, 1e-6)
    print('seed %d: %d x %d x %d x %d, scale %.3f, out %s, ratio %d, %d boxes: fwd %.1e bwd %.1e'
          % (seed, N, C, H, W, scale, out, ratio, K, e_f, e_b))
    assert e_f < 1e-5 and e_b < 1e-5


def _davis_feats(C, gen):
    from sfvos_amd import davis_pyramid
    return OrderedDict((k, torch.randn(1, C, h, w, generator=gen)) for k, (h, w) in davis_pyramid())


def test_multiscale_roi_align_matches_the_oracle_on_the_davis_pyramid():
    """The reference's configuration: feature maps '0'..'3' of the 5-level DAVIS pyramid ('pool' is not pooled from),
    image size after torchvision's transform 749 x 1333 -> scales 1/4 .. 1/32, k_min 2, k_max 5.  Boxes of every
    level, incl. the thresholds of the level mapper (sqrt(area) = 112, 224, 448) and an empty image."""
    from sfvos_amd import MultiScaleRoIAlign
    g = torch.Generator().manual_seed(8)
    x = _davis_feats(8, g)
    boxes = [torch.tensor([[100.0, 50.0, 180.0, 120.0],     # sqrt(area) 75   -> level 0
                           [10.0, 10.0, 122.0, 122.0],      # 112 exactly     -> level 1 (floor(3 + 1e-6))
                           [400.0, 200.0, 560.0, 360.0],    # 160             -> level 1
                           [0.0, 0.0, 224.0, 224.0],        # 224 exactly     -> level 2
                           [300.0, 100.0, 700.0, 500.0],    # 400             -> level 2
                           [100.0, 20.0, 1300.0, 740.0],    # 929             -> level 3
                           [650.0, 300.0, 1098.0, 748.0],   # 448 exactly     -> level 3
                           [5.0, 5.0, 6.0, 6.0]])]          # 1               -> level 0 (clamped)
    shapes = [(749, 1333)]
    oracle = OracleMultiScaleRoIAlign(['0', '1', '2', '3'], 14, 2)
    xr = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in x.items())
    ref = oracle(xr, boxes, shapes)
    up = torch.randn(ref.shape, generator=g)
    (ref * up).sum().backward()
    pool = MultiScaleRoIAlign(['0', '1', '2', '3'], 14, 2)
    xg = OrderedDict((k, v.to(DEV).requires_grad_(True)) for k, v in x.items())
    got = pool(xg, [b.to(DEV) for b in boxes], shapes)
    assert pool.scales == [0.25, 0.125, 0.0625, 0.03125] and (pool.k_min, pool.k_max) == (2, 5)
    (got * up.to(DEV)).sum().backward()
    e = relmax(got.detach().cpu(), ref.detach())
    print('MultiScaleRoIAlign on the DAVIS pyramid: forward max err / scale %.2e' % e)
    assert e < 1e-5
    for k in ('0', '1', '2', '3'):
        eb = relmax(xg[k].grad.cpu(), xr[k].grad)
        print('   level %s: gradient max err / scale %.2e, %d non-zero entries' % (k, eb, int((xr[k].grad != 0).sum())))
        assert eb < 1e-5 and float(xr[k].grad.abs().max()) > 0, k
    assert xg['pool'].grad is None and xr['pool'].grad is None
    # no boxes at all (no detection): an empty result that still back-propagates zeros
    empty = pool(xg, [torch.zeros(0, 4, device=DEV)], shapes)
    assert tuple(empty.shape) == (0, 8, 14, 14)
    for v in xg.values():
        v.grad = None
    empty.sum().backward()
    assert float(xg['0'].grad.abs().max()) == 0.0


def test_fused_maps_through_roi_align_and_mask_branch_end_to_end():
    """VERDICT r2 Next 7: SlowFastLayers -> fused maps -> MultiScaleRoIAlign -> MaskBranch -> maskrcnn_loss with the
    gradients flowing back into SlowFastLayers' parameters, and the inference chain -> paste -> >= 0.5 union
    (model.py:340-347, davis_evaluate.py:40-42), against the same chain of CPU restatements.  fp32; (sp, fp) = (3, 7);
    a 5-level pyramid of a 192 x 320 image.  Gradients behind ReLU masks: rel-L2 5e-3."""
    from golden_util import rel_err
    from oracle.closed_form import closed_form_state_dict
    from oracle.mask_head_ref import OracleMaskBranch, maskrcnn_inference as ref_inference, maskrcnn_loss as ref_loss
    from oracle.mask_head_ref import paste_masks_in_image as ref_paste
    from oracle.slowfast_ref import OracleSlowFastLayers
    from sfvos_amd import MaskBranch, MultiScaleRoIAlign, SlowFastLayers, maskrcnn_loss, union_mask
    sp, fp = 3, 7
    H, W = 192, 320
    levels = OrderedDict([('0', (48, 80)), ('1', (24, 40)), ('2', (12, 20)), ('3', (6, 10)), ('pool', (3, 5))])
    g = torch.Generator().manual_seed(31)
    fast = OrderedDict((k, torch.randn(fp, 256, h, w, generator=g)) for k, (h, w) in levels.items())
    slow = OrderedDict((k, v[2:5]) for k, v in fast.items())
    boxes = [torch.tensor([[20.0, 30.0, 100.0, 90.0], [150.0, 10.0, 310.0, 180.0], [0.0, 0.0, 319.0, 191.0],
                           [200.0, 100.0, 230.0, 140.0], [60.0, 60.0, 250.0, 190.0]])]
    labels = torch.tensor([1, 1, 1, 0, 1])
    targets = (torch.rand(5, 28, 28, generator=g) > 0.5).float()
    # ---- CPU chain
    torch.manual_seed(3)
    o_sf = OracleSlowFastLayers(256, torch.device('cpu'), sp, fp)
    o_sf.load_state_dict(closed_form_state_dict(o_sf))
    o_sf.train()
    o_mb = OracleMaskBranch(256, 2)
    o_pool = OracleMultiScaleRoIAlign(['0', '1', '2', '3'], 14, 2)
    fused_r = o_sf.temporally_enhance_features([slow], [fast])
    roi_r = o_pool(fused_r, boxes, [(H, W)])
    loss_r = ref_loss(o_mb(roi_r), labels, targets)
    loss_r.backward()
    # ---- GPU chain
    sf = SlowFastLayers(256, torch.device(DEV), sp, fp, precision='fp32')
    sf.load_state_dict(closed_form_state_dict(sf))   # (not o_sf's: its running statistics have already seen the clip)
    sf = sf.to(DEV).train()
    mb = MaskBranch(256, 2, 'fp32')
    mb.load_state_dict(o_mb.state_dict(), strict=True)
    mb = mb.to(DEV)
    pool = MultiScaleRoIAlign(['0', '1', '2', '3'], 14, 2)
    fused = sf.temporally_enhance_features([OrderedDict((k, v.to(DEV)) for k, v in slow.items())],
                                           [OrderedDict((k, v.to(DEV)) for k, v in fast.items())])
    roi = pool(fused, [b.to(DEV) for b in boxes], [(H, W)])
    assert relmax(roi.detach().cpu(), roi_r.detach()) < 1e-4
    loss = maskrcnn_loss(mb(roi), labels.to(DEV), targets.to(DEV))
    loss.backward()
    lv, lr = float(loss.detach()), float(loss_r.detach())
    assert abs(lv - lr) < 1e-4 * abs(lr), (lv, lr)
    worst = 0.0
    ref_p = dict(o_sf.named_parameters())
    for name, p in sf.named_parameters():
        assert p.grad is not None, name
        if name.endswith(('conv1.bias', 'conv2.bias', 'conv3.bias')):
            continue      # a conv bias in front of a train-mode BatchNorm: true gradient 0
        e = rel_err(p.grad.cpu().numpy(), ref_p[name].grad.numpy())
        worst = max(worst, e)
        assert e < 5e-3, (name, e)
    ref_m = dict(o_mb.named_parameters())
    for name, p in mb.named_parameters():
        e = rel_err(p.grad.cpu().numpy(), ref_m[name].grad.numpy())
        worst = max(worst, e)
        assert e < 5e-3, (name, e)
    print('end to end (SlowFastLayers -> RoIAlign -> MaskBranch -> loss): loss %.6f (oracle %.6f), worst parameter-gradient '
          'rel-L2 %.2e' % (lv, lr, worst))
    # ---- inference chain: eval-mode fused maps -> RoIAlign -> predict (sigmoid, paste) -> union
    sf.eval(); o_sf.eval()
    with torch.no_grad():
        fused_r = o_sf.temporally_enhance_features([slow], [fast])
        prob_r = ref_paste(ref_inference(o_mb(o_pool(fused_r, boxes, [(H, W)])), labels), boxes[0], (H, W))
        fused = sf.temporally_enhance_features([OrderedDict((k, v.to(DEV)) for k, v in slow.items())],
                                               [OrderedDict((k, v.to(DEV)) for k, v in fast.items())])
        prob = mb.predict(pool(fused, [b.to(DEV) for b in boxes], [(H, W)]), labels.to(DEV), boxes[0].to(DEV), (H, W))
    assert float((prob.cpu() - prob_r).abs().max()) < 1e-4
    total = np.zeros((H, W), dtype=bool)
    for mk in prob_r:
        total = np.logical_or(total, (mk.numpy() >= 0.5)[0])
    near = ((prob_r - 0.5).abs() < 1e-4).any(0)[0].numpy()
    uni = union_mask(prob).cpu().numpy()
    assert np.array_equal(uni[~near], total[~near])
