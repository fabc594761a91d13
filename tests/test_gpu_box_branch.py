"""GPU: the box branch of roi_heads (sfvos_amd.BoxBranch, fastrcnn_loss, RoIHeadsInference; reference
code/helpers/model.py:346-347,369) on libsfvos kernels against the torch-core restatements tests/box_branch_ref.py,
oracle/roi_align_ref.py, oracle/mask_head_ref.py and oracle/slowfast_ref.py.

PARITY UNPINNED BY THE REFERENCE: the arithmetic is torchvision's (third-party, not vendored, not installed here); the
restatements are written from its published sources.  Gates are the project's existing ones: forward 1e-4 (fp32) / 2e-2
(bf16) of the tensor's scale (tests/test_gpu_kernels.py); fp32 training step: loss 1e-5, gradients 5e-5 of the tensor's
scale on inputs without ReLU-mask flips (test_mask_branch_training_step_matches_the_oracle); FusedSGD trajectory 1e-2 /
5e-2 on the losses, 5e-2 / 0.15 on outputs and parameters (test_mask_branch_fused_sgd_trajectory_matches_the_oracle);
end to end 5e-3 rel-L2 (test_fused_maps_through_roi_align_and_mask_branch_end_to_end); pasted probabilities 1e-4.
bf16 gradients have no derived bound at module level: BF16_MEASURED below."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import box_branch_ref as R
from kernel_util import rel_l2, relmax
from oracle.roi_align_ref import OracleMultiScaleRoIAlign

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

LEVELS = OrderedDict([('0', (48, 80)), ('1', (24, 40)), ('2', (12, 20)), ('3', (6, 10)), ('pool', (3, 5))])
IMAGE = (192, 320)


def make(precision, num_classes=2, seed=5, predictor_scale=8.0):
    from sfvos_amd import BoxBranch
    torch.manual_seed(seed)
    o = R.RefBoxBranch(num_classes)
    with torch.no_grad():
        # the predictor's default initialisation gives logits and deltas of a few 1e-2: raise it, so that scores,
        # decoded boxes and both losses are exercised away from their trivial values
        o.box_predictor.cls_score.weight.mul_(predictor_scale)
        o.box_predictor.bbox_pred.weight.mul_(predictor_scale)
    m = BoxBranch(num_classes, precision)
    m.load_state_dict(o.state_dict(), strict=True)
    return m.to(DEV), o


def random_boxes(n, gen, image=IMAGE):
    H, W = image
    c = torch.rand(n, 2, generator=gen) * torch.tensor([W, H], dtype=torch.float32)
    s = 8 + torch.rand(n, 2, generator=gen) * torch.tensor([W * 0.6, H * 0.6])
    b = torch.cat([c - s / 2, c + s / 2], 1)
    b[:, 0::2] = b[:, 0::2].clamp(0, W)
    b[:, 1::2] = b[:, 1::2].clamp(0, H)
    return b


def pyramid(batch, gen, channels=256):
    return OrderedDict((k, torch.randn(batch, channels, h, w, generator=gen)) for k, (h, w) in LEVELS.items())


def to_dev(x, grad=False):
    return OrderedDict((k, v.to(DEV).requires_grad_(grad)) for k, v in x.items())


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_box_branch_forward_matches_the_restatement(precision):
    """BoxBranch.forward on the RoIAligned features of a random two-image pyramid: logits and deltas."""
    m, o = make(precision)
    g = torch.Generator().manual_seed(9)
    x = pyramid(2, g)
    props = [random_boxes(37, g), random_boxes(52, g)]
    shapes = [IMAGE, IMAGE]
    with torch.no_grad():
        roi_r = OracleMultiScaleRoIAlign(['0', '1', '2', '3'], 7, 2)(x, props, shapes)
        ref_l, ref_d = o(roi_r)
        got_l, got_d = m(to_dev(x), [p.to(DEV) for p in props], shapes)
        h_ref = o.box_head(roi_r)
        h_got = m.box_head(roi_r.to(DEV))
    with pytest.raises(RuntimeError, match='inference only'):      # on their own the two modules record no graph
        m.box_head(roi_r.to(DEV))
    with pytest.raises(RuntimeError, match='inference only'):
        m.box_predictor(h_ref.to(DEV))
    assert tuple(got_l.shape) == (89, 2) and tuple(got_d.shape) == (89, 8) and got_l.dtype == torch.float32
    tol = 1e-4 if precision == 'fp32' else 2e-2
    e = (relmax(h_got.cpu(), h_ref), relmax(got_l.cpu(), ref_l), relmax(got_d.cpu(), ref_d))
    print('box branch %s: head max err / scale %.2e, logits %.2e, deltas %.2e' % ((precision,) + e))
    assert max(e) < tol
    with torch.no_grad():     # the predictor alone through its own entry point; two runs bit-identical
        p_l, p_d = m.box_predictor(h_ref.to(DEV))
        again = m(to_dev(x), [p.to(DEV) for p in props], shapes)
    rl, rd = o.box_predictor(h_ref)
    assert relmax(p_l.cpu(), rl) < tol and relmax(p_d.cpu(), rd) < tol
    assert torch.equal(again[0], got_l) and torch.equal(again[1], got_d)


def _relu_mask_mismatches(m, o, roi):
    with torch.no_grad():
        _, h6, h7 = m.box_head.forward_rows(roi.to(DEV))
        r6 = torch.relu(o.box_head.fc6(roi.flatten(1)))
        r7 = torch.relu(o.box_head.fc7(r6))
    return int(((h6.float().cpu() > 0) != (r6 > 0)).sum()) + int(((h7.float().cpu() > 0) != (r7 > 0)).sum())


def training_inputs(seed, n_per_image=(23, 17)):
    g = torch.Generator().manual_seed(seed)
    x = pyramid(2, g)
    props = [random_boxes(n, g) for n in n_per_image]
    labels = [torch.randint(0, 2, (n,), generator=g) for n in n_per_image]
    gt = [p + torch.randn(p.shape, generator=g) * 6 for p in props]
    gt = [torch.cat([torch.minimum(b[:, :2], b[:, 2:] - 4), b[:, 2:]], 1) for b in gt]
    targets = [R.encode_boxes(b, p) for b, p in zip(gt, props)]
    return x, props, labels, targets


# rel-L2 of each tensor of the bf16 training step against the float64 restatement, measured on an MI355X; the gate is
# 2 x the measured value (this project's practice for bf16 gradients).  The proposals of the test reach levels 0 and 1.
BF16_MEASURED = {
    'loss_classifier': 1.252e-04,
    'loss_box_reg': 1.038e-04,
    'box_head.fc6.weight': 5.536e-02,
    'box_head.fc6.bias': 5.574e-02,
    'box_head.fc7.weight': 3.771e-02,
    'box_head.fc7.bias': 3.679e-02,
    'box_predictor.cls_score.weight': 3.302e-03,
    'box_predictor.cls_score.bias': 9.344e-04,
    'box_predictor.bbox_pred.weight': 4.502e-03,
    'box_predictor.bbox_pred.bias': 1.875e-03,
    'roi features': 5.838e-02,
    'fused map 0': 5.714e-02,
    'fused map 1': 8.183e-03,
}


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_box_branch_training_step_matches_the_restatement(precision):
    """fastrcnn_loss + backward: both losses, the 8 parameter gradients, the gradient w.r.t. the RoI features and,
    through MultiScaleRoIAlign, w.r.t. the fused maps.

    fp32, against the fp32 restatement: losses 1e-5, gradients 5e-5 of each tensor's scale.  The input is the first of
    the seeds 21.. whose ReLU masks of fc6 and fc7 are the same on both sides (a pre-activation within fp32 rounding of
    zero flips its mask and moves the gradients behind it by O(1e-3): a property of comparing two correct
    implementations, DESIGN.md 'ReLU masks').

    bf16, against the float64 restatement on the bf16-rounded maps: no derived bound exists at module level; rel-L2 per
    tensor is measured, printed as measured / gate and gated at 2 x the value measured on an MI355X (BF16_MEASURED):
    losses 1.3e-4 / 1.0e-4; fc6 weight / bias 5.5e-2 / 5.6e-2, fc7 3.8e-2 / 3.7e-2 (behind one and two bf16 ReLU layers),
    cls_score 3.3e-3 / 9.3e-4, bbox_pred 4.5e-3 / 1.9e-3; RoI features 5.8e-2, fused maps 5.7e-2 (level 0) and 8.2e-3
    (level 1)."""
    from sfvos_amd import fastrcnn_loss
    m, o = make(precision)
    pool_r = OracleMultiScaleRoIAlign(['0', '1', '2', '3'], 7, 2)
    shapes = [IMAGE, IMAGE]
    for seed in range(21, 29):
        x, props, labels, targets = training_inputs(seed)
        if precision == 'bf16':
            x = OrderedDict((k, v.bfloat16().float()) for k, v in x.items())
            break
        with torch.no_grad():
            roi = pool_r(x, props, shapes)
        if _relu_mask_mismatches(m, o, roi) == 0:
            break
    else:
        pytest.fail('no input without ReLU-mask flips in 8 seeds')
    if precision == 'bf16':
        o = o.double()
        xr = OrderedDict((k, v.double().requires_grad_(True)) for k, v in x.items())
    else:
        xr = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in x.items())
    roi_r = pool_r(xr, props, shapes)
    roi_r.retain_grad()
    lc_r, lb_r = R.fastrcnn_loss(*o(roi_r), labels, [t.to(roi_r.dtype) for t in targets])
    (lc_r + lb_r).backward()
    xg = to_dev(x, grad=True)
    roi = m.box_roi_pool(xg, [p.to(DEV) for p in props], shapes)
    roi.retain_grad()
    logits, deltas = m.forward_features(roi)
    assert logits.requires_grad and deltas.requires_grad
    lc, lb = fastrcnn_loss(logits, deltas, [l.to(DEV) for l in labels], [t.to(DEV) for t in targets])
    (lc + lb).backward()
    torch.cuda.synchronize()
    pairs = [('loss_classifier', lc.detach().cpu(), lc_r.detach()), ('loss_box_reg', lb.detach().cpu(), lb_r.detach())]
    names = dict(o.named_parameters())
    for name, p in m.named_parameters():
        assert p.grad is not None, name
        pairs.append((name, p.grad.cpu(), names[name].grad))
    pairs.append(('roi features', roi.grad.cpu(), roi_r.grad))
    for k in ('0', '1', '2', '3'):
        if xr[k].grad is None:     # no proposal is large enough for this level: zeros here, no gradient there
            assert float(xg[k].grad.abs().max()) == 0.0
            continue
        assert float(xr[k].grad.abs().max()) > 0
        pairs.append(('fused map ' + k, xg[k].grad.cpu(), xr[k].grad))
    assert sum(name.startswith('fused map') for name, _, _ in pairs) >= 2
    assert xg['pool'].grad is None
    print('box branch training %s (seed %d): losses %.6f %.6f (restatement %.6f %.6f)'
          % (precision, seed, float(lc), float(lb), float(lc_r), float(lb_r)))
    failed = []
    for name, got, ref in pairs:
        if precision == 'fp32':
            e = relmax(got, ref)
            gate = 1e-5 if name.startswith('loss') else 5e-5
        else:
            e = rel_l2(got, ref)
            gate = 2.0 * BF16_MEASURED[name] if BF16_MEASURED.get(name) is not None else float('nan')
        print('   %-34s measured %.3e / gate %.3e' % (name, e, gate))
        if not e <= gate:
            failed.append((name, e, gate))
    assert not failed, failed
    # frozen parameters get no gradient; nothing is recorded under no_grad
    for p in m.parameters():
        p.grad = None
    m.box_head.fc6.weight.requires_grad_(False)
    lc, lb = fastrcnn_loss(*m.forward_features(roi.detach()), labels, targets)
    (lc + lb).backward()
    assert m.box_head.fc6.weight.grad is None and m.box_head.fc7.weight.grad is not None
    with torch.no_grad():
        assert not m.forward_features(roi.detach())[0].requires_grad


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_box_and_mask_branch_fused_sgd_trajectory_matches_the_restatements(precision):
    """Four FusedSGD steps of BoxBranch + MaskBranch in ONE optimiser against the restatements under torch.optim.SGD
    (lr 0.02, momentum 0.9, weight decay 1e-4): the three losses of every step, the outputs after the last step and the
    parameters.  FusedSGD rewrites the parameters through raw pointers, so the packed images of fc6 / fc7 (forward and
    data gradient) must follow _lib.weight_epoch(): a stale image shows as step 2 repeating step 1's loss."""
    from oracle.mask_head_ref import OracleMaskBranch, maskrcnn_loss as ref_mask_loss
    from sfvos_amd import FusedSGD, MaskBranch, fastrcnn_loss, maskrcnn_loss
    m, o = make(precision, predictor_scale=1.0)    # default initialisation: lr 0.02 contracts from there
    torch.manual_seed(6)
    o_mb = OracleMaskBranch(256, 2)
    mb = MaskBranch(256, 2, precision)
    mb.load_state_dict(o_mb.state_dict(), strict=True)
    mb = mb.to(DEV)
    N = 12
    g = torch.Generator().manual_seed(77)
    roi7 = torch.randn(N, 256, 7, 7, generator=g).relu()
    roi14 = torch.randn(6, 256, 14, 14, generator=g).relu()
    if precision == 'bf16':
        roi7, roi14 = roi7.bfloat16().float(), roi14.bfloat16().float()
    labels = torch.tensor([1, 0, 1, 1, 0, 1, 1, 0, 0, 1, 1, 0])
    targets = torch.randn(N, 4, generator=g)
    mlabels = torch.tensor([1, 0, 1, 1, 0, 1])
    mtargets = (torch.rand(6, 28, 28, generator=g) > 0.5).float()
    opt = FusedSGD(list(m.parameters()) + list(mb.parameters()), lr=0.02, momentum=0.9, weight_decay=1e-4)
    ropt = torch.optim.SGD(list(o.parameters()) + list(o_mb.parameters()), lr=0.02, momentum=0.9, weight_decay=1e-4)
    a7, a14 = roi7.to(DEV), roi14.to(DEV)
    losses, rlosses = [], []
    for step in range(4):
        opt.zero_grad()
        lc, lb = fastrcnn_loss(*m.forward_features(a7), [labels.to(DEV)], [targets.to(DEV)])
        lm = maskrcnn_loss(mb(a14), mlabels.to(DEV), mtargets.to(DEV))
        (lc + lb + lm).backward()
        opt.step()
        ropt.zero_grad()
        rc, rb = R.fastrcnn_loss(*o(roi7), [labels], [targets])
        rm = ref_mask_loss(o_mb(roi14), mlabels, mtargets)
        (rc + rb + rm).backward()
        ropt.step()
        losses.append([float(lc.detach()), float(lb.detach()), float(lm.detach())])
        rlosses.append([float(rc.detach()), float(rb.detach()), float(rm.detach())])
    with torch.no_grad():
        got, ref = m.forward_features(a7), o(roi7)
    tol_l, tol_o = (1e-2, 5e-2) if precision == 'fp32' else (5e-2, 0.15)
    print('box + mask branch %s FusedSGD trajectory (classifier, box, mask):' % precision)
    for a, b in zip(losses, rlosses):
        print('   %s vs restatement %s' % (['%.5f' % v for v in a], ['%.5f' % v for v in b]))
    box = [a + b for a, b, _ in rlosses]
    assert min(abs(p - q) for p, q in zip(box, box[1:])) > 0.1 * abs(box[0]), 'every step must move the box losses'
    for a, b in zip(losses, rlosses):
        assert abs(sum(a[:2]) - sum(b[:2])) <= tol_l * abs(sum(b[:2])), (losses, rlosses)
        assert abs(a[2] - b[2]) <= tol_l * abs(b[2]), (losses, rlosses)
    assert relmax(got[0].cpu(), ref[0]) < tol_o and relmax(got[1].cpu(), ref[1]) < tol_o
    for mod, ref_mod in ((m, o), (mb, o_mb)):
        names = dict(ref_mod.named_parameters())
        for name, p in mod.named_parameters():
            assert rel_l2(p.detach().cpu(), names[name].detach()) < tol_o, name


def test_box_branch_without_rois_bad_labels_and_no_positive():
    from sfvos_amd import fastrcnn_loss
    m, _ = make('fp32')
    g = torch.Generator().manual_seed(2)
    x = to_dev(pyramid(1, g), grad=True)
    # no proposal at all: empty outputs that stay on the graph, zero losses, zero gradients
    logits, deltas = m(x, [torch.zeros(0, 4, device=DEV)], [IMAGE])
    assert tuple(logits.shape) == (0, 2) and tuple(deltas.shape) == (0, 8) and logits.requires_grad
    lc, lb = fastrcnn_loss(logits, deltas, [torch.zeros(0, dtype=torch.int64, device=DEV)],
                           [torch.zeros(0, 4, device=DEV)])
    assert float(lc) == 0.0 and float(lb) == 0.0
    (lc + lb).backward()
    assert float(x['0'].grad.abs().max()) == 0.0
    assert m.box_head.fc6.weight.grad is not None and float(m.box_head.fc6.weight.grad.abs().max()) == 0.0
    with torch.no_grad():
        assert m.detect(x, [torch.zeros(0, 4, device=DEV)], [IMAGE])[0]['boxes'].shape == (0, 4)
    # labels out of range: NaN losses, zero gradient for their rows, never an out-of-range read
    roi = torch.randn(3, 256, 7, 7, generator=g).relu().to(DEV)
    logits, deltas = m.forward_features(roi)
    logits, deltas = logits.detach().requires_grad_(True), deltas.detach().requires_grad_(True)
    lc, lb = fastrcnn_loss(logits, deltas, [torch.tensor([1, 7, -1], device=DEV)], [torch.zeros(3, 4, device=DEV)])
    assert torch.isnan(lc) and torch.isnan(lb)
    (lc + lb).backward()
    assert float(logits.grad[1:].abs().max()) == 0.0 and float(deltas.grad[1:].abs().max()) == 0.0
    # no positive RoI: the box loss is 0 and on the graph
    for p in m.parameters():
        p.grad = None
    logits, deltas = m.forward_features(roi)
    lc, lb = fastrcnn_loss(logits, deltas, [torch.zeros(3, dtype=torch.int64, device=DEV)],
                           [torch.zeros(3, 4, device=DEV)])
    assert float(lb) == 0.0 and lb.requires_grad and float(lc) > 0
    lb.backward()
    assert float(m.box_predictor.bbox_pred.weight.grad.abs().max()) == 0.0


def test_coder_functions_match_the_restatement():
    from sfvos_amd import decode_boxes, encode_boxes, resize_boxes
    g = torch.Generator().manual_seed(3)
    props, gt = random_boxes(50, g), random_boxes(50, g)
    t = encode_boxes(gt.to(DEV), props.to(DEV))
    assert relmax(t.cpu(), R.encode_boxes(gt.double(), props.double())) < 1e-5
    back = decode_boxes(t, props.to(DEV))
    assert tuple(back.shape) == (50, 1, 4) and float((back[:, 0].cpu() - gt).abs().max()) < 1e-3
    r = resize_boxes(gt.to(DEV), IMAGE, (480, 854))
    assert relmax(r.cpu(), R.resize_boxes(gt, IMAGE, (480, 854))) < 1e-6
    assert encode_boxes(gt[:0].to(DEV), props[:0].to(DEV)).shape == (0, 4)


def test_box_branch_loads_a_reference_checkpoint_slice_strictly():
    import io
    from sfvos_amd import BoxBranch
    from test_box_branch_cpu import WANT
    g = torch.Generator().manual_seed(1)
    ckpt = {'slow_fast.bn_f1.weight': torch.ones(32)}
    ckpt.update({'maskrcnn_model.roi_heads.' + k: torch.randn(s, generator=g) * 0.02 for k, s in WANT.items()})
    buf = io.BytesIO()
    torch.save(ckpt, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=True)
    prefix = 'maskrcnn_model.roi_heads.'
    sl = {k[len(prefix):]: v for k, v in loaded.items() if k.startswith(prefix)}
    m = BoxBranch(2, 'fp32')
    m.load_state_dict(sl, strict=True)
    o = R.RefBoxBranch(2)
    o.load_state_dict(m.state_dict(), strict=True)
    x = torch.randn(5, 256, 7, 7, generator=g).relu()
    with torch.no_grad():
        got, ref = m.to(DEV).forward_features(x.to(DEV)), o(x)
    assert relmax(got[0].cpu(), ref[0]) < 1e-4 and relmax(got[1].cpu(), ref[1]) < 1e-4


def _slowfast_pair(train):
    from oracle.closed_form import closed_form_state_dict
    from oracle.slowfast_ref import OracleSlowFastLayers
    from sfvos_amd import SlowFastLayers
    sp, fp = 3, 7
    torch.manual_seed(3)
    o_sf = OracleSlowFastLayers(256, torch.device('cpu'), sp, fp)
    o_sf.load_state_dict(closed_form_state_dict(o_sf))
    sf = SlowFastLayers(256, torch.device(DEV), sp, fp, precision='fp32')
    sf.load_state_dict(closed_form_state_dict(sf))
    sf = sf.to(DEV)
    (o_sf.train(), sf.train()) if train else (o_sf.eval(), sf.eval())
    g = torch.Generator().manual_seed(31)
    fast = OrderedDict((k, torch.randn(fp, 256, h, w, generator=g)) for k, (h, w) in LEVELS.items())
    slow = OrderedDict((k, v[2:5]) for k, v in fast.items())
    return sf, o_sf, slow, fast, g


def test_end_to_end_evaluation_fused_maps_to_union_mask():
    """SlowFastLayers (small (sp, fp), eval) -> RoIHeadsInference -> union_mask against the chain of restatements, with
    the two-stage rule: logits and deltas within the forward gate; the detections the restatement selects from the
    module's own candidates must equal the module's; masks of equal detections within the `predict` gate (1e-4); the
    union may differ only at pixels whose reference probability is within 1e-4 of 0.5 (their share is printed)."""
    from oracle.mask_head_ref import OracleMaskBranch, maskrcnn_inference as ref_inference
    from oracle.mask_head_ref import paste_masks_in_image as ref_paste
    from sfvos_amd import RoIHeadsInference, union_mask
    sf, o_sf, slow, fast, g = _slowfast_pair(train=False)
    _, o = make('fp32')
    torch.manual_seed(6)
    o_mb = OracleMaskBranch(256, 2)
    heads = RoIHeadsInference(2, 'fp32', box_detections_per_img=10)      # model.py:187
    heads.box.load_state_dict(o.state_dict(), strict=True)
    heads.mask.load_state_dict(o_mb.state_dict(), strict=True)
    heads = heads.to(DEV)
    props = [random_boxes(120, g)]
    shapes = [IMAGE]
    pd = [p.to(DEV) for p in props]
    with torch.no_grad():
        fused_r = o_sf.temporally_enhance_features([slow], [fast])
        fused = sf.temporally_enhance_features([OrderedDict((k, v.to(DEV)) for k, v in slow.items())],
                                               [OrderedDict((k, v.to(DEV)) for k, v in fast.items())])
        ref_l, ref_d = o(OracleMultiScaleRoIAlign(['0', '1', '2', '3'], 7, 2)(fused_r, props, shapes))
        got_l, got_d = heads.box(fused, pd, shapes)
        e = (relmax(got_l.cpu(), ref_l), relmax(got_d.cpu(), ref_d))
        print('end to end evaluation: logits max err / scale %.2e, deltas %.2e' % e)
        assert max(e) < 1e-4
        cb, cs, cl = heads.box.candidates(got_l, got_d, pd[0], IMAGE)
        rb, rs, _ = R.candidates(ref_l.double(), ref_d.double(), props[0].double(), IMAGE)
        assert float((cb.cpu() - rb).abs().max()) < 1e-2 and float((cs.cpu() - rs).abs().max()) < 1e-5
        dets = heads(fused, pd, shapes)[0]
        want = R.select_detections(cb.cpu().double(), cs.cpu().double(), cl.cpu(), 0.05, 0.5, 10)
        assert dets['index'].cpu().tolist() == want.tolist()
        D = want.numel()
        assert 1 <= D <= 10
        assert torch.equal(dets['boxes'].cpu(), cb.cpu()[want]) and torch.equal(dets['scores'].cpu(), cs.cpu()[want])
        boxes = dets['boxes'].cpu()
        roi_r = OracleMultiScaleRoIAlign(['0', '1', '2', '3'], 14, 2)(fused_r, [boxes], shapes)
        prob_r = ref_paste(ref_inference(o_mb(roi_r), dets['labels'].cpu()), boxes, IMAGE)
    prob = dets['masks']
    assert tuple(prob.shape) == (D, 1) + IMAGE
    assert float((prob.cpu() - prob_r).abs().max()) < 1e-4
    total = np.zeros(IMAGE, dtype=bool)
    for mk in prob_r:
        total = np.logical_or(total, (mk.numpy() >= 0.5)[0])
    near = ((prob_r - 0.5).abs() < 1e-4).any(0)[0].numpy()
    uni = union_mask(prob).cpu().numpy()
    print('end to end evaluation: %d detections, union mask %d px, %.4f %% of the pixels within 1e-4 of 0.5'
          % (D, int(total.sum()), 100.0 * near.mean()))
    assert np.array_equal(uni[~near], total[~near])
    # transform.postprocess: boxes resized and masks pasted at the original size
    with torch.no_grad():
        big = heads(fused, pd, shapes, original_image_sizes=[(480, 800)])[0]
    assert tuple(big['masks'].shape) == (D, 1, 480, 800)
    assert relmax(big['boxes'].cpu(), R.resize_boxes(boxes, IMAGE, (480, 800))) < 1e-6


def test_end_to_end_training_mask_and_box_losses_into_slowfast():
    """Mask loss + box losses summed, one backward into SlowFastLayers' parameters (model.py:369): every gradient within
    5e-3 rel-L2 of the chain of restatements (fp32)."""
    from golden_util import rel_err
    from oracle.mask_head_ref import OracleMaskBranch, maskrcnn_loss as ref_mask_loss
    from sfvos_amd import MaskBranch, MultiScaleRoIAlign, fastrcnn_loss, maskrcnn_loss
    sf, o_sf, slow, fast, g = _slowfast_pair(train=True)
    m, o = make('fp32')
    torch.manual_seed(6)
    o_mb = OracleMaskBranch(256, 2)
    mb = MaskBranch(256, 2, 'fp32')
    mb.load_state_dict(o_mb.state_dict(), strict=True)
    mb = mb.to(DEV)
    shapes = [IMAGE]
    props = [random_boxes(24, g)]
    labels = [torch.randint(0, 2, (24,), generator=g)]
    targets = [torch.randn(24, 4, generator=g)]
    pos = torch.where(labels[0] > 0)[0]
    mboxes = [props[0][pos]]
    mlabels = labels[0][pos]
    mtargets = (torch.rand(pos.numel(), 28, 28, generator=g) > 0.5).float()
    # ---- CPU chain
    fused_r = o_sf.temporally_enhance_features([slow], [fast])
    rc, rb = R.fastrcnn_loss(*o(OracleMultiScaleRoIAlign(['0', '1', '2', '3'], 7, 2)(fused_r, props, shapes)), labels,
                             targets)
    rm = ref_mask_loss(o_mb(OracleMultiScaleRoIAlign(['0', '1', '2', '3'], 14, 2)(fused_r, mboxes, shapes)), mlabels,
                       mtargets)
    (rc + rb + rm).backward()
    # ---- GPU chain
    fused = sf.temporally_enhance_features([OrderedDict((k, v.to(DEV)) for k, v in slow.items())],
                                           [OrderedDict((k, v.to(DEV)) for k, v in fast.items())])
    lc, lb = fastrcnn_loss(*m(fused, [p.to(DEV) for p in props], shapes), [l.to(DEV) for l in labels],
                           [t.to(DEV) for t in targets])
    roi14 = MultiScaleRoIAlign(['0', '1', '2', '3'], 14, 2)(fused, [b.to(DEV) for b in mboxes], shapes)
    lm = maskrcnn_loss(mb(roi14), mlabels.to(DEV), mtargets.to(DEV))
    (lc + lb + lm).backward()
    for a, b in ((lc, rc), (lb, rb), (lm, rm)):
        assert abs(float(a) - float(b)) < 1e-4 * abs(float(b)), (float(a), float(b))
    worst = 0.0
    for mod, ref_mod in ((sf, o_sf), (m, o), (mb, o_mb)):
        ref_p = dict(ref_mod.named_parameters())
        for name, p in mod.named_parameters():
            assert p.grad is not None, name
            if mod is sf and name.endswith(('conv1.bias', 'conv2.bias', 'conv3.bias')):
                continue      # a conv bias in front of a train-mode BatchNorm: true gradient 0
            e = rel_err(p.grad.cpu().numpy(), ref_p[name].grad.numpy())
            worst = max(worst, e)
            assert e < 5e-3, (name, e)
    print('end to end training (SlowFastLayers -> RoIAlign -> box + mask branches -> losses): %.6f %.6f %.6f '
          '(restatements %.6f %.6f %.6f), worst parameter-gradient rel-L2 %.2e'
          % (float(lc), float(lb), float(lm), float(rc), float(rb), float(rm), worst))
