"""GPU: sfvos_amd.roi_heads -- select_training_samples, project_masks_on_boxes and RoIHeads (reference
code/helpers/model.py:346 with targets, :369) -- on a tiny pyramid (the 192 x 320 image of tests/test_gpu_box_branch.py)
against the chain of restatements: tests/roi_targets_ref.py for the targets, tests/box_branch_ref.py,
oracle/roi_align_ref.py and oracle/mask_head_ref.py for the branches.  Two images, one without ground truth; proposals and
ground truth on the quarter-pixel grid (the matcher decides exactly) with sides that are multiples of 14 pixels (both
RoIAligns take the same interpolation weights on both sides, see `scene`); given keys; batch_size_per_image = 32.

PARITY UNPINNED BY THE REFERENCE.  Gates: those tests/test_gpu_box_branch.py applies to its own training step -- fp32
losses 1e-5, gradients 5e-5 of each tensor's scale, on the first of the seeds 21.. whose ReLU masks are the same on both
sides, each side on its own RoI features (a pre-activation within fp32 rounding of zero flips its mask and moves the gradients behind it by O(1e-3): a
property of comparing two correct implementations, DESIGN.md 'ReLU masks'); bf16: the losses only, finite and within that
file's bf16 gate for forward quantities, 2e-2."""
from collections import OrderedDict

import pytest
import torch

import box_branch_ref as R
import roi_targets_ref as T
from kernel_util import TRANS, U22, check_abs, relmax
from oracle.mask_head_ref import OracleMaskBranch, maskrcnn_loss as ref_mask_loss
from oracle.roi_align_ref import OracleMultiScaleRoIAlign
from test_gpu_box_branch import DEV, IMAGE, make as make_box, pyramid, to_dev

pytestmark = pytest.mark.gpu
SHAPES = [IMAGE, IMAGE]
BATCH = 32
NAMES = ['0', '1', '2', '3']


def make_heads(precision, **kw):
    """RoIHeads with the weights of the two restated branches."""
    from sfvos_amd import RoIHeads
    _, o_box = make_box('fp32')
    torch.manual_seed(6)
    o_mask = OracleMaskBranch(256, 2)
    heads = RoIHeads(2, precision, box_batch_size_per_image=BATCH, **kw)
    sd = dict(o_box.state_dict())
    sd.update(o_mask.state_dict())
    heads.load_state_dict(sd, strict=True)
    return heads.to(DEV), o_box, o_mask


def scene():
    """-> (proposals, targets, keys) on the cpu.  Image 0: three objects, 64 proposals around them and elsewhere; image 1:
    no ground truth, 37 proposals.  Corners on the quarter-pixel grid and every side a multiple of 14 pixels, inside the
    image: at every level (scales 1/4 ... 1/32) the bins of both RoIAligns (7 x 7 and 14 x 14, sampling ratio 2) and all
    their sample coordinates are dyadic, so the module's RoIAlign and the restatement's compute the SAME interpolation
    weights whether or not the device compiler fuses a multiply-add in the coordinates, and the RoI features of the two
    sides differ by summation order only (RoIAlign on arbitrary boxes has its own file, tests/test_gpu_roi_align.py)."""
    H, W = IMAGE
    g = torch.Generator().manual_seed(12)

    def place(xy, wh):     # inside the image, the size kept
        xy = torch.minimum(xy.clamp(min=0), torch.tensor([float(W), float(H)]) - wh)
        return torch.cat([xy, xy + wh], 1)

    gt_xy = torch.tensor([[20.0, 30.5], [150.0, 10.0], [200.5, 100.25]])
    gt_wh = torch.tensor([[84.0, 56.0], [154.0, 168.0], [28.0, 42.0]])
    gt = place(gt_xy, gt_wh)
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing='ij')
    masks = torch.stack([(((xx - (b[0] + b[2]) / 2) / ((b[2] - b[0]) / 2)) ** 2 +
                          ((yy - (b[1] + b[3]) / 2) / ((b[3] - b[1]) / 2)) ** 2) < 1 for b in gt]).to(torch.uint8)
    which = torch.randint(0, 3, (64,), generator=g)
    near_wh = (gt_wh[which] + 14.0 * torch.randint(-1, 2, (64, 2), generator=g)).clamp(min=14.0)
    near_xy = gt_xy[which] + torch.randint(-48, 49, (64, 2), generator=g).float() / 4
    far_wh = 14.0 * torch.randint(1, 8, (64, 2), generator=g).float()
    far_xy = torch.round(torch.rand(64, 2, generator=g) * (torch.tensor([float(W), float(H)]) - far_wh) * 4) / 4
    near, far = place(near_xy, near_wh), place(far_xy, far_wh)
    p0 = torch.where((torch.arange(64) % 2 == 1)[:, None], far, near)
    p1 = far[:37].clone()
    targets = [{'boxes': gt, 'labels': torch.ones(3, dtype=torch.int64), 'masks': masks},
               {'boxes': torch.zeros(0, 4), 'labels': torch.zeros(0, dtype=torch.int64),
                'masks': torch.zeros((0, H, W), dtype=torch.uint8)}]
    keys = [torch.rand(67, generator=g), torch.rand(37, generator=g)]
    return [p0, p1], targets, keys


def dev_targets(targets):
    return [{k: v.to(DEV) for k, v in t.items()} for t in targets]


def reference_samples(props, targets, keys):
    return [T.select_training_samples(p, t['boxes'], t['labels'], k, BATCH, 0.25) for p, t, k in zip(props, targets, keys)]


def reference_step(o_box, o_mask, x, sel, targets):
    """-> (losses, roi7, roi14) of the chain of restatements on the fused maps x."""
    boxes = [s['boxes'] for s in sel]
    roi7 = OracleMultiScaleRoIAlign(NAMES, 7, 2)(x, boxes, SHAPES)
    logits, deltas = o_box(roi7)
    lc, lb = R.fastrcnn_loss(logits, deltas, [s['labels'] for s in sel], [s['regression_targets'].float() for s in sel])
    mboxes = [s['boxes'][s['pos_slot']] for s in sel]
    mlabels = torch.cat([s['labels'][s['pos_slot']] for s in sel])
    roi14 = OracleMultiScaleRoIAlign(NAMES, 14, 2)(x, mboxes, SHAPES)
    mt = torch.cat([T.project_masks_on_boxes(t['masks'], b, s['matched'][s['pos_slot']], 28)
                    for t, b, s in zip(targets, mboxes, sel)]).float()
    lm = ref_mask_loss(o_mask(roi14), mlabels, mt)
    return {'loss_classifier': lc, 'loss_box_reg': lb, 'loss_mask': lm}, roi7, roi14


def relu_mask_flips(heads, o_box, o_mask, x, sel, roi7, roi14):
    """Elements whose ReLU mask differs between the module's activations on ITS OWN RoI features and the restatements' on
    theirs (the two RoIAligns agree to 1e-6, which is enough to move a pre-activation across zero): fc6, fc7, the four
    mask convs and conv5_mask."""
    with torch.no_grad():
        xd = to_dev(x)
        g7 = heads.box_roi_pool(xd, [s['boxes'].to(DEV) for s in sel], SHAPES)
        g14 = heads.mask_roi_pool(xd, [s['boxes'][s['pos_slot']].to(DEV) for s in sel], SHAPES)
        _, h6, h7 = heads.box_head.forward_rows(g7)
        r6 = torch.relu(o_box.box_head.fc6(roi7.flatten(1)))
        r7 = torch.relu(o_box.box_head.fc7(r6))
        n = int(((h6.float().cpu() > 0) != (r6 > 0)).sum()) + int(((h7.float().cpu() > 0) != (r7 > 0)).sum())
        acts = heads.mask_head.forward_nhwc(g14, keep=True)
        y5 = heads.mask_predictor._deconv_nhwc(acts[-1])
        h = roi14
        for i in range(1, 5):
            h = torch.relu(getattr(o_mask.mask_head, 'mask_fcn%d' % i)(h))
            n += int(((acts[i].float().permute(0, 3, 1, 2).cpu() > 0) != (h > 0)).sum())
        r5 = torch.relu(o_mask.mask_predictor.conv5_mask(h))
        n += int(((y5.float().permute(0, 3, 1, 2).cpu() > 0) != (r5 > 0)).sum())
    return n


def test_targets_equal_the_restatement():
    from sfvos_amd import project_masks_on_boxes, select_training_samples
    props, targets, keys = scene()
    sel = reference_samples(props, targets, keys)
    assert [s['index'].numel() for s in sel] == [BATCH, BATCH] and [s['pos_slot'].numel() for s in sel] == [8, 0]
    assert int((T.match(props[0], targets[0]['boxes'], targets[0]['labels'])['labels'] > 0).sum()) > 8 + 3
    pd, kd, td = [p.to(DEV) for p in props], [k.to(DEV) for k in keys], dev_targets(targets)
    got = select_training_samples(pd, td, kd, batch_size_per_image=BATCH)
    again = select_training_samples(pd, td, kd, batch_size_per_image=BATCH)
    for b, s in enumerate(sel):
        boxes, matched, labels, reg = (v[b].cpu() for v in got)
        assert matched.dtype == torch.int64 and labels.dtype == torch.int64
        assert torch.equal(boxes, s['boxes']) and torch.equal(matched, s['matched']) and torch.equal(labels, s['labels'])
        want = s['regression_targets']
        inf = torch.isinf(want)
        assert torch.equal(torch.isinf(reg), inf) and torch.equal(reg[inf].double(), want[inf])
        assert bool(inf.any()) == (b == 1)      # no ground truth: torchvision encodes a box of zeros
        p = s['boxes'].double()
        r = (targets[b]['boxes'] if b == 0 else torch.zeros(1, 4))[s['matched']].double()
        pw, ph = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
        gcx, gcy = (r[:, 0] + r[:, 2]).abs() / 2, (r[:, 1] + r[:, 3]).abs() / 2
        pcx, pcy = (p[:, 0] + p[:, 2]).abs() / 2, (p[:, 1] + p[:, 3]).abs() / 2
        fin = torch.where(inf, torch.zeros_like(want), want)
        allow = TRANS * torch.stack([10 * (gcx + pcx) / pw, 10 * (gcy + pcy) / ph, 5 * (fin[:, 2].abs() / 5 + 1),
                                     5 * (fin[:, 3].abs() / 5 + 1)], 1)
        check_abs('regression_targets image %d' % b, torch.where(inf, torch.zeros_like(reg), reg), fin, allow)
        for a, c in zip(got, again):
            assert torch.equal(a[b], c[b])
    # keys drawn on the device: the same generator state gives the same sample, S and P as the quota says
    gen = torch.Generator(device=DEV).manual_seed(5)
    one = select_training_samples(pd, td, generator=gen, batch_size_per_image=BATCH)
    gen.manual_seed(5)
    two = select_training_samples(pd, td, generator=gen, batch_size_per_image=BATCH)
    assert all(torch.equal(a, c) for x, y in zip(one, two) for a, c in zip(x, y))
    assert [int((l > 0).sum()) for l in one[2]] == [8, 0] and [l.numel() for l in one[2]] == [BATCH, BATCH]
    # mask targets of the positives of image 0, uint8 / bool / fp32 / fp64 masks
    s = sel[0]
    mb, mi = s['boxes'][s['pos_slot']], s['matched'][s['pos_slot']]
    ref, grids = T.roi_align_adaptive(targets[0]['masks'], mb, mi, 28)
    K = (4 * grids[:, 0] * grids[:, 1]).double()[:, None, None]
    m8 = targets[0]['masks'].to(DEV)
    got_t = project_masks_on_boxes(m8, mb.to(DEV), mi.to(DEV), 28)
    assert tuple(got_t.shape) == (8, 28, 28) and got_t.dtype == torch.float32 and float(ref.max()) > 0.9
    check_abs('project_masks_on_boxes', got_t.cpu(), ref, 2.0 * (K + 1) * U22 * ref)
    for other in (m8.bool(), m8.float(), m8.double()):
        assert torch.equal(project_masks_on_boxes(other, mb.to(DEV), mi.to(DEV), 28), got_t)
    assert project_masks_on_boxes(m8, mb[:0].to(DEV), mi[:0].to(DEV), 28).shape == (0, 28, 28)


def test_roi_heads_training_step_matches_the_restatements():
    from sfvos_amd import FusedSGD
    heads, o_box, o_mask = make_heads('fp32')
    assert heads.training
    props, targets, keys = scene()
    sel = reference_samples(props, targets, keys)
    for seed in range(21, 29):
        x = pyramid(2, torch.Generator().manual_seed(seed))
        with torch.no_grad():
            _, roi7, roi14 = reference_step(o_box, o_mask, x, sel, targets)
        if relu_mask_flips(heads, o_box, o_mask, x, sel, roi7, roi14) == 0:
            break
    else:
        pytest.fail('no input without ReLU-mask flips in 8 seeds')
    xr = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in x.items())
    ref, _, _ = reference_step(o_box, o_mask, xr, sel, targets)
    sum(ref.values()).backward()
    xg = to_dev(x, grad=True)
    pd, kd, td = [p.to(DEV) for p in props], [k.to(DEV) for k in keys], dev_targets(targets)
    with pytest.raises(ValueError, match='should not be None'):
        heads(xg, pd, SHAPES)
    dets, losses = heads(xg, pd, SHAPES, td, kd)
    assert dets == [] and sorted(losses) == ['loss_box_reg', 'loss_classifier', 'loss_mask']
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    pairs = [(k, losses[k].detach().cpu(), ref[k].detach()) for k in sorted(losses)]
    ref_p = dict(list(o_box.named_parameters()) + list(o_mask.named_parameters()))
    for name, p in heads.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) > 0, name
        pairs.append((name, p.grad.cpu(), ref_p[name].grad))
    assert len(pairs) == 3 + 20
    n_maps = 0
    for k in NAMES:
        if xr[k].grad is None:     # no sampled box is large enough for this level: zeros here, no gradient there
            assert float(xg[k].grad.abs().max()) == 0.0
            continue
        n_maps += 1
        pairs.append(('fused map ' + k, xg[k].grad.cpu(), xr[k].grad))
    assert n_maps >= 2 and xg['pool'].grad is None
    print('roi_heads training fp32 (seed %d): %s' % (seed, ', '.join('%s %.6f (restatement %.6f)' % (
        k, float(losses[k]), float(ref[k])) for k in sorted(losses))))
    failed = []
    for name, got, want in pairs:
        e, gate = relmax(got, want), (1e-5 if name.startswith('loss') else 5e-5)
        print('   %-40s measured %.3e / gate %.3e' % (name, e, gate))
        if not e <= gate:
            failed.append((name, e, gate))
    assert not failed, failed
    # one optimiser step moves all 20 parameters
    before = {n: p.detach().clone() for n, p in heads.named_parameters()}
    grads = {n: p.grad.clone() for n, p in heads.named_parameters()}
    opt = FusedSGD(heads.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
    for n, p in heads.named_parameters():
        p.grad.copy_(grads[n])
    opt.step()
    torch.cuda.synchronize()
    after = dict(heads.named_parameters())
    assert len(after) == 20
    for n, b in before.items():
        assert not torch.equal(after[n].detach(), b), n
    _, losses2 = heads(to_dev(x), pd, SHAPES, td, kd)
    assert all(bool(torch.isfinite(v)) for v in losses2.values())
    assert float(sum(losses2.values())) != float(sum(losses.values()))


def test_roi_heads_bf16_losses_and_images_without_positives():
    heads, o_box, o_mask = make_heads('bf16')
    props, targets, keys = scene()
    sel = reference_samples(props, targets, keys)
    x = OrderedDict((k, v.bfloat16().float()) for k, v in pyramid(2, torch.Generator().manual_seed(21)).items())
    with torch.no_grad():
        ref, _, _ = reference_step(o_box, o_mask, x, sel, targets)
    pd, kd, td = [p.to(DEV) for p in props], [k.to(DEV) for k in keys], dev_targets(targets)
    _, losses = heads(to_dev(x, grad=True), pd, SHAPES, td, kd)
    for k in sorted(losses):
        got, want = float(losses[k]), float(ref[k])
        print('roi_heads bf16 %-16s %.6f (restatement %.6f): %.2e / gate 2e-2' % (k, got, want, abs(got - want) / abs(want)))
        assert got == got and abs(got) != float('inf') and abs(got - want) <= 2e-2 * abs(want), k
    # only the image without ground truth: no positive, the mask loss is a zero that stays on the graph
    heads32, _, _ = make_heads('fp32')
    for grad in (True, False):
        _, losses = heads32(to_dev(x, grad=grad), pd[1:], SHAPES[:1], td[1:], kd[1:])
        assert float(losses['loss_mask']) == 0.0 and losses['loss_mask'].requires_grad
        assert float(losses['loss_box_reg']) == 0.0 and float(losses['loss_classifier']) > 0
        for p in heads32.parameters():
            p.grad = None
        losses['loss_mask'].backward()
        assert float(heads32.mask_head.mask_fcn1.weight.grad.abs().max()) == 0.0


def test_roi_heads_evaluation_equals_roi_heads_inference():
    from sfvos_amd import RoIHeadsInference
    heads, o_box, o_mask = make_heads('fp32', box_detections_per_img=10)
    inf = RoIHeadsInference(2, 'fp32', box_detections_per_img=10)
    inf.box.load_state_dict(o_box.state_dict(), strict=True)
    inf.mask.load_state_dict(o_mask.state_dict(), strict=True)
    inf = inf.to(DEV)
    heads.eval()
    props, _, _ = scene()
    pd = [p.to(DEV) for p in props]
    x = to_dev(pyramid(2, torch.Generator().manual_seed(3)))
    for per_img in (10, 3):
        heads.detections_per_img = per_img          # set after construction, as model.py:187 does
        inf.box.detections_per_img = per_img
        dets, losses = heads(x, pd, SHAPES)
        want = inf(x, pd, SHAPES)
        assert losses == {} and len(dets) == 2
        for d, w in zip(dets, want):
            assert sorted(d) == sorted(w) and d['boxes'].shape[0] == w['boxes'].shape[0] <= per_img
            for k in w:
                assert torch.equal(d[k], w[k]), k
            assert tuple(d['masks'].shape) == (d['boxes'].shape[0], 1) + IMAGE
        if per_img == 3:
            assert max(d['boxes'].shape[0] for d in dets) == 3, 'the cap must be reached for the test to show it'
