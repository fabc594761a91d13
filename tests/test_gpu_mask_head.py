"""GPU: the mask branch behind RoIAlign (MaskRCNNHeads + MaskRCNNPredictor + maskrcnn_inference +
paste_masks_in_image, reference code/helpers/model.py:17-25,346-347) on libsfvos kernels against the torch-core
restatement in oracle/mask_head_ref.py.

PARITY UNPINNED BY THE REFERENCE: the arithmetic is torchvision's (third-party, not vendored, not installed here) and no
reference fixture covers it; the oracle restates torchvision's published modules.  Tolerances: fp32 1e-4 of the tensor
scale (exact-f32 MFMA, summation order only), bf16 2e-2; pasted probabilities 1e-5 absolute; the >= 0.5 union
(davis_evaluate.py:40-42) identical wherever the oracle's probability is not within 1e-5 of 0.5."""
import numpy as np
import pytest
import torch

from kernel_util import rel_l2, relmax
from oracle.mask_head_ref import OracleMaskBranch
from oracle.mask_head_ref import maskrcnn_inference as ref_inference
from oracle.mask_head_ref import maskrcnn_loss as ref_loss
from oracle.mask_head_ref import paste_masks_in_image as ref_paste

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def make(precision):
    from sfvos_amd import MaskBranch
    torch.manual_seed(5)
    o = OracleMaskBranch(256, 2)
    with torch.no_grad():
        for p in o.parameters():   # non-zero biases, so that they are exercised
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape) * 0.1)
    m = MaskBranch(256, 2, precision)
    m.load_state_dict(o.state_dict(), strict=True)
    return m.to(DEV), o


BOXES = torch.tensor([[10.3, 20.7, 110.2, 90.5],      # ordinary
                      [-15.0, -8.0, 40.0, 30.0],      # sticks out at the top left
                      [800.0, 400.0, 870.0, 500.0],   # sticks out at the bottom right
                      [200.0, 100.0, 201.0, 101.5],   # tiny
                      [300.5, 50.2, 300.5, 50.2],     # degenerate (zero area)
                      [0.0, 0.0, 853.0, 479.0],       # the whole image
                      [420.9, 250.1, 470.3, 470.8]])  # tall


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_mask_branch_logits_match_the_oracle(precision):
    m, o = make(precision)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(7, 256, 14, 14, generator=g).relu()      # RoIAlign output of post-ReLU-ish features
    if precision == 'bf16':
        x = x.bfloat16().float()
    with torch.no_grad():
        ref = o(x)
        got = m(x.to(DEV))
        h_ref = o.mask_head(x)
        h_got = m.mask_head(x.to(DEV))
    assert tuple(got.shape) == (7, 2, 28, 28) and got.dtype == torch.float32
    tol = 1e-4 if precision == 'fp32' else 2e-2
    e_h, e_l = relmax(h_got.cpu(), h_ref), relmax(got.cpu(), ref)
    print('mask branch %s: heads max err / scale %.2e, logits %.2e' % (precision, e_h, e_l))
    assert e_h < tol and e_l < tol
    # the predictor alone, through its NCHW entry point
    with torch.no_grad():
        p_ref = o.mask_predictor(h_ref)
        p_got = m.mask_predictor(h_ref.to(DEV))
    assert relmax(p_got.cpu(), p_ref) < tol


def test_inference_and_paste_match_the_oracle():
    from sfvos_amd import maskrcnn_inference, paste_masks_in_image, union_mask
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(7, 2, 28, 28, generator=g) * 3
    labels = torch.tensor([1, 1, 0, 1, 1, 1, 0])
    ref_p = ref_inference(logits, labels)
    got_p = maskrcnn_inference(logits.to(DEV), labels.to(DEV))
    assert tuple(got_p.shape) == (7, 1, 28, 28)
    assert float((got_p.cpu() - ref_p).abs().max()) < 1e-6
    H, W = 480, 854
    ref = ref_paste(ref_p, BOXES, (H, W))
    got = paste_masks_in_image(ref_p.to(DEV), BOXES.to(DEV), (H, W))
    assert tuple(got.shape) == (7, 1, H, W)
    err = (got.cpu() - ref).abs()
    for i in range(7):
        print('paste box %d: max abs err %.2e, pasted pixels %d' % (i, float(err[i].max()), int((ref[i] != 0).sum())))
    assert float(err.max()) < 1e-5
    # the evaluation-side reducer on top (davis_evaluate.py:40-42): OR_k (mask_k >= 0.5)
    total = np.zeros((H, W), dtype=bool)
    for mk in ref:
        total = np.logical_or(total, (mk.numpy() >= 0.5)[0])
    uni = union_mask(got).cpu().numpy()
    near = ((ref - 0.5).abs() < 1e-5).any(0)[0].numpy()
    assert np.array_equal(uni[~near], total[~near])
    assert paste_masks_in_image(ref_p[:0].to(DEV), BOXES[:0].to(DEV), (H, W)).shape == (0, 1, H, W)


def test_predict_end_to_end_matches_the_oracle():
    m, o = make('fp32')
    g = torch.Generator().manual_seed(21)
    x = torch.randn(7, 256, 14, 14, generator=g).relu()
    labels = torch.tensor([1, 1, 1, 1, 1, 1, 1])      # the reference has one foreground class (num_classes = 2)
    H, W = 480, 854
    with torch.no_grad():
        ref = ref_paste(ref_inference(o(x), labels), BOXES, (H, W))
    got = m.predict(x.to(DEV), labels.to(DEV), BOXES.to(DEV), (H, W))
    assert float((got.cpu() - ref).abs().max()) < 1e-4


def test_mask_head_refuses_cpu():
    from sfvos_amd import MaskBranch, paste_masks_in_image
    m = MaskBranch()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m(torch.zeros(1, 256, 14, 14))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        paste_masks_in_image(torch.zeros(1, 1, 28, 28), torch.zeros(1, 4), (8, 8))


def _relu_mask_mismatches(m, o, x):
    """Elements whose ReLU mask differs between the GPU activations and the oracle's (a pre-activation within fp32
    rounding of zero): one such element changes the gradients behind it by O(1e-3) -- a property of comparing two
    correct implementations, not an error ('ReLU masks')."""
    with torch.no_grad():
        acts = m.mask_head.forward_nhwc(x.to(DEV), keep=True)
        y5 = m.mask_predictor._deconv_nhwc(acts[-1])
        n, h = 0, x
        for i in range(1, 5):
            h = torch.relu(getattr(o.mask_head, 'mask_fcn%d' % i)(h))
            n += int(((acts[i].float().permute(0, 3, 1, 2).cpu() > 0) != (h > 0)).sum())
        r5 = torch.relu(o.mask_predictor.conv5_mask(h))
        n += int(((y5.float().permute(0, 3, 1, 2).cpu() > 0) != (r5 > 0)).sum())
    return n


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_mask_branch_training_step_matches_the_oracle(precision):
    """maskrcnn_loss + backward through the whole branch (the reference trains roi_heads, model.py:176-179,369):
    loss, gradient w.r.t. the RoI features and all 12 parameter gradients against torch autograd on the restatement.
    fp32: 5e-5 of each tensor's scale on an input without ReLU-mask flips (exact-f32 MFMA: summation order only);
    bf16: activations and the gradients between layers are bf16, and bf16 rounding flips ReLU masks of near-zero
    pre-activations in each of the five ReLU layers the gradient crosses -> rel-L2 bounds (parameters 0.1, the input
    gradient behind all five 0.2), measured and printed."""
    from sfvos_amd import maskrcnn_loss
    m, o = make(precision)
    N = 9
    labels = torch.tensor([1, 0, 1, 1, 0, 1, 1, 1, 0])
    for seed in range(21, 29):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(N, 256, 14, 14, generator=g).relu()
        targets = (torch.rand(N, 28, 28, generator=g) > 0.5).float()
        if precision == 'bf16':
            x = x.bfloat16().float()
            break
        if _relu_mask_mismatches(m, o, x) == 0:
            break
    else:
        pytest.fail('no input without ReLU-mask flips in 8 seeds')
    xr = x.clone().requires_grad_(True)
    loss_ref = ref_loss(o(xr), labels, targets)
    loss_ref.backward()
    xg = x.to(DEV).requires_grad_(True)
    logits = m(xg)
    assert logits.requires_grad and tuple(logits.shape) == (N, 2, 28, 28)
    loss = maskrcnn_loss(logits, labels.to(DEV), targets.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    tol_l = 1e-5 if precision == 'fp32' else 2e-2
    lv, lr = float(loss.detach()), float(loss_ref.detach())
    assert abs(lv - lr) <= tol_l * abs(lr), (lv, lr)

    worst = 0.0
    names = dict(o.named_parameters())
    for name, p in m.named_parameters():
        assert p.grad is not None, name
        ref = names[name].grad
        if precision == 'fp32':
            e = relmax(p.grad.cpu(), ref)
            assert e < 5e-5, (name, e)
        else:
            e = rel_l2(p.grad.cpu(), ref)
            assert e < 0.1, (name, e)
        worst = max(worst, e)
    if precision == 'fp32':
        ex = relmax(xg.grad.cpu(), xr.grad)
        assert ex < 5e-5, ex
    else:
        ex = rel_l2(xg.grad.cpu(), xr.grad)
        assert ex < 0.2, ex
    print('mask branch training %s (seed %d): loss %.6f (ref %.6f), worst parameter-gradient error %.2e, input '
          'gradient %.2e' % (precision, seed, lv, lr, worst, ex))
    # frozen parameters get no gradient, and the inference path is unchanged under no_grad
    for p in m.parameters():
        p.grad = None
    m.mask_head.mask_fcn1.weight.requires_grad_(False)
    maskrcnn_loss(m(x.to(DEV)), labels.to(DEV), targets.to(DEV)).backward()
    assert m.mask_head.mask_fcn1.weight.grad is None and m.mask_head.mask_fcn2.weight.grad is not None
    with torch.no_grad():
        assert not m(x.to(DEV)).requires_grad


def test_maskrcnn_loss_alone_and_without_rois():
    from sfvos_amd import maskrcnn_loss
    g = torch.Generator().manual_seed(4)
    logits = (torch.randn(5, 3, 28, 28, generator=g) * 4).requires_grad_(True)
    labels = torch.tensor([2, 0, 1, 1, 2])
    targets = (torch.rand(5, 28, 28, generator=g) > 0.3).float()
    ref = ref_loss(logits, labels, targets)
    ref.backward()
    lg = logits.detach().to(DEV).requires_grad_(True)
    got = maskrcnn_loss(lg, labels.to(DEV), targets.to(DEV))
    (got * 3.0).backward()
    assert abs(float(got.detach()) - float(ref.detach())) < 1e-6 * abs(float(ref.detach())) + 1e-7
    assert float((lg.grad.cpu() / 3.0 - logits.grad).abs().max()) < 1e-8 + 1e-5 * float(logits.grad.abs().max())
    empty = torch.zeros(0, 3, 28, 28, device=DEV, requires_grad=True)
    z = maskrcnn_loss(empty, torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(0, 28, 28, device=DEV))
    assert float(z.detach()) == 0.0


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_mask_branch_fused_sgd_trajectory_matches_the_oracle(precision):
    """the reference trains roi_heads under the same SGD as everything else (train.py:80,
    model.py:176-179).  FusedSGD rewrites the parameters through raw pointers, so the branch's packed weight images
    (3x3 fwd / dgrad, deconv fwd / dgrad) must follow _lib.weight_epoch(): four optimiser steps of MaskBranch under
    the package's FusedSGD against the oracle under torch.optim.SGD -- losses of every step (a stale image shows from
    step 2 on), logits after the last step, and the parameters themselves.  lr is raised to 0.02 so that one step
    moves the loss far beyond the tolerance (a stale image leaves the step-2 loss at its step-1 value); the trajectory
    itself amplifies the ReLU-mask flips of two correct implementations, hence 1e-2 on later losses in fp32."""
    from sfvos_amd import FusedSGD, maskrcnn_loss
    m, o = make(precision)
    N = 6
    labels = torch.tensor([1, 0, 1, 1, 0, 1])
    g = torch.Generator().manual_seed(77)
    x = torch.randn(N, 256, 14, 14, generator=g).relu()
    targets = (torch.rand(N, 28, 28, generator=g) > 0.5).float()
    if precision == 'bf16':
        x = x.bfloat16().float()
    opt = FusedSGD(m.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
    ropt = torch.optim.SGD(o.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
    xg = x.to(DEV)
    losses, rlosses = [], []
    for step in range(4):
        opt.zero_grad()
        loss = maskrcnn_loss(m(xg), labels.to(DEV), targets.to(DEV))
        loss.backward()
        opt.step()
        ropt.zero_grad()
        rl = ref_loss(o(x), labels, targets)
        rl.backward()
        ropt.step()
        losses.append(float(loss.detach()))
        rlosses.append(float(rl.detach()))
    with torch.no_grad():
        got, ref = m(xg).cpu(), o(x)
    tol_l, tol_o = (1e-2, 5e-2) if precision == 'fp32' else (5e-2, 0.15)
    print('mask branch %s FusedSGD trajectory: losses %s vs oracle %s; logits after 4 steps %.2e'
          % (precision, ['%.5f' % v for v in losses], ['%.5f' % v for v in rlosses], relmax(got, ref)))
    assert min(abs(a - b) for a, b in zip(rlosses, rlosses[1:])) > 0.1 * abs(rlosses[0]), 'every step must move the loss'
    for a, b in zip(losses, rlosses):
        assert abs(a - b) <= tol_l * abs(b), (losses, rlosses)
    assert relmax(got, ref) < tol_o
    names = dict(o.named_parameters())
    for name, p in m.named_parameters():
        a, b = p.detach().cpu().double().flatten(), names[name].detach().double().flatten()
        assert float((a - b).norm() / b.norm()) < tol_o, name


def test_mask_branch_without_rois_and_with_bad_labels():
    """forward() with zero RoIs returns an empty [0,K,28,28] that stays on the graph (torchvision's
    heads do); a label outside [0, num_classes) never becomes an out-of-bounds read -- probabilities and the loss are
    NaN (torch raises an index error there), its gradient is zero."""
    from sfvos_amd import maskrcnn_loss
    m, _ = make('fp32')
    x0 = torch.zeros(0, 256, 14, 14, device=DEV, requires_grad=True)
    out = m(x0)
    assert tuple(out.shape) == (0, 2, 28, 28) and out.requires_grad
    maskrcnn_loss(out, torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(0, 28, 28, device=DEV)).backward()
    assert x0.grad is not None and x0.grad.shape == x0.shape
    with torch.no_grad():
        assert tuple(m(x0.detach()).shape) == (0, 2, 28, 28)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 256, 14, 14, generator=g).relu().to(DEV)
    bad = torch.tensor([1, 7, -1], device=DEV)
    with torch.no_grad():
        _, prob = m.mask_predictor.forward_from_nhwc(m.mask_head.forward_nhwc(x), bad, want_logits=False, want_prob=True)
    assert torch.isfinite(prob[0]).all() and torch.isnan(prob[1]).all() and torch.isnan(prob[2]).all()
    logits = m(x).detach().requires_grad_(True)
    loss = maskrcnn_loss(logits, bad, torch.zeros(3, 28, 28, device=DEV))
    assert torch.isnan(loss)
    loss.backward()
    assert float(logits.grad[1:].abs().max()) == 0.0


def test_mask_branch_loads_a_reference_checkpoint_slice_strictly():
    """ADVICE r2 (low) / INTEGRATION.md 2b: the `roi_heads.mask_head.*` / `roi_heads.mask_predictor.*` slice of a
    reference-format checkpoint (torchvision's key names and shapes: model.py:17-25, train.py:115-117), saved with
    torch.save and read back with weights_only=True, loads with strict=True, and the branch's own state_dict goes
    the other way.  Parity unpinned (torchvision absent): names and shapes are torchvision's published ones."""
    import io
    from sfvos_amd import MaskBranch
    want = {'mask_head.mask_fcn%d.%s' % (i, k): s for i in range(1, 5)
            for k, s in (('weight', (256, 256, 3, 3)), ('bias', (256,)))}
    want.update({'mask_predictor.conv5_mask.weight': (256, 256, 2, 2), 'mask_predictor.conv5_mask.bias': (256,),
                 'mask_predictor.mask_fcn_logits.weight': (2, 256, 1, 1), 'mask_predictor.mask_fcn_logits.bias': (2,)})
    g = torch.Generator().manual_seed(1)
    ckpt = {'slow_fast.bn_f1.weight': torch.ones(32)}    # other keys of a SegmentationModel checkpoint are skipped
    ckpt.update({'maskrcnn_model.roi_heads.' + k: torch.randn(s, generator=g) for k, s in want.items()})
    buf = io.BytesIO()
    torch.save(ckpt, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=True)
    prefix = 'maskrcnn_model.roi_heads.'
    sl = {k[len(prefix):]: v for k, v in loaded.items() if k.startswith(prefix)}
    m = MaskBranch(256, 2, 'fp32')
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    m.load_state_dict(sl, strict=True)
    o = OracleMaskBranch(256, 2)
    o.load_state_dict(m.state_dict(), strict=True)
    x = torch.randn(2, 256, 14, 14, generator=g).relu()
    with torch.no_grad():
        assert relmax(m.to(DEV)(x.to(DEV)).cpu(), o(x)) < 1e-4
