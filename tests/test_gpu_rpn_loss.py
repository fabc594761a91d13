"""GPU: the training call of sfvos_amd.RegionProposalNetwork against the torch-core restatement tests/rpn_loss_ref.py, on
rpn_ref.module_case (pyramid (24,40), (12,20), (6,10), (3,5) of a 96 x 160 batch tensor, B = 2), fp32 and bf16.

The restatement runs on the module's OWN objectness and deltas (the head has its own tests), with the same explicit keys:
the same anchors are sampled (the ground truth sits on quarter pixels, so the matcher is exact) and both losses agree within
the mean of the per-term bounds of tests/test_gpu_rpn_loss_kernels.py plus one fp32 rounding.  A box term also carries the
allowance of its regression target (the kernel encodes it in fp32; smooth-L1 has slope <= 1 in the target): TRANS times
the magnitudes of the encoder's terms, as the sampler's test allows.  PARITY UNPINNED BY THE REFERENCE."""
import types

import pytest
import torch

import rpn_loss_ref as T
import rpn_ref as R
from kernel_util import FLT_MIN, TRANS, U22
from test_gpu_rpn import make_rpn

pytestmark = pytest.mark.gpu

GT = [torch.tensor(T.CASE_A), torch.tensor([[20.25, 10.5, 140.75, 90.25], [60.5, 30.25, 75.75, 44.5]])]


def frozen_rpn(seed, precision):
    rpn, feats_d, _, _ = make_rpn(seed, precision)
    for p in rpn.parameters():
        p.requires_grad_(False)
    return rpn.train(), feats_d


def images():
    return types.SimpleNamespace(tensors=torch.zeros(2, 3, *R.TENSOR, device='cuda'), image_sizes=list(R.IMAGES))


def make_keys(seed, N=3825, B=2):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(N, generator=g) for _ in range(B)]


def check_losses(tag, losses, rpn, obj, dl, shapes, gts, keys, beta=1.0 / 9):
    anc = T.anchors(R.SHAPES, R.TENSOR)
    lg, dd = T.per_image(obj.cpu(), dl.cpu(), shapes, len(gts))
    want = T.rpn_losses(lg, dd, anc, gts, [k.cpu() for k in keys], rpn.batch_size_per_image, rpn.positive_fraction,
                        float(torch.tensor(beta, dtype=torch.float32)))
    counts, index = (t.cpu() for t in rpn.last_sample)
    assert counts.tolist() == [list(c) for c in want['counts']], (tag, counts.tolist(), want['counts'])
    for b, idx in enumerate(want['index']):
        assert torch.equal(index[b, :idx.numel()].long(), idx) and bool((index[b, idx.numel():] == -1).all()), tag
    s_tot = want['s_tot']
    bounds = {'loss_objectness': float((((2.0 * 3 * U22 + TRANS) * want['bce_mag']) + FLT_MIN).sum()) / s_tot,
              'loss_rpn_box_reg': (float((2.0 * 9 * U22 * want['box_mag']).sum())
                                   + TRANS * float(want['target_allow'].sum())) / s_tot}
    for name, bound in bounds.items():
        v = losses[name]
        assert v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda and not v.requires_grad
        err, bound = abs(float(v) - want[name]), bound + 2.0 ** -24 * abs(want[name])
        print('%-46s error/bound %.4f (value %.6f)' % (tag + name, err / bound if bound else 0.0, want[name]))
        assert err <= bound, (tag, name, float(v), want[name], bound)
    return want


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_forward_in_training_returns_both_losses_and_the_same_proposals(precision):
    rpn, feats_d = frozen_rpn(R.SEEDS[0], precision)
    keys = [k.cuda() for k in make_keys(3)]
    targets = [dict(boxes=g.cuda()) for g in GT]
    plain, none = rpn(images(), feats_d)
    assert none == {}                                           # training without targets: as before
    proposals, losses = rpn(images(), feats_d, targets, keys)
    assert sorted(losses) == ['loss_objectness', 'loss_rpn_box_reg']
    assert len(proposals) == len(plain) == 2 and all(torch.equal(a, b) for a, b in zip(proposals, plain))
    obj, dl, shapes, B = rpn.head_outputs(feats_d)
    want = check_losses('rpn forward %s ' % precision, losses, rpn, obj, dl, shapes, GT, keys)
    assert want['counts'][0] == (256, 49) and want['counts'][1][0] == 256 and want['counts'][1][1] > 0
    # evaluation mode with targets: no losses, and the same call as without them
    rpn.eval()
    p_eval, l_eval = rpn(images(), feats_d, targets, keys)
    assert l_eval == {} and all(torch.equal(a, b) for a, b in zip(p_eval, rpn(images(), feats_d)[0]))


@pytest.mark.parametrize('beta', [0.0, 1.0 / 9])
def test_an_image_with_empty_boxes_and_both_betas(beta):
    rpn, feats_d = frozen_rpn(R.SEEDS[1], 'fp32')
    rpn.smooth_l1_beta = beta
    gts = [GT[1], torch.zeros((0, 4))]
    keys = [k.cuda() for k in make_keys(4)]
    obj, dl, shapes, B = rpn.head_outputs(feats_d)
    losses = rpn.compute_loss(obj, dl, shapes, B, R.TENSOR, [dict(boxes=g.cuda()) for g in gts], keys)
    want = check_losses('rpn empty boxes beta %.3g ' % beta, losses, rpn, obj, dl, shapes, gts, keys, beta)
    assert want['counts'][1] == (256, 0) and want['counts'][0][1] > 0
    # every image empty: only background is sampled, the box loss is exactly 0
    none = [dict(boxes=torch.zeros((0, 4), device='cuda'))] * 2
    losses = rpn.compute_loss(obj, dl, shapes, B, R.TENSOR, none, keys)
    check_losses('rpn no boxes at all ', losses, rpn, obj, dl, shapes, [torch.zeros((0, 4))] * 2, keys, beta)
    assert float(losses['loss_rpn_box_reg']) == 0.0


def test_anchor_targets_are_the_restatements():
    rpn, _ = frozen_rpn(R.SEEDS[2], 'fp32')
    anc = T.anchors(R.SHAPES, R.TENSOR)
    for gt in (GT[0], GT[1], torch.zeros((0, 4))):
        labels, matched = rpn.anchor_targets(R.SHAPES, R.TENSOR, gt.cuda())
        want = T.match(anc, gt)
        assert labels.dtype == torch.int32 and matched.dtype == torch.int32 and labels.is_cuda
        assert torch.equal(labels.cpu().long(), want['labels']) and torch.equal(matched.cpu().long(), want['matched'])


def test_keys_none_draws_them_and_gives_finite_losses():
    rpn, feats_d = frozen_rpn(R.SEEDS[3], 'fp32')
    targets = [dict(boxes=g.cuda()) for g in GT]
    anc = T.anchors(R.SHAPES, R.TENSOR)
    n_pos = [min(int((T.match(anc, g)['labels'] == 1).sum()), 128) for g in GT]
    torch.manual_seed(1)
    _, a = rpn(images(), feats_d, targets)
    counts = rpn.last_sample[0].cpu().tolist()
    index_a = rpn.last_sample[1].clone()
    assert counts == [[256, n_pos[0]], [256, n_pos[1]]]          # the counts do not depend on the keys
    _, b = rpn(images(), feats_d, targets)
    for losses in (a, b):
        assert all(bool(torch.isfinite(v)) and float(v) > 0 for v in losses.values())
    assert not torch.equal(index_a, rpn.last_sample[1])           # another draw, another sample


def test_compute_loss_is_capturable():
    rpn, feats_d = frozen_rpn(R.SEEDS[4], 'bf16')
    keys = [k.cuda() for k in make_keys(5)]
    targets = [dict(boxes=g.cuda()) for g in GT]
    obj, dl, shapes, B = rpn.head_outputs(feats_d)
    want = {k: v.clone() for k, v in rpn.compute_loss(obj, dl, shapes, B, R.TENSOR, targets, keys).items()}   # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):       # a single branch: every launch goes to the capture stream
        out = rpn.compute_loss(obj, dl, shapes, B, R.TENSOR, targets, keys)
    for v in out.values():
        v.fill_(-5)
    graph.replay()
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(out[k], want[k]) and bool(torch.isfinite(out[k])), k
