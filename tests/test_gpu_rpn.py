"""GPU: sfvos_amd.RegionProposalNetwork against the torch-core restatement tests/rpn_ref.py, on the pyramid (24,40),
(12,20), (6,10), (3,5) of a 96 x 160 batch tensor with images (90,150) and (96,160), B = 2, fp32 and bf16, training and
testing mode with the top-n lowered to 50 / 30 so that both limits bite.

Head, fp32: the conv against float64 under kernel_util's per-element criterion with K = 9 * 256 (one chain over taps and
channels, no split), the two 1x1 heads against float64 on the kernel's own hidden map with K = 256.  Head, bf16: no
derived bound exists at module level; relmax / rel-L2 against the float64 restatement on the bf16-rounded maps and conv
weights are gated at 2 x the values measured on an MI355X (BF16_MEASURED; this project's practice for bf16 gates).

Proposals: the restatement runs in float64 on the module's own fp32 objectness and deltas, on the 16 margin-safe seeds
(tests/test_rpn_ref_cpu.py asserts 16 of 16): same indices, same order, same counts; boxes and scores within the decode
allowance (rpn_ref.decode_allowance, kernel_util's transcendental allowance).  PARITY UNPINNED BY THE REFERENCE."""
import types
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

import rpn_ref as R
from kernel_util import TRANS, check, check_abs, rel_l2, relmax

pytestmark = pytest.mark.gpu

# (relmax, rel-L2) of the bf16 head against float64 on the bf16-rounded operands, measured on an MI355X (seed 0)
BF16_MEASURED = {'hidden': (2.28e-3, 1.66e-3), 'objectness': (2.06e-3, 1.89e-3), 'deltas': (1.79e-3, 1.71e-3)}


def make_rpn(seed, precision, dev='cuda'):
    from sfvos_amd import AnchorGenerator, RegionProposalNetwork, RPNHead
    feats, sd = R.module_case(seed)
    rpn = RegionProposalNetwork(AnchorGenerator(R.SIZES, R.RATIOS), RPNHead(256, 3, precision), R.PRE, R.POST,
                                precision=precision)
    rpn.head.load_state_dict(sd, strict=True)
    rpn.to(dev)
    return rpn, OrderedDict((k, v.to(dev)) for k, v in feats.items()), feats, sd


def per_level(obj, dl, shapes, B, A=3):
    """flat [P, A], [P, 4A] -> per-level [B, n_l] and [B, n_l, 4] (cpu)."""
    lg, dd, off = [], [], 0
    obj, dl = obj.cpu(), dl.cpu()
    for H, W in shapes:
        n = B * H * W
        lg.append(obj[off:off + n].reshape(B, H * W * A))
        dd.append(dl[off:off + n].reshape(B, H * W * A, 4))
        off += n
    return lg, dd


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_head_outputs_against_float64(precision):
    rpn, feats_d, feats, sd = make_rpn(R.SEEDS[0], precision)
    head = rpn.head
    maps = list(feats_d.values())
    shapes, B = [tuple(m.shape[2:]) for m in maps], 2
    with torch.no_grad():
        t = head.conv_pyramid(head.maps_to_pyramid(maps), shapes, B)
        obj, dl = head.predict(t)
        lg_list, dl_list = head(maps)
    torch.cuda.synchronize()
    rnd = (lambda v: v.bfloat16().double()) if precision == 'bf16' else (lambda v: v.double())
    w, bias = rnd(sd['conv.weight']), sd['conv.bias'].double()
    wc, bc = sd['cls_logits.weight'].double().view(3, 256), sd['cls_logits.bias'].double()
    wb, bb = sd['bbox_pred.weight'].double().view(12, 256), sd['bbox_pred.bias'].double()
    t_c, off = t.float().cpu().double(), 0
    ref_t, ref_o, ref_d = [], [], []
    for x in feats.values():
        x = rnd(x)
        pre = F.conv2d(x, w, bias, padding=1)
        mag = F.conv2d(x.abs(), w.abs(), bias.abs(), padding=1)
        n = B * x.shape[2] * x.shape[3]
        r = F.relu(pre).permute(0, 2, 3, 1).reshape(n, 256)
        ref_t.append(r)
        ref_o.append(r @ wc.t() + bc)
        ref_d.append(r @ wb.t() + bb)
        if precision == 'fp32':
            tag = 'rpn head fp32 level %dx%d ' % tuple(x.shape[2:])
            check(tag + 'conv + relu', t_c[off:off + n], r, mag.permute(0, 2, 3, 1).reshape(n, 256), 9 * 256, 0.0)
            own = t_c[off:off + n]
            check(tag + 'cls_logits', obj[off:off + n].cpu(), own @ wc.t() + bc, own.abs() @ wc.abs().t() + bc.abs(), 256,
                  0.0)
            check(tag + 'bbox_pred', dl[off:off + n].cpu(), own @ wb.t() + bb, own.abs() @ wb.abs().t() + bb.abs(), 256,
                  0.0)
        # the NCHW views of forward() are the same numbers
        H, W = x.shape[2:]
        lvl = len(ref_t) - 1
        assert torch.equal(lg_list[lvl].permute(0, 2, 3, 1).reshape(n, 3), obj[off:off + n])
        assert torch.equal(dl_list[lvl].permute(0, 2, 3, 1).reshape(n, 12), dl[off:off + n])
        assert lg_list[lvl].shape == (B, 3, H, W) and dl_list[lvl].shape == (B, 12, H, W)
        off += n
    ref_t, ref_o, ref_d = torch.cat(ref_t), torch.cat(ref_o), torch.cat(ref_d)
    got = {'hidden': (t_c, ref_t), 'objectness': (obj.cpu(), ref_o), 'deltas': (dl.cpu(), ref_d)}
    for name, (a, b) in got.items():
        e = (relmax(a, b), rel_l2(a, b))
        print('rpn head %s %-10s relmax %.3e rel-L2 %.3e' % (precision, name, e[0], e[1]))
        if precision == 'bf16':
            m = BF16_MEASURED[name]
            assert e[0] <= 2 * m[0] and e[1] <= 2 * m[1], (name, e, m)


@pytest.mark.parametrize('mode', ['testing', 'training'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_proposals_equal_the_restatement(precision, mode):
    anchors = R.grid_anchors(R.SHAPES, R.TENSOR, R.SIZES, R.RATIOS)
    k, post = R.PRE[mode], R.POST[mode]
    n_props = 0
    for seed in R.SEEDS:
        rpn, feats_d, _, _ = make_rpn(seed, precision)
        rpn.train(mode == 'training')
        assert (rpn.pre_nms_top_n(), rpn.post_nms_top_n()) == (k, post)
        with torch.no_grad():
            obj, dl, shapes, B = rpn.head_outputs(feats_d)
            ob, osc, cnt, oi = rpn.filter_proposals(obj, dl, shapes, B, R.IMAGES, R.TENSOR)
            props = rpn.propose(feats_d, R.IMAGES, R.TENSOR)
        counts, index = (t.cpu() for t in rpn.last_selection)
        ob, osc, cnt, oi = ob.cpu(), osc.cpu(), cnt.cpu(), oi.cpu()
        assert ob.shape == (B, post, 4) and osc.shape == (B, post) and cnt.shape == (B,)
        lg, dd = per_level(obj, dl, shapes, B)
        for b in range(B):
            want = R.filter_proposals([z[b].double() for z in lg], [d[b].double() for d in dd],
                                      [a.double() for a in anchors], R.IMAGES[b], k, post)
            d = int(cnt[b])
            tag = 'rpn %s %s seed %d image %d ' % (precision, mode, seed, b)
            assert d == len(want['level']), (tag, d, len(want['level']))
            e = oi[b, :d].to(torch.int64)
            assert (e // k).tolist() == want['level'], tag
            assert (e % k).tolist() == want['rank'], tag
            assert [int(index[(int(x) // k) * B + b, int(x) % k]) for x in e] == want['anchor'], tag
            lv, an = torch.tensor(want['level']), torch.tensor(want['anchor'])
            a_sel = torch.stack([anchors[int(l)][int(a)] for l, a in zip(lv, an)])
            d_sel = torch.stack([dd[int(l)][b][int(a)] for l, a in zip(lv, an)])
            check_abs(tag + 'boxes', ob[b, :d], want['boxes'], R.decode_allowance(d_sel, a_sel, TRANS))
            check_abs(tag + 'scores', osc[b, :d], want['scores'], TRANS * want['scores'] + 2.0 ** -126)
            assert bool((oi[b, d:] == -1).all()) and bool((ob[b, d:] == 0).all()) and bool((osc[b, d:] == 0).all())
            assert torch.equal(props[b].cpu(), ob[b, :d])
            n_props += d
    print('rpn %s %s: %d proposals over 16 seeds' % (precision, mode, n_props))
    assert n_props > 16 * 2 * 20


@pytest.mark.parametrize('layout,precision', [('ndhwc', 'fp32'), ('grouped', 'bf16')])
def test_propose_packed_reads_the_frame_in_place(layout, precision):
    from sfvos_amd import PackedClip
    rpn, _, _, _ = make_rpn(R.SEEDS[1], precision)
    rpn.eval()
    tdt = torch.float32 if precision == 'fp32' else torch.bfloat16
    g = torch.Generator().manual_seed(77)
    B, T = 2, 4          # a 5-frame window: one zero-padding frame in front, 4 stored
    levels = [torch.randn(B, T, H, W, 256, generator=g).to(tdt).cuda() for H, W in R.SHAPES]
    clip = PackedClip.from_levels(levels, layout=layout, pad=(1, 0))
    assert clip.window == 5 and clip.layout == layout
    with torch.no_grad():
        for frame in (None, 0, 3):
            f = 5 // 2 - 1 if frame is None else frame
            maps = OrderedDict((str(l), x[:, f].permute(0, 3, 1, 2).float()) for l, x in enumerate(levels))
            want = rpn.propose_padded(maps, R.IMAGES, R.TENSOR)
            got = rpn.propose_packed(clip, frame, R.IMAGES, R.TENSOR)
            for a, b in zip(got, want):
                assert torch.equal(a, b), (layout, frame)
            assert int(got[2].min()) > 0
        for frame in (-1, 4):
            with pytest.raises(RuntimeError, match='padding frame'):
                rpn.propose_packed(clip, frame, R.IMAGES, R.TENSOR)
        M = B * T * sum(h * w for h, w in R.SHAPES)
        e4m3 = PackedClip(torch.zeros((4, M, 64), dtype=torch.uint8, device='cuda'), R.SHAPES, B, T, pad=(1, 0))
        with pytest.raises(RuntimeError, match='grouped8'):
            rpn.propose_packed(e4m3, None, R.IMAGES, R.TENSOR)


def test_forward_feeds_the_box_branch_and_modes():
    from sfvos_amd import BoxBranch
    rpn, feats_d, _, _ = make_rpn(R.SEEDS[2], 'fp32')
    images = types.SimpleNamespace(tensors=torch.zeros(2, 3, *R.TENSOR, device='cuda'), image_sizes=list(R.IMAGES))
    # a head that requires grad raises: the RPN is inference only
    with pytest.raises(RuntimeError, match='inference only'):
        rpn(images, feats_d)
    for p in rpn.parameters():
        p.requires_grad_(False)
    rpn.eval()
    proposals, losses = rpn(images, feats_d)            # frozen parameters: no no_grad needed
    assert isinstance(proposals, list) and len(proposals) == 2 and losses == {}
    assert all(p.dim() == 2 and p.shape[1] == 4 and 0 < p.shape[0] <= R.POST['testing'] for p in proposals)
    rpn.train()
    assert all(p.shape[0] <= R.POST['training'] for p in rpn(images, feats_d)[0])
    with torch.no_grad():
        assert rpn.propose_padded(feats_d, R.IMAGES, R.TENSOR)[0].shape == (2, R.POST['training'], 4)
        assert rpn.eval().propose_padded(feats_d, R.IMAGES, R.TENSOR)[0].shape == (2, R.POST['testing'], 4)
    torch.manual_seed(5)
    box = BoxBranch(2, 'fp32').cuda()
    dets = box.detect(feats_d, proposals, R.IMAGES)
    assert len(dets) == 2
    for d, (H, W) in zip(dets, R.IMAGES):
        b = d['boxes']
        assert bool(torch.isfinite(b).all())
        assert bool((b[:, 0::2] >= 0).all()) and bool((b[:, 0::2] <= W).all())
        assert bool((b[:, 1::2] >= 0).all()) and bool((b[:, 1::2] <= H).all())
    print('detections from RPN proposals: %s' % [int(d['boxes'].shape[0]) for d in dets])


def test_propose_padded_is_capturable():
    rpn, feats_d, _, _ = make_rpn(R.SEEDS[3], 'bf16')
    rpn.eval()
    with torch.no_grad():
        want = [t.clone() for t in rpn.propose_padded(feats_d, R.IMAGES, R.TENSOR)]     # warm-up: images, tables
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):       # a single branch: every launch goes to the capture stream
            out = rpn.propose_padded(feats_d, R.IMAGES, R.TENSOR)
        for t in out:
            t.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
    for a, b in zip(out, want):
        assert torch.equal(a, b)
    assert int(want[2].min()) > 0
