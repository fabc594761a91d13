"""GPU: sfvos_amd.FeaturePyramidNetwork, fp32 and bf16, stage by stage against float64 (tests/fpn_ref.py), so that every
bound is the derived per-element criterion of kernel_util and no tolerance is invented:

  inner map l   from x_l and the module's OWN coarser inner map (as stored), K = c_in + 1
  output map l  from the module's OWN inner map (as stored), K = 9 out_channels
  'pool'        bit-equal to the subsample of the coarsest output
  forward       bit-equal to forward_pyramid, unpacked
  write_frames  bit-equal to forward_pyramid of the same frames, neighbours and guards untouched, version bumped
  RPN           propose_packed on a written frame == the RPN on forward's maps of that frame (out_channels 256)

Inputs 19x27, 10x14, 5x7, 3x4 with B = 2: 2 n and 2 n - 1 mixed at every step."""
import functools
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

import fpn_ref as R
from kernel_util import PRECS, SENT, TDT, U_OUT, Out, check, rnd

pytestmark = pytest.mark.gpu

CH = (32, 64, 96, 128)
SHAPES = [(19, 27), (10, 14), (5, 7), (3, 4)]
OUT_SHAPES = SHAPES + [(2, 2)]
WIDTHS = [64, 256]


def _inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    return OrderedDict((str(l), torch.randn(B, c, h, w, generator=g)) for l, (c, (h, w)) in enumerate(zip(CH, SHAPES)))


@functools.lru_cache(maxsize=None)
def _setup(prec, C):
    """(module, reference module with the same parameters, CPU inputs, forward_pyramid's results on the CPU)."""
    from sfvos_amd import FeaturePyramidNetwork
    torch.manual_seed(100 + C)
    ref = R.FeaturePyramidNetwork(CH, C)
    with torch.no_grad():
        for conv in list(ref.inner_blocks) + list(ref.layer_blocks):
            conv.bias.normal_()          # torchvision's init leaves zeros: they would hide a missing bias
    fpn = FeaturePyramidNetwork(CH, C, precision=prec)
    fpn.load_state_dict(ref.state_dict(), strict=True)
    fpn.cuda().eval()
    for p in fpn.parameters():
        p.requires_grad_(False)
    x = _inputs(2, 7)
    xd = OrderedDict((k, v.cuda()) for k, v in x.items())
    flat, shapes, inner = fpn.forward_pyramid(xd, return_inner=True)
    torch.cuda.synchronize()
    assert shapes == OUT_SHAPES and flat.dtype == TDT[prec] and tuple(flat.shape) == (2 * sum(h * w for h, w in shapes), C)
    return fpn, ref, x, xd, flat.cpu(), [t.cpu() for t in inner]


def _levels(flat, B, shapes):
    out, off = [], 0
    for h, w in shapes:
        out.append(flat[off:off + B * h * w])
        off += B * h * w
    return out


@pytest.mark.parametrize('C', WIDTHS)
@pytest.mark.parametrize('prec', PRECS)
def test_inner_maps_stage_by_stage(prec, C):
    fpn, ref, x, _, _, inner = _setup(prec, C)
    for l in (3, 2, 1, 0):
        conv = ref.inner_blocks[l]
        xl, wt = rnd(x[str(l)], prec).double(), rnd(conv.weight.detach(), prec).double()
        top = None if l == 3 else R.nchw(inner[l + 1].double(), 2, *SHAPES[l + 1])
        want = R.inner_step(xl, wt, conv.bias.detach().double(), top)
        mag = R.inner_step(xl.abs(), wt.abs(), conv.bias.detach().double().abs(), None if top is None else top.abs())
        check('fpn inner %d %s C%d' % (l, prec, C), inner[l].float(), R.nhwc(want), R.nhwc(mag), CH[l] + 1, U_OUT[prec])


@pytest.mark.parametrize('C', WIDTHS)
@pytest.mark.parametrize('prec', PRECS)
def test_output_maps_stage_by_stage_and_pool(prec, C):
    fpn, ref, _, _, flat, inner = _setup(prec, C)
    outs = _levels(flat, 2, OUT_SHAPES)
    for l in range(4):
        conv = ref.layer_blocks[l]
        a = R.nchw(inner[l].double(), 2, *SHAPES[l])
        wt, b = rnd(conv.weight.detach(), prec).double(), conv.bias.detach().double()
        want, mag = R.output_step(a, wt, b), R.output_step(a.abs(), wt.abs(), b.abs())
        check('fpn output %d %s C%d' % (l, prec, C), outs[l].float(), R.nhwc(want), R.nhwc(mag), 9 * C, U_OUT[prec])
    coarsest = R.nchw(outs[3], 2, *SHAPES[3])
    assert torch.equal(R.nchw(outs[4], 2, 2, 2), coarsest[:, :, ::2, ::2])
    assert torch.equal(R.nchw(outs[4].float(), 2, 2, 2), R.last_level_max_pool(coarsest.float()))


@pytest.mark.parametrize('C', WIDTHS)
@pytest.mark.parametrize('prec', PRECS)
def test_forward_is_the_pyramid_unpacked_and_state_dict_round_trips(prec, C):
    fpn, ref, _, xd, flat, _ = _setup(prec, C)
    out = fpn(xd)
    assert list(out.keys()) == ['0', '1', '2', '3', 'pool']
    for (k, v), lv, (h, w) in zip(out.items(), _levels(flat, 2, OUT_SHAPES), OUT_SHAPES):
        assert v.dtype == torch.float32 and tuple(v.shape) == (2, C, h, w), k
        assert torch.equal(v.cpu(), R.nchw(lv.float(), 2, h, w)), k
    sd = fpn.state_dict()
    assert list(sd.keys()) == list(ref.state_dict().keys())
    for k, v in ref.state_dict().items():
        assert torch.equal(sd[k].cpu(), v), k
    R.FeaturePyramidNetwork(CH, C).load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    # a list of maps serves as well; a trainable module refuses
    out2 = fpn(list(xd.values()))
    assert all(torch.equal(a, b) for a, b in zip(out.values(), out2.values()))
    fpn.layer_blocks[0].bias.requires_grad_(True)
    try:
        with pytest.raises(RuntimeError, match='inference only'):
            fpn(xd)
    finally:
        fpn.layer_blocks[0].bias.requires_grad_(False)


def _written_sequence(fpn, prec, C, xd, frames=5, first=1):
    from sfvos_amd import PackedClip
    M = sum(h * w for h, w in OUT_SHAPES)
    buf = Out((frames * M, C), TDT[prec])
    seq = PackedClip(buf.t, OUT_SHAPES, 1, frames)
    before = seq.data._version
    assert fpn.write_frames(xd, seq, first) is seq
    torch.cuda.synchronize()
    return buf, seq, before


@pytest.mark.parametrize('C', WIDTHS)
@pytest.mark.parametrize('prec', PRECS)
def test_write_frames_in_place(prec, C):
    fpn = _setup(prec, C)[0]
    xd = OrderedDict((k, v.cuda()) for k, v in _inputs(3, 8).items())
    flat, shapes = fpn.forward_pyramid(xd)
    buf, seq, before = _written_sequence(fpn, prec, C, xd)
    assert seq.data._version > before
    got, want = buf.cpu(), _levels(flat.cpu(), 3, shapes)
    off = 0
    for (h, w), lv in zip(shapes, want):
        level = got[off:off + 5 * h * w].view(5, h * w, C)
        assert torch.equal(level[1:4].reshape(-1, C), lv), (h, w)
        assert bool((level[0] == SENT).all()) and bool((level[4] == SENT).all()), (h, w)
        off += 5 * h * w
    with pytest.raises(RuntimeError, match='outside the sequence'):
        fpn.write_frames(xd, seq, 3)


@pytest.mark.parametrize('prec', PRECS)
def test_rpn_reads_the_written_frames_in_place(prec):
    from sfvos_amd import RegionProposalNetwork
    fpn = _setup(prec, 256)[0]
    torch.manual_seed(5)
    rpn = RegionProposalNetwork(precision=prec).cuda().eval()
    sizes, tensor = [(70, 100)], (76, 108)
    xd = OrderedDict((k, v.cuda()) for k, v in _inputs(3, 9).items())
    with torch.no_grad():
        maps = fpn(xd)
        buf, seq, _ = _written_sequence(fpn, prec, 256, xd)
        for b in range(3):
            want = rpn.propose_padded(OrderedDict((k, v[b:b + 1]) for k, v in maps.items()), sizes, tensor)
            got = rpn.propose_packed(seq, 1 + b, sizes, tensor)
            for a, c in zip(got, want):
                assert torch.equal(a, c), b
            assert int(got[2].min()) > 0
    assert buf.guards_ok()
