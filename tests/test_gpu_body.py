"""GPU: sfvos_amd.ResNetBody and BackboneWithFPN, fp32 and bf16, ResNet-50 proper with random weights and frozen-norm
buffers (running_var in [0.5, 2]) on 2 x 3x70x100 (odd sides at every level: 35x50, 18x25, 9x13, 5x7, 3x4) and 1 x 3x64x96.

Link by link (return_stages=True): every launch's output against float64 computed from the module's OWN input to that
launch (as stored) and the operands as the kernel sees them, so that every bound is the derived per-element criterion of
kernel_util and no bf16 tolerance is invented -- a ReLU flip cannot accumulate:
  conv1 (stem)    K = 148;  maxpool  equal to F.max_pool2d of the stored stem output
  every conv      K = c_in * taps + 2 (products, shift, residual), mag = |scale| sum |x||W| + |shift| + |residual|
End to end against the float64 restatement (tests/body_ref.py): fp32 within the project's module gate (1e-3 of the
tensor's scale); bf16 printed per level, not gated (the links are the gate).  forward == forward_channels_last unpacked,
BackboneWithFPN.forward == fpn(body(x)), write_frames == that pyramid in place, all bit for bit."""
import functools
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

import body_ref as R
from kernel_util import PRECS, SENT, TDT, U_OUT, Out, check, rel_l2, relmax, rnd

pytestmark = pytest.mark.gpu

IMAGES = {'2x70x100': (2, 70, 100), '1x64x96': (1, 64, 96)}


@functools.lru_cache(maxsize=None)
def _state():
    return R.random_state(31)


@functools.lru_cache(maxsize=None)
def _image(name):
    B, h, w = IMAGES[name]
    return torch.randn(B, 3, h, w, generator=torch.Generator().manual_seed(32))


@functools.lru_cache(maxsize=None)
def _body(prec, eps=0.0):
    from sfvos_amd import ResNetBody
    body = ResNetBody(precision=prec, eps=eps)
    body.load_state_dict(_state(), strict=True)
    body.cuda().eval()
    for p in body.parameters():
        p.requires_grad_(False)
    return body


@functools.lru_cache(maxsize=None)
def _run(prec, name):
    """(maps on the CPU, shapes, stages with x / y / residual on the CPU)."""
    body = _body(prec)
    maps, shapes, stages = body.forward_channels_last(_image(name).cuda(), return_stages=True)
    torch.cuda.synchronize()
    assert all(m.dtype == TDT[prec] for m in maps)
    out = []
    for st in stages:
        st = dict(st)
        for k in ('x', 'y', 'residual'):
            if st.get(k) is not None:
                st[k] = st[k].cpu()
        out.append(st)
    return [m.cpu() for m in maps], shapes, out


@functools.lru_cache(maxsize=None)
def _reference(name):
    return R.ResNetBody(_state())(_image(name).double())


@pytest.mark.parametrize('name', list(IMAGES))
@pytest.mark.parametrize('prec', PRECS)
def test_every_launch_against_float64_of_its_own_input(prec, name):
    B, H, W = IMAGES[name]
    maps, shapes, stages = _run(prec, name)
    assert shapes == [tuple(s) for s in _body(prec).level_shapes((H, W))]
    assert [s['name'] for s in stages[:2]] == ['conv1', 'maxpool'] and len(stages) == 54
    sd = _state()
    for st in stages:
        (h, w), (oh, ow) = st['in_hw'], st['out_hw']
        if st['kind'] == 'pool':
            a = R.nchw(st['x'].float(), B, h, w)
            assert torch.equal(R.nhwc(F.max_pool2d(a, 3, 2, 1)), st['y'].float())
            continue
        if st['kind'] == 'stem':
            x, wt, bn, stride, pad, K = rnd(st['x'], prec).double(), sd['conv1.weight'], _body(prec).bn1, 2, 3, 148
            relu, resid = True, None
        else:
            x = R.nchw(st['x'].double(), B, h, w)
            wt, bn, stride = st['conv'].weight.detach().cpu(), st['bn'], st['stride']
            pad, K = (1 if wt.shape[2] == 3 else 0), wt.shape[1] * wt.shape[2] * wt.shape[3] + 2
            relu, resid = st['relu'], st['residual']
        wt = rnd(wt, prec).double()
        scale, shift = (t.cpu().double() for t in bn.coefficients())
        ref = R.nhwc(F.conv2d(x, wt, None, stride, pad)) * scale + shift
        mag = R.nhwc(F.conv2d(x.abs(), wt.abs(), None, stride, pad)) * scale.abs() + shift.abs()
        if resid is not None:
            ref, mag = ref + resid.double(), mag + resid.double().abs()
        if relu:
            ref = ref.clamp_min(0)
        assert tuple(st['y'].shape) == (B * oh * ow, wt.shape[0])
        check('body %s %s %s' % (prec, name, st['name']), st['y'].float(), ref, mag, K, U_OUT[prec])
    for m, last in zip(maps, ('layer1.2.conv3', 'layer2.3.conv3', 'layer3.5.conv3', 'layer4.2.conv3')):
        assert torch.equal(m, [s for s in stages if s['name'] == last][0]['y'])


@pytest.mark.parametrize('name', list(IMAGES))
@pytest.mark.parametrize('prec', PRECS)
def test_end_to_end_against_the_float64_restatement(prec, name):
    B = IMAGES[name][0]
    maps, shapes, _ = _run(prec, name)
    ref = _reference(name)
    for l, (m, (h, w)) in enumerate(zip(maps, shapes)):
        want = ref[str(l)]
        got = R.nchw(m.float(), B, h, w)
        assert got.shape == want.shape
        print('body end to end %s %s C%d: max error / max |ref| %.3e, rel-L2 %.3e'
              % (prec, name, l + 2, relmax(got, want), rel_l2(got, want)))
        if prec == 'fp32':
            assert relmax(got, want) < 1e-3, l


@pytest.mark.parametrize('prec', PRECS)
def test_forward_is_channels_last_unpacked_and_state_dict_round_trips(prec):
    from sfvos_amd import ResNetBody
    body = _body(prec)
    maps, shapes, _ = _run(prec, '2x70x100')
    out = body(_image('2x70x100').cuda())
    assert list(out.keys()) == ['0', '1', '2', '3']
    for (k, v), m, (h, w) in zip(out.items(), maps, shapes):
        assert v.dtype == torch.float32 and tuple(v.shape) == (2, m.shape[1], h, w), k
        assert torch.equal(v.cpu(), R.nchw(m.float(), 2, h, w)), k
    sd = body.state_dict()
    assert list(sd.keys()) == list(_state().keys())
    for k, v in _state().items():
        assert torch.equal(sd[k].cpu(), v), k
    ResNetBody().load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    # a slice of a wider tensor is read through its strides; a trainable module refuses
    big = torch.zeros(2, 3, 72, 108, device='cuda')
    big[:, :, 1:71, 4:104] = _image('2x70x100').cuda()
    out2 = body(big[:, :, 1:71, 4:104])
    assert all(torch.equal(a, b) for a, b in zip(out.values(), out2.values()))
    body.layer1[0].conv1.weight.requires_grad_(True)
    try:
        with pytest.raises(RuntimeError, match='inference only'):
            body(big)
    finally:
        body.layer1[0].conv1.weight.requires_grad_(False)


@pytest.mark.parametrize('prec', PRECS)
def test_eps_changes_the_coefficients_as_the_formula_says(prec):
    sd = _state()
    b0, b1 = _body(prec), _body(prec, 1e-5)
    for name, bn0, bn1 in (('bn1', b0.bn1, b1.bn1), ('layer4.2.bn3', b0.layer4[2].bn3, b1.layer4[2].bn3)):
        w, b = sd[name + '.weight'].double(), sd[name + '.bias'].double()
        rm, rv = sd[name + '.running_mean'].double(), sd[name + '.running_var'].double()
        for bn, eps in ((bn0, 0.0), (bn1, 1e-5)):
            scale, shift = (t.cpu().double() for t in bn.coefficients())
            want = w * (rv + eps).rsqrt()
            assert float(((scale - want).abs() / want.abs()).max()) <= 2.0 ** -22
            assert float(((shift - (b - rm * want)).abs() / (b.abs() + (rm * want).abs())).max()) <= 2.0 ** -22
        assert not torch.equal(bn0.coefficients()[0], bn1.coefficients()[0])
    # ... and the stem follows them
    x = _image('1x64x96')
    _, _, stages = b1.forward_channels_last(x.cuda(), return_stages=True)
    torch.cuda.synchronize()
    wt = rnd(sd['conv1.weight'], prec).double()
    scale = sd['bn1.weight'].double() * (sd['bn1.running_var'].double() + 1e-5).rsqrt()
    shift = sd['bn1.bias'].double() - sd['bn1.running_mean'].double() * scale
    xr = rnd(x, prec).double()
    ref = (R.nhwc(F.conv2d(xr, wt, None, 2, 3)) * scale + shift).clamp_min(0)
    mag = R.nhwc(F.conv2d(xr.abs(), wt.abs(), None, 2, 3)) * scale.abs() + shift.abs()
    check('body stem eps=1e-5 %s' % prec, stages[0]['y'].float(), ref, mag, 148, U_OUT[prec])
    assert not torch.equal(stages[0]['y'].cpu(), _run(prec, '1x64x96')[2][0]['y'])


@functools.lru_cache(maxsize=None)
def _backbone(prec):
    from sfvos_amd import BackboneWithFPN
    torch.manual_seed(33)
    net = BackboneWithFPN(precision=prec)
    net.body.load_state_dict(_state(), strict=True)
    with torch.no_grad():
        for conv in list(net.fpn.inner_blocks) + list(net.fpn.layer_blocks):
            conv.bias.normal_()
    net.cuda().eval()
    for p in net.parameters():
        p.requires_grad_(False)
    return net


@pytest.mark.parametrize('prec', PRECS)
def test_backbone_is_the_fpn_of_the_body_and_writes_frames_in_place(prec):
    from sfvos_amd import PackedClip
    net = _backbone(prec)
    x = _image('2x70x100').cuda()
    out = net(x)
    want = net.fpn(net.body(x))
    assert list(out.keys()) == ['0', '1', '2', '3', 'pool'] and net.out_channels == 256
    shapes = [(18, 25), (9, 13), (5, 7), (3, 4), (2, 2)]
    for (k, v), (h, w) in zip(out.items(), shapes):
        assert tuple(v.shape) == (2, 256, h, w) and torch.equal(v, want[k]), k
    # the body inside the backbone is the body alone
    alone = _body(prec)(x)
    assert all(torch.equal(a, b) for a, b in zip(net.body(x).values(), alone.values()))
    # the same two images as frames 1, 2 of a resident clip of 4 frames
    flat, fshapes = net.fpn.forward_pyramid(net.body(x))
    assert fshapes == shapes
    M = sum(h * w for h, w in shapes)
    buf = Out((4 * M, 256), TDT[prec])
    seq = PackedClip(buf.t, shapes, 1, 4)
    before = seq.data._version
    assert net.write_frames(x, seq, 1) is seq
    torch.cuda.synchronize()
    assert seq.data._version > before
    got, flat, off, src = buf.cpu(), flat.cpu(), 0, 0
    for h, w in shapes:
        level = got[off:off + 4 * h * w].view(4, h * w, 256)
        assert torch.equal(level[1:3].reshape(-1, 256), flat[src:src + 2 * h * w]), (h, w)
        assert bool((level[0] == SENT).all()) and bool((level[3] == SENT).all()), (h, w)
        off += 4 * h * w
        src += 2 * h * w
