"""CPU (no GPU): the host side of the ResNet-body entry points (csrc/body.hip) and of sfvos_amd.body -- the calls they
refuse before any kernel is launched (a refused call returns -1 and leaves a message that starts with the entry point's
name), the ABI revision and bindings, the state-dict surface of ResNetBody and BackboneWithFPN (torchvision's names), the
host-side refusals of forward, and the coverage of sfvos_conv2d_plan's configurations by the GPU kernel tests."""
import ctypes

import pytest
import torch

import body_ref as R

P = 1 << 40                   # never dereferenced (16-byte aligned)

# entry point -> (argument names, defaults of a call that passes every check); pointers default to P, the stream to NULL
ENTRY = {
    'conv2d': ('x ld_x weight scale shift residual ld_res y ld_y batch h w c_in c_out taps stride relu dtype workspace '
               'stream',
               dict(ld_x=64, ld_res=256, ld_y=256, batch=2, h=9, w=13, c_in=64, c_out=256, taps=1, stride=1, relu=1,
                    dtype=1)),
    'body_stem': ('x stride_b stride_c stride_h stride_w batch h w weight scale shift y ld_y dtype stream',
                  dict(stride_b=3 * 70 * 100, stride_c=70 * 100, stride_h=100, stride_w=1, batch=2, h=70, w=100, ld_y=64,
                       dtype=0)),
    'maxpool3x3s2': ('src ld_src dst ld_dst batch h w C dtype stream',
                     dict(ld_src=64, ld_dst=64, batch=2, h=5, w=7, C=64, dtype=1)),
}

REFUSALS = [
    ('conv2d', dict(x=None)), ('conv2d', dict(weight=None)), ('conv2d', dict(scale=None)), ('conv2d', dict(shift=None)),
    ('conv2d', dict(y=None)),
    ('conv2d', dict(x=P + 8)), ('conv2d', dict(weight=P + 4)), ('conv2d', dict(y=P + 2)), ('conv2d', dict(residual=P + 8)),
    ('conv2d', dict(scale=P + 4)),
    ('conv2d', dict(c_in=96, ld_x=96)), ('conv2d', dict(c_in=0)), ('conv2d', dict(c_out=288, ld_y=288, ld_res=288)),
    ('conv2d', dict(c_out=32)), ('conv2d', dict(c_out=0)), ('conv2d', dict(c_in=2112, ld_x=2112)),
    ('conv2d', dict(c_out=2112, ld_y=2112, ld_res=2112)),
    ('conv2d', dict(taps=3)), ('conv2d', dict(taps=0)), ('conv2d', dict(taps=49)),
    ('conv2d', dict(stride=0)), ('conv2d', dict(stride=3)), ('conv2d', dict(dtype=2)), ('conv2d', dict(dtype=-1)),
    ('conv2d', dict(ld_x=32)), ('conv2d', dict(ld_x=68)), ('conv2d', dict(ld_y=255)), ('conv2d', dict(ld_y=192)),
    ('conv2d', dict(ld_res=128)), ('conv2d', dict(relu=2)),
    ('conv2d', dict(batch=0)), ('conv2d', dict(h=0)), ('conv2d', dict(w=0)),
    ('conv2d', dict(batch=1 << 20, h=64, w=64)),
    # a K-split shape without its workspace
    ('conv2d', dict(c_in=512, ld_x=512, c_out=512, ld_y=512, ld_res=512, taps=9, batch=1, h=3, w=4, workspace=None)),
    ('body_stem', dict(x=None)), ('body_stem', dict(weight=None)), ('body_stem', dict(scale=None)),
    ('body_stem', dict(shift=None)), ('body_stem', dict(y=None)),
    ('body_stem', dict(stride_w=2)), ('body_stem', dict(stride_w=0)), ('body_stem', dict(stride_c=-7000)),
    ('body_stem', dict(ld_y=32)), ('body_stem', dict(ld_y=66)), ('body_stem', dict(dtype=2)),
    ('body_stem', dict(batch=0)), ('body_stem', dict(h=0)), ('body_stem', dict(w=0)),
    ('body_stem', dict(weight=P + 8)), ('body_stem', dict(y=P + 4)), ('body_stem', dict(batch=1 << 20, h=64, w=64)),
    ('maxpool3x3s2', dict(src=None)), ('maxpool3x3s2', dict(dst=None)),
    ('maxpool3x3s2', dict(ld_src=56)), ('maxpool3x3s2', dict(ld_dst=32)), ('maxpool3x3s2', dict(ld_src=68)),
    ('maxpool3x3s2', dict(C=60)), ('maxpool3x3s2', dict(C=0)), ('maxpool3x3s2', dict(dtype=2)),
    ('maxpool3x3s2', dict(batch=0)), ('maxpool3x3s2', dict(h=0)), ('maxpool3x3s2', dict(w=0)),
    ('maxpool3x3s2', dict(src=P + 4)),
]


def _load():
    from sfvos_amd import _lib
    return _lib, _lib.load()


def _call(name, **over):
    _, lib = _load()
    names, defaults = ENTRY[name]
    args = [over[a] if a in over else defaults.get(a, None if a == 'stream' else P) for a in names.split()]
    rc = getattr(lib, 'sfvos_' + name)(*args)
    msg = lib.sfvos_last_error()
    return rc, (msg.decode() if msg else '')


@pytest.mark.parametrize('name,over', REFUSALS, ids=['%s-%s' % (n, sorted(o.items(), key=str)) for n, o in REFUSALS])
def test_refused_by_message_before_any_launch(name, over):
    rc, msg = _call(name, **over)
    assert rc == -1, (rc, msg)
    assert msg.startswith(name + ':'), msg


def test_plan_and_workspace_refuse_bad_shapes():
    _, lib = _load()
    sp = ctypes.c_int(7)
    for bad in (dict(c_in=96), dict(c_out=32), dict(taps=4), dict(stride=3), dict(dtype=2), dict(h=0), dict(cus=-1)):
        a = dict(dtype=1, batch=1, h=9, w=13, c_in=64, c_out=64, taps=9, stride=1, cus=256)
        a.update(bad)
        rc = lib.sfvos_conv2d_plan(a['dtype'], a['batch'], a['h'], a['w'], a['c_in'], a['c_out'], a['taps'], a['stride'],
                                   a['cus'], ctypes.byref(sp))
        assert rc == -1 and lib.sfvos_last_error().decode().startswith('conv2d_plan:'), bad
        if 'cus' not in bad:
            assert lib.sfvos_conv2d_workspace_bytes(a['dtype'], a['batch'], a['h'], a['w'], a['c_in'], a['c_out'],
                                                    a['taps'], a['stride']) == 0
    # a pure function of its arguments; splits may be NULL
    one = lib.sfvos_conv2d_plan(1, 1, 24, 42, 512, 512, 9, 1, 256, ctypes.byref(sp))
    assert (one, sp.value) == (5, 2) and lib.sfvos_conv2d_plan(1, 1, 24, 42, 512, 512, 9, 1, 256, None) == 5
    assert lib.sfvos_conv2d_plan(1, 1, 24, 42, 512, 512, 9, 1, 2048, ctypes.byref(sp)) == 5 and sp.value == 8
    assert lib.sfvos_conv2d_plan(1, 1, 24, 42, 512, 512, 9, 1, 64, ctypes.byref(sp)) == 1 and sp.value == 1


def test_abi_revision_bindings_and_sources():
    import importlib.util
    import os
    _lib, lib = _load()
    assert _lib.ABI_REVISION >= 308 and lib.sfvos_version() >= 308
    for name, n_args in (('sfvos_conv2d', 20), ('sfvos_conv2d_plan', 10), ('sfvos_conv2d_workspace_bytes', 8),
                         ('sfvos_body_stem', 15), ('sfvos_maxpool3x3s2', 10)):
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and len(_lib.SIGNATURES[name][1]) == n_args
    path = os.path.join(os.path.dirname(_lib.__file__), 'build.py')
    spec = importlib.util.spec_from_file_location('sfvos_build_for_body_test', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert 'body.hip' in mod.SOURCES


@pytest.mark.parametrize('dtype', [0, 1], ids=['fp32', 'bf16'])
def test_every_plan_of_a_full_frame_is_covered_by_the_gpu_kernel_tests(dtype):
    """The 52 conv shapes of a 768x1344 frame on a 256-CU device: every configuration sfvos_conv2d_plan returns for them
    is also the configuration of at least one exact case of test_gpu_body_kernels.py."""
    import test_gpu_body_kernels as K
    _, lib = _load()

    def plan(B, h, w, c_in, c_out, taps, stride):
        sp = ctypes.c_int()
        pid = lib.sfvos_conv2d_plan(dtype, B, h, w, c_in, c_out, taps, stride, 256, ctypes.byref(sp))
        assert pid >= 0 and (sp.value > 1) == (pid >= 3)
        return pid

    shapes = R.conv_shapes((192, 336))
    assert len(shapes) == 52
    frame = {plan(1, h, w, ci, co, t, s) for _, h, w, ci, co, t, s in shapes}
    tested = {plan(c[4], c[5], c[6], c[2], c[3], c[0], c[1]) for c in K.EXACT}
    assert frame <= tested, (frame, tested)
    assert frame == {0, 1, 2, 5}


def test_state_dict_surface_and_strict_loads():
    import sfvos_amd
    from sfvos_amd import BackboneWithFPN, ResNetBody
    assert {'ResNetBody', 'BackboneWithFPN'} <= set(sfvos_amd.__all__)
    want = R.expected_state()
    body = ResNetBody()
    assert {k: tuple(v.shape) for k, v in body.state_dict().items()} == dict(want)
    assert list(body.state_dict().keys()) == list(want.keys())
    assert [n for n, _ in body.named_parameters()] == [k for k, s in want.items() if len(s) == 4]
    assert body.layer2[0].conv2.stride == (2, 2) and body.layer2[0].conv1.stride == (1, 1)      # v1.5
    assert body.layer1[0].downsample[0].stride == (1, 1) and body.layer3[0].downsample[0].stride == (2, 2)
    assert not hasattr(body, 'fc') and body.bn1.eps == 0.0 and ResNetBody(eps=1e-5).layer4[2].bn3.eps == 1e-5
    sd = R.random_state(4)
    prefix = 'maskrcnn_model.backbone.body.'
    ckpt = {prefix + k: v for k, v in sd.items()}
    for k in list(sd):
        if k.endswith('running_var'):
            ckpt[prefix + k.replace('running_var', 'num_batches_tracked')] = torch.tensor(0)
    ckpt['maskrcnn_model.backbone.fpn.inner_blocks.0.weight'] = torch.zeros(256, 256, 1, 1)
    body.load_state_dict({k[len(prefix):]: v for k, v in ckpt.items() if k.startswith(prefix)}, strict=True)
    for k in want:
        assert torch.equal(body.state_dict()[k], sd[k])
    assert 'bn1.num_batches_tracked' not in body.state_dict()
    with pytest.raises(RuntimeError):
        body.load_state_dict({k: v for k, v in sd.items() if k != 'layer3.4.bn2.running_mean'}, strict=True)
    with pytest.raises(RuntimeError):
        body.load_state_dict(dict(sd, **{'fc.weight': torch.zeros(1000, 2048)}), strict=True)
    # scale and shift in torchvision's order
    bn = body.layer1[0].bn1
    scale, shift = bn.coefficients()
    assert torch.equal(scale, bn.weight * (bn.running_var + 0.0).rsqrt())
    assert torch.equal(shift, bn.bias - bn.running_mean * scale)
    # the whole backbone
    net = BackboneWithFPN()
    assert net.out_channels == 256 and isinstance(net.body, ResNetBody)
    keys = set(net.state_dict().keys())
    assert keys == {'body.' + k for k in want} | {'fpn.' + k for k in net.fpn.state_dict()}
    g = torch.Generator().manual_seed(5)
    full = {'body.' + k: v for k, v in sd.items()}
    full.update({'fpn.' + k: torch.randn(v.shape, generator=g) for k, v in net.fpn.state_dict().items()})
    full['body.bn1.num_batches_tracked'] = torch.tensor(3)
    net.load_state_dict(dict(full), strict=True)
    assert torch.equal(net.body.layer4[2].conv3.weight, sd['layer4.2.conv3.weight'])
    assert torch.equal(net.fpn.layer_blocks[3].bias, full['fpn.layer_blocks.3.bias'])
    with pytest.raises(RuntimeError):
        net.load_state_dict({k: v for k, v in full.items() if k != 'fpn.inner_blocks.1.bias'}, strict=True)
    with pytest.raises(ValueError):
        ResNetBody(precision='fp8')
    with pytest.raises(ValueError):
        ResNetBody(layers=(3, 4, 6))


def test_forward_refuses_cpu_tensors_and_gradients():
    from sfvos_amd import BackboneWithFPN, ResNetBody
    body = ResNetBody(layers=(1, 1, 1, 1))
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match='inference only'):      # the parameters require grad
        body(x)
    with torch.no_grad():
        for call in (body, body.forward_channels_last):
            with pytest.raises(RuntimeError, match='no CPU fallback'):
                call(x)
    for p in body.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        body(x)
    with pytest.raises(RuntimeError, match='inference only'):      # an input that requires grad
        body(torch.zeros(1, 3, 32, 32, requires_grad=True))
    net = BackboneWithFPN()
    with pytest.raises(RuntimeError, match='inference only'):
        net(x)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            net(x)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            net.write_frames(x, None, 0)
    assert ResNetBody.level_shapes((70, 100)) == [(18, 25), (9, 13), (5, 7), (3, 4)]
    assert ResNetBody.level_shapes((768, 1344)) == [(192, 336), (96, 168), (48, 84), (24, 42)]
