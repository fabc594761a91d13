"""CPU (no GPU): the host side of the feature-pyramid entry points (csrc/fpn.hip) and of sfvos_amd.fpn -- the calls they
refuse before any kernel is launched (a refused call returns -1 and leaves a message that starts with the entry point's
name), the ABI revision, the state-dict surface of FeaturePyramidNetwork (torchvision's names; the newer `.0.` spelling
loads too) and the host-side refusals of forward and write_frames."""
from collections import OrderedDict

import pytest
import torch

P = 1 << 40                   # never dereferenced (16-byte aligned)

# entry point -> (argument names, defaults of a call that passes every check); pointers default to P, the stream to NULL
ENTRY = {
    'fpn_lateral': ('x stride_b stride_c stride_h stride_w batch c_in h w weight bias c_out top top_h top_w ld_top y ld_y '
                    'dtype stream',
                    dict(stride_b=64 * 35, stride_c=35, stride_h=7, stride_w=1, batch=2, c_in=64, h=5, w=7, c_out=256,
                         top_h=3, top_w=4, ld_top=256, ld_y=256, dtype=0)),
    'fpn_pool': ('src ld_src dst ld_dst batch h w C dtype stream',
                 dict(ld_src=64, ld_dst=64, batch=2, h=5, w=7, C=64, dtype=1)),
}

REFUSALS = [
    ('fpn_lateral', dict(x=None)), ('fpn_lateral', dict(weight=None)), ('fpn_lateral', dict(bias=None)),
    ('fpn_lateral', dict(y=None)),
    ('fpn_lateral', dict(c_in=48)), ('fpn_lateral', dict(c_in=0)), ('fpn_lateral', dict(c_out=288)),
    ('fpn_lateral', dict(c_out=48)), ('fpn_lateral', dict(c_out=0)),
    ('fpn_lateral', dict(stride_w=2)), ('fpn_lateral', dict(stride_w=0)), ('fpn_lateral', dict(stride_c=-35)),
    ('fpn_lateral', dict(top_h=2)), ('fpn_lateral', dict(top_h=4)), ('fpn_lateral', dict(top_w=3)),
    ('fpn_lateral', dict(top_w=5)), ('fpn_lateral', dict(h=7)), ('fpn_lateral', dict(w=9)),
    ('fpn_lateral', dict(top_h=0)),
    ('fpn_lateral', dict(ld_y=255)), ('fpn_lateral', dict(ld_top=128)),
    ('fpn_lateral', dict(dtype=2)), ('fpn_lateral', dict(dtype=3)),
    ('fpn_lateral', dict(batch=0)), ('fpn_lateral', dict(h=0, top=None)), ('fpn_lateral', dict(weight=P + 8)),
    ('fpn_lateral', dict(batch=1 << 20, h=64, w=64, top=None)),
    ('fpn_pool', dict(src=None)), ('fpn_pool', dict(dst=None)),
    ('fpn_pool', dict(ld_src=56)), ('fpn_pool', dict(ld_dst=32)), ('fpn_pool', dict(ld_src=68)),
    ('fpn_pool', dict(C=60)), ('fpn_pool', dict(C=0)), ('fpn_pool', dict(dtype=2)),
    ('fpn_pool', dict(batch=0)), ('fpn_pool', dict(h=0)), ('fpn_pool', dict(w=0)), ('fpn_pool', dict(src=P + 4)),
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


@pytest.mark.parametrize('name,over', REFUSALS, ids=['%s-%s' % (n, sorted(o.items())) for n, o in REFUSALS])
def test_refused_by_message_before_any_launch(name, over):
    rc, msg = _call(name, **over)
    assert rc == -1, (rc, msg)
    assert msg.startswith(name + ':'), msg


def test_abi_revision_bindings_and_sources():
    import importlib.util
    import os
    _lib, lib = _load()
    assert _lib.ABI_REVISION >= 307 and lib.sfvos_version() >= 307
    for name, n_args in (('sfvos_fpn_lateral', 20), ('sfvos_fpn_pool', 10)):
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and len(_lib.SIGNATURES[name][1]) == n_args
    path = os.path.join(os.path.dirname(_lib.__file__), 'build.py')
    spec = importlib.util.spec_from_file_location('sfvos_build_for_fpn_test', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert 'fpn.hip' in mod.SOURCES


CH = (256, 512, 1024, 2048)
WANT = {}
for _i, _c in enumerate(CH):
    WANT['inner_blocks.%d.weight' % _i] = (256, _c, 1, 1)
    WANT['inner_blocks.%d.bias' % _i] = (256,)
    WANT['layer_blocks.%d.weight' % _i] = (256, 256, 3, 3)
    WANT['layer_blocks.%d.bias' % _i] = (256,)


def test_state_dict_surface_and_strict_loads():
    import fpn_ref as R
    import sfvos_amd
    from sfvos_amd import FeaturePyramidNetwork
    assert 'FeaturePyramidNetwork' in sfvos_amd.__all__
    fpn = FeaturePyramidNetwork()
    assert {k: tuple(v.shape) for k, v in fpn.state_dict().items()} == WANT
    ref = R.FeaturePyramidNetwork(CH, 256)
    assert [n for n, _ in fpn.named_parameters()] == [n for n, _ in ref.named_parameters()]
    assert all(float(c.bias.detach().abs().max()) == 0 for c in list(fpn.inner_blocks) + list(fpn.layer_blocks))
    bound = (6.0 / (1 + 1) / 256) ** 0.5       # kaiming_uniform_(a=1): sqrt(6 / ((1 + a^2) fan_in))
    w = fpn.inner_blocks[0].weight.detach()
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
    g = torch.Generator().manual_seed(3)
    ckpt = {'maskrcnn_model.backbone.fpn.' + k: torch.randn(s, generator=g) for k, s in WANT.items()}
    ckpt['maskrcnn_model.backbone.body.conv1.weight'] = torch.zeros(64, 3, 7, 7)
    prefix = 'maskrcnn_model.backbone.fpn.'
    fpn.load_state_dict({k[len(prefix):]: v for k, v in ckpt.items() if k.startswith(prefix)}, strict=True)
    for k in WANT:
        assert torch.equal(fpn.state_dict()[k], ckpt[prefix + k])
    # the newer spelling (Conv2dNormActivation wraps each conv: `.0.`)
    new = {k.replace('.weight', '.0.weight').replace('.bias', '.0.bias'): torch.randn(s, generator=g)
           for k, s in WANT.items()}
    fpn.load_state_dict(dict(new), strict=True)
    assert torch.equal(fpn.inner_blocks[2].weight, new['inner_blocks.2.0.weight'])
    assert torch.equal(fpn.layer_blocks[3].bias, new['layer_blocks.3.0.bias'])
    holder = torch.nn.Module()
    holder.fpn = FeaturePyramidNetwork()
    holder.load_state_dict({'fpn.' + k: v for k, v in new.items()}, strict=True)
    assert torch.equal(holder.fpn.layer_blocks[0].weight, new['layer_blocks.0.0.weight'])
    with pytest.raises(RuntimeError):
        fpn.load_state_dict({k: v for k, v in new.items() if k != 'layer_blocks.1.0.bias'}, strict=True)
    ref.load_state_dict(fpn.state_dict(), strict=True)
    with pytest.raises(ValueError):
        FeaturePyramidNetwork((48,), 256)
    with pytest.raises(ValueError):
        FeaturePyramidNetwork((64,), 288)
    with pytest.raises(ValueError):
        FeaturePyramidNetwork((64,), 64, precision='fp8')


def _maps(B=1, ch=(32, 64), shapes=((5, 7), (3, 4)), **kw):
    return OrderedDict((str(l), torch.zeros(B, c, h, w, **kw)) for l, (c, (h, w)) in enumerate(zip(ch, shapes)))


def test_forward_refuses_cpu_tensors_and_gradients():
    from sfvos_amd import FeaturePyramidNetwork
    fpn = FeaturePyramidNetwork((32, 64), 64)
    with pytest.raises(RuntimeError, match='inference only'):      # the parameters require grad
        fpn(_maps())
    with torch.no_grad():
        for call in (fpn, fpn.forward_pyramid):
            with pytest.raises(RuntimeError, match='no CPU fallback'):
                call(_maps())
    for p in fpn.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fpn(_maps())
    with pytest.raises(RuntimeError, match='inference only'):      # an input that requires grad
        fpn(_maps(requires_grad=True))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='maps for'):
            fpn(OrderedDict(list(_maps().items())[:1]))


def test_write_frames_refuses_unsupported_clips():
    """Every refusal comes before the first launch.  The device check (no CPU fallback) comes first of all, so on a
    machine without a GPU the checks are reached through a stand-in for it."""
    from sfvos_amd import FeaturePyramidNetwork, PackedClip
    from sfvos_amd import fpn as F
    fpn = FeaturePyramidNetwork((32, 64), 64, precision='bf16')
    shapes = [(5, 7), (3, 4), (2, 2)]
    M = sum(h * w for h, w in shapes)
    with torch.no_grad():
        seq = PackedClip(torch.zeros(4 * M, 64, dtype=torch.bfloat16), shapes, 1, 4)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            fpn.write_frames(_maps(2), seq, 0)
        real, F._check_gpu = F._check_gpu, lambda t, what: None
        try:
            bad = [
                (PackedClip(torch.zeros(2, 4 * M, 32, dtype=torch.bfloat16), shapes, 1, 4), 0, 'layout'),
                (PackedClip(torch.zeros(1, 4 * M, 64, dtype=torch.uint8), shapes, 1, 4), 0, 'layout'),
                (PackedClip(torch.zeros(2 * 4 * M, 64, dtype=torch.bfloat16), shapes, 2, 4), 0, 'B = 1'),
                (PackedClip(torch.zeros(4 * M, 64, dtype=torch.bfloat16), shapes, 1, 4, pad=(1, 0)), 0, 'B = 1'),
                (PackedClip(torch.zeros(4 * M, 64, dtype=torch.float32), shapes, 1, 4), 0, 'must hold'),
                (PackedClip(torch.zeros(4 * M, 96, dtype=torch.bfloat16), shapes, 1, 4), 0, 'must hold'),
                (PackedClip(torch.zeros(4 * M, 128, dtype=torch.bfloat16)[:, :64], shapes, 1, 4), 0, 'must hold'),
                (PackedClip(torch.zeros(4 * (M - 4 + 6), 64, dtype=torch.bfloat16), [(5, 7), (3, 4), (2, 3)], 1, 4), 0,
                 'levels'),
                (PackedClip(torch.zeros(4 * (M - 4), 64, dtype=torch.bfloat16), shapes[:2], 1, 4), 0, 'levels'),
                (seq, 3, 'outside the sequence'), (seq, -1, 'outside the sequence'),
            ]
            for clip, first, match in bad:
                with pytest.raises(RuntimeError, match=match):
                    fpn.write_frames(_maps(2), clip, first)
        finally:
            F._check_gpu = real
