"""CPU (no GPU): the host side of the transform's entry points (csrc/transform.hip) and of sfvos_amd.transform -- the calls
they refuse before any kernel is launched (a refused call returns -1 and leaves a message that starts with the entry
point's name), the ABI revision and bindings, the host-side refusals of GeneralizedRCNNTransform, and the state-dict
surface of MaskRCNN (torchvision's key set, one strict load of a full checkpoint)."""
import pytest
import torch

P = 1 << 40                   # never dereferenced (16-byte aligned)

# entry point -> (argument names, defaults of a call that passes every check); pointers default to P, the stream to NULL
ENTRY = {
    'transform_image': ('src src_dtype stride_b stride_c stride_h stride_w batch h w mean0 mean1 mean2 std0 std1 std2 dst '
                        'dst_stride_b dst_stride_c dst_stride_h oh ow Hp Wp stream',
                        dict(src_dtype=0, stride_b=3 * 37 * 53, stride_c=37 * 53, stride_h=53, stride_w=1, batch=2, h=37,
                             w=53, mean0=0.485, mean1=0.456, mean2=0.406, std0=0.229, std1=0.224, std2=0.225,
                             dst_stride_b=3 * 64 * 96, dst_stride_c=64 * 96, dst_stride_h=96, oh=58, ow=83, Hp=64, Wp=96)),
    'transform_masks': ('src G h w dst oh ow stream', dict(G=3, h=37, w=53, oh=58, ow=83)),
}

REFUSALS = [
    ('transform_image', dict(src=None)), ('transform_image', dict(dst=None)),
    ('transform_image', dict(dst=P + 4)), ('transform_image', dict(dst=P + 8)), ('transform_image', dict(src=P + 2)),
    ('transform_image', dict(stride_w=2)), ('transform_image', dict(stride_w=0)), ('transform_image', dict(stride_w=3)),
    ('transform_image', dict(stride_b=-1)), ('transform_image', dict(stride_c=-37 * 53)),
    ('transform_image', dict(stride_h=-53)), ('transform_image', dict(src_dtype=3, stride_w=-3)),
    ('transform_image', dict(batch=0)), ('transform_image', dict(h=0)), ('transform_image', dict(w=0)),
    ('transform_image', dict(h=-5)), ('transform_image', dict(oh=0)), ('transform_image', dict(ow=0)),
    ('transform_image', dict(Hp=0)), ('transform_image', dict(Wp=0)), ('transform_image', dict(ow=-1)),
    ('transform_image', dict(oh=65)), ('transform_image', dict(ow=97)), ('transform_image', dict(Hp=57)),
    ('transform_image', dict(Wp=82, dst_stride_h=96)),
    ('transform_image', dict(src_dtype=1)), ('transform_image', dict(src_dtype=2)), ('transform_image', dict(src_dtype=4)),
    ('transform_image', dict(src_dtype=-1)),
    ('transform_image', dict(std0=0.0)), ('transform_image', dict(std1=-0.224)), ('transform_image', dict(std2=float('nan'))),
    ('transform_image', dict(std2=-0.0)), ('transform_image', dict(mean1=float('nan'))),
    ('transform_image', dict(dst_stride_h=92)), ('transform_image', dict(dst_stride_h=98)),
    ('transform_image', dict(dst_stride_c=64 * 96 + 2)), ('transform_image', dict(dst_stride_b=3 * 64 * 96 + 1)),
    ('transform_image', dict(dst_stride_b=-4)), ('transform_image', dict(dst_stride_c=-4)),
    ('transform_image', dict(Hp=1 << 20, Wp=1 << 20, dst_stride_h=1 << 20)),
    ('transform_masks', dict(G=-1)), ('transform_masks', dict(h=0)), ('transform_masks', dict(w=0)),
    ('transform_masks', dict(oh=0)), ('transform_masks', dict(ow=-3)), ('transform_masks', dict(src=None)),
    ('transform_masks', dict(dst=None)), ('transform_masks', dict(oh=1 << 16, ow=1 << 16)),
    ('transform_masks', dict(G=0, h=0)),
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


def test_no_masks_is_a_no_op():
    assert _call('transform_masks', G=0)[0] == 0
    assert _call('transform_masks', G=0, src=None, dst=None)[0] == 0


def test_abi_revision_bindings_and_sources():
    import importlib.util
    import os
    _lib, lib = _load()
    assert _lib.ABI_REVISION >= 309 and lib.sfvos_version() >= 309
    assert (_lib.F32, _lib.U8) == (0, 3)
    for name, n_args in (('sfvos_transform_image', 24), ('sfvos_transform_masks', 8)):
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and len(_lib.SIGNATURES[name][1]) == n_args
        assert len(ENTRY[name[len('sfvos_'):]][0].split()) == n_args
    assert len(_lib.SIGNATURES) >= 96
    path = os.path.join(os.path.dirname(_lib.__file__), 'build.py')
    spec = importlib.util.spec_from_file_location('sfvos_build_for_transform_test', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert 'transform.hip' in mod.SOURCES


def test_exports():
    import sfvos_amd
    assert {'GeneralizedRCNNTransform', 'ImageList', 'MaskRCNN'} <= set(sfvos_amd.__all__)
    for name in ('GeneralizedRCNNTransform', 'ImageList', 'MaskRCNN'):
        assert hasattr(sfvos_amd, name)
    assert len(set(sfvos_amd.__all__)) == len(sfvos_amd.__all__)


def test_transform_refuses_cpu_tensors_and_gradients():
    from sfvos_amd import GeneralizedRCNNTransform, ImageList
    from sfvos_amd.transform import resize_masks
    t = GeneralizedRCNNTransform(min_size=48, max_size=80).eval()
    assert list(t.parameters()) == [] and list(t.buffers()) == [] and t.state_dict() == {}
    img = torch.rand(3, 20, 30)
    for images in ([img], [img, torch.rand(3, 25, 18)], torch.rand(2, 3, 20, 30),
                   torch.zeros(2, 20, 30, 3, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            t(images)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        resize_masks(torch.zeros(2, 20, 30, dtype=torch.uint8), (48, 72))
    with pytest.raises(RuntimeError, match='no backward'):
        t([torch.rand(3, 20, 30, requires_grad=True)])
    with pytest.raises(RuntimeError, match='no backward'):
        t(torch.rand(1, 3, 20, 30, requires_grad=True))
    for bad in ([], [torch.rand(20, 30)], [torch.rand(1, 20, 30)], [torch.zeros(3, 20, 30, dtype=torch.uint8)],
                torch.rand(3, 20, 30), torch.rand(2, 1, 20, 30), torch.zeros(2, 3, 20, 30, dtype=torch.uint8),
                torch.zeros(2, 20, 30, 3, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match='GeneralizedRCNNTransform'):
            t(bad)
    with pytest.raises(RuntimeError, match='targets'):
        t([img], [{}, {}])
    inputs = torch.rand(2, 3, 20, 30)
    keep = inputs.clone()
    with pytest.raises(RuntimeError):
        t(inputs)
    assert torch.equal(inputs, keep)
    lst = ImageList(torch.zeros(2, 3, 64, 96), [(48, 72), (48, 72)])
    assert lst.image_sizes == [(48, 72), (48, 72)] and lst.to('cpu').tensors.shape == (2, 3, 64, 96)
    assert lst.to('cpu').image_sizes == lst.image_sizes


def test_targets_without_boxes_pass_through():
    """The reference pads its target list with {} for the frames without objects (model.py:303-312)."""
    from sfvos_amd import GeneralizedRCNNTransform
    t = GeneralizedRCNNTransform(min_size=48, max_size=80)
    empty = {}
    assert t._resize_target(empty, (20, 30), (48, 72)) is empty and empty == {}
    labels = torch.tensor([1])
    only = {'labels': labels, 'masks': torch.zeros(1, 20, 30, dtype=torch.uint8)}
    out = t._resize_target(only, (20, 30), (48, 72))
    assert out is only and out['labels'] is labels and out['masks'].shape == (1, 20, 30)
    assert t._resize_target(None, (20, 30), (48, 72)) is None
    # a target with boxes needs the GPU, as resize_boxes does
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        t._resize_target({'boxes': torch.zeros(1, 4)}, (20, 30), (48, 72))
    # postprocess in training mode is the identity
    result = [{'boxes': torch.zeros(1, 4)}]
    assert t.train().postprocess(result, [(48, 72)], [(20, 30)]) is result
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        t.eval().postprocess(result, [(48, 72)], [(20, 30)])


@pytest.fixture(scope='module')
def model():
    from sfvos_amd import MaskRCNN
    torch.manual_seed(7)
    return MaskRCNN()


def test_maskrcnn_surface(model):
    from sfvos_amd import (BackboneWithFPN, GeneralizedRCNNTransform, MaskRCNN, RegionProposalNetwork, RoIHeads)
    m = model
    assert isinstance(m.transform, GeneralizedRCNNTransform) and isinstance(m.backbone, BackboneWithFPN)
    assert isinstance(m.rpn, RegionProposalNetwork) and isinstance(m.roi_heads, RoIHeads)
    assert [n for n, _ in m.named_children()] == ['transform', 'backbone', 'rpn', 'roi_heads']
    assert m.transform.min_size == (800,) and m.transform.max_size == 1333 and m.precision == 'fp32'
    assert m.roi_heads.paste_masks is False and RoIHeads().paste_masks is True
    want = ['backbone.' + k for k in m.backbone.state_dict()] + ['rpn.' + k for k in m.rpn.state_dict()] + \
        ['roi_heads.' + k for k in m.roi_heads.state_dict()]
    assert list(m.state_dict().keys()) == want
    keys = set(want)
    # torchvision's prefixes, and the parts built on their own have the same keys
    assert {k.split('.')[0] for k in keys} == {'backbone', 'rpn', 'roi_heads'}
    assert {k.split('.')[1] for k in keys if k.startswith('backbone.')} == {'body', 'fpn'}
    assert {k for k in keys if k.startswith('rpn.')} == {'rpn.head.' + n + s for n in ('conv', 'cls_logits', 'bbox_pred')
                                                         for s in ('.weight', '.bias')}
    assert {k[len('roi_heads.'):] for k in keys if k.startswith('roi_heads.')} == set(RoIHeads().state_dict().keys())
    assert {k[len('rpn.'):] for k in keys if k.startswith('rpn.')} == set(RegionProposalNetwork().state_dict().keys())
    assert 'backbone.body.layer4.2.bn3.running_var' in keys and 'backbone.fpn.layer_blocks.3.bias' in keys
    assert 'roi_heads.mask_predictor.mask_fcn_logits.weight' in keys and 'roi_heads.box_head.fc6.weight' in keys
    # keyword arguments reach the parts; an unknown one is refused
    small = dict(min_size=64, max_size=96, rpn_pre_nms_top_n_test=50, rpn_post_nms_top_n_test=20, box_detections_per_img=7,
                 box_score_thresh=0.0, rpn_batch_size_per_image=64, box_batch_size_per_image=32)
    with pytest.raises(TypeError, match='nonsense'):
        MaskRCNN(nonsense=1, **small)
    with pytest.raises(ValueError):
        MaskRCNN(precision='fp8')


def test_full_checkpoint_loads_strictly(model):
    m = model
    g = torch.Generator().manual_seed(11)
    ckpt = {}
    for k, v in m.state_dict().items():
        ckpt[k] = torch.rand(v.shape, generator=g) + 0.5
        if k.endswith('running_var'):
            ckpt[k.replace('running_var', 'num_batches_tracked')] = torch.tensor(0)
    assert sum(k.endswith('num_batches_tracked') for k in ckpt) == 53
    m.load_state_dict(dict(ckpt), strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, ckpt[k]), k
    assert not any(k.endswith('num_batches_tracked') for k in m.state_dict())
    m.roi_heads.detections_per_img = 10           # model.py:187
    assert m.roi_heads._branches()[0].detections_per_img == 10
    missing = {k: v for k, v in ckpt.items() if k != 'rpn.head.cls_logits.bias'}
    with pytest.raises(RuntimeError, match='rpn.head.cls_logits.bias'):
        m.load_state_dict(missing, strict=True)
    extra = dict(ckpt, **{'roi_heads.keypoint_head.weight': torch.zeros(1)})
    with pytest.raises(RuntimeError, match='keypoint_head'):
        m.load_state_dict(extra, strict=True)
    with pytest.raises(RuntimeError, match='transform'):
        m.load_state_dict(dict(ckpt, **{'transform.image_mean': torch.zeros(3)}), strict=True)


def test_maskrcnn_forward_refusals(model):
    m = model
    img = [torch.rand(3, 20, 30)]
    with pytest.raises(ValueError, match='targets should be passed'):
        m.train()(img)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.eval()(img)
