"""CPU (no GPU): the host side of the roi_heads training-target entry points (csrc/roi_targets.hip) and of
sfvos_amd.roi_heads -- the calls they refuse before any kernel is launched (a refused call returns -1 and leaves a message
that starts with the entry point's name; a call that got past the checks would return -2 without a device), the workspace
query, the ABI revision, and the state-dict surface of RoIHeads (torchvision's names: the `roi_heads.*` slice of a
reference checkpoint loads with strict=True)."""
import pytest
import torch

P = 1 << 40                   # never dereferenced

# entry point -> (argument names, defaults of a call that passes every check); pointers default to P, the stream to NULL
ENTRY = {
    'roi_match': ('proposals n_p gt_boxes gt_labels G high low matched labels max_iou stream',
                  dict(n_p=2000, G=3, high=0.5, low=0.5)),
    'roi_sample': ('labels matched keys proposals n_p gt_boxes G batch fraction wx wy ww wh ws counts index out_boxes '
                   'out_labels out_matched targets pos_slot stream',
                   dict(n_p=2000, G=3, batch=512, fraction=0.25, wx=10.0, wy=10.0, ww=5.0, wh=5.0)),
    'mask_targets': ('masks u8 G H W boxes matched P M targets stream', dict(u8=1, G=3, H=749, W=1333, P=128, M=28)),
}

REFUSALS = [
    ('roi_match', dict(n_p=8190)), ('roi_match', dict(n_p=8193, G=0)), ('roi_match', dict(G=1025)),
    ('roi_match', dict(n_p=-1)), ('roi_match', dict(G=-1)), ('roi_match', dict(proposals=None)),
    ('roi_match', dict(gt_boxes=None)), ('roi_match', dict(gt_labels=None)), ('roi_match', dict(matched=None)),
    ('roi_match', dict(labels=None)),
    ('roi_sample', dict(n_p=8190)), ('roi_sample', dict(G=1025)), ('roi_sample', dict(n_p=-1)),
    ('roi_sample', dict(batch=0)), ('roi_sample', dict(batch=4097)), ('roi_sample', dict(fraction=-0.01)),
    ('roi_sample', dict(fraction=1.01)), ('roi_sample', dict(fraction=float('nan'))), ('roi_sample', dict(wx=0.0)),
    ('roi_sample', dict(labels=None)), ('roi_sample', dict(matched=None)), ('roi_sample', dict(keys=None)),
    ('roi_sample', dict(proposals=None)), ('roi_sample', dict(gt_boxes=None)), ('roi_sample', dict(ws=None)),
    ('roi_sample', dict(counts=None)), ('roi_sample', dict(index=None)), ('roi_sample', dict(out_boxes=None)),
    ('roi_sample', dict(out_labels=None)), ('roi_sample', dict(out_matched=None)), ('roi_sample', dict(targets=None)),
    ('roi_sample', dict(pos_slot=None)),
    ('mask_targets', dict(M=0)), ('mask_targets', dict(M=65)), ('mask_targets', dict(H=0)), ('mask_targets', dict(W=0)),
    ('mask_targets', dict(P=-1)), ('mask_targets', dict(masks=None)), ('mask_targets', dict(boxes=None)),
    ('mask_targets', dict(matched=None)), ('mask_targets', dict(targets=None)),
]


def _load():
    from sfvos_amd import _lib
    return _lib, _lib.load()


def _call(name, **over):
    _lib, lib = _load()
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


def test_calls_without_work_return_ok_and_launch_nothing():
    assert _call('mask_targets', P=0, boxes=None, matched=None, targets=None, masks=None)[0] == 0
    assert _call('roi_match', n_p=0, G=0, proposals=None, gt_boxes=None, gt_labels=None)[0] == 0


def test_workspace_query():
    _, lib = _load()
    q = lib.sfvos_roi_sample_workspace_bytes
    for n in (-1, 8193, 1 << 30):
        assert q(n) == 0, n
    assert q(2003) == 4 * 2003 + 4 and q(8192) == 4 * 8192 and q(1) == 16 and q(0) == 16     # one rank per candidate


def test_abi_revision_and_bindings():
    _lib, lib = _load()
    assert _lib.ABI_REVISION >= 305 and lib.sfvos_version() >= 305
    for name in ('sfvos_roi_match', 'sfvos_roi_sample_workspace_bytes', 'sfvos_roi_sample', 'sfvos_mask_targets'):
        assert name in _lib.SIGNATURES, name


WANT = {'box_head.fc6.weight': (1024, 12544), 'box_head.fc6.bias': (1024,), 'box_head.fc7.weight': (1024, 1024),
        'box_head.fc7.bias': (1024,), 'box_predictor.cls_score.weight': (2, 1024), 'box_predictor.cls_score.bias': (2,),
        'box_predictor.bbox_pred.weight': (8, 1024), 'box_predictor.bbox_pred.bias': (8,),
        'mask_predictor.conv5_mask.weight': (256, 256, 2, 2), 'mask_predictor.conv5_mask.bias': (256,),
        'mask_predictor.mask_fcn_logits.weight': (2, 256, 1, 1), 'mask_predictor.mask_fcn_logits.bias': (2,)}
for _i in range(1, 5):
    WANT['mask_head.mask_fcn%d.weight' % _i] = (256, 256, 3, 3)
    WANT['mask_head.mask_fcn%d.bias' % _i] = (256,)


def test_roi_heads_state_dict_surface_and_strict_loads():
    from sfvos_amd import BoxBranch, MaskBranch, RoIHeads
    h = RoIHeads()
    assert {k: tuple(v.shape) for k, v in h.state_dict().items()} == WANT
    assert len(list(h.parameters())) == 20 and h.training
    for name in ('box_roi_pool', 'box_head', 'box_predictor', 'mask_roi_pool', 'mask_head', 'mask_predictor'):
        assert isinstance(getattr(h, name), torch.nn.Module), name
    assert h.box_roi_pool.output_size == (7, 7) and h.mask_roi_pool.output_size == (14, 14)
    torch.manual_seed(3)
    box, mask = BoxBranch(2), MaskBranch(256, 2)
    sd = dict(box.state_dict())
    sd.update(mask.state_dict())
    h.load_state_dict(sd, strict=True)
    for k, v in sd.items():
        assert torch.equal(h.state_dict()[k], v), k
    # the slice of a reference checkpoint
    prefix = 'maskrcnn_model.roi_heads.'
    ckpt = {prefix + k: v + 1 for k, v in sd.items()}
    ckpt['maskrcnn_model.rpn.head.conv.bias'] = torch.zeros(256)
    h.load_state_dict({k[len(prefix):]: v for k, v in ckpt.items() if k.startswith(prefix)}, strict=True)
    assert torch.equal(h.box_head.fc7.bias, sd['box_head.fc7.bias'] + 1)
    with pytest.raises(RuntimeError):
        h.load_state_dict({k: v for k, v in sd.items() if k != 'mask_head.mask_fcn3.bias'}, strict=True)
    # the branches whose code runs see the same parameters
    assert h._box.box_head.fc6.weight is h.box_head.fc6.weight
    assert h._mask.mask_predictor.conv5_mask.weight is h.mask_predictor.conv5_mask.weight


def test_the_unregistered_branches_own_nothing_outside_the_shared_modules():
    """RoIHeads keeps its BoxBranch and MaskBranch outside the module registry: everything they hold that .to(), .eval()
    or a state dict must reach has to live in the six modules RoIHeads registers."""
    from sfvos_amd import RoIHeads
    h = RoIHeads()
    shared = {id(t) for t in list(h.parameters()) + list(h.buffers())}
    modules = {id(m) for m in h.modules()}
    for branch in (h._box, h._mask):
        assert not list(branch.parameters(recurse=False)) and not list(branch.buffers(recurse=False))
        assert {id(t) for t in list(branch.parameters()) + list(branch.buffers())} <= shared
        assert all(id(c) in modules for c in branch.children()), [n for n, _ in branch.named_children()]
    assert len(list(h.buffers())) == 0
    h.eval()
    assert all(not c.training for b in (h._box, h._mask) for c in b.children())
    h.train()
    assert all(c.training for b in (h._box, h._mask) for c in b.children())
    import inspect
    from sfvos_amd import box_head, mask_head
    for cls in (box_head.BoxBranch, mask_head.MaskBranch):
        assert 'self.training' not in inspect.getsource(cls), cls.__name__


def test_roi_heads_attributes_are_read_at_call_time():
    from sfvos_amd import RoIHeads
    h = RoIHeads(box_detections_per_img=100)
    assert (h.score_thresh, h.nms_thresh, h.detections_per_img) == (0.05, 0.5, 100)
    assert (h.batch_size_per_image, h.positive_fraction, h.fg_iou_thresh, h.bg_iou_thresh) == (512, 0.25, 0.5, 0.5)
    h.detections_per_img = 10      # model.py:187
    h.score_thresh, h.nms_thresh = 0.2, 0.3
    box, _ = h._branches()
    assert (box.detections_per_img, box.score_thresh, box.nms_thresh) == (10, 0.2, 0.3)


def test_targets_are_checked_as_torchvision_checks_them():
    from sfvos_amd import RoIHeads, select_training_samples
    props = [torch.zeros(4, 4)]
    boxes, labels = torch.zeros(1, 4), torch.ones(1, dtype=torch.int64)
    with pytest.raises(ValueError, match='should not be None'):
        select_training_samples(props, None)
    with pytest.raises(ValueError, match='boxes'):
        select_training_samples(props, [{'labels': labels}])
    with pytest.raises(ValueError, match='labels'):
        select_training_samples(props, [{'boxes': boxes}])
    with pytest.raises(TypeError, match='float'):
        select_training_samples(props, [{'boxes': boxes.long(), 'labels': labels}])
    with pytest.raises(TypeError, match='int64'):
        select_training_samples(props, [{'boxes': boxes, 'labels': labels.int()}])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        select_training_samples(props, [{'boxes': boxes, 'labels': labels}])
    h = RoIHeads()
    with pytest.raises(ValueError, match='should not be None'):
        h({}, props, [(8, 8)])
    with pytest.raises(ValueError, match='masks'):
        h({}, props, [(8, 8)], [{'boxes': boxes, 'labels': labels}])
