"""CPU (no GPU): the host side of the region-proposal entry points (csrc/rpn.hip) and of sfvos_amd.rpn -- the calls they
refuse before any kernel is launched (a refused call returns -1 and leaves a message that starts with the entry point's
name; a call that got past the checks would return -2 without a device), the workspace query, the ABI revision, and the
state-dict surface of RPNHead (torchvision's names; the newer `conv.0.0.*` spelling loads too)."""
import ctypes

import pytest
import torch

P = 1 << 40                   # never dereferenced


def _load():
    from sfvos_amd import _lib
    return _lib, _lib.load()


def _pyr(_lib, n=4, **kw):
    m = min(max(n, 1), 8)     # the struct holds 8 levels; n_levels itself may lie outside
    p = _lib.make_pyramid([(24, 40), (12, 20), (6, 10), (3, 5)][:min(m, 4)] + [(2, 2)] * max(0, m - 4))
    p.n_levels = n
    for k, v in kw.items():
        getattr(p, k)[1] = v
    return ctypes.byref(p)


# entry point -> (argument names, defaults of a call that passes every check); pointers default to P, the stream to NULL
ENTRY = {
    'rpn_select': ('objectness pyr batch A k counts index stream', dict(batch=2, A=3, k=1000)),
    'rpn_decode': ('objectness deltas counts index pyr batch A k base th tw sizes clip min_size score_thresh boxes logits '
                   'scores valid stream',
                   dict(batch=2, A=3, k=1000, th=96, tw=160, clip=4.135, min_size=1e-3, score_thresh=0.0)),
    'rpn_nms': ('boxes logits scores valid counts n_levels batch k nms_thresh post ws out_boxes out_scores out_index '
                'out_count stream', dict(n_levels=4, batch=2, k=1000, nms_thresh=0.7, post=1000)),
}

REFUSALS = [
    ('rpn_select', dict(objectness=None)), ('rpn_select', dict(counts=None)), ('rpn_select', dict(index=None)),
    ('rpn_select', dict(pyr=None)), ('rpn_select', dict(k=0)), ('rpn_select', dict(k=4097)),
    ('rpn_select', dict(A=0)), ('rpn_select', dict(A=9)), ('rpn_select', dict(batch=0)),
    ('rpn_select', dict(pyr=('levels', 9))), ('rpn_select', dict(pyr=('levels', 0))),
    ('rpn_select', dict(pyr=('h', 0))),
    ('rpn_decode', dict(deltas=None)), ('rpn_decode', dict(base=None)), ('rpn_decode', dict(sizes=None)),
    ('rpn_decode', dict(valid=None)), ('rpn_decode', dict(pyr=None)), ('rpn_decode', dict(k=0)),
    ('rpn_decode', dict(k=4097)), ('rpn_decode', dict(A=0)), ('rpn_decode', dict(A=9)),
    ('rpn_decode', dict(pyr=('levels', 9))), ('rpn_decode', dict(th=0)), ('rpn_decode', dict(tw=0)),
    ('rpn_nms', dict(boxes=None)), ('rpn_nms', dict(ws=None)), ('rpn_nms', dict(out_count=None)),
    ('rpn_nms', dict(k=0)), ('rpn_nms', dict(k=4097)), ('rpn_nms', dict(n_levels=9)), ('rpn_nms', dict(n_levels=0)),
    ('rpn_nms', dict(batch=0)), ('rpn_nms', dict(post=0)),
]


def _call(name, **over):
    _lib, lib = _load()
    names, defaults = ENTRY[name]
    args = []
    for a in names.split():
        v = over[a] if a in over else defaults.get(a, None if a == 'stream' else P)
        if a == 'pyr':
            if v == P:
                v = _pyr(_lib)
            elif isinstance(v, tuple):
                v = _pyr(_lib, v[1]) if v[0] == 'levels' else _pyr(_lib, 4, **{v[0]: v[1]})
        args.append(v)
    rc = getattr(lib, 'sfvos_' + name)(*args)
    msg = lib.sfvos_last_error()
    return rc, (msg.decode() if msg else '')


@pytest.mark.parametrize('name,over', REFUSALS, ids=['%s-%s' % (n, sorted(o.items())) for n, o in REFUSALS])
def test_refused_by_message_before_any_launch(name, over):
    rc, msg = _call(name, **over)
    assert rc == -1, (rc, msg)
    assert msg.startswith(name + ':'), msg


def test_workspace_query():
    _, lib = _load()
    q = lib.sfvos_rpn_workspace_bytes
    for args in [(4, 2, 0), (4, 2, 4097), (0, 2, 1000), (9, 2, 1000), (4, 0, 1000)]:
        assert q(*args) == 0, args
    # masks (segments x 64 ceil(k / 64) rows x ceil(k / 64) words) + kept list + its logits + kept counts
    k, segs = 1000, 8
    nw = 16
    assert q(4, 2, k) == segs * 64 * nw * nw * 8 + 2 * segs * k * 4 + 32
    assert q(5, 1, 2000) >= 5 * 2000 * 32 * 8
    assert q(8, 1, 4096) > 0


def test_abi_revision_and_bindings():
    _lib, lib = _load()
    assert _lib.ABI_REVISION >= 304 and lib.sfvos_version() >= 304
    for name in ('sfvos_rpn_workspace_bytes', 'sfvos_rpn_select', 'sfvos_rpn_decode', 'sfvos_rpn_nms'):
        assert name in _lib.SIGNATURES, name


WANT = {'conv.weight': (256, 256, 3, 3), 'conv.bias': (256,), 'cls_logits.weight': (3, 256, 1, 1),
        'cls_logits.bias': (3,), 'bbox_pred.weight': (12, 256, 1, 1), 'bbox_pred.bias': (12,)}


def test_state_dict_surface_and_strict_loads():
    import rpn_ref as R
    from sfvos_amd import RegionProposalNetwork, RPNHead
    h = RPNHead(256, 3)
    assert {k: tuple(v.shape) for k, v in h.state_dict().items()} == WANT
    assert [n for n, _ in h.named_parameters()] == [n for n, _ in R.RPNHead(256, 3).named_parameters()]
    g = torch.Generator().manual_seed(2)
    ckpt = {'maskrcnn_model.rpn.head.' + k: torch.randn(s, generator=g) for k, s in WANT.items()}
    ckpt['maskrcnn_model.roi_heads.box_head.fc7.bias'] = torch.zeros(1024)
    prefix = 'maskrcnn_model.rpn.'
    rpn = RegionProposalNetwork()
    rpn.load_state_dict({k[len(prefix):]: v for k, v in ckpt.items() if k.startswith(prefix)}, strict=True)
    for k, s in WANT.items():
        assert torch.equal(rpn.state_dict()['head.' + k], ckpt[prefix + 'head.' + k])
    # the newer spelling of the first conv
    new = {k.replace('conv.', 'conv.0.0.') if k.startswith('conv.') else k: torch.randn(s, generator=g)
           for k, s in WANT.items()}
    h.load_state_dict(dict(new), strict=True)
    assert torch.equal(h.conv.weight, new['conv.0.0.weight']) and torch.equal(h.conv.bias, new['conv.0.0.bias'])
    rpn.load_state_dict({'head.' + k: v for k, v in new.items()}, strict=True)
    assert torch.equal(rpn.head.conv.weight, new['conv.0.0.weight'])
    with pytest.raises(RuntimeError):
        h.load_state_dict({k: v for k, v in new.items() if k != 'bbox_pred.bias'}, strict=True)
    R.RPNHead(256, 3).load_state_dict(h.state_dict(), strict=True)


def test_modes_and_host_side_refusals():
    from sfvos_amd import AnchorGenerator, PackedClip, RegionProposalNetwork, RPNHead
    rpn = RegionProposalNetwork()
    assert rpn.training and (rpn.pre_nms_top_n(), rpn.post_nms_top_n()) == (2000, 2000)
    rpn.eval()
    assert (rpn.pre_nms_top_n(), rpn.post_nms_top_n()) == (1000, 1000)
    rpn = RegionProposalNetwork(pre_nms_top_n=dict(training=50, testing=30), post_nms_top_n=dict(training=30, testing=50))
    assert (rpn.pre_nms_top_n(), rpn.post_nms_top_n()) == (50, 30)
    assert (rpn.eval().pre_nms_top_n(), rpn.post_nms_top_n()) == (30, 50)
    with pytest.raises(ValueError):
        RPNHead(256, 9)
    with pytest.raises(ValueError):
        RegionProposalNetwork(AnchorGenerator(((32, 64),), ((1.0,),)), RPNHead(256, 3))
    feats = {'0': torch.zeros(1, 256, 4, 4)}
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            rpn.propose(feats, [(16, 16)], (16, 16))
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            rpn.propose_padded(feats, [(16, 16)], (16, 16))
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            rpn.head([feats['0']])
        clip = PackedClip(torch.zeros(16, 256), [(4, 4)], 1, 1)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            rpn.propose_packed(clip, None, [(16, 16)], (16, 16))
