"""CPU (no GPU): the host side of the RPN training entry points (csrc/rpn_targets.hip) and of
sfvos_amd.RegionProposalNetwork's training call -- the calls they refuse before any kernel is launched (a refused call
returns -1 and leaves a message that starts with the entry point's name), the workspace query, the ABI revision and the
bindings, the constructor keywords and "no CPU fallback" for the new methods."""
import ctypes
import types

import pytest
import torch

P = 1 << 40                   # never dereferenced
N_SMALL = 3825                # anchors of the pyramid below with A = 3


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
    'rpn_match': ('pyr A base th tw gt G high low lowq ws matched labels max_iou stream',
                  dict(A=3, th=96, tw=160, G=3, high=0.7, low=0.3, lowq=1)),
    'rpn_sample': ('labels matched keys N pyr A base th tw gt G batch fraction ws counts index targets stream',
                   dict(N=N_SMALL, A=3, th=96, tw=160, G=3, batch=256, fraction=0.5)),
    'rpn_loss': ('objectness deltas pyr images A index counts targets batch beta per_sample out stream',
                 dict(images=2, A=3, batch=256, beta=1.0 / 9)),
}

NAN = float('nan')
REFUSALS = [
    ('rpn_match', dict(pyr=None)), ('rpn_match', dict(pyr=('levels', 0))), ('rpn_match', dict(pyr=('levels', 9))),
    ('rpn_match', dict(pyr=('h', 0))), ('rpn_match', dict(pyr=('h', 1 << 23))), ('rpn_match', dict(A=0)),
    ('rpn_match', dict(A=9)), ('rpn_match', dict(th=0)), ('rpn_match', dict(tw=0)), ('rpn_match', dict(G=-1)),
    ('rpn_match', dict(G=1025)), ('rpn_match', dict(high=1.5)), ('rpn_match', dict(high=-0.1)),
    ('rpn_match', dict(low=1.5)), ('rpn_match', dict(low=NAN)), ('rpn_match', dict(base=None)),
    ('rpn_match', dict(gt=None)), ('rpn_match', dict(ws=None)), ('rpn_match', dict(matched=None)),
    ('rpn_match', dict(labels=None)),
    ('rpn_sample', dict(pyr=None)), ('rpn_sample', dict(pyr=('levels', 9))), ('rpn_sample', dict(A=0)),
    ('rpn_sample', dict(A=9)), ('rpn_sample', dict(N=N_SMALL - 1)), ('rpn_sample', dict(G=1025)),
    ('rpn_sample', dict(batch=0)), ('rpn_sample', dict(batch=4097)), ('rpn_sample', dict(fraction=-0.1)),
    ('rpn_sample', dict(fraction=1.1)), ('rpn_sample', dict(fraction=NAN)), ('rpn_sample', dict(th=0)),
    ('rpn_sample', dict(labels=None)), ('rpn_sample', dict(matched=None)), ('rpn_sample', dict(keys=None)),
    ('rpn_sample', dict(base=None)), ('rpn_sample', dict(gt=None)), ('rpn_sample', dict(ws=None)),
    ('rpn_sample', dict(counts=None)), ('rpn_sample', dict(index=None)), ('rpn_sample', dict(targets=None)),
    ('rpn_sample', dict(pyr=('h', 1 << 23))),
    ('rpn_loss', dict(pyr=None)), ('rpn_loss', dict(pyr=('levels', 0))), ('rpn_loss', dict(A=9)),
    ('rpn_loss', dict(images=0)), ('rpn_loss', dict(batch=0)), ('rpn_loss', dict(batch=4097)),
    ('rpn_loss', dict(beta=-1e-3)), ('rpn_loss', dict(beta=NAN)), ('rpn_loss', dict(objectness=None)),
    ('rpn_loss', dict(deltas=None)), ('rpn_loss', dict(index=None)), ('rpn_loss', dict(counts=None)),
    ('rpn_loss', dict(targets=None)), ('rpn_loss', dict(out=None)),
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


def _id(v):
    return 'nan' if isinstance(v, float) and v != v else v


@pytest.mark.parametrize('name,over', REFUSALS,
                         ids=['%s-%s' % (n, [(k, _id(v)) for k, v in sorted(o.items())]) for n, o in REFUSALS])
def test_refused_by_message_before_any_launch(name, over):
    rc, msg = _call(name, **over)
    assert rc == -1, (rc, msg)
    assert msg.startswith(name + ':'), msg


def test_a_whole_image_must_stay_below_2_to_the_24_anchors():
    _lib, lib = _load()
    p = _lib.make_pyramid([(2048, 1024)] * 3)           # each level alone fits (6.3e6 anchors), the image does not
    rc = lib.sfvos_rpn_match(ctypes.byref(p), 3, P, 4096, 4096, P, 3, 0.7, 0.3, 1, P, P, P, None, None)
    msg = lib.sfvos_last_error().decode()
    assert rc == -1 and msg.startswith('rpn_match:') and '2^24' in msg, msg
    assert lib.sfvos_rpn_targets_workspace_bytes(ctypes.byref(p), 3, 3, 256) == 0


def test_workspace_query():
    _lib, lib = _load()
    q = lib.sfvos_rpn_targets_workspace_bytes
    pyr = _pyr(_lib)
    for args in [(None, 3, 3, 256), (_pyr(_lib, 0), 3, 3, 256), (_pyr(_lib, 9), 3, 3, 256), (pyr, 0, 3, 256),
                 (pyr, 9, 3, 256), (pyr, 3, -1, 256), (pyr, 3, 1025, 256), (pyr, 3, 3, 0), (pyr, 3, 3, 4097)]:
        assert q(*args) == 0, args[1:]
    # highest[1024] + 5 passes x 2 classes x 4096 bins + the select state + the list of sampled anchors
    base = 1024 * 4 + 5 * 2 * 4096 * 4 + 256
    assert q(pyr, 3, 3, 256) == base + 256 * 4
    assert q(pyr, 3, 0, 1) == base + 16 and q(pyr, 8, 1024, 4096) == base + 4096 * 4


def test_abi_revision_and_bindings():
    _lib, lib = _load()
    assert _lib.ABI_REVISION >= 306 and lib.sfvos_version() >= 306
    for name in ('sfvos_rpn_targets_workspace_bytes', 'sfvos_rpn_match', 'sfvos_rpn_sample', 'sfvos_rpn_loss'):
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES['sfvos_rpn_match'][1]) == 15 and len(_lib.SIGNATURES['sfvos_rpn_sample'][1]) == 18
    assert len(_lib.SIGNATURES['sfvos_rpn_loss'][1]) == 13


def test_constructor_keywords_and_no_cpu_fallback():
    import inspect
    from sfvos_amd import RegionProposalNetwork
    names = list(inspect.signature(RegionProposalNetwork.__init__).parameters)
    assert names[-5:] == ['fg_iou_thresh', 'bg_iou_thresh', 'batch_size_per_image', 'positive_fraction', 'smooth_l1_beta']
    assert names[1:9] == ['anchor_generator', 'head', 'pre_nms_top_n', 'post_nms_top_n', 'nms_thresh', 'score_thresh',
                          'min_size', 'precision']
    rpn = RegionProposalNetwork()
    assert (rpn.fg_iou_thresh, rpn.bg_iou_thresh, rpn.batch_size_per_image, rpn.positive_fraction) == (0.7, 0.3, 256, 0.5)
    assert rpn.smooth_l1_beta == 1.0 / 9
    rpn = RegionProposalNetwork(fg_iou_thresh=0.6, bg_iou_thresh=0.2, batch_size_per_image=64, positive_fraction=0.25,
                                smooth_l1_beta=0.0)
    assert (rpn.fg_iou_thresh, rpn.bg_iou_thresh, rpn.batch_size_per_image, rpn.positive_fraction,
            rpn.smooth_l1_beta) == (0.6, 0.2, 64, 0.25, 0.0)
    assert list(inspect.signature(rpn.forward).parameters) == ['images', 'features', 'targets', 'keys']
    shapes = [(24, 40), (12, 20), (6, 10), (3, 5), (2, 3)]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rpn.anchor_targets(shapes, (96, 160), torch.zeros(2, 4))
    n = 3 * sum(h * w for h, w in shapes)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rpn.compute_loss(torch.zeros(n, 1).view(-1, 3), torch.zeros(n, 4).view(-1, 12), shapes, 1, (96, 160),
                         [dict(boxes=torch.zeros(1, 4))])
    # the inference-only rule stands
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rpn(types.SimpleNamespace(tensors=torch.zeros(1, 3, 16, 16), image_sizes=[(16, 16)]),
            {'0': torch.zeros(1, 256, 4, 4)}, [dict(boxes=torch.zeros(1, 4))])
