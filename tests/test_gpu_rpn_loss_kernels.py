"""GPU: the RPN training kernels (csrc/rpn_targets.hip) one by one through the C ABI, against tests/rpn_loss_ref.py.  Guard
bands and sentinel fills around every output, NaN-filled workspace, two runs compared with torch.equal; no element is left
out unless stated.  PARITY UNPINNED BY THE REFERENCE.

Two pyramids with rpn_ref.SIZES / RATIOS, A = 3: the small one (rpn_ref.SHAPES, tensor 96 x 160, N = 3825) and the large
one ((96,160), (48,80), (24,40), (12,20), tensor 384 x 640, N = 61 200: 240 workgroups of the match, 15 of the select).

match.  Anchors are integers and the ground truth sits on quarter pixels with coordinates below 1024, so every fp32
subtraction, product and sum of the IoU is exact (sides below 2^12 quarter pixels, areas and their sums below 2^24
sixteenths) and the one division is correctly rounded on both sides: `labels`, `matched` EQUAL the restatement and
`max_iou` is bit-equal; the equality with `highest` of the low-quality rule is an equality of identical quotients.  On
real-valued boxes max_iou is checked per element against the float64 IoU with K = 4 (tests/test_gpu_roi_targets_kernels.py
derives it) and labels / matches are compared where the float64 restatement is margin-safe (rpn_loss_ref.margin_safe; at
most 0.5 % of the anchors are left out, asserted on the CPU).

sample.  No arithmetic but the regression targets: counts and index equal the restatement's stable sort; the targets per
element under the allowance of the sfvos_roi_sample test with weights 1.

loss.  per_sample per element against float64 on the same fp32 inputs.  BCE term max(x, 0) - x z + log1p(exp(-|x|)): the
maximum and x z (z is 0 or 1) are exact, so K = 2 rounded operations (the subtraction and the addition) under
kernel_util's criterion, plus TRANS times the magnitude of the terms for exp / log1p, plus an absolute 2^-126: for x
below -87 and z = 0 the result lies below fp32's normal range and carries no relative precision (exp underflows; the
kernel may return 0 there, as kernel_util says of the sigmoid).  Box term: per coordinate one
subtraction, then 0.5 d d / beta (the halving is exact: 2 roundings) or |d| - 0.5 beta (1 rounding), then 4 additions:
K = 8 covers the doubled relative error of d in the square.  Every term of both is >= 0 or enters the magnitude by its
absolute value.  The two scalars are double sums of the fp32 terms divided by S_tot and rounded once: the mean of the
per-term bounds plus 2^-24 of the reference."""
import ctypes

import pytest
import torch

import rpn_loss_ref as T
import rpn_ref as R
from kernel_util import FLT_MIN, SENT, TRANS, U22, Out, P, S, check, check_abs, lib  # noqa: F401

pytestmark = pytest.mark.gpu
ISENT = int(SENT)
A = 3
_CACHE = {}


def setup(lib, pyramid):
    """(pyramid struct, byref, base table on the device, tensor size, anchors on the CPU) -- made once per pyramid."""
    if pyramid not in _CACHE:
        shapes, tensor = T.PYRAMIDS[pyramid]
        pyr = lib.make_pyramid(shapes)
        base = torch.stack(R.base_anchors(*T.ANCHOR_SIZES[pyramid])).float().contiguous().cuda()
        _CACHE[pyramid] = (pyr, base, tensor, T.anchors(shapes, tensor, *T.ANCHOR_SIZES[pyramid]))
    return _CACHE[pyramid]


def workspace(lib, pyr, G, batch):
    nbytes = lib.load().sfvos_rpn_targets_workspace_bytes(ctypes.byref(pyr), A, G, batch)
    assert nbytes > 0 and nbytes % 4 == 0
    return Out((nbytes // 4,), torch.float32, fill=float('nan'))


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- match ------------------------------------------------------------------------------------------------------------

def run_match(lib, pyramid, gt, high=T.HIGH, low=T.LOW, lowq=1, want_iou=True):
    pyr, base, tensor, anc = setup(lib, pyramid)
    N, G = anc.shape[0], gt.shape[0]
    gd = gt.float().contiguous().cuda()
    outs = []
    for _ in range(2):
        ws = workspace(lib, pyr, G, 1)
        matched, labels, iou = Out((N,), torch.int32), Out((N,), torch.int32), Out((N,))
        lib.call('sfvos_rpn_match', ctypes.byref(pyr), A, P(base), tensor[0], tensor[1], P(gd) if G else None, G, high, low,
                 lowq, P(ws.t), P(matched.t), P(labels.t), P(iou.t) if want_iou else None, S())
        torch.cuda.synchronize()
        assert ws.guards_ok(), 'wrote outside the workspace'
        outs.append((matched.cpu(), labels.cpu(), iou.cpu()))
        if not want_iou:
            assert bool((outs[-1][2] == SENT).all())
    for a, b in zip(*outs):
        assert torch.equal(a, b), 'two runs differ'
    return outs[0]


def assert_match_equal(lib, pyramid, gt, high=T.HIGH, low=T.LOW):
    """Both settings of allow_low_quality equal the restatement; -> the restatement with the rule on."""
    anc = setup(lib, pyramid)[3]
    for lowq in (1, 0):
        matched, labels, iou = run_match(lib, pyramid, gt, high, low, lowq)
        want = T.match(anc, gt, high, low, bool(lowq))
        assert torch.equal(bits(iou), bits(want['max_iou'])), (pyramid, lowq)
        assert torch.equal(labels.long(), want['labels']), (pyramid, lowq, int((labels.long() != want['labels']).sum()))
        assert torch.equal(matched.long(), want['matched']), (pyramid, lowq)
    return T.match(anc, gt, high, low, True)


@pytest.mark.parametrize('name', sorted(T.CASES))
def test_match_committed_cases(lib, name):
    pyramid, gt, want = T.CASES[name]
    m = assert_match_equal(lib, pyramid, torch.tensor(gt))
    lab = m['labels']
    got = (m['pos_high'], int((lab == 1).sum()), int((lab == 0).sum()), int((lab == -1).sum()))
    assert all(w is None or w == g for w, g in zip(want, got)), (got, want)      # so the kernel's counts are the table's
    if name == 'f':      # the box no anchor overlaps marks every anchor; each keeps its own argmax
        matched, labels, iou = run_match(lib, pyramid, torch.tensor(gt))
        assert bool((labels == 1).all()) and int((matched == 1).sum()) == 0 and int((iou > 0).sum()) > 0
    run_match(lib, pyramid, torch.tensor(gt), want_iou=False)       # max_iou may be NULL


@pytest.mark.parametrize('pyramid', ['small', 'large'])
@pytest.mark.parametrize('G', [0, 1, 65, 200])
def test_match_is_exact_on_random_quarter_pixel_boxes(lib, pyramid, G):
    gt = T.quarter_pixel_gt(pyramid, G, G)
    m = assert_match_equal(lib, pyramid, gt)
    if G == 0:
        assert bool((m['labels'] == 0).all()) and bool((m['max_iou'] == 0).all())
    if G >= 65:
        assert set(m['labels'].tolist()) == {-1, 0, 1} and int(m['matched'].max()) >= 64     # more than one tile of 64
    assert_match_equal(lib, pyramid, gt, 0.5, 0.5)      # dyadic thresholds, no ignored band


@pytest.mark.parametrize('pyramid,seed,G', T.REAL_CASES)
def test_match_on_real_valued_boxes(lib, pyramid, seed, G):
    anc, gt = T.real_case(pyramid, seed, G)
    matched, labels, iou = run_match(lib, pyramid, gt)
    ref = T.match(anc, gt)
    best64 = ref['iou64'].max(1).values
    check('rpn_match max_iou %s G %d' % (pyramid, G), iou, best64, best64, 4, 0.0)
    safe = T.margin_safe(ref['iou64'])
    assert 1.0 - float(safe.double().mean()) <= T.MAX_UNSAFE_SHARE
    assert torch.equal(labels.long()[safe], ref['labels'][safe])
    assert torch.equal(matched.long()[safe], ref['matched'][safe])
    print('   %d positive, %d ignored, %d background; %d left out; %d labels differ from the fp32 restatement'
          % (int((labels == 1).sum()), int((labels == -1).sum()), int((labels == 0).sum()), int((~safe).sum()),
             int((labels.long() != ref['labels']).sum())))


# ---- sample -----------------------------------------------------------------------------------------------------------

def run_sample(lib, pyramid, labels, matched, keys, gt, batch, fraction):
    """-> (S, P, index [batch], targets [batch, 4]) on the cpu."""
    pyr, base, tensor, anc = setup(lib, pyramid)
    N, G = anc.shape[0], gt.shape[0]
    ld, md, kd = labels.to(torch.int32).cuda(), matched.to(torch.int32).cuda(), keys.float().cuda()
    gd = gt.float().contiguous().cuda()
    runs = []
    for _ in range(2):
        ws = workspace(lib, pyr, G, batch)
        cnt, index, targets = Out((2,), torch.int32), Out((batch,), torch.int32), Out((batch, 4))
        lib.call('sfvos_rpn_sample', P(ld), P(md), P(kd), N, ctypes.byref(pyr), A, P(base), tensor[0], tensor[1],
                 P(gd) if G else None, G, batch, fraction, P(ws.t), P(cnt.t), P(index.t), P(targets.t), S())
        torch.cuda.synchronize()
        assert ws.guards_ok(), 'wrote outside the workspace'
        runs.append([cnt.cpu(), index.cpu(), targets.cpu()])
    for a, b in zip(*runs):
        assert torch.equal(a, b), 'two runs differ'
    cnt, index, targets = runs[0]
    return int(cnt[0]), int(cnt[1]), index, targets


def check_sample(lib, pyramid, labels, keys, batch, fraction, tag):
    anc = setup(lib, pyramid)[3]
    N = anc.shape[0]
    g = torch.Generator().manual_seed(11)
    gt = T.real_case(pyramid, 9, 3)[1]
    matched = torch.randint(0, 3, (N,), generator=g)
    Sg, Pg, index, targets = run_sample(lib, pyramid, labels, matched, keys, gt, batch, fraction)
    pos, neg = T.sample(labels, keys, batch, fraction)
    Sw, Pw = pos.numel() + neg.numel(), pos.numel()
    assert (Sg, Pg) == (Sw, Pw), (tag, Sg, Pg, Sw, Pw)
    assert torch.equal(index[:Sw].long(), torch.cat([pos, neg])), tag
    assert bool((index[Sw:] == -1).all()) and bool((targets[Pw:] == SENT).all()), tag      # untouched behind P
    if Pw:
        want = T.encode(gt[matched[pos]], anc[pos])
        check_abs('rpn_sample targets %s' % tag, targets[:Pw], want, T.encode_allowance(gt[matched[pos]], anc[pos], TRANS))
    return Sw, Pw


def key_sets(N, seed):
    g = torch.Generator().manual_seed(seed)
    special = torch.rand(N, generator=g) - 0.5
    special[::7] = 0.0
    special[3::7] = -0.0
    special[5::50] = float('inf')
    special[6::50] = float('-inf')
    special[8::50] = float('nan')
    special[9::50] = 1e-42          # denormals
    special[10::50] = -1e-42
    return {'uniform': torch.rand(N, generator=g), 'eighths': torch.randint(0, 8, (N,), generator=g).float() / 8,
            'all equal': torch.full((N,), 0.5), 'special': special}


def regimes(N):
    """name -> ((#pos, #neg), (S, P) at batch 256, fraction 0.5); the rest of the N anchors is ignored."""
    return {'positives over the cap': ((300, N - 1000), (256, 128)), 'positives under the cap': ((40, N - 1000), (256, 40)),
            'too few negatives': ((30, 100), (130, 30)), 'no positives': ((0, N - 100), (256, 0)),
            'no negatives': ((N, 0), (128, 128)), 'everything ignored': ((0, 0), (0, 0))}


def regime_labels(n_pos, n_neg, N, seed):
    lab = torch.cat([torch.ones(n_pos, dtype=torch.int64), torch.zeros(n_neg, dtype=torch.int64),
                     -torch.ones(N - n_pos - n_neg, dtype=torch.int64)])
    return lab[torch.randperm(N, generator=torch.Generator().manual_seed(seed))]


@pytest.mark.parametrize('pyramid', ['small', 'large'])
@pytest.mark.parametrize('regime', sorted(regimes(3825)))
def test_sample_regimes_and_key_sets(lib, pyramid, regime):
    N = setup(lib, pyramid)[3].shape[0]
    (n_pos, n_neg), want = regimes(N)[regime]
    labels = regime_labels(n_pos, n_neg, N, 5)
    for kind, keys in key_sets(N, 6).items():
        got = check_sample(lib, pyramid, labels, keys, 256, 0.5, '%s %s %s' % (pyramid, regime, kind))
        assert got == want, (regime, kind, got, want)
        check_sample(lib, pyramid, labels, keys, 4096, 0.5, '%s %s %s batch 4096' % (pyramid, regime, kind))


@pytest.mark.parametrize('pyramid', ['small', 'large'])
def test_sample_on_the_matchers_labels_and_other_fractions(lib, pyramid):
    name = 'a' if pyramid == 'small' else 'e'
    anc = setup(lib, pyramid)[3]
    gt = torch.tensor(T.CASES[name][1])
    m = T.match(anc, gt)
    keys = key_sets(anc.shape[0], 8)
    for batch, fraction in ((256, 0.5), (256, 0.25), (64, 0.0), (64, 1.0), (1, 0.5), (4096, 0.5)):
        for kind in ('uniform', 'eighths'):
            check_sample(lib, pyramid, m['labels'], keys[kind], batch, fraction, '%s batch %d fraction %g %s'
                         % (pyramid, batch, fraction, kind))


def test_match_and_sample_on_the_davis_pyramid(lib):
    """The size the reference trains at: five levels, 257 796 anchors (1008 workgroups of the match, 63 of the select)."""
    gt = torch.tensor(T.CASE_DAVIS)
    m = assert_match_equal(lib, 'davis', gt)
    assert (int((m['labels'] == 1).sum()), int((m['labels'] == 0).sum())) == (9, 257203)
    keys = torch.rand(m['labels'].numel(), generator=torch.Generator().manual_seed(12))
    gt_real, anc = T.real_case('davis', 9, 3)[1], setup(lib, 'davis')[3]
    for batch in (256, 4096):
        Sg, Pg, index, targets = run_sample(lib, 'davis', m['labels'], m['matched'], keys, gt_real, batch, 0.5)
        pos, neg = T.sample(m['labels'], keys, batch, 0.5)
        assert (Sg, Pg) == (batch, 9) and torch.equal(index.long(), torch.cat([pos, neg]))
        ref = gt_real[m['matched'][pos]]
        check_abs('rpn_sample targets davis', targets[:Pg], T.encode(ref, anc[pos]), T.encode_allowance(ref, anc[pos], TRANS))


# ---- loss -------------------------------------------------------------------------------------------------------------

def run_loss(lib, pyramid, batch, obj, dl, index, counts, targets, bspi, beta, want_rows=True):
    pyr = setup(lib, pyramid)[0]
    od, dd = obj.float().contiguous().cuda(), dl.float().contiguous().cuda()
    idx, cnt, tg = index.to(torch.int32).cuda(), counts.to(torch.int32).cuda(), targets.float().contiguous().cuda()
    runs = []
    for _ in range(2):
        rows, out = Out((batch, bspi, 2)), Out((2,))
        lib.call('sfvos_rpn_loss', P(od), P(dd), ctypes.byref(pyr), batch, A, P(idx), P(cnt), P(tg), bspi, beta,
                 P(rows.t) if want_rows else None, P(out.t), S())
        torch.cuda.synchronize()
        assert rows.guards_ok() and out.guards_ok()
        runs.append((rows.t.cpu(), out.t.cpu()))
    assert torch.equal(bits(runs[0][0]), bits(runs[1][0])) and torch.equal(bits(runs[0][1]), bits(runs[1][1]))
    return runs[0]


@pytest.mark.parametrize('beta', [0.0, 1.0 / 9])
@pytest.mark.parametrize('pyramid', ['small', 'large', 'davis'])
def test_loss(lib, pyramid, beta):
    shapes = T.PYRAMIDS[pyramid][0]
    N = setup(lib, pyramid)[3].shape[0]
    B, bspi = 3, 256
    beta32 = float(torch.tensor(beta, dtype=torch.float32))      # what the entry point receives
    g = torch.Generator().manual_seed(21)
    positions = B * N // A
    obj = torch.randn(positions, A, generator=g) * 4
    dl = torch.randn(positions, 4 * A, generator=g) * 0.3
    sp = torch.tensor([200., -200., 0., -0., 88., -88., 104., -104., 1e-30, -1e-30, 17., -17.])
    flat = obj.view(-1)
    flat[torch.randperm(flat.numel(), generator=g)[:B * N // 4]] = sp.repeat(B * N // 4 // 12 + 1)[:B * N // 4]
    counts = torch.tensor([[256, 100], [180, 0], [37, 37]])      # different S; an image without positives; only positives
    index = torch.full((B, bspi), -1, dtype=torch.int64)
    targets = torch.full((B, bspi, 4), SENT)
    lg, dd = T.per_image(obj, dl, shapes, B, A)
    for b, (s, p) in enumerate(counts.tolist()):
        index[b, :s] = torch.randperm(N, generator=g)[:s]
        # differences that straddle beta: just below, just above, far above, tiny, zero, and random ones
        diff = torch.randn(p, 4, generator=g) * 0.2
        if p:
            pick = torch.tensor([beta32 * (1 - 1e-3), -beta32 * (1 + 1e-3), beta32, 5.0, 1e-6, 0.0, -beta32 * 0.5])
            diff.view(-1)[:4 * p:3] = pick.repeat(4 * p // 3 // 7 + 1)[:diff.view(-1)[:4 * p:3].numel()]
        targets[b, :p] = dd[b][index[b, :p]] - diff
    rows, out = run_loss(lib, pyramid, B, obj, dl, index, counts, targets, bspi, beta)
    sums, bounds, s_tot = [0.0, 0.0], [0.0, 0.0], int(counts[:, 0].sum())
    for b, (s, p) in enumerate(counts.tolist()):
        bce, box, bce_mag, box_mag = T.loss_terms(lg[b], dd[b], index[b, :s], p, targets[b, :p], beta32)
        tag = 'rpn_loss %s beta %.3g image %d ' % (pyramid, beta, b)
        allow = [(2.0 * (2 + 1) * U22 + TRANS) * bce_mag + FLT_MIN, 2.0 * (8 + 1) * U22 * box_mag]
        check_abs(tag + 'bce', rows[b, :s, 0], bce, allow[0])
        check_abs(tag + 'box', rows[b, :s, 1], box, allow[1])
        assert bool((rows[b, p:s, 1] == 0).all()) and bool((rows[b, s:] == SENT).all())
        if p and beta:
            d = (dd[b][index[b, :p]].double() - targets[b, :p].double()).abs()
            assert bool((d < beta32).any()) and bool((d > beta32).any())
        for t, (v, a) in enumerate(zip((bce, box), allow)):
            sums[t] += float(v.sum())
            bounds[t] += float(a.sum())
    for t, name in enumerate(('loss_objectness', 'loss_rpn_box_reg')):
        ref = sums[t] / s_tot
        err, bound = abs(float(out[t]) - ref), bounds[t] / s_tot + 2.0 ** -24 * abs(ref)
        print('%-46s error/bound %.4f (value %.6f)' % ('rpn_loss %s beta %.3g %s' % (pyramid, beta, name), err / bound, ref))
        assert err <= bound, (name, float(out[t]), ref, bound)
    # per_sample may be NULL: the same scalars
    assert torch.equal(bits(run_loss(lib, pyramid, B, obj, dl, index, counts, targets, bspi, beta, want_rows=False)[1]),
                       bits(out))


def test_loss_of_nothing_sampled_is_nan_and_a_bad_index_reads_nothing(lib):
    N = setup(lib, 'small')[3].shape[0]
    obj, dl = torch.zeros(N // A, A), torch.zeros(N // A, 4 * A)
    index = torch.full((1, 8), -1, dtype=torch.int64)
    rows, out = run_loss(lib, 'small', 1, obj, dl, index, torch.tensor([[0, 0]]), torch.zeros(1, 8, 4), 8, 0.0)
    assert bool(torch.isnan(out).all()) and bool((rows == SENT).all())          # 0 / 0, as torch's mean of nothing
    index[0, :3] = torch.tensor([5, N, -7])                                      # outside [0, N): NaN, nothing read
    rows, out = run_loss(lib, 'small', 1, obj, dl, index, torch.tensor([[3, 1]]), torch.zeros(1, 8, 4), 8, 0.0)
    assert bool(torch.isnan(out[0])) and float(out[1]) == 0.0 and bool(torch.isnan(rows[0, 1:3, 0]).all())
    assert abs(float(rows[0, 0, 0]) - 0.6931471805599453) < 1e-6 and float(rows[0, 0, 1]) == 0.0
