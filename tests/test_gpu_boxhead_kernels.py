"""GPU: the box-branch kernels (csrc/dense.hip, csrc/boxes.hip, csrc/project.hip) one by one through the C ABI, each
against float64 on the operands the kernel sees, under the per-element criterion of tests/kernel_util.py (its docstring):

    |got - ref|  <=  u_out * |ref|  +  2 * (K + 1) * 2^-22 * mag

K = the longest chain of fp32 additions one product passes through -- dense layer: the inputs of one K split plus the
number of splits (the slabs are added in fp32); weight gradient: M; predictor: its 1024 (C) inputs -- and u_out = 2^-8
for a bf16 store, 0 for fp32.  Transcendental outputs (softmax, log-sum-exp, exp in decode, log in encode) get that
file's 2^-20 allowance on the magnitudes of their terms.  Guard bands, sentinel fills and NaN-filled workspaces as
there; no element is left out.  NMS is compared exactly (index lists) on quarter-pixel boxes; detections on real-valued
boxes in two stages (candidates per element; the selection against the restatement run on the kernel's own fp32
candidates, margin-safe seeds only, at most 2 of 16 skipped).  PARITY UNPINNED BY THE REFERENCE: the restatement
(tests/box_branch_ref.py) is written from torchvision's published sources."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import box_branch_ref as R
from test_box_branch_cpu import quarter_pixel_boxes
from kernel_util import DT, PRECS, TDT, TRANS, U22, U_OUT, Out, P, S, check, check_abs, lib, rnd  # noqa: F401

pytestmark = pytest.mark.gpu

STAGE = {'fp32': 32, 'bf16': 64}      # inputs one LDS stage of the dense kernel covers


def dense_chain(lib, prec, m, n, k):
    """(splits, longest fp32 chain): a split covers whole stages."""
    splits = lib.load().sfvos_dense_splits(DT(lib, prec), m, n, k)
    stages = -(-k // STAGE[prec])
    per = -(-stages // splits) * STAGE[prec]
    return splits, min(k, per) + splits


def perm_cols(k, hw):
    """state-dict column of channels-last column k' = p*C + c:  c*HW + p."""
    C = k // hw
    kp = torch.arange(k)
    return (kp % C) * hw + kp // C


def run_dense(lib, prec, x, image, bias, n, relu):
    m, k = x.shape
    nbytes = lib.load().sfvos_dense_workspace_bytes(DT(lib, prec), m, n, k)
    splits = lib.load().sfvos_dense_splits(DT(lib, prec), m, n, k)
    assert nbytes == (splits * m * n * 4 if splits > 1 else 0)
    ws = Out((max(nbytes // 4, 1),), torch.float32, fill=float('nan'))
    y = Out((m, n), TDT[prec])
    lib.call('sfvos_dense', P(x), P(image), P(bias) if bias is not None else None, P(y.t), DT(lib, prec), m, n, k, relu,
             P(ws.t) if nbytes else None, S())
    torch.cuda.synchronize()
    assert ws.guards_ok(), 'wrote outside the workspace'
    return y.cpu()


DENSE_CASES = [
    # M     N     K     HW
    (1000, 1024, 12544, 49),   # fc6, evaluation
    (512, 1024, 12544, 49),    # fc6, training
    (1000, 1024, 1024, 1),     # fc7
    (512, 1024, 1024, 1),
    (1, 1024, 12544, 49),      # one row: 16 splits
    (1, 32, 32, 1),            # one stage (bf16: half of one), one split
    (130, 96, 160, 1),         # M = 128 + 2, N below the tile; bf16: K = 2.5 stages (the half stage behind K)
    (300, 64, 2048, 1),        # three tiles: several splits of a few stages
    (77, 160, 1568, 49),       # a small fc6: 32 channels x 49 positions
]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('n,k,hw', [(32, 32, 1), (96, 1568, 49), (1024, 12544, 49)])
def test_dense_packers_are_exact_permutations(lib, prec, n, k, hw):
    """forward image wp[n][p*C + c] = w[n][c*HW + p]; data-gradient image wd[p*C + c][n]; bf16 = the fp32 value rounded to
    nearest even (ties among the values)."""
    g = torch.Generator().manual_seed(5)
    w = torch.randn(n, k, generator=g)
    w.view(-1)[:4] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8)])
    wd = w.cuda()
    fwd, dgr = Out((n, k), TDT[prec]), Out((k, n), TDT[prec])
    lib.call('sfvos_pack_dense_fwd', P(wd), P(fwd.t), DT(lib, prec), n, k, hw, S())
    lib.call('sfvos_pack_dense_dgrad', P(wd), P(dgr.t), DT(lib, prec), n, k, hw, S())
    torch.cuda.synchronize()
    want = w[:, perm_cols(k, hw)].to(TDT[prec])
    assert torch.equal(fwd.cpu(), want)
    assert torch.equal(dgr.cpu(), want.t().contiguous())


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', DENSE_CASES)
def test_dense_forward(lib, prec, case):
    """y = act(x . W^T + b) on channels-last rows against F.linear on torchvision's NCHW flatten, float64.  ReLU on and
    off, bias on and off; two runs bit-identical."""
    m, n, k, hw = case
    g = torch.Generator().manual_seed(41)
    C = k // hw
    x_nchw = rnd(torch.randn(m, C, hw, generator=g), prec)             # distinct values per (c, p)
    w = torch.randn(n, k, generator=g) / np.sqrt(k)
    bias = torch.randn(n, generator=g) * 0.3
    wr = rnd(w, prec).double()
    flat = x_nchw.reshape(m, k).double()                               # torchvision: x.flatten(start_dim=1)
    rows = x_nchw.permute(0, 2, 1).reshape(m, k).to(TDT[prec]).cuda()  # what the kernel reads
    image = torch.empty(n * k, dtype=TDT[prec], device='cuda')
    wd, bd = w.cuda(), bias.cuda()
    lib.call('sfvos_pack_dense_fwd', P(wd), P(image), DT(lib, prec), n, k, hw, S())
    splits, chain = dense_chain(lib, prec, m, n, k)
    for relu, with_bias in ((1, True), (0, False)):
        b64 = bias.double() if with_bias else None
        ref = F.linear(flat, wr, b64)
        mag = F.linear(flat.abs(), wr.abs(), b64.abs() if with_bias else None)
        y1 = run_dense(lib, prec, rows, image, bd if with_bias else None, n, relu)
        y2 = run_dense(lib, prec, rows, image, bd if with_bias else None, n, relu)
        check('dense fwd %s %s splits %d relu %d' % (prec, case, splits, relu), y1, ref.clamp_min(0) if relu else ref,
              mag, chain, U_OUT[prec])
        assert torch.equal(y1, y2), 'the dense layer must be bit-identical from run to run'
    if case == (1, 1024, 12544, 49):
        assert splits > 1
    if case in ((1, 32, 32, 1), (130, 96, 160, 1)):
        assert splits == 1


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', DENSE_CASES)
def test_dense_data_gradient(lib, prec, case):
    """dx[m][p*C + c] = sum_n dz[m][n] w[n][c*HW + p]: sfvos_dense on the image of sfvos_pack_dense_dgrad."""
    m, n, k, hw = case
    g = torch.Generator().manual_seed(42)
    dz = rnd(torch.randn(m, n, generator=g), prec)
    w = torch.randn(n, k, generator=g) / np.sqrt(n)
    wr = rnd(w, prec).double()
    cols = perm_cols(k, hw)
    ref = (dz.double() @ wr)[:, cols]
    mag = (dz.double().abs() @ wr.abs())[:, cols]
    image = torch.empty(n * k, dtype=TDT[prec], device='cuda')
    wd, dzd = w.cuda(), dz.to(TDT[prec]).cuda()
    lib.call('sfvos_pack_dense_dgrad', P(wd), P(image), DT(lib, prec), n, k, hw, S())
    splits, chain = dense_chain(lib, prec, m, k, n)
    dx = run_dense(lib, prec, dzd, image, None, k, 0)
    check('dense dgrad %s %s splits %d' % (prec, case, splits), dx, ref, mag, chain, U_OUT[prec])


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', DENSE_CASES)
def test_dense_weight_gradient(lib, prec, case):
    """dW[n][c*HW + p] = sum_m dz[m][n] x[m][p*C + c]: one chain over the M rows (K = M), fp32 store in the state-dict
    layout; accumulate adds one; bit-identical from run to run."""
    m, n, k, hw = case
    g = torch.Generator().manual_seed(43)
    x = rnd(torch.randn(m, k, generator=g), prec)          # channels-last rows
    dz = rnd(torch.randn(m, n, generator=g), prec)
    inv = torch.argsort(perm_cols(k, hw))                  # channels-last column of state-dict column
    ref = (dz.double().t() @ x.double())[:, inv]
    mag = (dz.double().abs().t() @ x.double().abs())[:, inv]
    xd, dzd = x.to(TDT[prec]).cuda(), dz.to(TDT[prec]).cuda()
    runs = []
    for _ in range(2):
        gw = Out((n, k))
        lib.call('sfvos_dense_wgrad', P(xd), P(dzd), DT(lib, prec), m, n, k, hw, P(gw.t), 0, S())
        torch.cuda.synchronize()
        runs.append(gw.cpu().clone())
    check('dense wgrad %s %s' % (prec, case), runs[0], ref, mag, m, 0.0)
    assert torch.equal(runs[0], runs[1])
    old = torch.randn(n, k, generator=g)
    gw = Out((n, k))
    gw.t.copy_(old)
    lib.call('sfvos_dense_wgrad', P(xd), P(dzd), DT(lib, prec), m, n, k, hw, P(gw.t), 1, S())
    torch.cuda.synchronize()
    check('dense wgrad %s %s accumulate' % (prec, case), gw.cpu(), old.double() + ref, old.double().abs() + mag, m + 1, 0.0)


def test_dense_refuses_bad_shapes(lib):
    x = torch.zeros(64, 64, device='cuda')
    for m, n, k in ((0, 32, 32), (4, 48, 32), (4, 32, 40)):
        with pytest.raises(RuntimeError, match='dense'):
            lib.call('sfvos_dense', P(x), P(x), None, P(x), lib.F32, m, n, k, 0, None, S())
    with pytest.raises(RuntimeError, match='positions'):
        lib.call('sfvos_pack_dense_fwd', P(x), P(x), lib.F32, 32, 64, 7, S())
    with pytest.raises(RuntimeError, match='bad dtype'):
        lib.call('sfvos_dense', P(x), P(x), None, P(x), 2, 4, 32, 32, 0, None, S())


# ---- predictor ----------------------------------------------------------------------------------------------------------

def predictor_operands(m, c, K, prec, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, c, generator=g).clamp_min(0)
    x.view(-1)[::7] = -0.0
    x.view(-1)[5::53] = -0.25
    x = rnd(x, prec)
    wc, wb = torch.randn(K, c, generator=g) / np.sqrt(c), torch.randn(4 * K, c, generator=g) / np.sqrt(c)
    bc, bb = torch.randn(K, generator=g) * 0.5, torch.randn(4 * K, generator=g) * 0.5
    return x, wc, bc, wb, bb


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('m,c,K', [(1000, 1024, 2), (1, 64, 1), (5, 96, 8), (513, 1024, 3)])
def test_box_predictor(lib, prec, m, c, K):
    """K = C: a lane adds C / 64 products, six shuffle steps and the bias follow."""
    x, wc, bc, wb, bb = predictor_operands(m, c, K, prec, 51)
    lo, de = Out((m, K)), Out((m, 4 * K))
    xd, wcd, bcd, wbd, bbd = x.to(TDT[prec]).cuda(), wc.cuda(), bc.cuda(), wb.cuda(), bb.cuda()
    lib.call('sfvos_box_predictor', P(xd), DT(lib, prec), P(wcd), P(bcd), P(wbd), P(bbd), m, c, K, P(lo.t), P(de.t), S())
    torch.cuda.synchronize()
    x64 = x.double()
    tag = 'box_predictor %s (%d,%d,%d) ' % (prec, m, c, K)
    check(tag + 'logits', lo.cpu(), F.linear(x64, wc.double(), bc.double()),
          F.linear(x64.abs(), wc.double().abs(), bc.double().abs()), c, 0.0)
    check(tag + 'deltas', de.cpu(), F.linear(x64, wb.double(), bb.double()),
          F.linear(x64.abs(), wb.double().abs(), bb.double().abs()), c, 0.0)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('relu', [1, 0])
@pytest.mark.parametrize('m,c,K', [(512, 1024, 2), (1, 64, 1), (70, 96, 8), (130, 300, 3)])
def test_box_predictor_bwd(lib, prec, relu, m, c, K):
    """dz: K = 5 num_classes.  Partials after sfvos_reduce_rows: K = 64 + rows (64 rows per block in fp32, the blocks in
    f64).  The column sums are those of the unrounded dz."""
    x, wc, _, wb, _ = predictor_operands(m, c, K, prec, 52)
    g = torch.Generator().manual_seed(53)
    dl, dd = torch.randn(m, K, generator=g), torch.randn(m, 4 * K, generator=g)
    J = 5 * K
    gcat, wcat = torch.cat([dl, dd], 1).double(), torch.cat([wc, wb], 0).double()
    live = (x > 0) if relu else torch.ones_like(x, dtype=torch.bool)
    zero = torch.zeros((), dtype=torch.float64)
    dz_ref = torch.where(live, gcat @ wcat, zero)
    dz_mag = torch.where(live, gcat.abs() @ wcat.abs(), zero)
    rows = lib.load().sfvos_box_predictor_bwd_rows(m)
    assert rows == -(-m // 64)
    L = J * c + J + c
    dz, part, red = Out((m, c), TDT[prec]), Out((rows, L), fill=float('nan')), Out((L,))
    xd, dld, ddd, wcd, wbd = x.to(TDT[prec]).cuda(), dl.cuda(), dd.cuda(), wc.cuda(), wb.cuda()
    lib.call('sfvos_box_predictor_bwd', P(xd), DT(lib, prec), P(dld), P(ddd), P(wcd), P(wbd), m, c, K, relu, P(dz.t),
             P(part.t), S())
    lib.call('sfvos_reduce_rows', P(part.t), rows, L, P(red.t), 0, S())
    torch.cuda.synchronize()
    tag = 'box_predictor_bwd %s (%d,%d,%d) relu %d ' % (prec, m, c, K, relu)
    check(tag + 'dz', dz.cpu(), dz_ref, dz_mag, J, U_OUT[prec])
    assert bool(torch.isfinite(part.cpu()).all()), 'a partial row was not written'
    r = red.cpu()
    Kp = 64 + rows
    check(tag + 'grad w', r[:J * c].view(J, c), gcat.t() @ x.double(), gcat.abs().t() @ x.double().abs(), Kp, 0.0)
    check(tag + 'grad b', r[J * c:J * c + J], gcat.sum(0), gcat.abs().sum(0), Kp, 0.0)
    check(tag + 'column sums of dz', r[J * c + J:], dz_ref.sum(0), dz_mag.sum(0), Kp, 0.0)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('m,c', [(1, 64), (130, 128)])
def test_box_and_mask_projections_are_one_kernel(lib, prec, m, c):
    """The box predictor with one class (J = 5 outputs) and the mask head's entry points called with positions = 1,
    num_classes = 5 on the concatenated weights are the same projection: outputs, dz and the raw partial rows are equal
    bit for bit, forward and backward (ReLU on and off)."""
    K, J = 1, 5
    x, wc, bc, wb, bb = predictor_operands(m, c, K, prec, 54)
    g = torch.Generator().manual_seed(55)
    dl, dd = torch.randn(m, K, generator=g), torch.randn(m, 4 * K, generator=g)
    xd, wcd, bcd, wbd, bbd = x.to(TDT[prec]).cuda(), wc.cuda(), bc.cuda(), wb.cuda(), bb.cuda()
    wcat, bcat = torch.cat([wc, wb], 0).cuda(), torch.cat([bc, bb], 0).cuda()
    dld, ddd, gcat = dl.cuda(), dd.cuda(), torch.cat([dl, dd], 1).cuda()
    lo, de, both = Out((m, K)), Out((m, 4 * K)), Out((m, J))
    lib.call('sfvos_box_predictor', P(xd), DT(lib, prec), P(wcd), P(bcd), P(wbd), P(bbd), m, c, K, P(lo.t), P(de.t), S())
    lib.call('sfvos_mask_logits', P(xd), DT(lib, prec), P(wcat), P(bcat), None, m, 1, c, J, P(both.t), None, S())
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([lo.cpu(), de.cpu()], 1), both.cpu())
    rows = lib.load().sfvos_box_predictor_bwd_rows(m)
    assert rows == lib.load().sfvos_mask_logits_bwd_rows(m, 1)
    L = J * c + J + c
    for relu in (1, 0):
        dz_b, part_b = Out((m, c), TDT[prec]), Out((rows, L), fill=float('nan'))
        dz_m, part_m = Out((m, c), TDT[prec]), Out((rows, L), fill=float('nan'))
        lib.call('sfvos_box_predictor_bwd', P(xd), DT(lib, prec), P(dld), P(ddd), P(wcd), P(wbd), m, c, K, relu,
                 P(dz_b.t), P(part_b.t), S())
        lib.call('sfvos_mask_logits_bwd', P(xd), DT(lib, prec), P(gcat), P(wcat), m, 1, c, J, relu, P(dz_m.t),
                 P(part_m.t), S())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(part_b.cpu()).all()) and bool(torch.isfinite(part_m.cpu()).all())
        assert torch.equal(dz_b.cpu(), dz_m.cpu()), 'dz differs (relu %d)' % relu
        assert torch.equal(part_b.cpu(), part_m.cpu()), 'partial rows differ (relu %d)' % relu


# ---- fastrcnn_loss ------------------------------------------------------------------------------------------------------

def loss_operands(n, K, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(n, K, generator=g) * scale
    deltas = torch.randn(n, 4 * K, generator=g)
    labels = torch.randint(0, K, (n,), generator=g)
    targets = deltas.view(n, K, 4)[torch.arange(n), labels] + torch.randn(n, 4, generator=g) * 0.15   # both branches
    return logits, deltas, labels, targets


def run_loss(lib, logits, deltas, labels, targets, upstream=None):
    n, K = logits.shape
    losses, gl, gd = Out((2,)), Out((n, K)), Out((n, 4 * K))
    a, b, c, d = logits.cuda(), deltas.cuda(), labels.cuda(), targets.cuda()
    up = upstream.cuda() if upstream is not None else None
    lib.call('sfvos_fastrcnn_loss', P(a), P(b), P(c), P(d), n, K, 1.0 / 9, P(losses.t), S())
    lib.call('sfvos_fastrcnn_loss_grad', P(a), P(b), P(c), P(d), P(up) if up is not None else None, n, K, 1.0 / 9,
             P(gl.t), P(gd.t), S())
    torch.cuda.synchronize()
    return losses.cpu(), gl.cpu(), gd.cpu()


@pytest.mark.parametrize('n,K,scale', [(512, 2, 3.0), (1, 2, 1.0), (1000, 2, 30.0), (77, 8, 3.0), (2048, 3, 3.0)])
def test_fastrcnn_loss_and_gradient(lib, n, K, scale):
    """Both scalars and both gradients against float64 autograd of the restatement.  Allowance: 2^-20 times the float64
    magnitudes of the terms of the kernel's formula (|max| + |log sum exp| + |z_label| per RoI for the classifier loss,
    the smooth-L1 terms themselves for the box loss; softmax + one for the logit gradient; 1 / N for a delta gradient),
    plus, for the smooth-L1 terms, the rounding of the fp32 difference d = delta - target carried through them
    (2^-24 (|delta| + |target|) per term, times the slope <= 1).  scale 30: saturated softmax, stable log-sum-exp."""
    logits, deltas, labels, targets = loss_operands(n, K, 61, scale)
    up = torch.tensor([0.7, 1.9])
    lg, dl = logits.double().requires_grad_(True), deltas.double().requires_grad_(True)
    lc, lb = R.fastrcnn_loss(lg, dl, [labels], [targets.double()])
    (up[0].double() * lc + up[1].double() * lb).backward()
    got, gl, gd = run_loss(lib, logits, deltas, labels, targets, up)
    z = logits.double()
    mx = z.max(1).values
    lse = torch.log(torch.exp(z - mx[:, None]).sum(1))
    mag_c = (mx.abs() + lse.abs() + z[torch.arange(n), labels].abs()).sum() / n
    pos = labels > 0
    dsel = deltas.view(n, K, 4)[torch.arange(n), labels].double()
    d = (dsel - targets.double())[pos]
    terms = torch.where(d.abs() < 1 / 9, 0.5 * d * d * 9, d.abs() - 0.5 / 9)
    carry = (2.0 ** -24) * (dsel[pos].abs() + targets.double()[pos].abs())
    mag_b = (terms.sum() + carry.sum() / TRANS) / n
    tag = 'fastrcnn_loss (%d,%d,%g) ' % (n, K, scale)
    check_abs(tag + 'losses', got, torch.stack([lc, lb]).detach(), TRANS * torch.stack([mag_c, mag_b]) + 2.0 ** -126)
    sm = torch.softmax(z, 1)
    check_abs(tag + 'grad logits', gl, lg.grad, TRANS * float(up[0]) * (sm + 1.0) / n)
    # a delta gradient is up d / (beta N) inside the quadratic zone: the rounding of d is carried at slope 1 / beta
    allow = torch.zeros(n, K, 4, dtype=torch.float64)
    a_sel = float(up[1]) / n * (TRANS + 9.0 * (2.0 ** -24) * (dsel.abs() + targets.double().abs()))
    allow[torch.arange(n), labels] = a_sel
    check_abs(tag + 'grad deltas', gd, dl.grad, allow.view(n, 4 * K) + 1e-300)
    assert float(gd.view(n, K, 4)[~pos].abs().max() if bool((~pos).any()) else 0.0) == 0.0
    # upstream NULL = 1
    _, gl1, gd1 = run_loss(lib, logits, deltas, labels, targets, None)
    _, gl2, gd2 = run_loss(lib, logits, deltas, labels, targets, torch.ones(2))
    assert torch.equal(gl1, gl2) and torch.equal(gd1, gd2)


def test_fastrcnn_loss_bad_labels_and_no_positive(lib):
    logits, deltas, labels, targets = loss_operands(9, 3, 62)
    bad = labels.clone()
    bad[2], bad[5] = 3, -1
    got, gl, gd = run_loss(lib, logits, deltas, bad, targets)
    assert bool(torch.isnan(got).all())
    assert float(gl[[2, 5]].abs().max()) == 0.0 and float(gd[[2, 5]].abs().max()) == 0.0
    ok = [i for i in range(9) if i not in (2, 5)]
    _, gl_ok, gd_ok = run_loss(lib, logits, deltas, labels, targets)
    assert torch.equal(gl[ok], gl_ok[ok]) and torch.equal(gd[ok], gd_ok[ok])
    none = torch.zeros(9, dtype=torch.int64)
    got, gl, gd = run_loss(lib, logits, deltas, none, targets)
    assert float(got[1]) == 0.0 and float(gd.abs().max()) == 0.0 and bool(torch.isfinite(got[0]))


# ---- box coder ------------------------------------------------------------------------------------------------------------

def decode_allowance(deltas, props, K):
    """Per-element allowance of a decoded coordinate in float64: 2^-20 on the magnitudes of its terms (|dx| w + |cx| +
    exp(dw) w / 2: one division, one exp, five roundings), and the rounding of the exponent's argument carried through
    exp (|dw| 2^-24 times the half size)."""
    m = props.shape[0]
    p = props.double()
    w, h = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    cx, cy = p[:, 0] + 0.5 * w, p[:, 1] + 0.5 * h
    d = deltas.double().view(m, K, 4)
    dw, dh = (d[..., 2] / 5).clamp(max=R.BBOX_XFORM_CLIP), (d[..., 3] / 5).clamp(max=R.BBOX_XFORM_CLIP)
    hw_, hh_ = 0.5 * torch.exp(dw) * w[:, None], 0.5 * torch.exp(dh) * h[:, None]
    mx = (d[..., 0].abs() / 10) * w[:, None] + cx.abs()[:, None] + hw_ * (1 + dw.abs() * 2.0 ** -4)
    my = (d[..., 1].abs() / 10) * h[:, None] + cy.abs()[:, None] + hh_ * (1 + dh.abs() * 2.0 ** -4)
    return TRANS * torch.stack([mx, my, mx, my], 2)


@pytest.mark.parametrize('m,K', [(1000, 2), (1, 2), (257, 5), (64, 8)])
def test_box_decode_softmax_clip(lib, m, K):
    g = torch.Generator().manual_seed(71)
    if K == 2:
        logits, deltas, props = [t.float() for t in R.detection_inputs(3, m)]
    else:
        props = quarter_pixel_boxes(m, 9, 100).float() + torch.rand(m, 4, generator=g) * 0.2
        logits = torch.randn(m, K, generator=g) * 4
        deltas = torch.randn(m, 4 * K, generator=g) * torch.tensor([1., 1., .5, .5] * K)
    deltas[0, 2::4] = 40.0       # dw far above the clamp
    n = m * (K - 1)
    bo, sc, la = Out((n, 4)), Out((n,)), Out((n,), torch.int64)
    a, b, c = logits.cuda(), deltas.cuda(), props.cuda()
    H, W = R.IMAGE
    lib.call('sfvos_box_decode', P(a), P(b), P(c), m, K, 1, 10.0, 10.0, 5.0, 5.0, R.BBOX_XFORM_CLIP, float(H), float(W),
             P(bo.t), P(sc.t), P(la.t), S())
    torch.cuda.synchronize()
    rb, rs, rl = R.candidates(logits.double(), deltas.double(), props.double(), R.IMAGE)
    allow = decode_allowance(deltas, props, K)[:, 1:].reshape(-1, 4)
    tag = 'box_decode (%d,%d) ' % (m, K)
    check_abs(tag + 'boxes', bo.cpu(), rb, allow)     # clipping is monotone: the allowance of the unclipped value holds
    z = logits.double()
    zmax = (z - z.max(1, keepdim=True).values)
    # softmax = exp(z_k - max) / sum: 2^-20 of the value for the evaluation, and the fp32 rounding of z_k - max (2^-24
    # |z_k - max|, carried at slope p) in numerator and denominator
    carry = (zmax.abs().max(1, keepdim=True).values * 2.0 ** -23)[:, :1].expand(m, K - 1).reshape(-1)
    check_abs(tag + 'scores', sc.cpu(), rs, rs * (TRANS + carry) + 2.0 ** -126)
    assert torch.equal(la.cpu(), rl)
    assert bool((bo.cpu()[:, 0::2] >= 0).all()) and bool((bo.cpu()[:, 0::2] <= W).all())
    # plain decode (all classes, no clipping, no scores): the Python decode_boxes path
    bo2 = Out((m * K, 4))
    lib.call('sfvos_box_decode', None, P(b), P(c), m, K, 0, 10.0, 10.0, 5.0, 5.0, R.BBOX_XFORM_CLIP, 0.0, 0.0, P(bo2.t),
             None, None, S())
    torch.cuda.synchronize()
    check_abs(tag + 'all classes, unclipped', bo2.cpu(), R.decode_boxes(deltas.double(), props.double()).reshape(-1, 4),
              decode_allowance(deltas, props, K).reshape(-1, 4))


@pytest.mark.parametrize('m', [1, 300])
def test_box_encode(lib, m):
    g = torch.Generator().manual_seed(72)
    props = quarter_pixel_boxes(m, 10, 100).float() + torch.rand(m, 4, generator=g) * 0.2
    ref_boxes = quarter_pixel_boxes(m, 11, 100).float()
    out = Out((m, 4))
    a, b = ref_boxes.cuda(), props.cuda()
    lib.call('sfvos_box_encode', P(a), P(b), m, 10.0, 10.0, 5.0, 5.0, P(out.t), S())
    torch.cuda.synchronize()
    want = R.encode_boxes(ref_boxes.double(), props.double())
    # centre terms: w (|gcx| + |pcx|) / pw; size terms: w (|log| + 1): the rounding of the ratio enters the log at slope 1
    p, r = props.double(), ref_boxes.double()
    pw, ph = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    gcx, gcy = (r[:, 0] + r[:, 2]).abs() / 2, (r[:, 1] + r[:, 3]).abs() / 2
    pcx, pcy = (p[:, 0] + p[:, 2]).abs() / 2, (p[:, 1] + p[:, 3]).abs() / 2
    allow = TRANS * torch.stack([10 * (gcx + pcx) / pw, 10 * (gcy + pcy) / ph, 5 * (want[:, 2].abs() / 5 + 1),
                                 5 * (want[:, 3].abs() / 5 + 1)], 1)
    check_abs('box_encode %d' % m, out.cpu(), want, allow)


def test_box_scale(lib):
    b = torch.tensor([[1.5, 2.25, 3.0, 4.0], [0.0, 7.0, 9.0, 11.0]])
    out = Out((2, 4))
    bd = b.cuda()
    lib.call('sfvos_box_scale', P(bd), 2, 0.5, 3.0, P(out.t), S())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), b * torch.tensor([3.0, 0.5, 3.0, 0.5]))


# ---- detections -----------------------------------------------------------------------------------------------------------

def run_detections(lib, boxes, scores, labels, score_thresh, min_size, nms_thresh, max_det, per_roi=1, ratios=(1.0, 1.0)):
    n = boxes.shape[0]
    nbytes = lib.load().sfvos_detections_workspace_bytes(n)
    assert nbytes > 0
    ws = Out((nbytes // 4 + 1,), torch.float32, fill=float('nan'))
    cnt = Out((16,), torch.int32)
    ob, osc = Out((max_det, 4)), Out((max_det,))
    ol, oi, orr = Out((max_det,), torch.int64), Out((max_det,), torch.int32), Out((max_det,), torch.int32)
    a, b, c = boxes.float().cuda(), scores.float().cuda(), labels.to(torch.int64).cuda()
    lib.call('sfvos_detections', P(a), P(b), P(c), n, per_roi, score_thresh, min_size, nms_thresh, max_det, ratios[0],
             ratios[1], P(ws.t), P(cnt.t), P(ob.t), P(osc.t), P(ol.t), P(oi.t), P(orr.t), S())
    torch.cuda.synchronize()
    assert ws.guards_ok(), 'wrote outside the workspace'
    d = int(cnt.cpu()[0])
    assert bool((cnt.cpu()[1:] == int(-768)).all())
    oi_c = oi.cpu()
    assert bool((oi_c[d:] == -1).all()) and bool((osc.cpu()[d:] == 0).all())
    return d, ob.cpu(), osc.cpu(), ol.cpu(), oi_c, orr.cpu()


@pytest.mark.parametrize('case', ['distinct', 'ties', 'classes', 'one', 'many'])
def test_nms_alone_is_exact(lib, case):
    """Boxes on a quarter-pixel grid (areas, intersections and unions exact in fp32, IEEE division on both sides): the
    kept index list equals the restatement's -- pairs at IoU exactly 0.5 (not suppressed), tied scores (lower index
    first), several classes (never suppressing each other)."""
    n = {'one': 1, 'many': 3000}.get(case, 500)
    boxes = quarter_pixel_boxes(n, 20, 60 if case != 'many' else 200)
    g = torch.Generator().manual_seed(21)
    scores = torch.rand(n, generator=g).double()
    if case == 'ties':
        scores = (scores * 16).floor() / 16
    labels = torch.randint(1, 4, (n,), generator=g) if case in ('classes', 'many') else torch.ones(n, dtype=torch.int64)
    if n > 8:
        # IoU exactly 0.5 (inter 1, union 2), in score order right behind each other; and exactly above it
        boxes[:4] = torch.tensor([[300., 300., 302., 301.], [300., 300., 301., 301.],
                                  [310., 300., 312., 301.], [310., 300., 311.25, 301.]], dtype=torch.float64)
        scores[:4] = torch.tensor([0.99, 0.98, 0.97, 0.96], dtype=torch.float64)
        labels[:4] = 1
        assert float(R.box_iou(boxes[:1], boxes[1:2])) == 0.5 and float(R.box_iou(boxes[2:3], boxes[3:4])) > 0.5
    scores = scores.float().double()       # the kernel's fp32 scores
    want = R.batched_nms(boxes, scores, labels, 0.5)
    d, ob, osc, ol, oi, _ = run_detections(lib, boxes, scores, labels, -1.0, 0.0, 0.5, n)
    assert d == want.numel(), (d, want.numel())
    assert oi[:d].tolist() == want.tolist()
    assert torch.equal(ob[:d].double(), boxes[want]) and torch.equal(osc[:d].double(), scores[want])
    assert torch.equal(ol[:d], labels[want])
    if n > 8:
        kept = set(oi[:d].tolist())
        assert {0, 1, 2} <= kept and 3 not in kept
    print('nms %s: %d of %d kept' % (case, d, n))


def test_detections_filters_top_k_and_resize(lib):
    boxes = torch.tensor([[0., 0., 10., 10.], [20., 20., 30., 30.], [40., 40., 40.005, 50.], [60., 60., 70., 70.],
                          [0., 0., 10., 10.5], [80., 80., 90., 90.]])
    scores = torch.tensor([0.9, 0.05, 0.8, 0.7, float('nan'), 0.06])
    labels = torch.ones(6, dtype=torch.int64)
    # 1: score not above 0.05; 2: narrower than 1e-2; 4: NaN score; top 2 of the remaining (0, 3, 5)
    d, ob, osc, ol, oi, orr = run_detections(lib, boxes, scores, labels, 0.05, 1e-2, 0.5, 2, per_roi=2, ratios=(2.0, 0.5))
    assert d == 2 and oi.tolist() == [0, 3] and orr.tolist() == [0, 1]
    assert torch.equal(ob, torch.tensor([[0., 0., 5., 20.], [30., 120., 35., 140.]]))
    d, *_ = run_detections(lib, boxes, torch.zeros(6), labels, 0.05, 1e-2, 0.5, 4)
    assert d == 0


def test_detections_on_real_valued_boxes(lib):
    """Two stages.  (a) the kernel's fp32 candidates against float64, per element (test_box_decode_softmax_clip's
    allowances).  (b) threshold, small-box filter, NMS, ranking, top 100 against the restatement run on the kernel's own
    fp32 candidates: score order is exact, only the fp32 rounding of an IoU can differ, so seeds are compared when the
    restatement returns the same list at thresholds (0.05 +- 1e-5, 0.5 +- 1e-5); the others are reported as skipped and
    at most 2 of the 16 may be."""
    H, W = R.IMAGE
    skipped = []
    for seed in range(16):
        logits, deltas, props = [t.float() for t in R.detection_inputs(seed)]
        m, K = logits.shape
        n = m * (K - 1)
        bo, sc, la = Out((n, 4)), Out((n,)), Out((n,), torch.int64)
        a, b, c = logits.cuda(), deltas.cuda(), props.cuda()
        lib.call('sfvos_box_decode', P(a), P(b), P(c), m, K, 1, 10.0, 10.0, 5.0, 5.0, R.BBOX_XFORM_CLIP, float(H),
                 float(W), P(bo.t), P(sc.t), P(la.t), S())
        torch.cuda.synchronize()
        cb, cs, cl = bo.cpu(), sc.cpu(), la.cpu()
        rb, rs, _ = R.candidates(logits.double(), deltas.double(), props.double(), R.IMAGE)
        check_abs('detections seed %d candidate boxes' % seed, cb, rb,
                  decode_allowance(deltas, props, K)[:, 1:].reshape(-1, 4))
        zr = (logits.double()[:, 0] - logits.double()[:, 1]).abs()
        check_abs('detections seed %d candidate scores' % seed, cs, rs, rs * (TRANS + zr * 2.0 ** -23) + 2.0 ** -126)
        safe, want = R.margin_safe(cb.double(), cs.double(), cl)
        if not safe:
            skipped.append(seed)
            continue
        d, ob, osc, ol, oi, orr = run_detections(lib, cb, cs, cl, 0.05, 1e-2, 0.5, 100, per_roi=K - 1)
        assert d == want.numel() == 100
        assert oi[:d].tolist() == want.tolist(), 'seed %d' % seed
        assert torch.equal(ob[:d], cb[want]) and torch.equal(osc[:d], cs[want]) and torch.equal(ol[:d], cl[want])
        assert orr[:d].tolist() == (want // (K - 1)).tolist()
    print('detections: %d of 16 seeds compared, skipped (not margin-safe) %s' % (16 - len(skipped), skipped))
    assert len(skipped) <= 2, skipped
