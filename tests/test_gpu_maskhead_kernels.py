"""GPU: the mask-branch, loss and small helper kernels one by one, called through the C ABI (ctypes) like
test_gpu_kernels.py, each against the plain torch operation in float64 on the CPU on the operands the kernel sees
(bf16: rounded to bf16 first, then widened).

Pass criterion: the per-element bound of tests/kernel_util.py (its docstring), K stated beside each case.

Every output buffer has a guard band in front and behind (and sentinel-filled unused columns where it is pitched), the
body is sentinel-filled too, so an unwritten element shows as an error; workspaces and partial rows are NaN-filled.  No
element is left out of a comparison; where the contract says NaN the test asserts NaN.  Every test prints its worst
error / bound (pytest -s shows them)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kernel_util import (DT, FLT_MIN, PRECS, SENT, TDT, TRANS, U22, U_OUT, Out, P, S, check, check_abs,  # noqa: F401
                         lib, make_desc, rnd, to_pyr)

pytestmark = pytest.mark.gpu


# ---- ConvTranspose2d(2, 2, 0): packers, forward, data gradient, weight gradient ---------------------------------------

DECONV_CASES = [
    # n  h   w   c_in c_out
    (7, 14, 14, 256, 256),   # the module's; M = 1372 = 42 * 32 + 28
    (1, 1, 3, 32, 32),       # M < 32: one row tile; one column block; three idle waves in the data gradient
    (2, 3, 5, 96, 160),      # h != w; forward: five 128-column blocks; data gradient: 96 columns = 3 live waves of 4
    (1, 1, 1, 288, 32),      # one position
    (3, 14, 14, 64, 96),
]


def deconv_operands(case, prec, seed):
    n, h, w, cin, cout = case
    g = torch.Generator().manual_seed(seed)
    x = rnd(torch.randn(n, h, w, cin, generator=g), prec)
    wt = torch.randn(cin, cout, 2, 2, generator=g) / np.sqrt(cin)
    bias = torch.randn(cout, generator=g) * 0.3
    dz = rnd(torch.randn(n, 2 * h, 2 * w, cout, generator=g), prec)
    return x, wt, bias, dz


def nchw(t):
    return t.permute(0, 3, 1, 2).double()


def nhwc(t):
    return t.permute(0, 2, 3, 1)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('cin,cout', [(32, 32), (96, 160), (288, 32), (256, 256)])
def test_deconv_packers_are_exact_permutations(lib, prec, cin, cout):
    """sfvos_pack_deconv2x2: wp[(a*2+b)*Cout + co][ci]; sfvos_pack_deconv2x2_dgrad: wd[ci][(a*2+b)*Cout + co]; the bf16
    image is the rounded (nearest even) fp32 image.  Ties (1 + 2^-8, 1 + 3 * 2^-8) are among the values."""
    g = torch.Generator().manual_seed(5)
    w = torch.randn(cin, cout, 2, 2, generator=g)
    w.view(-1)[:4] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8)])
    wd = w.cuda()
    fwd, dgr = Out((4 * cout, cin), TDT[prec]), Out((cin, 4 * cout), TDT[prec])
    lib.call('sfvos_pack_deconv2x2', P(wd), P(fwd.t), DT(lib, prec), cin, cout, S())
    lib.call('sfvos_pack_deconv2x2_dgrad', P(wd), P(dgr.t), DT(lib, prec), cin, cout, S())
    torch.cuda.synchronize()
    assert torch.equal(fwd.cpu(), w.permute(2, 3, 1, 0).reshape(4 * cout, cin).to(TDT[prec]))
    assert torch.equal(dgr.cpu(), w.permute(0, 2, 3, 1).reshape(cin, 4 * cout).to(TDT[prec]))
    print('packers %s %dx%d exact' % (prec, cin, cout))


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('relu,with_bias', [(1, True), (0, True), (1, False)])
@pytest.mark.parametrize('case', DECONV_CASES)
def test_deconv2x2_forward(lib, prec, case, relu, with_bias):
    """K = c_in (one MFMA chain over the input channels), then the bias add."""
    n, h, w, cin, cout = case
    x, wt, bias, _ = deconv_operands(case, prec, 11)
    wr = rnd(wt, prec)
    b64 = bias.double() if with_bias else None
    ref = nhwc(F.conv_transpose2d(nchw(x), wr.double(), b64, stride=2))
    mag = nhwc(F.conv_transpose2d(nchw(x).abs(), wr.double().abs(), b64.abs() if with_bias else None, stride=2))
    wp = torch.empty(4 * cin * cout, dtype=TDT[prec], device='cuda')
    wtd = wt.cuda()
    lib.call('sfvos_pack_deconv2x2', P(wtd), P(wp), DT(lib, prec), cin, cout, S())
    y = Out((n, 2 * h, 2 * w, cout), TDT[prec])
    xd, bd = x.to(TDT[prec]).cuda(), bias.cuda()     # named: two temporaries in one call would share their memory
    lib.call('sfvos_deconv2x2_relu', P(xd), P(wp), P(bd) if with_bias else None, P(y.t),
             DT(lib, prec), n, h, w, cin, cout, relu, S())
    torch.cuda.synchronize()
    check('deconv fwd %s %s relu %d bias %d' % (prec, case, relu, with_bias), y.cpu(),
          ref.clamp_min(0) if relu else ref, mag, cin, U_OUT[prec])   # u_out * |post-ReLU ref|: 0 where ref < 0, tighter than the docstring allows


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', DECONV_CASES)
def test_deconv2x2_dgrad(lib, prec, case):
    """K = 4 * c_out: the four sub-positions of a pixel run through one accumulator."""
    n, h, w, cin, cout = case
    _, wt, _, dz = deconv_operands(case, prec, 12)
    wr = rnd(wt, prec).double()

    def grad(g, wv):
        xin = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(xin, wv, None, stride=2).backward(g)
        return nhwc(xin.grad)
    ref, mag = grad(nchw(dz), wr), grad(nchw(dz).abs(), wr.abs())
    wd = torch.empty(4 * cin * cout, dtype=TDT[prec], device='cuda')
    wtd, dzd = wt.cuda(), dz.to(TDT[prec]).cuda()
    lib.call('sfvos_pack_deconv2x2_dgrad', P(wtd), P(wd), DT(lib, prec), cin, cout, S())
    dx = Out((n, h, w, cin), TDT[prec])
    lib.call('sfvos_deconv2x2_dgrad', P(dzd), P(wd), P(dx.t), DT(lib, prec), n, h, w, cin, cout, S())
    torch.cuda.synchronize()
    check('deconv dgrad %s %s' % (prec, case), dx.cpu(), ref, mag, 4 * cout, U_OUT[prec])


def deconv_wgrad_split(M):
    """(splits, per_split) as sfvos_deconv2x2_wgrad picks them: >= 256 positions per split, at most 64 splits, whole
    k-pairs."""
    splits = min(64, max(1, -(-M // 256)))
    per = -(-M // splits)
    return splits, (per + 1) & ~1


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', DECONV_CASES + [
    (1, 1, 257, 32, 64),     # M = 257: two splits, per_split 129 rounded up to 130
    (90, 14, 14, 32, 32),    # M = 17640: the 64-split cap, per_split 276 = 17 * 16 + 4 (ragged 16-row unroll)
])
def test_deconv2x2_wgrad(lib, prec, case):
    """K = per_split + splits (+ 1 with accumulate): a split is one MFMA chain over its positions, sfvos_reduce_rows
    combines the split rows (in f64, rounded once).  M = 17640: 276 + 64.  Bit-identical from run to run; the workspace
    is exactly sfvos_deconv2x2_wgrad_workspace_bytes, NaN-filled, with a guard behind it."""
    n, h, w, cin, cout = case
    x, _, _, dz = deconv_operands(case, prec, 13)
    M = n * h * w
    splits, per = deconv_wgrad_split(M)
    if M == 257:
        assert (splits, per) == (2, 130)
    if M == 17640:
        assert (splits, per) == (64, 276)

    def grad(xv, g):
        wv = torch.zeros(cin, cout, 2, 2, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(xv, wv, None, stride=2).backward(g)
        return wv.grad
    ref, mag = grad(nchw(x), nchw(dz)), grad(nchw(x).abs(), nchw(dz).abs())
    nbytes = lib.load().sfvos_deconv2x2_wgrad_workspace_bytes(n, h, w, cin, cout)
    assert nbytes == splits * cin * cout * 4 * 4
    xd, dzd = x.to(TDT[prec]).cuda(), dz.to(TDT[prec]).cuda()
    g0 = torch.Generator().manual_seed(14)
    old = torch.randn(cin, cout, 2, 2, generator=g0)
    runs = []
    for rep in range(2):
        ws = Out((nbytes // 4,), torch.float32, fill=float('nan'))
        gw = Out((cin, cout, 2, 2))
        lib.call('sfvos_deconv2x2_wgrad', P(xd), P(dzd), DT(lib, prec), n, h, w, cin, cout, P(gw.t), 0, P(ws.t), S())
        torch.cuda.synchronize()
        assert ws.guards_ok(), 'wrote outside the workspace'
        runs.append(gw.cpu().clone())
    check('deconv wgrad %s %s splits %d x %d' % (prec, case, splits, per), runs[0], ref, mag, per + splits, 0.0)
    assert torch.equal(runs[0], runs[1]), 'the weight gradient must be bit-identical from run to run'
    ws = Out((nbytes // 4,), torch.float32, fill=float('nan'))
    gw = Out((cin, cout, 2, 2))
    gw.t.copy_(old)
    lib.call('sfvos_deconv2x2_wgrad', P(xd), P(dzd), DT(lib, prec), n, h, w, cin, cout, P(gw.t), 1, P(ws.t), S())
    torch.cuda.synchronize()
    assert ws.guards_ok()
    check('deconv wgrad %s %s accumulate' % (prec, case), gw.cpu(), old.double() + ref, old.double().abs() + mag,
          per + splits + 1, 0.0)


# ---- mask_fcn_logits: conv1x1 C -> K, sigmoid of the label's channel ----------------------------------------------------

def logits_operands(n, pos, C, K, prec, seed, wscale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = rnd(torch.randn(n, pos, C, generator=g), prec)
    w = torch.randn(K, C, generator=g) * (wscale / np.sqrt(C))
    bias = torch.randn(K, generator=g) * 0.5
    labels = torch.randint(0, K, (n,), generator=g)
    return x, w, bias, labels


def run_mask_logits(lib, prec, x, w, bias, labels, want_logits, want_prob):
    n, pos, C = x.shape
    K = w.shape[0]
    lo = Out((n, K, pos)) if want_logits else None
    pr = Out((n, 1, pos)) if want_prob else None
    xd, wd = x.to(TDT[prec]).cuda(), w.cuda()
    bd = bias.cuda() if bias is not None else None
    ld = labels.cuda() if labels is not None else None
    lib.call('sfvos_mask_logits', P(xd), DT(lib, prec), P(wd), P(bd) if bd is not None else None,
             P(ld) if ld is not None else None,
             n, pos, C, K, P(lo.t) if lo else None, P(pr.t) if pr else None, S())
    torch.cuda.synchronize()
    return (lo.cpu() if lo else None), (pr.cpu() if pr else None)


def logits_ref(x, w, bias):
    ref = torch.einsum('npc,kc->nkp', x.double(), w.double())
    mag = torch.einsum('npc,kc->nkp', x.double().abs(), w.double().abs())
    if bias is not None:
        ref, mag = ref + bias.double()[None, :, None], mag + bias.double().abs()[None, :, None]
    return ref, mag


def check_prob(name, prob, ref, mag, labels, C, own_logits=None):
    """prob = sigmoid(s), s = the kernel's fp32 logit.  Two comparisons, both in float64:
    * against sigmoid(z) of the float64 logit z: |s - z| <= zb (the derived bound of the logit) and the sigmoid is
      monotone, so sigmoid(s) lies between sigmoid(z - zb) and sigmoid(z + zb); the allowance is that distance, taken
      where it acts (it vanishes where the sigmoid is flat), plus 2^-20 * sigmoid(z + zb) + 2^-126 for the evaluation;
    * where the same call returned its logits (already checked against float64, and the kernel takes the sigmoid of
      exactly the value it stores): against the float64 sigmoid of those logits under the bare 2^-20 * p + 2^-126, which
      pins the transcendental itself at 16 ulps everywhere, the saturated ends included."""
    n = ref.shape[0]
    rows = torch.arange(n)
    z = ref[rows, labels]
    zb = 2.0 * (C + 1) * U22 * mag[rows, labels]
    p, hi, lo = torch.sigmoid(z), torch.sigmoid(z + zb), torch.sigmoid(z - zb)
    worst = check_abs(name, prob[:, 0], p, TRANS * hi + FLT_MIN + torch.maximum(hi - p, p - lo))
    if own_logits is not None:
        q = torch.sigmoid(own_logits.double()[rows, labels])
        worst = max(worst, check_abs(name + ' vs its own logits', prob[:, 0], q, TRANS * q + FLT_MIN))
    return worst


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', [(7, 784, 256, 2), (1, 5, 32, 1), (3, 49, 96, 8), (2, 10, 512, 11)])
def test_mask_logits(lib, prec, case):
    """K = C: a lane adds C / 64 products, six shuffle steps and the bias follow (C = 32: half the lanes idle).
    (1,5,32,1): labels = NULL and bias = NULL; (2,10,512,11): the forward has no class cap.  logits only, prob only and
    both must give the same values."""
    n, pos, C, K = case
    x, w, bias, labels = logits_operands(n, pos, C, K, prec, 21)
    if K == 1:
        bias, labels_arg = None, None
    else:
        labels_arg = labels
    ref, mag = logits_ref(x, w, bias)
    lo1, _ = run_mask_logits(lib, prec, x, w, bias, labels_arg, True, False)
    _, pr2 = run_mask_logits(lib, prec, x, w, bias, labels_arg, False, True)
    lo3, pr3 = run_mask_logits(lib, prec, x, w, bias, labels_arg, True, True)
    tag = 'mask_logits %s %s ' % (prec, case)
    check(tag + 'logits', lo1, ref, mag, C, 0.0)
    assert torch.equal(lo1, lo3)
    lab = labels if K > 1 else torch.zeros(n, dtype=torch.long)
    assert torch.equal(pr2, pr3)
    check_prob(tag + 'prob', pr3, ref, mag, lab, C, own_logits=lo3)


@pytest.mark.parametrize('prec', PRECS)
def test_mask_logits_bad_labels_give_nan_for_their_roi_only(lib, prec):
    n, pos, C, K = 3, 49, 96, 8
    x, w, bias, _ = logits_operands(n, pos, C, K, prec, 22)
    labels = torch.tensor([8, 2, -1])          # out of range, valid, negative
    ref, mag = logits_ref(x, w, bias)
    for want_logits in (True, False):
        lo, pr = run_mask_logits(lib, prec, x, w, bias, labels, want_logits, True)
        if want_logits:
            check('mask_logits bad labels %s logits' % prec, lo, ref, mag, C, 0.0)   # every RoI's logits stay defined
        assert bool(torch.isnan(pr[0]).all()) and bool(torch.isnan(pr[2]).all())
        check_prob('mask_logits bad labels %s prob of the valid RoI' % prec, pr[1:2], ref[1:2], mag[1:2],
                   labels[1:2], C, own_logits=lo[1:2] if want_logits else None)


@pytest.mark.parametrize('prec', PRECS)
def test_mask_logits_sigmoid_saturates(lib, prec):
    """Weights scaled until the logits reach about +-100: prob is within the allowance of the float64 sigmoid (which
    leaves only exactly 1 above z = 17.4 and at most 2^-126 below z = -88) and of the sigmoid of its own logits, never
    NaN."""
    n, pos, C, K = 2, 300, 256, 3
    x, w, bias, labels = logits_operands(n, pos, C, K, prec, 23, wscale=40.0)
    ref, mag = logits_ref(x, w, bias)
    assert float(ref.max()) > 90 and float(ref.min()) < -90
    lo, pr = run_mask_logits(lib, prec, x, w, bias, labels, True, True)
    check('mask_logits saturating %s logits' % prec, lo, ref, mag, C, 0.0)
    check_prob('mask_logits saturating %s prob' % prec, pr, ref, mag, labels, C, own_logits=lo)
    assert bool(((pr >= 0) & (pr <= 1)).all())
    z = ref[torch.arange(n), labels]
    assert bool((pr[:, 0][z < -110] == 0).all())     # below the smallest fp32 denormal


# ---- backward of mask_fcn_logits and of the ReLU in front of it ----------------------------------------------------------

@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('relu', [1, 0])
@pytest.mark.parametrize('case', [
    (9, 784, 256, 2),    # the module's
    (1, 3, 64, 1),       # 3 of a block's 64 pixels; a quarter of its 256 column threads
    (2, 41, 128, 5),     # 82 pixels: the first block spans both RoIs, the second has 18
    (3, 196, 512, 6),    # the largest C: two column blocks
    (2, 100, 512, 8),    # the largest C with the most classes
])
def test_mask_logits_bwd(lib, prec, case, relu):
    """dz: K = num_classes.  The three partial blocks (weight gradient | logits-bias gradient | column sums of dz) after
    sfvos_reduce_rows: K = 64 + rows (a block sums its 64 pixels in fp32, one after the other;
    sfvos_reduce_rows adds the rows in f64).  The column sums are those of the unrounded dz.  y holds exact zeros, -0.0
    and a few negative values; part is exactly sfvos_mask_logits_bwd_rows rows, NaN-filled."""
    n, pos, C, K = case
    g = torch.Generator().manual_seed(31)
    y = torch.randn(n, pos, C, generator=g).clamp_min(0)
    y.view(-1)[::7] = -0.0
    y.view(-1)[3::11] = 0.0
    y.view(-1)[5::53] = -0.25
    y = rnd(y, prec)
    dl = torch.randn(n, K, pos, generator=g)
    w = torch.randn(K, C, generator=g) / np.sqrt(C)
    live = (y > 0) if relu else torch.ones_like(y, dtype=torch.bool)
    zero = torch.zeros((), dtype=torch.float64)
    dz_ref = torch.where(live, torch.einsum('nkp,kc->npc', dl.double(), w.double()), zero)
    dz_mag = torch.where(live, torch.einsum('nkp,kc->npc', dl.double().abs(), w.double().abs()), zero)
    rows = lib.load().sfvos_mask_logits_bwd_rows(n, pos)
    assert rows == -(-n * pos // 64)
    L = K * C + K + C
    dz, part, red = Out((n, pos, C), TDT[prec]), Out((rows, L), fill=float('nan')), Out((L,))
    yd, dld, wd = y.to(TDT[prec]).cuda(), dl.cuda(), w.cuda()
    lib.call('sfvos_mask_logits_bwd', P(yd), DT(lib, prec), P(dld), P(wd), n, pos, C, K,
             relu, P(dz.t), P(part.t), S())
    lib.call('sfvos_reduce_rows', P(part.t), rows, L, P(red.t), 0, S())
    torch.cuda.synchronize()
    tag = 'mask_logits_bwd %s %s relu %d ' % (prec, case, relu)
    check(tag + 'dz', dz.cpu(), dz_ref, dz_mag, K, U_OUT[prec])
    assert bool(torch.isfinite(part.cpu()).all()), 'a partial row was not written'
    r = red.cpu()
    Kp = 64 + rows
    check(tag + 'grad w', r[:K * C].view(K, C), torch.einsum('nkp,npc->kc', dl.double(), y.double()),
          torch.einsum('nkp,npc->kc', dl.double().abs(), y.double().abs()), Kp, 0.0)
    check(tag + 'grad logits bias', r[K * C:K * C + K], dl.double().sum((0, 2)), dl.double().abs().sum((0, 2)), Kp, 0.0)
    check(tag + 'grad deconv bias', r[K * C + K:], dz_ref.sum((0, 1)), dz_mag.sum((0, 1)), Kp, 0.0)


# ---- ReLU backward + column sums ---------------------------------------------------------------------------------------------

# One column block (up to 64 16-byte chunks per row) of a power-of-two chunk count (1, 8 and 64): the mask head's path
RELU_CASES = [(prec, c, m) for m in (1, 63, 64, 65, 1764)
              for prec, c in (('fp32', 4), ('fp32', 32), ('fp32', 256), ('bf16', 8), ('bf16', 64), ('bf16', 512))]
# Tiled over columns: 65 chunks = a second block of one chunk (fp32 260, bf16 520); blocks that are no power of two,
# with idle threads: 24 / 12 and 48 chunks (96, bf16 384), 75 = 64 + 11 (fp32 300); the box head's 1024 = 4 / 2 blocks
RELU_CASES += [(prec, c, m) for m in (1, 63, 64, 65, 130)
               for prec, c in (('fp32', 260), ('bf16', 520), ('fp32', 96), ('bf16', 96), ('bf16', 384), ('fp32', 300),
                               ('fp32', 1024), ('bf16', 1024))]
RELU_CASES += [('fp32', 1024, 1000), ('bf16', 1024, 1000), ('bf16', 32, 1)]


@pytest.mark.parametrize('prec,c,m', RELU_CASES, ids=['%d-%s-%d' % (m, prec, c) for prec, c, m in RELU_CASES])
def test_relu_bwd(lib, prec, c, m):
    """dz is exact; a partial row sums at most 64 positions (K = 64), the total
    behind sfvos_reduce_rows has K = 64 + rows.  a holds 0, -0.0 and NaN: `a > 0` is false there, the gradient is 0 (what
    torch.where(a > 0, dy, 0) gives in float64).  Variants: all outputs, a = NULL, dz = NULL, col_part = NULL, in place."""
    g = torch.Generator().manual_seed(41)
    dy = rnd(torch.randn(m, c, generator=g), prec)
    a = rnd(torch.randn(m, c, generator=g), prec)
    a.view(-1)[::5] = 0.0
    a.view(-1)[1::7] = -0.0
    a.view(-1)[2::13] = float('nan')
    rows = lib.load().sfvos_relu_bwd_rows(m)
    assert rows == -(-m // 64)
    dyd, ad = dy.to(TDT[prec]).cuda(), a.to(TDT[prec]).cuda()
    for variant in ('all', 'a_null', 'dz_null', 'part_null', 'in_place'):
        want = dy if variant == 'a_null' else torch.where(a > 0, dy, torch.zeros(()))
        dz = Out((m, c), TDT[prec])
        if variant == 'in_place':
            dz.t.copy_(dyd)
        part, red = Out((rows, c), fill=float('nan')), Out((c,))
        src = dz.t if variant == 'in_place' else dyd
        lib.call('sfvos_relu_bwd', P(src), None if variant == 'a_null' else P(ad),
                 None if variant == 'dz_null' else P(dz.t), DT(lib, prec), m, c,
                 None if variant == 'part_null' else P(part.t), S())
        if variant != 'part_null':
            lib.call('sfvos_reduce_rows', P(part.t), rows, c, P(red.t), 0, S())
        torch.cuda.synchronize()
        tag = 'relu_bwd %s m %d c %d %s ' % (prec, m, c, variant)
        if variant == 'dz_null':
            assert bool((dz.cpu() == SENT).all())
        else:
            assert torch.equal(dz.cpu().float(), want), tag + 'dz'
        if variant == 'part_null':
            assert bool(torch.isnan(part.cpu()).all())
            continue
        w64 = want.double()
        pad = torch.zeros(rows * 64 - m, c, dtype=torch.float64)
        blocks = torch.cat([w64, pad]).view(rows, 64, c)
        check(tag + 'partial rows', part.cpu(), blocks.sum(1), blocks.abs().sum(1), 64, 0.0)
        check(tag + 'column sums', red.cpu(), w64.sum(0), w64.abs().sum(0), 64 + rows, 0.0)


# ---- maskrcnn_loss: BCE with logits on the label's channel ------------------------------------------------------------------

def bce_operands(n, K, pos, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, K, pos, generator=g) * 3
    special = torch.tensor([0.0, 88.8, -88.8, 1e4, -1e4, -0.0, 20.0, -20.0])
    flat = z.view(-1)
    k = min(flat.numel(), 4 * special.numel())
    flat[:k] = special.repeat(4)[:k]
    z = flat[torch.randperm(flat.numel(), generator=g)].view(n, K, pos).contiguous()
    t = torch.rand(n, pos, generator=g)                       # soft targets (RoIAligned masks) ...
    hard = torch.rand(n, pos, generator=g) < 0.5              # ... and exact 0 / 1
    t = torch.where(hard, (t > 0.5).float(), t)
    labels = torch.randint(0, K, (n,), generator=g)
    return z, t, labels


def bce_ref(z, t, labels, up):
    """float64: loss, its magnitude (max(z,0) + |z t| + log1p(exp(-|z|)), mean), dlogits and its magnitude."""
    n, K, pos = z.shape
    z64 = z.double().requires_grad_(True)
    sel = z64[torch.arange(n), labels]
    loss = F.binary_cross_entropy_with_logits(sel, t.double())
    (loss * up).backward()
    s = sel.detach()
    lmag = (s.clamp_min(0) + (s * t.double()).abs() + torch.log1p(torch.exp(-s.abs()))).mean()
    gmag = torch.zeros(n, K, pos, dtype=torch.float64)
    gmag[torch.arange(n), labels] = (torch.sigmoid(s) + t.double() + FLT_MIN / TRANS) * abs(up) / (n * pos)
    return loss.detach(), lmag, z64.grad, gmag


@pytest.mark.parametrize('upstream', [None, -2.5])
@pytest.mark.parametrize('case', [(9, 2, 784), (1, 1, 1), (3, 8, 333)])
def test_mask_bce_loss_and_grad(lib, case, upstream):
    """n * positions below and above the 1024 threads of the loss block and not a multiple of it; logits with 0, -0.0,
    +-20, +-88.8 (expf over / underflows beside it) and +-1e4; soft and hard targets; upstream NULL and a device scalar.
    Channels other than the label's have a zero allowance: exactly 0."""
    n, K, pos = case
    z, t, labels = bce_operands(n, K, pos, 51)
    up = 1.0 if upstream is None else upstream
    loss_ref, lmag, g_ref, gmag = bce_ref(z, t, labels, up)
    zd, td, ld = z.cuda(), t.cuda(), labels.cuda()
    upd = None if upstream is None else torch.tensor([upstream], device='cuda')
    loss, dl = Out((1,)), Out((n, K, pos))
    lib.call('sfvos_mask_bce_loss', P(zd), P(ld), P(td), n, K, pos, P(loss.t), S())
    lib.call('sfvos_mask_bce_loss_grad', P(zd), P(ld), P(td), P(upd) if upd is not None else None, n, K, pos, P(dl.t), S())
    torch.cuda.synchronize()
    tag = 'mask_bce %s upstream %s ' % (case, upstream)
    check_abs(tag + 'loss', loss.cpu()[0], loss_ref, TRANS * lmag)
    check_abs(tag + 'dlogits', dl.cpu(), g_ref, TRANS * gmag)
    off = torch.ones(n, K, pos, dtype=torch.bool)
    off[torch.arange(n), labels] = False
    assert bool((dl.cpu()[off] == 0).all())


def test_mask_bce_bad_label_gives_nan_loss_and_zero_gradient(lib):
    n, K, pos = 3, 8, 333
    z, t, labels = bce_operands(n, K, pos, 52)
    for bad in (K, -1):
        lab = labels.clone()
        lab[1] = bad
        loss, dl = Out((1,)), Out((n, K, pos))
        zd, ld, td = z.cuda(), lab.cuda(), t.cuda()
        lib.call('sfvos_mask_bce_loss', P(zd), P(ld), P(td), n, K, pos, P(loss.t), S())
        lib.call('sfvos_mask_bce_loss_grad', P(zd), P(ld), P(td), None, n, K, pos, P(dl.t), S())
        torch.cuda.synchronize()
        assert bool(torch.isnan(loss.cpu()).all())
        got = dl.cpu()
        assert bool((got[1] == 0).all()), 'the RoI with the bad label must get a zero gradient'
        keep = torch.tensor([0, 2])
        # the other RoIs: the gradient of the loss over all n RoIs (same 1 / (n * positions))
        _, _, g_ref, gmag = bce_ref(z, t, torch.where(lab == bad, torch.zeros_like(lab), lab), 1.0)
        check_abs('mask_bce bad label %d dlogits of the other RoIs' % bad, got[keep], g_ref[keep], TRANS * gmag[keep])


# ---- stand-in MSE loss, called directly --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('numels', [[1], [7], [1, 7, 7, 1, 1030, 7, 1, 7]])
def test_mse_loss_direct_call(lib, numels):
    """upstream = NULL, a one-tensor and a SFVOS_MAX_LEVELS-tensor table, numel 1 and 7 (no whole 16-byte group; all but
    the first tensor of a table sit at unaligned addresses of one buffer).  Value: each term passes three fp32 roundings
    (difference, square, and the last store; the sums run in f64): K = 1 with mag = sum_l mean((|o| + |t|)^2).
    Gradient 2 (o - t) / numel: three roundings, K = 1 with mag = 2 (|o| + |t|) / numel."""
    assert len(numels) in (1, lib.MAX_LEVELS)
    g = torch.Generator().manual_seed(61)
    total = sum(numels) + 3 * len(numels)
    o, t = torch.randn(total, generator=g), torch.randn(total, generator=g)
    od, td = o.cuda(), t.cuda()
    gr = Out((total,))
    tab = lib.MseTable()
    tab.n = len(numels)
    off, spans = 0, []
    for l, k in enumerate(numels):
        tab.out[l], tab.target[l], tab.grad[l] = od.data_ptr() + 4 * off, td.data_ptr() + 4 * off, gr.t.data_ptr() + 4 * off
        tab.numel[l] = k
        spans.append((off, k))
        off += k + 3
    rows = lib.load().sfvos_mse_loss_rows(ctypes.byref(tab))
    assert rows > 0
    part, loss = Out((rows,), fill=float('nan')), Out((1,))
    lib.call('sfvos_mse_loss', ctypes.byref(tab), P(part.t), P(loss.t), S())
    lib.call('sfvos_mse_loss_grad', ctypes.byref(tab), None, S())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(part.cpu()).all())
    o64, t64 = o.double(), t.double()
    ref = sum(((o64[a:a + k] - t64[a:a + k]) ** 2).mean() for a, k in spans)
    mag = sum(((o64[a:a + k].abs() + t64[a:a + k].abs()) ** 2).mean() for a, k in spans)
    check('mse_loss %s value' % numels, loss.cpu()[0], ref, mag, 1, 0.0)
    got = gr.cpu()
    written = torch.zeros(total, dtype=torch.bool)
    for a, k in spans:
        written[a:a + k] = True
        check('mse_loss %s grad' % numels, got[a:a + k], 2 * (o64[a:a + k] - t64[a:a + k]) / k,
              2 * (o64[a:a + k].abs() + t64[a:a + k].abs()) / k, 1, 0.0)
    assert bool((got[~written] == SENT).all()), 'wrote between the gradient tensors'


# ---- eval-mode BatchNorm coefficients -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', [32, 224])
def test_bn_eval_coeffs(lib, C):
    """scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale, mean = running_mean,
    rstd = 1 / sqrt(running_var + eps); one running_var entry is 0.  64 threads per block: 32 is half a block, 224 = 3.5.
    At most six fp32 roundings of <= 2^-23 (add, sqrt, divide, two products, subtract) lie between the inputs and any
    output: K = 2 with mag = the output's terms in absolute value (6 * 2^-22 * mag)."""
    g = torch.Generator().manual_seed(71)
    gamma, beta, rm = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g) * 2
    rv[3] = 0.0
    eps = 1e-5
    outs = [Out((C,)) for _ in range(4)]
    ins = [t.cuda() for t in (gamma, beta, rm, rv)]
    lib.call('sfvos_bn_eval_coeffs', *[P(t) for t in ins], eps, C,
             *[P(o.t) for o in outs], S())
    torch.cuda.synchronize()
    mean, rstd, scale, shift = [o.cpu() for o in outs]
    eps32 = float(np.float32(eps))
    r = 1.0 / torch.sqrt(rv.double() + eps32)
    assert torch.equal(mean, rm)
    check('bn_eval_coeffs C %d rstd' % C, rstd, r, r, 2, 0.0)
    check('bn_eval_coeffs C %d scale' % C, scale, gamma.double() * r, (gamma.double() * r).abs(), 2, 0.0)
    check('bn_eval_coeffs C %d shift' % C, shift, beta.double() - rm.double() * gamma.double() * r,
          beta.double().abs() + (rm.double() * gamma.double() * r).abs(), 2, 0.0)


# ---- max |x| over strided frames ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(3, 5, 7, 13), (5, 64, 12, 21), (1, 1, 1, 1)])   # 1365 elements: no whole block
def test_frames_absmax(lib, shape):
    """Strided source as in the layout test (the [C,T,H,W] view of a frame stack), cut out of a larger tensor whose
    border holds huge values that must not be read.  Exact (a maximum has no rounding); an initial *amax above the data
    stays, one below is replaced; one huge negative element is found; bit-equal from run to run."""
    T, C, H, W = shape
    g = torch.Generator().manual_seed(81)
    big = torch.full((T, C, H + 2, W + 3), 1e30)
    frames = torch.randn(T, C, H, W, generator=g)
    big[:, :, 1:H + 1, 2:W + 2] = frames
    view = big.cuda()[:, :, 1:H + 1, 2:W + 2].unsqueeze(0).transpose(1, 2)[0]     # [C,T,H,W]
    args = (view.stride(1), view.stride(0), view.stride(2), view.stride(3), T, C, H, W)
    want = frames.abs().max()

    def run(src, start):
        amax = Out((1,))
        amax.t.fill_(start)
        lib.call('sfvos_frames_absmax', P(src), *args, P(amax.t), S())
        torch.cuda.synchronize()
        return amax.cpu()[0]
    first = run(view, 0.0)
    assert torch.equal(first, want) and torch.equal(run(view, 0.0), first)
    assert float(run(view, 1e3)) == 1e3                               # larger than the data's: kept
    assert torch.equal(run(view, float(want) / 2), want)              # smaller: replaced
    big2 = big.clone()
    big2[T - 1, C - 1, H, W + 1] = -3.5e7                             # the last element of the cut-out
    view2 = big2.cuda()[:, :, 1:H + 1, 2:W + 2].unsqueeze(0).transpose(1, 2)[0]
    assert float(run(view2, 0.0)) == 3.5e7
    print('frames_absmax %s exact' % (shape,))


# ---- the 3x3 convs of the mask head: sfvos_conv3d / sfvos_conv3d_wgrad at kt = 1, t_in = 1, taps = 9 --------------------------

HEAD_CONV_CASES = [
    # RoIs level    c_in c_out
    (1, (14, 14), 256, 256),
    (9, (14, 14), 256, 256),     # the module's
    (33, (14, 14), 256, 256),
    (9, (7, 7), 256, 256),
    (1, (7, 7), 256, 32),
    (33, (7, 7), 256, 32),
]


def head_conv_operands(case, prec, seed):
    B, (H, W), cin, cout = case
    g = torch.Generator().manual_seed(seed)
    x = rnd(torch.randn(B, cin, H, W, generator=g), prec)
    w = torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)
    bias = torch.randn(cout, generator=g) * 0.3
    dy = rnd(torch.randn(B, cout, H, W, generator=g), prec)
    return x, w, bias, dy


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', HEAD_CONV_CASES)
def test_head_conv3x3_forward_bias_relu(lib, prec, case):
    """K = 9 * c_in; bias + ReLU epilogue; pitched input and output (the unused columns keep the sentinel)."""
    B, (H, W), cin, cout = case
    x, w, bias, _ = head_conv_operands(case, prec, 91)
    wr = rnd(w, prec).double()
    ref = F.conv2d(x.double(), wr, bias.double(), padding=1)
    mag = F.conv2d(x.double().abs(), wr.abs(), bias.double().abs(), padding=1)
    ld_x, ld_y = cin + 32, cout + 64
    xd = to_pyr([x.unsqueeze(2)], prec, ld_x)
    d, t_out = make_desc(lib, prec, B, 1, [(H, W)], cin, cout, 1, 9, 0, ld_x, ld_y)
    d.relu = 1
    assert t_out == 1
    wp = torch.empty(w.numel(), dtype=TDT[prec], device='cuda')
    wdev, bdev = w.cuda(), bias.cuda()
    lib.call('sfvos_pack_weights_fwd', P(wdev), P(wp), d.dtype, cout, cin, 1, 9, S())
    y = Out((B * H * W, ld_y), TDT[prec])
    lib.call('sfvos_conv3d', ctypes.byref(d), P(xd), P(wp), P(bdev), P(y.t), None, S())
    torch.cuda.synchronize()
    yc = y.cpu()
    assert bool((yc[:, cout:] == SENT).all()), 'wrote outside its channel slice'
    got = yc[:, :cout].float().reshape(B, H, W, cout).permute(0, 3, 1, 2)
    check('head conv3x3 fwd %s %s' % (prec, case), got, ref.clamp_min(0), mag, 9 * cin, U_OUT[prec])


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', HEAD_CONV_CASES)
def test_head_conv3x3_dgrad(lib, prec, case):
    """The data gradient as the mask branch runs it: sfvos_conv3d on a sfvos_pack_weights_dgrad image, channels
    swapped.  K = 9 * c_out."""
    B, (H, W), cin, cout = case
    _, w, _, dy = head_conv_operands(case, prec, 92)
    wr = rnd(w, prec).double()

    def grad(g, wv):
        xin = torch.zeros(B, cin, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(xin, wv, None, padding=1).backward(g)
        return xin.grad
    ref, mag = grad(dy.double(), wr), grad(dy.double().abs(), wr.abs())
    dyd = to_pyr([dy.unsqueeze(2)], prec)
    d, _ = make_desc(lib, prec, B, 1, [(H, W)], cout, cin, 1, 9, 0, cout, cin)
    wp = torch.empty(w.numel(), dtype=TDT[prec], device='cuda')
    wdev = w.cuda()
    lib.call('sfvos_pack_weights_dgrad', P(wdev), P(wp), d.dtype, cout, cin, 1, 9, S())
    dx = Out((B * H * W, cin), TDT[prec])
    lib.call('sfvos_conv3d', ctypes.byref(d), P(dyd), P(wp), None, P(dx.t), None, S())
    torch.cuda.synchronize()
    got = dx.cpu().float().reshape(B, H, W, cin).permute(0, 3, 1, 2)
    check('head conv3x3 dgrad %s %s' % (prec, case), got, ref, mag, 9 * cout, U_OUT[prec])


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case', HEAD_CONV_CASES)
def test_head_conv3x3_wgrad(lib, prec, case):
    """K = the whole term count B * H * W (the split of sfvos_conv3d_wgrad is a plan, not read off here): tight for one
    RoI (196 / 49 terms), loose for 33."""
    B, (H, W), cin, cout = case
    x, _, _, dy = head_conv_operands(case, prec, 93)

    def grad(xv, g):
        wv = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(xv, wv, None, padding=1).backward(g)
        return wv.grad
    ref, mag = grad(x.double(), dy.double()), grad(x.double().abs(), dy.double().abs())
    ld_x, ld_y = cin + 32, cout + 32
    xd, dyd = to_pyr([x.unsqueeze(2)], prec, ld_x), to_pyr([dy.unsqueeze(2)], prec, ld_y)
    d, _ = make_desc(lib, prec, B, 1, [(H, W)], cin, cout, 1, 9, 0, ld_x, ld_y)
    nbytes = lib.load().sfvos_conv3d_wgrad_workspace_bytes(ctypes.byref(d))
    assert nbytes > 0 and nbytes % 4 == 0
    ws = Out((nbytes // 4,), fill=float('nan'))
    gw = Out((cout, cin, 1, 3, 3))
    lib.call('sfvos_conv3d_wgrad', ctypes.byref(d), P(xd), P(dyd), P(gw.t), 0, P(ws.t), S())
    torch.cuda.synchronize()
    assert ws.guards_ok(), 'wrote outside the workspace'
    check('head conv3x3 wgrad %s %s' % (prec, case), gw.cpu()[:, :, 0], ref, mag, B * H * W, 0.0)
