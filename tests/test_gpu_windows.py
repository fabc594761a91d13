"""GPU: sfvos_amd.SlowFastWindows (first-layer reuse across consecutive training windows) and its kernel
sfvos_shift_frames, against torch, the CPU oracle driven through the reference's training loop
(code/helpers/model.py:316-374) and the plain path (reuse=False)."""
import ctypes
from collections import OrderedDict

import pytest
import torch

from golden_util import SMALL_LEVELS, max_rel_err, rel_err
from kernel_util import rel_l2
from oracle.closed_form import closed_form_features, closed_form_state_dict, slice_slow
from oracle.slowfast_ref import OracleSlowFastLayers, proxy_loss

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
FIVE_ODD = OrderedDict([('0', (9, 13)), ('1', (5, 7)), ('2', (3, 5)), ('3', (2, 3)), ('pool', (1, 1))])
LAYER3 = ('slow_conv3.', 'fast_conv3.', 'bn_s3.', 'bn_f3.')
ZERO_GRAD_BIAS = ('conv1.bias', 'conv2.bias', 'conv3.bias')   # conv bias in front of a train-mode BN: gradient 0


# ---------------------------------------------------------------------------------------------- 1. the kernel
def _pyramid_buffer(shapes, B, T, ld, dtype, gen):
    M = B * T * sum(h * w for h, w in shapes)
    return torch.randn((M, ld), generator=gen, device=DEV).to(dtype)


def _levels(buf, shapes, B, T):
    """Views [B, T, h*w, ld] of the levels of a level-major pyramid buffer."""
    out, off = [], 0
    for h, w in shapes:
        n = B * T * h * w
        out.append(buf[off:off + n].view(B, T, h * w, buf.shape[1]))
        off += n
    return out


@pytest.mark.parametrize('pyr_name', ['small', 'five_odd'])
@pytest.mark.parametrize('C', [32, 192])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_shift_kernel_matches_torch(dtype, C, pyr_name):
    """out bit-identical to the per-level torch.cat of the shifted frames; the statistics rows (level-major, counted
    by sfvos_shift_frames_stat_rows) sum to the torch per-level sums; prev and fresh are not written; channels past C
    of a wider pitch are not written either."""
    from sfvos_amd import _lib
    lib = _lib.load()
    shapes = list((SMALL_LEVELS if pyr_name == 'small' else FIVE_ODD).values())
    B, T = (1, 6) if pyr_name == 'small' else (2, 5)
    ld = C if pyr_name == 'small' else C + 32
    dt_id = _lib.BF16 if dtype == torch.bfloat16 else _lib.F32
    pyr = _lib.make_pyramid(shapes)
    gen = torch.Generator(device=DEV).manual_seed(C + T)
    rows_pl = (ctypes.c_int * _lib.MAX_LEVELS)()
    rows = lib.sfvos_shift_frames_stat_rows(ctypes.byref(pyr), B, T, C, rows_pl)
    assert rows == sum(rows_pl[:len(shapes)]) and rows > 0
    prev = _pyramid_buffer(shapes, B, T, ld, dtype, gen)
    for s in sorted({1, 2, T - 1}):
        fresh = _pyramid_buffer(shapes, B, s, ld, dtype, gen)
        prev0, fresh0 = prev.clone(), fresh.clone()
        out = torch.full_like(prev, 7.0)
        part = torch.full((rows, 2, C), float('nan'), device=DEV)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.call('sfvos_shift_frames', ctypes.c_void_p(prev.data_ptr()), ctypes.c_void_p(fresh.data_ptr()),
                  ctypes.c_void_p(out.data_ptr()), dt_id, ctypes.byref(pyr), B, T, s, C, ld,
                  ctypes.c_void_p(part.data_ptr()), st)
        torch.cuda.synchronize()
        assert torch.equal(prev, prev0) and torch.equal(fresh, fresh0), 'prev / fresh written'
        r0 = 0
        for l, (p, f, o) in enumerate(zip(_levels(prev, shapes, B, T), _levels(fresh, shapes, B, s),
                                          _levels(out, shapes, B, T))):
            want = torch.cat([p[:, s:], f], 1)
            assert torch.equal(o[..., :C], want[..., :C]), (l, s)
            assert bool((o[..., C:] == 7.0).all()), 'wrote past C'
            x = want[..., :C].double().reshape(-1, C)
            got = part[r0:r0 + rows_pl[l]].double().sum(0)
            r0 += rows_pl[l]
            tol = 1e-6 if dtype == torch.float32 else 1e-5
            assert torch.allclose(got[0], x.sum(0), rtol=0, atol=tol * float(x.abs().sum(0).max())), (l, s)
            assert torch.allclose(got[1], (x * x).sum(0), rtol=tol, atol=0), (l, s)
        # without statistics: the same copy
        out2 = torch.empty_like(prev)
        _lib.call('sfvos_shift_frames', ctypes.c_void_p(prev.data_ptr()), ctypes.c_void_p(fresh.data_ptr()),
                  ctypes.c_void_p(out2.data_ptr()), dt_id, ctypes.byref(pyr), B, T, s, C, ld, None, st)
        torch.cuda.synchronize()
        for o, o2 in zip(_levels(out, shapes, B, T), _levels(out2, shapes, B, T)):
            assert torch.equal(o[..., :C], o2[..., :C])


# ---------------------------------------------------------------------------------------------- helpers
def _video(n, levels, bf16):
    """n frames of closed-form features: OrderedDict level -> [n,256,H,W] fp32 (bf16-representable for bf16)."""
    v = closed_form_features(n, levels, clip=3)
    if bf16:
        v = OrderedDict((k, t.bfloat16().float()) for k, t in v.items())
    return v


def _seq(video, precision):
    from sfvos_amd import PackedClip
    tdt = torch.bfloat16 if precision == 'bf16' else torch.float32
    levels = [v.permute(0, 2, 3, 1).unsqueeze(0).to(DEV, tdt).contiguous() for v in video.values()]   # [1,N,H,W,C]
    return PackedClip.from_levels(levels, keys=list(video.keys()), layout='grouped' if precision == 'bf16' else 'ndhwc')


def _window(video, i, fp):
    """The reference's window around centre i: zero frames beyond the ends (model.py:215-225)."""
    out = OrderedDict()
    for k, v in video.items():
        n = v.shape[0]
        idx = [i - fp // 2 + j for j in range(fp)]
        out[k] = torch.stack([v[t] if 0 <= t < n else torch.zeros_like(v[0]) for t in idx])
    return out


def _module(sp, fp, precision):
    from sfvos_amd import SlowFastLayers
    m = SlowFastLayers(256, DEV, sp, fp, precision=precision)
    m.load_state_dict(closed_form_state_dict(m))
    return m.to(DEV).train()


KW = dict(lr=1e-3, momentum=0.9, weight_decay=1e-4)


def _oracle_trajectory(sp, fp, video):
    """The reference's loop on the CPU oracle: per centre forward, loss, backward; SGD after every second clip."""
    o = OracleSlowFastLayers(256, torch.device('cpu'), sp, fp)
    o.load_state_dict(closed_form_state_dict(o))
    o.train()
    opt = torch.optim.SGD(o.parameters(), **KW)
    opt.zero_grad()
    p0 = {k: p.detach().clone() for k, p in o.named_parameters()}
    steps = []
    for i in range(next(iter(video.values())).shape[0]):
        w = _window(video, i, fp)
        out = o.temporally_enhance_features([slice_slow(w, sp)], [w])
        loss = proxy_loss(out)
        loss.backward()
        steps.append(dict(out={k: v.detach() for k, v in out.items()}, loss=float(loss.detach()),
                          grad={k: p.grad.detach().clone() for k, p in o.named_parameters()}))
        if i % 2 == 1:
            opt.step()
            opt.zero_grad()
    params = {k: p.detach().clone() for k, p in o.named_parameters()}
    stats = {k: b.detach().clone() for k, b in o.named_buffers() if 'running' in k}
    return steps, p0, params, stats


def _gpu_trajectory(sp, fp, precision, video, reuse, fused):
    from sfvos_amd import FusedSGD, SlowFastWindows
    m = _module(sp, fp, precision)
    seq = _seq(video, precision)
    win = SlowFastWindows(m, seq, reuse=reuse)
    opt = FusedSGD(m.parameters(), **KW).attach(m) if fused else torch.optim.SGD(m.parameters(), **KW)
    opt.zero_grad()
    steps = []
    for i in range(seq.frames):
        out = win.enhance(i)
        loss = proxy_loss(out)
        loss.backward()
        steps.append(dict(out={k: v.detach().cpu() for k, v in out.items()}, loss=float(loss),
                          grad={k: p.grad.detach().cpu() for k, p in m.named_parameters()},
                          reused=dict(win.reused)))
        if i % 2 == 1:
            opt.step()
            opt.zero_grad()
    torch.cuda.synchronize()
    params = {k: p.detach().cpu() for k, p in m.named_parameters()}
    stats = {k: b.detach().cpu() for k, b in m.named_buffers() if 'running' in k}
    return steps, params, stats


# ---------------------------------------------------------------------------------------------- 2. the training loop
_ORACLE = {}


@pytest.mark.parametrize('sp,fp,precision', [(3, 7, 'fp32'), (3, 7, 'bf16'), (4, 32, 'fp32'), (4, 32, 'bf16'),
                                             (1, 1, 'fp32')])
def test_reference_training_loop_matches_oracle_and_plain_path(sp, fp, precision):
    """Centres 0 .. N-1 of an N = fp + 3 frame video through the reference's cycle (forward, loss, backward, SGD after
    every second clip; model.py:316-374), with FusedSGD and with torch.optim.SGD, against the CPU oracle on the same
    loop and against SlowFastWindows(reuse=False).  Every second clip reuses t_out - 1 frames of fast_conv1, every
    first one (after a step) none.
    fp32 gates: maps and loss 1e-3 of the oracle's scale (maps: or no worse than twice the plain path, which drifts to
    1.4e-3 at (4,32)); every loss within 1e-5 of the plain path's, the maps of the first pair (same weights, the second
    clip reused) within 1e-5 and later ones within 1e-3 (measured 2.4e-4: the two runs' weights may differ after a
    ReLU-mask flip in an earlier clip's gradient); the worst gradient over all clips, the accumulated updates and the
    running statistics at the gates tests/test_gpu_parity.py applies to the plain path over a trajectory of centre frames
    (test_c1_eight_centre_frames_trajectory_matches_the_oracle): 1e-2 rel-L2, 1e-2, 1e-5 -- or, where the plain path
    itself is further from the oracle, no worse than twice the plain path.  At (4,32) over 35 clips both paths meet the
    same ReLU-mask flips (they move the first layers' cancelling weight-gradient sums): worst
    gradient 4.05e-2 with FusedSGD, 6.85e-2 with torch.optim.SGD, equal for both paths.  Every figure is printed.
    The plain run each reuse run is compared with uses the same optimiser (the two optimisers round differently).  bf16: errors against the oracle printed and gated at the plain bf16 path's gates (maps
    5e-2 of the scale, loss 2e-2), the same quantities of the plain path printed beside them."""
    bf16 = precision == 'bf16'
    N = fp + 3
    video = _video(N, SMALL_LEVELS, bf16)
    key = (sp, fp, bf16)
    if key not in _ORACLE:
        _ORACLE[key] = _oracle_trajectory(sp, fp, video)
    ref, p0, ref_params, ref_stats = _ORACLE[key]
    from sfvos_amd import SlowFastPlan
    t_out = SlowFastPlan(256, sp, fp).layer('f1').t_out
    for fused in (True, False):
        plain = _gpu_trajectory(sp, fp, precision, video, reuse=False, fused=fused)   # the same optimiser
        steps, params, stats = _gpu_trajectory(sp, fp, precision, video, reuse=True, fused=fused)
        worst = dict(out=0.0, loss=0.0, out_plain=0.0, grad=0.0, plain_grad=0.0, plain_out=0.0, plain_loss=0.0)
        for i, (g, r, pl) in enumerate(zip(steps, ref, plain[0])):
            assert g['reused']['f1'] == (t_out - 1 if i % 2 == 1 else 0), (i, g['reused'])
            assert pl['reused'] == {'f1': 0, 's1': 0}
            for k in g['out']:
                if i < 2:
                    worst['pair0_plain'] = max(worst.get('pair0_plain', 0.0),
                                               max_rel_err(g['out'][k].numpy(), pl['out'][k].numpy()))
                worst['out'] = max(worst['out'], max_rel_err(g['out'][k].numpy(), r['out'][k].numpy()))
                worst['plain_out'] = max(worst['plain_out'], max_rel_err(pl['out'][k].numpy(), r['out'][k].numpy()))
                worst['out_plain'] = max(worst['out_plain'], max_rel_err(g['out'][k].numpy(), pl['out'][k].numpy()))
            worst['loss'] = max(worst['loss'], abs(g['loss'] - r['loss']) / abs(r['loss']))
            worst['plain_loss'] = max(worst['plain_loss'], abs(pl['loss'] - r['loss']) / abs(r['loss']))
            if not bf16:
                assert abs(g['loss'] - pl['loss']) <= 1e-5 * abs(pl['loss']), (i, g['loss'], pl['loss'])
                gscale = max(float(v.abs().max()) for v in r['grad'].values())
                for name, gr in g['grad'].items():
                    if name.endswith(ZERO_GRAD_BIAS):
                        assert float(gr.abs().max()) < 1e-3 * gscale, (i, name)
                        continue
                    e = rel_err(gr.numpy(), r['grad'][name].numpy())
                    e_plain = rel_err(pl['grad'][name].numpy(), r['grad'][name].numpy())
                    worst['grad'], worst['plain_grad'] = max(worst['grad'], e), max(worst['plain_grad'], e_plain)
        eu = max(rel_l2(params[n] - p0[n], ref_params[n] - p0[n]) for n in params if not n.endswith(ZERO_GRAD_BIAS))
        es = max(max_rel_err(stats[n].numpy(), ref_stats[n].numpy()) for n in stats)
        eu_plain = max(rel_l2(plain[1][n] - p0[n], ref_params[n] - p0[n]) for n in params
                       if not n.endswith(ZERO_GRAD_BIAS))
        es_plain = max(max_rel_err(plain[2][n].numpy(), ref_stats[n].numpy()) for n in stats)
        print('(%d,%d) %s %s: vs oracle maps %.2e loss %.2e grads %.2e updates %.2e running %.2e | vs plain maps %.2e '
              '| plain vs oracle maps %.2e loss %.2e grads %.2e'
              % (sp, fp, precision, 'FusedSGD' if fused else 'torch.optim.SGD', worst['out'], worst['loss'],
                 worst['grad'], eu, es, worst['out_plain'], worst['plain_out'], worst['plain_loss'], worst['plain_grad']))
        print('    plain path: updates %.2e running %.2e' % (eu_plain, es_plain))
        if bf16:
            assert worst['out'] < 5e-2 and worst['loss'] < 2e-2
            assert eu < 0.25 and es < 2e-2
        else:
            assert worst['out'] < max(1e-3, 2.0 * worst['plain_out']) and worst['loss'] < 1e-3
            assert worst['pair0_plain'] < 1e-5 and worst['out_plain'] < 1e-3, worst
            assert worst['grad'] < max(1e-2, 2.0 * worst['plain_grad']), worst
            assert eu < max(1e-2, 2.0 * eu_plain) and es < max(1e-5, 2.0 * es_plain)


# ---------------------------------------------------------------------------------------------- 3. what is reused
@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_reused_raw_buffers_equal_the_plain_ones(precision):
    """The layer-1 pre-BN buffers of a reused window (frames shifted over from the previous window + the freshly
    computed ones): bit-identical to a whole recompute in bf16 (same kernels, same per-frame summation order), within
    1e-6 of the scale in fp32."""
    from sfvos_amd import SlowFastWindows
    sp, fp = 4, 32
    video = _video(12, SMALL_LEVELS, precision == 'bf16')
    m = _module(sp, fp, precision)
    seq = _seq(video, precision)
    win, full = SlowFastWindows(m, seq), SlowFastWindows(m, seq)
    for i in (5, 6, 9):
        win.enhance(i)
        full.reset()
        full.enhance(i)
        assert full.reused == {'f1': 0, 's1': 0}
        for n in ('f1', 's1'):
            a, b = win._raw[n].float(), full._raw[n].float()
            if precision == 'bf16':
                assert torch.equal(win._raw[n], full._raw[n]), (i, n)
            else:
                assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()), (i, n)
    assert win.reused == {'f1': 22 - 3, 's1': 0}


# ---------------------------------------------------------------------------------------------- 4. gaps and ends
def test_gaps_and_sequence_ends():
    """Centres 5, 6, 9, 10 (a gap of s = 3: the reference skips frames without boxes, model.py:286-294,318-319) match
    the plain path; the windows at the ends of the sequence (sticking out on both sides) equal enhance_packed of a
    PackedClip that stores the real frames and names the zero frames with `pad`."""
    from sfvos_amd import PackedClip, SlowFastWindows
    sp, fp = 4, 32
    video = _video(12, SMALL_LEVELS, False)
    m = _module(sp, fp, 'fp32')
    seq = _seq(video, 'fp32')
    win, plain = SlowFastWindows(m, seq), SlowFastWindows(m, seq, reuse=False)
    expect = {5: 0, 6: 21, 9: 19, 10: 21}
    for i in (5, 6, 9, 10):
        a, b = win.enhance(i), plain.enhance(i)
        assert win.reused['f1'] == expect[i] and win.reused['s1'] == (2 if expect[i] == 21 else 0), (i, win.reused)
        proxy_loss(a).backward()
        for k in a:
            assert max_rel_err(a[k].detach().cpu().numpy(), b[k].detach().cpu().numpy()) < 1e-5, (i, k)
    N = seq.frames
    for i in range(N):
        a = win.enhance(i)
        lo, hi = max(0, i - fp // 2), min(N, i - fp // 2 + fp)
        levels = [v[lo:hi].permute(0, 2, 3, 1).unsqueeze(0).to(DEV).contiguous() for v in video.values()]
        clip = PackedClip.from_levels(levels, keys=list(video.keys()), pad=(lo - (i - fp // 2), i - fp // 2 + fp - hi))
        b = m.enhance_packed(clip)
        assert win.reused['f1'] == (0 if i == 0 else 21)
        for k in a:
            assert max_rel_err(a[k].detach().cpu().numpy(), b[k].detach().cpu().numpy()) < 1e-5, (i, k)


# ---------------------------------------------------------------------------------------------- 5. full size
def test_full_size_bf16_two_consecutive_centres():
    """(4,32) bf16 on the DAVIS pyramid, two consecutive centres of a resident sequence, against the plain path: maps
    within 1e-2 rel-L2, and their largest difference within FULL_GATES[('c2', 'bf16')]['out'] of the scale (measured
    1.07e-2: the first layers' BN statistics are sums of the stored bf16 values instead of the f32 accumulators, which
    moves single bf16 roundings -- one unit is 3.9e-3 relative -- and they add up through layers 2 and 3; the plain bf16
    path is 1.3e-2 from the fp32 oracle by the same measure); loss, and every parameter gradient at
    FULL_GATES[('c2', 'bf16')] (g12 / g3): differing BN statistics can flip ReLU masks."""
    from test_gpu_parity import FULL_GATES
    from sfvos_amd import MSEProxyLoss, PackedClip, SlowFastWindows, davis_pyramid
    gates = FULL_GATES[('c2', 'bf16')]
    sp, fp, N = 4, 32, 20
    pyr = davis_pyramid()
    gen = torch.Generator(device=DEV).manual_seed(11)
    levels = [torch.randn((1, N, h, w, 256), generator=gen, device=DEV).bfloat16() for _, (h, w) in pyr]
    seq = PackedClip.from_levels(levels, keys=[k for k, _ in pyr], layout='grouped')
    del levels
    loss_fn = MSEProxyLoss({k: torch.randn((1, 256, h, w), generator=gen, device=DEV) for k, (h, w) in pyr})
    res = []
    for reuse in (True, False):
        m = _module(sp, fp, 'bf16')
        win = SlowFastWindows(m, seq, reuse=reuse)
        for i in (9, 10):
            m.zero_grad(set_to_none=True)
            out = win.enhance(i)
            loss = loss_fn(out)
            loss.backward()
        assert win.reused == ({'f1': 21, 's1': 2} if reuse else {'f1': 0, 's1': 0})
        res.append((OrderedDict((k, v.detach()) for k, v in out.items()), float(loss),
                    {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
        del m, win
    (o1, l1, g1), (o0, l0, g0) = res
    eo = max(float((o1[k] - o0[k]).abs().max() / o0[k].abs().max()) for k in o0)
    e2 = max(rel_l2(o1[k], o0[k]) for k in o0)
    el = abs(l1 - l0) / abs(l0)
    print('full size (4,32) bf16, reuse vs plain: maps max %.2e of the scale, rel-L2 %.2e, loss %.2e' % (eo, e2, el))
    assert e2 < 1e-2 and eo < gates['out'] and el < gates['loss']
    gscale = max(float(v.abs().max()) for v in g0.values())
    for k in g0:
        if k.endswith(ZERO_GRAD_BIAS):
            assert float(g1[k].abs().max()) < gates['g3'][1] * gscale, k
            continue
        e2, emax = rel_l2(g1[k], g0[k]), float((g1[k] - g0[k]).abs().max() / g0[k].abs().max())
        gate = gates['g3'] if k.startswith(LAYER3) else gates['g12']
        print('  grad %-18s rel-L2 %.2e, max / scale %.2e (gate %s)' % (k, e2, emax, gate))
        assert e2 < gate[0] and emax < gate[1], (k, e2, emax)


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals():
    from sfvos_amd import PackedClip, SlowFastLayers, SlowFastWindows
    video = _video(5, SMALL_LEVELS, False)
    m = _module(3, 7, 'fp32')
    seq = _seq(video, 'fp32')
    win = SlowFastWindows(m, seq)
    for i in (-1, 5):
        with pytest.raises(IndexError):
            win.enhance(i)
    g = PackedClip(seq.data.clone().requires_grad_(True), seq.shapes, 1, 5, seq.keys)
    with pytest.raises(RuntimeError, match='grad'):
        SlowFastWindows(m, g)
    m8 = SlowFastLayers(256, DEV, 3, 7, precision='fp8').to(DEV)
    with pytest.raises(RuntimeError, match='fp8|inference'):
        SlowFastWindows(m8, seq)
    narrow = PackedClip(seq.data[:, :128].contiguous(), seq.shapes, 1, 5, seq.keys)
    with pytest.raises(RuntimeError, match='channels'):
        SlowFastWindows(m, narrow)
    both = PackedClip(torch.cat([seq.data, seq.data]), seq.shapes, 2, 5, seq.keys)   # two clips
    with pytest.raises(RuntimeError, match='B = 1'):
        SlowFastWindows(m, both)
    with pytest.raises(RuntimeError):
        SlowFastWindows(_module(3, 7, 'bf16'), seq)     # fp32 sequence for a bf16 module
