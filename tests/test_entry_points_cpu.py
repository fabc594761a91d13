"""CPU (no GPU): the host side of the entry points outside the conv family (batchnorm.hip, elementwise.hip,
maskhead.hip, roialign.hip) -- the values their sizing functions return, and the calls they refuse before any kernel
is launched.  A refused call returns -1 and leaves a message that starts with the entry point's name.
shift_frames and shift_frames_stat_rows are covered by test_windows_cpu.py.

Pointers are NULL or P, an address that is never dereferenced.  Every call in REFUSALS breaks one condition of one
check of a call that would otherwise launch; without a device, a call that got past the checks would return -2.

The sizing values were recorded from the library before its host code was rewritten."""
import ctypes

import pytest

P = 1 << 40                   # never dereferenced
F32, BF16, FP8, BAD = 0, 1, 2, 7


def _load():
    from sfvos_amd import _lib
    return _lib, _lib.load()


# ---- arguments that are structs or arrays, built once the binding is loaded ------------------------------------------

def _lv(*m, n=None):
    """sfvos_levels with m[l] positions per level (n_levels = n or len(m))."""
    def make(_lib):
        lv = _lib.Levels()
        lv.n_levels = len(m) if n is None else n
        for i, v in enumerate(m):
            lv.m[i] = v
        return ctypes.byref(lv)
    make.tag = 'levels%r' % ((n,) + m if n is not None else m,)
    return make


def _run(**kw):
    """sfvos_bn_running with every pointer P, 2 updates, and the fields in kw."""
    def make(_lib):
        r = _lib.BnRunning(running_mean=P, running_var=P, means=P, vars_unbiased=P, num_batches_tracked=P,
                           n_updates=2, momentum=0.1)
        for k, v in kw.items():
            setattr(r, k, v)
        return ctypes.byref(r)
    make.tag = 'running%r' % sorted(kw.items())
    return make


def _mse(n, **level1):
    """sfvos_mse_table of n levels (1000 elements each) with the fields in level1 set on level 1."""
    def make(_lib):
        t = _lib.MseTable()
        t.n = n
        for l in range(_lib.MAX_LEVELS):
            t.out[l], t.target[l], t.grad[l], t.numel[l] = P, P, P, 1000
        for k, v in level1.items():
            getattr(t, k)[1] = v
        return ctypes.byref(t)
    make.tag = 'mse%r' % ([n] + sorted(level1.items()))
    return make


def _planar(n, **last):
    """n contiguous 8 x 8 planar levels of T=2, C=64 (sfvos_planar_level[]), the fields in last set on the last one."""
    def make(_lib):
        a = (_lib.PlanarLevel * n)()
        for l in range(n):
            a[l].ptr, a[l].stride_t, a[l].stride_c, a[l].stride_h, a[l].stride_w, a[l].h, a[l].w = \
                P, 64 * 64, 64, 8, 1, 8, 8
        for k, v in last.items():
            setattr(a[n - 1], k, v)
        return a
    make.tag = 'planar%r' % ([n] + sorted(last.items()))
    return make


def _items(n, **last):
    """n pack items (64 x 64 x 3 x 9, pointers P), the fields in last set on the last one."""
    def make(_lib):
        a = (_lib.PackItem * n)()
        for i in range(n):
            a[i].w, a[i].packed, a[i].c_out, a[i].c_in, a[i].kt, a[i].taps, a[i].dgrad = P, P, 64, 64, 3, 9, i % 2
        for k, v in last.items():
            setattr(a[n - 1], k, v)
        return a
    make.tag = 'items%r' % ([n] + sorted(last.items()))
    return make


def _ints(ctype, *v):
    def make(_lib):
        return (ctype * len(v))(*v)
    make.tag = '%r' % (v,)
    return make


LV = _lv(1000, 200)
FRAMES = dict(st=64 * 64, sc=64, sh=8, sw=1, T=2, C=64, H=8, W=8)   # contiguous [T=2][C=64][8][8] floats
DECONV = dict(dtype=BF16, n=2, h=14, w=14, c_in=256, c_out=256)
ROI = dict(B=2, C=256, H=48, W=84, level=0, n=4, spatial_scale=0.25, pooled=14, sr=2)

# entry point (without sfvos_) -> (argument names, the values of a call that passes every check).  A pointer argument
# left out is P; the stream is NULL.
ENTRY = {
    'bn_finalize': ('part n_levels rows count gamma beta eps C mean rstd scale shift var coef_stride stream',
                    dict(n_levels=2, rows=_ints(ctypes.c_int, 3, 3), count=_ints(ctypes.c_int64, 100, 100), eps=1e-5, C=64, coef_stride=64)),
    'bn_eval_coeffs': ('gamma beta rm rv eps C mean rstd scale shift stream', dict(eps=1e-5, C=64)),
    'bn_running_update': ('rm rv means vars n coef_stride C momentum nbt stream',
                          dict(n=2, coef_stride=64, C=64, momentum=0.1)),
    'bn_apply': ('x ld_x y ld_y dtype lv C scale shift coef_stride relu running stream',
                 dict(ld_x=64, ld_y=64, dtype=BF16, lv=LV, C=64, coef_stride=64, relu=1, running=None)),
    'bn_apply_fp8': ('x ld_x y ld_y lv C scale shift coef_stride relu act_scale sat_count running stream',
                     dict(ld_x=64, ld_y=64, lv=LV, C=64, coef_stride=64, relu=1, act_scale=1.0, running=None)),
    'bn_bwd_reduce': ('dy ld_dy x ld_x dtype lv C scale shift mean rstd coef_stride relu part stream',
                      dict(ld_dy=64, ld_x=64, dtype=BF16, lv=LV, C=64, coef_stride=64, relu=1)),
    'bn_bwd_finalize': ('part lv gamma mean rstd coef_stride C train coefA coefB coefK sum_dz sum_dzx stream',
                        dict(lv=LV, coef_stride=64, C=64, train=1)),
    'bn_bwd_apply': ('dy ld_dy x ld_x dx ld_dx dtype lv C scale shift coef_stride relu coefA coefB coefK bias_part '
                     'sum_dz sum_dzx dgamma dbeta accumulate stream',
                     dict(ld_dy=64, ld_x=64, ld_dx=64, dtype=F32, lv=LV, C=64, coef_stride=64, relu=1, accumulate=0)),
    'frames_to_ndhwc': ('src st sc sh sw dst dtype T C H W ld stream', dict(FRAMES, dtype=BF16, ld=64)),
    'frames_to_groups': ('src st sc sh sw dst dtype T C H W group_stride stream',
                         dict(FRAMES, dtype=BF16, group_stride=2 * 64 * 32)),
    'frames_to_groups_fp8': ('src st sc sh sw dst T C H W group_stride scale sat_count stream',
                             dict(FRAMES, group_stride=2 * 64 * 64, scale=1.0)),
    'frames_absmax': ('src st sc sh sw T C H W amax stream', FRAMES),
    'add_inplace': ('dst src dtype n stream', dict(dtype=BF16, n=1024)),
    'mse_loss': ('tab part loss stream', dict(tab=_mse(2))),
    'mse_loss_grad': ('tab upstream stream', dict(tab=_mse(2))),
    'pack_weights_fp8': ('w bias packed bias_descale c_out c_in kt taps act_scale stream',
                         dict(c_out=64, c_in=64, kt=3, taps=9, act_scale=1.0)),
    'planar_to_ndhwc': ('src dst dtype M C ld stream', dict(dtype=BF16, M=4096, C=64, ld=64)),
    'ndhwc_to_frames': ('src dtype dst st sc sh sw T C H W ld accumulate stream',
                        dict(FRAMES, dtype=BF16, ld=64, accumulate=0)),
    'pyramid_to_frames': ('src dtype levels n_levels T C ld accumulate stream',
                          dict(dtype=BF16, levels=_planar(2), n_levels=2, T=2, C=64, ld=64, accumulate=0)),
    'frames_to_pyramid': ('levels n_levels dst dtype T C ld stream',
                          dict(levels=_planar(2), n_levels=2, dtype=BF16, T=2, C=64, ld=64)),
    'ndhwc_to_planar': ('src dtype dst M C ld stream', dict(dtype=BF16, M=4096, C=64, ld=64)),
    'pack_weights_fwd': ('w packed dtype c_out c_in kt taps stream', dict(dtype=BF16, c_out=64, c_in=64, kt=3, taps=9)),
    'pack_weights_dgrad': ('w packed dtype c_out c_in kt taps stream',
                           dict(dtype=BF16, c_out=64, c_in=64, kt=3, taps=9)),
    'pack_weights_batch': ('items n dtype stream', dict(items=_items(2), n=2, dtype=BF16)),
    'mask_union': ('masks n hw threshold out stream', dict(n=2, hw=4096, threshold=0.5)),
    'reduce_rows': ('part rows C out accumulate stream', dict(rows=4, C=64, accumulate=0)),
    'sgd_step': ('p g buf n lr momentum wd first stream', dict(n=1024, lr=0.1, momentum=0.9, wd=0.0, first=0)),
    'scale': ('x n s stream', dict(n=1024, s=2.0)),
    'pack_deconv2x2': ('w packed dtype c_in c_out stream', dict(dtype=BF16, c_in=256, c_out=256)),
    'pack_deconv2x2_dgrad': ('w packed dtype c_in c_out stream', dict(dtype=BF16, c_in=256, c_out=256)),
    'deconv2x2_relu': ('x w_packed bias y dtype n h w c_in c_out relu stream', dict(DECONV, relu=1)),
    'deconv2x2_dgrad': ('dz w_packed dx dtype n h w c_in c_out stream', DECONV),
    'deconv2x2_wgrad': ('x dz dtype n h w c_in c_out grad_w accumulate workspace stream', dict(DECONV, accumulate=0)),
    'mask_logits': ('x dtype w bias labels n positions c num_classes logits prob stream',
                    dict(dtype=BF16, n=2, positions=784, c=256, num_classes=1)),
    'paste_masks': ('masks boxes n mask_size padding img_h img_w out stream',
                    dict(n=2, mask_size=28, padding=1, img_h=64, img_w=64)),
    'relu_bwd': ('dy a dz dtype m c col_part stream', dict(dtype=BF16, m=1000, c=256)),
    'mask_bce_loss': ('logits labels targets n num_classes positions loss stream',
                      dict(n=2, num_classes=1, positions=784)),
    'mask_bce_loss_grad': ('logits labels targets upstream n num_classes positions dlogits stream',
                           dict(n=2, num_classes=1, positions=784)),
    'mask_logits_bwd': ('y dtype dlogits w n positions c num_classes relu dz part stream',
                        dict(dtype=BF16, n=2, positions=784, c=256, num_classes=1, relu=1)),
    'roi_levels': ('rois n k_min k_max canonical_scale canonical_level eps levels stream',
                   dict(n=4, k_min=2, k_max=5, canonical_scale=224.0, canonical_level=4.0, eps=1e-6)),
    'roi_align': ('feat B C H W rois levels level n spatial_scale pooled sr workspace out stream', ROI),
    'roi_align_bwd': ('dout B C H W rois levels level n spatial_scale pooled sr workspace dfeat accumulate stream',
                      dict(ROI, accumulate=0)),
}

BN_ACT = [dict(dtype=BAD), dict(dtype=FP8), dict(C=48), dict(C=288), dict(C=0)]   # check_act: dtype, C
BN_LEVELS = [dict(lv=None), dict(lv=_lv(n=0)), dict(lv=_lv(*[100] * 8, n=9)), dict(lv=_lv(1000, 0))]
PACK = [dict(w=None), dict(packed=None), dict(c_out=48), dict(c_in=16), dict(kt=0), dict(taps=3), dict(dtype=BAD),
        dict(dtype=FP8)]
PACK_DECONV = [dict(w=None), dict(packed=None), dict(c_in=0), dict(c_out=48), dict(c_in=-32), dict(dtype=BAD),
               dict(dtype=FP8)]
BIG_M = dict(n=1 << 12, h=1 << 10, w=1 << 10)    # 2^32 positions
ROI_CHECK = [dict(B=0), dict(C=0), dict(H=0), dict(W=-1), dict(n=-1), dict(pooled=0), dict(sr=0), dict(pooled=33),
             dict(n=1 << 20, C=1 << 12, pooled=32), dict(B=1 << 11, H=1 << 10, W=1 << 10)]

# (entry point, arguments that differ from ENTRY's, prefix of the message when it is not the entry point's name)
REFUSALS = [(e, kw, None) for e, kws in [
    ('bn_finalize', [dict(part=None), dict(var=None), dict(rows=None), dict(n_levels=0), dict(n_levels=9),
                     dict(C=48), dict(C=0), dict(coef_stride=32), dict(rows=_ints(ctypes.c_int, 3, 0)), dict(count=_ints(ctypes.c_int64, 100, 0))]),
    ('bn_eval_coeffs', [dict(gamma=None), dict(shift=None), dict(C=0)]),
    ('bn_running_update', [dict(rm=None), dict(vars=None), dict(n=-1), dict(C=0), dict(coef_stride=32)]),
    ('bn_apply', BN_ACT + BN_LEVELS + [dict(ld_x=32), dict(ld_y=68), dict(running=_run(running_mean=None)),
                                      dict(running=_run(n_updates=-1)), dict(x=None), dict(scale=None),
                                      dict(coef_stride=32)]),
    ('bn_apply_fp8', BN_LEVELS + [dict(running=_run(vars_unbiased=None)), dict(x=None), dict(y=None),
                                  dict(act_scale=0.0), dict(coef_stride=32), dict(C=24), dict(C=0), dict(ld_x=68),
                                  dict(ld_y=72), dict(y=P + 8)]),
    ('bn_bwd_reduce', BN_ACT + BN_LEVELS + [dict(ld_dy=36), dict(ld_x=68), dict(part=None), dict(rstd=None),
                                           dict(coef_stride=32)]),
    ('bn_bwd_finalize', BN_LEVELS + [dict(part=None), dict(sum_dzx=None), dict(C=48), dict(C=0),
                                     dict(coef_stride=32)]),
    ('bn_bwd_apply', BN_ACT + BN_LEVELS + [dict(ld_x=32), dict(dtype=BF16, ld_dy=68), dict(dx=None),
                                          dict(coefK=None), dict(coef_stride=32), dict(ld_dx=32), dict(ld_dx=66),
                                          dict(dtype=BF16, ld_dx=68), dict(sum_dz=None), dict(dbeta=P, sum_dzx=None)]),
    ('frames_to_ndhwc', [dict(src=None), dict(dst=None), dict(T=0), dict(C=0), dict(H=0), dict(W=-1), dict(ld=32),
                         dict(C=60), dict(ld=68), dict(dtype=BAD), dict(dtype=FP8)]),
    ('frames_to_groups', [dict(src=None), dict(W=0), dict(dtype=F32), dict(dtype=BAD), dict(C=48),
                          dict(group_stride=2 * 64 * 32 + 4), dict(group_stride=2048)]),
    ('frames_to_groups_fp8', [dict(src=None), dict(dst=None), dict(H=0), dict(scale=0.0), dict(C=32),
                              dict(group_stride=2 * 64 * 64 + 8), dict(group_stride=4096)]),
    ('frames_absmax', [dict(src=None), dict(amax=None), dict(T=0), dict(C=0)]),
    ('add_inplace', [dict(dst=None), dict(n=0), dict(n=12), dict(src=P + 8), dict(dtype=BAD), dict(dtype=FP8)]),
    ('mse_loss', [dict(tab=None), dict(tab=_mse(0)), dict(tab=_mse(9)), dict(tab=_mse(2, numel=0)),
                  dict(tab=_mse(2, out=None)), dict(tab=_mse(2, target=None)), dict(part=None), dict(loss=None)]),
    ('mse_loss_grad', [dict(tab=None), dict(tab=_mse(9)), dict(tab=_mse(2, grad=None)),
                       dict(tab=_mse(2, numel=-5))]),
    ('pack_weights_fp8', [dict(w=None), dict(bias_descale=None), dict(c_out=0), dict(kt=0), dict(taps=3),
                          dict(act_scale=0.0), dict(c_in=32), dict(c_out=48)]),
    ('planar_to_ndhwc', [dict(M=0), dict(M=1 << 31)]),
    ('ndhwc_to_frames', [dict(src=None), dict(dst=None), dict(T=0), dict(W=0), dict(ld=32), dict(C=60), dict(ld=68),
                         dict(dtype=BAD), dict(dtype=FP8)]),
    ('pyramid_to_frames', [dict(src=None), dict(ld=32), dict(C=60), dict(ld=68), dict(levels=None),
                           dict(n_levels=0), dict(n_levels=9), dict(T=0), dict(C=0),
                           dict(levels=_planar(2, ptr=None)), dict(levels=_planar(2, h=0)),
                           dict(levels=_planar(2, h=1 << 20, w=1 << 20)), dict(dtype=BAD), dict(dtype=FP8)]),
    ('frames_to_pyramid', [dict(dst=None), dict(ld=32), dict(C=60), dict(levels=None), dict(n_levels=9),
                           dict(T=0), dict(levels=_planar(2, w=0)), dict(levels=_planar(2, h=1 << 20, w=1 << 20)),
                           dict(dtype=BAD), dict(dtype=FP8)]),
    ('ndhwc_to_planar', [dict(M=0), dict(M=1 << 31)]),
    ('pack_weights_fwd', PACK),
    ('pack_weights_dgrad', PACK),
    ('pack_weights_batch', [dict(items=None), dict(n=0), dict(n=17), dict(items=_items(2, w=None)),
                            dict(items=_items(2, packed=None)), dict(items=_items(2, c_out=0)),
                            dict(items=_items(2, c_in=40)), dict(items=_items(2, kt=0)),
                            dict(items=_items(2, taps=2)),
                            dict(items=_items(2, c_out=1 << 16, c_in=1 << 16, kt=1 << 10)), dict(dtype=BAD),
                            dict(dtype=FP8)]),
    ('mask_union', [dict(out=None), dict(hw=0), dict(n=-1), dict(masks=None)]),
    ('reduce_rows', [dict(part=None), dict(out=None), dict(rows=0), dict(C=0)]),
    ('sgd_step', [dict(p=None), dict(g=None), dict(buf=None), dict(n=0)]),
    ('scale', [dict(x=None), dict(n=0)]),
    ('pack_deconv2x2', PACK_DECONV),
    ('pack_deconv2x2_dgrad', PACK_DECONV),
    ('deconv2x2_relu', [dict(x=None), dict(y=None), dict(n=0), dict(w=0), dict(c_in=0), dict(c_out=40), BIG_M,
                        dict(dtype=BAD), dict(dtype=FP8)]),
    ('deconv2x2_dgrad', [dict(dz=None), dict(dx=None), dict(h=0), dict(c_in=40), dict(c_out=0),
                         dict(n=1 << 9, h=1 << 10, w=1 << 10), dict(dtype=BAD), dict(dtype=FP8)]),
    ('deconv2x2_wgrad', [dict(x=None), dict(workspace=None), dict(grad_w=None), dict(n=0), dict(c_in=0),
                         dict(c_out=48), dict(n=1 << 9, h=1 << 10, w=1 << 10), dict(dtype=BAD), dict(dtype=FP8)]),
    ('mask_logits', [dict(x=None), dict(w=None), dict(n=0), dict(positions=0), dict(c=0), dict(num_classes=0),
                     dict(logits=None, prob=None), dict(labels=None, num_classes=2), dict(dtype=BAD),
                     dict(dtype=FP8)]),
    ('paste_masks', [dict(masks=None), dict(out=None), dict(n=0), dict(mask_size=0), dict(padding=-1),
                     dict(img_w=0)]),
    ('relu_bwd', [dict(dy=None), dict(m=0), dict(dz=None, col_part=None), dict(c=0), dict(c=36), dict(c=300),
                  dict(dtype=F32, c=258), dict(c=(1 << 20) + 8), dict(m=1 << 37), dict(dtype=BAD), dict(dtype=FP8)]),
    ('mask_bce_loss', [dict(logits=None), dict(loss=None), dict(n=0), dict(num_classes=0), dict(positions=0)]),
    ('mask_bce_loss_grad', [dict(labels=None), dict(dlogits=None), dict(n=0), dict(positions=-1)]),
    ('mask_logits_bwd', [dict(y=None), dict(part=None), dict(n=0), dict(positions=0), dict(c=96), dict(c=576),
                         dict(c=0), dict(num_classes=0), dict(num_classes=9), dict(dtype=BAD), dict(dtype=FP8)]),
    ('roi_levels', [dict(n=-1), dict(k_min=6), dict(rois=None), dict(levels=None)]),
    ('roi_align', ROI_CHECK + [dict(feat=None), dict(rois=None), dict(workspace=None), dict(out=None)]),
    ('roi_align_bwd', ROI_CHECK + [dict(dfeat=None), dict(dout=None), dict(rois=None), dict(workspace=None)]),
] for kw in kws] + [
    # the planar aliases hand every other check to the frames pass they call
    ('planar_to_ndhwc', dict(C=60), 'frames_to_ndhwc'),
    ('planar_to_ndhwc', dict(dtype=BAD), 'frames_to_ndhwc'),
    ('ndhwc_to_planar', dict(C=60), 'ndhwc_to_frames'),
    ('ndhwc_to_planar', dict(dtype=BAD), 'ndhwc_to_frames'),
]


def _id(case):
    e, kw, _ = case
    return e + ':' + ','.join('%s=%s' % (k, getattr(v, 'tag', v)) for k, v in sorted(kw.items()))


def _call(_lib, lib, entry, kw):
    names, base = ENTRY[entry]
    fn = getattr(lib, 'sfvos_' + entry)
    names = names.split()
    assert len(names) == len(fn.argtypes), entry
    args = []
    for name, t in zip(names, fn.argtypes):
        if name in kw:
            v = kw[name]
        elif name in base:
            v = base[name]
        else:
            assert t is ctypes.c_void_p, (entry, name)
            v = None if name == 'stream' else P
        args.append(v(_lib) if callable(v) else v)
    return fn(*args)


def test_every_launching_entry_point_has_refusals():
    assert sorted(ENTRY) == sorted({e for e, _, _ in REFUSALS})
    # each entry point that takes a dtype is refused one it does not handle
    for e, (names, _) in ENTRY.items():
        if 'dtype' in names.split():
            assert any(kw.get('dtype') == BAD for x, kw, _ in REFUSALS if x == e), e


@pytest.mark.parametrize('case', REFUSALS, ids=[_id(c) for c in REFUSALS])
def test_bad_call_is_refused_before_any_launch(case):
    _lib, lib = _load()
    entry, kw, prefix = case
    rc = _call(_lib, lib, entry, kw)
    msg = lib.sfvos_last_error().decode()
    assert rc == -1, (rc, msg)
    assert msg.startswith((prefix or entry) + ':'), msg


# ---- sizing functions -------------------------------------------------------------------------------------------------

# function -> [(arguments, value recorded from the parent)].  bn_bwd_rows takes (positions per level[, n_levels]) or
# None; its first five rows are the DAVIS pyramid at (batch, frames) = (1, 1), (2, 3), (2, 7), (1, 22), (4, 32), and
# the 20 x 36 level at (2, 5) is the small shape of the GPU tests.  mse_loss_rows takes the level count of a table or
# None.  packed_weight_bytes: the layers of the (4, 32) plan.
SIZES = {
    'bn_bwd_rows': [
        (([64512, 16128, 4032, 1008, 252],), 169), (([387072, 96768, 24192, 6048, 1512],), 764),
        (([903168, 225792, 56448, 14112, 3528],), 1099), (([1419264, 354816, 88704, 22176, 5544],), 1253),
        (([8257536, 2064384, 516096, 129024, 32256],), 1851), (([7200],), 15), (([1],), 1), (([511, 512, 513],), 4),
        (([262144, 262145],), 1024), (([100, 100, 100, 100, 100, 100, 100, 100],), 8), (([],), -1), (([0],), -1),
        (([-5],), -1), (([100, 0],), -1), (([100, 100, 100, 100, 100, 100, 100, 100], 9), -1), (None, -1),
    ],
    'mse_loss_rows': [
        (-1, -1), (0, -1), (1, 256), (2, 512), (5, 1280), (8, 2048), (9, -1), (None, -1),
    ],
    'relu_bwd_rows': [
        (-5, 0), (0, 0), (1, 1), (63, 1), (64, 1), (65, 2), (392, 7), (1568, 25), (1000000, 15625),
        (2147483648, 33554432),
    ],
    'mask_logits_bwd_rows': [
        ((2, 784), 25), ((1, 1), 1), ((3, 64), 3), ((3, 65), 4), ((100, 784), 1225), ((0, 784), 0), ((2, 0), 0),
        ((-1, 5), 0),
    ],
    'deconv2x2_wgrad_workspace_bytes': [
        ((2, 14, 14, 256, 256), 2097152), ((1, 1, 1, 32, 32), 16384), ((1, 16, 16, 32, 64), 32768),
        ((100, 14, 14, 256, 256), 67108864), ((0, 14, 14, 256, 256), 0), ((2, -1, 14, 256, 256), 0),
        ((2, 14, 14, 0, 256), 0), ((2, 14, 14, 256, -32), 0),
    ],
    'roi_align_workspace_bytes': [
        (-3, 2048), (0, 2048), (1, 2048), (7, 14336), (100, 204800),
    ],
    'packed_weight_bytes': [
        ((0, 32, 32, 11, 9), 405504), ((0, 32, 32, 12, 9), 442368), ((0, 32, 256, 11, 9), 3244032),
        ((0, 64, 32, 11, 1), 90112), ((0, 64, 32, 20, 1), 163840), ((0, 192, 256, 2, 9), 3538944),
        ((0, 224, 256, 2, 9), 4128768), ((1, 32, 32, 11, 9), 202752), ((1, 32, 32, 12, 9), 221184),
        ((1, 32, 256, 11, 9), 1622016), ((1, 64, 32, 11, 1), 45056), ((1, 64, 32, 20, 1), 81920),
        ((1, 192, 256, 2, 9), 1769472), ((1, 224, 256, 2, 9), 2064384), ((2, 192, 256, 2, 9), 3538944),
        ((7, 192, 256, 2, 9), 3538944), ((1, 0, 64, 3, 9), 0), ((0, 64, 64, 0, 9), 0),
        ((1, -32, 64, 3, 9), 18446744073709441024),
    ],
}


def _size(_lib, lib, fn, a):
    f = getattr(lib, 'sfvos_' + fn)
    if fn == 'bn_bwd_rows':
        return f(None if a is None else _lv(*a[0], n=a[1] if len(a) > 1 else None)(_lib))
    if fn == 'mse_loss_rows':
        return f(None if a is None else _mse(a)(_lib))
    return f(*a) if isinstance(a, tuple) else f(a)


@pytest.mark.parametrize('fn', sorted(SIZES))
def test_sizing_function_values_match_recorded(fn):
    _lib, lib = _load()
    got = [(a, _size(_lib, lib, fn, a)) for a, _ in SIZES[fn]]
    assert got == SIZES[fn]
