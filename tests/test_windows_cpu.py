"""CPU: the reuse planner of sfvos_amd.SlowFastWindows and the host side of sfvos_shift_frames (no GPU needed)."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reuse_shift_planner():
    from sfvos_amd.windows import reuse_shift
    tag = ('seq', 1)
    assert reuse_shift(4, 5, 22, tag, tag) == 1
    assert reuse_shift(6, 9, 22, tag, tag) == 3          # a gap: frames without boxes are skipped
    assert reuse_shift(0, 21, 22, tag, tag) == 21
    assert reuse_shift(0, 22, 22, tag, tag) == 0         # s >= t_out: nothing left to reuse
    assert reuse_shift(0, 30, 22, tag, tag) == 0
    assert reuse_shift(5, 5, 22, tag, tag) == 0          # s <= 0
    assert reuse_shift(5, 4, 22, tag, tag) == 0
    assert reuse_shift(None, 0, 22, None, tag) == 0      # nothing cached
    assert reuse_shift(4, 5, 22, ('seq', 0), tag) == 0   # anything the frames depend on changed
    assert reuse_shift(2, 3, 3, tag, tag) == 1           # slow_conv1 at (4,32): t_out = 3
    assert reuse_shift(0, 3, 3, tag, tag) == 0


def _seq(n=3):
    from sfvos_amd import PackedClip
    levels = [torch.zeros(1, n, 4, 5, 32), torch.zeros(1, n, 2, 3, 32)]
    return PackedClip.from_levels(levels)


def test_window_tag_follows_weights_epoch_and_sequence():
    from sfvos_amd import _lib
    from sfvos_amd.windows import reuse_shift, window_tag
    conv = torch.nn.Conv3d(32, 32, (3, 3, 3), padding=(0, 1, 1))
    seq = _seq()
    t0 = window_tag(seq, conv, 'fp32')
    assert window_tag(seq, conv, 'fp32') == t0
    assert reuse_shift(0, 1, 5, t0, window_tag(seq, conv, 'fp32')) == 1
    _lib.bump_weight_epoch()                                  # FusedSGD.step()
    t1 = window_tag(seq, conv, 'fp32')
    assert t1 != t0 and reuse_shift(0, 1, 5, t0, t1) == 0
    with torch.no_grad():
        conv.weight.add_(1.0)                                 # torch.optim.SGD.step(), load_state_dict
    t2 = window_tag(seq, conv, 'fp32')
    assert t2 != t1 and reuse_shift(0, 1, 5, t1, t2) == 0
    with torch.no_grad():
        conv.bias.mul_(2.0)
    t3 = window_tag(seq, conv, 'fp32')
    assert t3 != t2
    assert window_tag(_seq(), conv, 'fp32') != t3             # another sequence
    assert window_tag(seq, conv, 'bf16') != t3                # another precision
    seq.data.add_(1.0)                                        # the sequence itself was written
    assert window_tag(seq, conv, 'fp32') != t3


def test_pathway_1_1_never_reuses():
    from sfvos_amd import SlowFastPlan
    from sfvos_amd.windows import reuse_shift
    plan = SlowFastPlan(256, 1, 1)
    for name in ('f1', 's1'):
        t_out = plan.layer(name).t_out
        assert t_out == 1
        assert all(reuse_shift(c, c + s, t_out, 'x', 'x') == 0 for c in range(4) for s in range(-1, 3))
    plan = SlowFastPlan(256, 4, 32)
    assert (plan.layer('f1').t_out, plan.layer('s1').t_out) == (22, 3)


def test_shift_kernel_is_built_and_bound():
    import importlib.util
    from sfvos_amd import _lib
    spec = importlib.util.spec_from_file_location(
        'b', os.path.join(ROOT, 'applying-slowfast-networks-to-video-object-segmentation_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert 'window_shift.hip' in b.SOURCES and '--offload-arch=gfx950' in b.FLAGS
    assert _lib.ABI_REVISION >= 301
    for name in ('sfvos_shift_frames', 'sfvos_shift_frames_stat_rows'):
        assert name in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libsfvos.so not built (run `python __graft_entry__.py`)')
    obj = os.path.join(os.path.dirname(_lib.LIB_PATH), 'window_shift.o')
    assert os.path.exists(obj) and b'gfx950' in open(obj, 'rb').read()


def _lib_or_skip():
    from sfvos_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libsfvos.so not built (run `python __graft_entry__.py`)')
    return _lib, _lib.load()


def test_shift_stat_rows_are_level_major_and_capped():
    _lib, lib = _lib_or_skip()
    pyr = _lib.make_pyramid([(12, 21), (6, 10)])
    rows = (ctypes.c_int * _lib.MAX_LEVELS)()
    # one row per 512-position run of a frame, at most 512 per level
    assert lib.sfvos_shift_frames_stat_rows(ctypes.byref(pyr), 1, 5, 32, rows) == 5 + 5
    assert list(rows[:2]) == [5, 5]
    davis = _lib.make_pyramid([(192, 336), (96, 168), (48, 84), (24, 42), (12, 21)])
    n = lib.sfvos_shift_frames_stat_rows(ctypes.byref(davis), 1, 22, 32, rows)
    assert list(rows[:5]) == [512, 512, 176, 44, 22] and n == sum(rows[:5])
    assert lib.sfvos_shift_frames_stat_rows(ctypes.byref(pyr), 2, 3, 192, None) == 12
    for bad in ((1, 1, 32), (0, 5, 32), (1, 5, 48), (1, 5, 288)):   # T < 2, B < 1, C not a multiple of 32 / > 256
        assert lib.sfvos_shift_frames_stat_rows(ctypes.byref(pyr), *bad, rows) < 0


def test_shift_refuses_bad_arguments_before_any_launch():
    """Argument checks run on the host: none of these calls reaches the device (the pointers are never touched)."""
    _lib, lib = _lib_or_skip()
    pyr = _lib.make_pyramid([(4, 5), (2, 3)])
    M, C, es = 1 * 4 * (20 + 6), 32, 4            # B = 1, T = 4 positions of prev / out, fp32
    base = 1 << 40                                # never dereferenced
    prev, out, fresh = base, base + M * C * es, base + 2 * M * C * es
    stream = None

    def call(prev=prev, fresh=fresh, out=out, dtype=_lib.F32, T=4, s=1, C=C, ld=C):
        return lib.sfvos_shift_frames(prev, fresh, out, dtype, ctypes.byref(pyr), 1, T, s, C, ld, None, stream)
    assert call(s=0) < 0 and call(s=4) < 0 and call(T=1) < 0                    # 1 <= s < T
    assert call(dtype=_lib.FP8) < 0
    assert call(C=48) < 0 and call(ld=16) < 0 and call(dtype=_lib.BF16, ld=36) < 0
    assert call(out=prev) < 0 and call(out=prev + 64) < 0 and call(out=prev - 64) < 0   # never in place
    assert call(out=fresh) < 0                                                   # nor over the new frames
    assert call(prev=0) < 0 and call(out=prev + 8) < 0
    msg = lib.sfvos_last_error().decode()
    assert 'shift_frames' in msg
