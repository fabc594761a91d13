"""CPU (no GPU): what the conv planners return through the ABI -- statistics rows per level (sfvos_conv3d_stat_rows)
and weight-gradient workspace bytes (sfvos_conv3d_wgrad_workspace_bytes) -- for the descriptors of every layer, and
the refusal of malformed descriptors.  Without a device the planners see 256 compute units, the MI355X's count.

The expected values are recorded in tests/golden/conv_plan_cpu.json."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_plan_cpu.json')
CONFIGS = [(1, 1), (3, 7), (4, 32), (4, 64)]
SMALL = [('0', (20, 36))]


F32, BF16, FP8 = 0, 1, 2   # SFVOS_F32, SFVOS_BF16, SFVOS_FP8


def _load():
    from sfvos_amd import _lib
    return _lib, _lib.load()


def _pyr(_lib, levels):
    p = _lib.Pyramid()
    p.n_levels = len(levels)
    for i, (_, (h, w)) in enumerate(levels):
        p.h[i], p.w[i] = h, w
    return p


def _desc(_lib, dt, pyr, batch, kt, taps, c_in, c_out, t_in, ld_x, ld_y, t_alloc=None, t_offset=0, pad_t=0,
          accumulate=0):
    d = _lib.ConvDesc()
    d.dtype, d.batch, d.kt, d.taps, d.pyr = dt, batch, kt, taps, pyr
    d.t_in, d.c_in, d.c_out, d.pad_t, d.accumulate = t_in, c_in, c_out, pad_t, accumulate
    d.t_alloc, d.t_offset = (t_in if t_alloc is None else t_alloc), t_offset
    d.ld_x, d.ld_y = ld_x, ld_y
    return d


def plan_cases(_lib):
    """(label, kind, desc): kind 'rows' -> sfvos_conv3d_stat_rows, 'ws' -> sfvos_conv3d_wgrad_workspace_bytes."""
    from sfvos_amd import SlowFastPlan, davis_pyramid
    cases = []
    for sp, fp in CONFIGS:
        plan = SlowFastPlan(256, sp, fp)
        for pname, levels in (('davis', davis_pyramid()), ('small', SMALL)):
            pyr = _pyr(_lib, levels)
            P = sum(h * w for _, (h, w) in levels)
            for dname, dt in (('f32', F32), ('bf16', BF16)):
                for l in plan.layers:
                    tag = '%d-%d/%s/%s/%s' % (sp, fp, pname, dname, l.name)
                    fwd = dict(kt=l.kt, taps=l.taps, c_in=l.c_in, c_out=l.c_out, t_in=l.t_in)
                    cases.append((tag + '/fwd', 'rows', _desc(_lib, dt, pyr, 2, ld_x=l.c_in, ld_y=l.c_out, **fwd)))
                    # level-major window sticking out of a larger buffer (t_alloc > t_in, t_offset > 0)
                    cases.append((tag + '/fwd-window', 'rows', _desc(_lib, dt, pyr, 2, ld_x=256, ld_y=256,
                                                                     t_alloc=l.t_in + 3, t_offset=2, **fwd)))
                    for acc in (0, 1):
                        d = _desc(_lib, dt, pyr, 2, l.kt, l.taps, l.c_out, l.c_in, l.t_out, ld_x=l.c_out, ld_y=l.c_in,
                                  pad_t=l.kt - 1, accumulate=acc)
                        cases.append((tag + '/dgrad-acc%d' % acc, 'rows', d))
                    cases.append((tag + '/wgrad', 'ws', _desc(_lib, dt, pyr, 2, ld_x=l.c_in, ld_y=l.c_out, **fwd)))
                    cases.append((tag + '/wgrad-window', 'ws', _desc(_lib, dt, pyr, 2, ld_x=256, ld_y=256,
                                                                     t_alloc=l.t_in + 3, t_offset=2, **fwd)))
                    # frame-major ring (SlowFastStream): batch 1, frames at a stride of one frame of all levels
                    for g in (1, 2):
                        d = _desc(_lib, dt, pyr, 1, l.kt, l.taps, l.c_in, l.c_out, l.kt + g - 1, ld_x=l.c_in,
                                  ld_y=l.c_out, t_alloc=2 * (l.kt + 2), t_offset=3)
                        d.x_frame_stride = d.y_frame_stride = P
                        cases.append((tag + '/ring-g%d' % g, 'rows', d))
                    if l.c_in == 256:   # channel-group-major x: [C/32][M][32] bf16, [C/64][M][64] e4m3
                        for gname, gdt, ge in (('bf16', BF16, 32), ('e4m3', FP8, 64)):
                            if dname == 'f32' or (gdt == FP8 and l.taps != 9):
                                continue
                            d = _desc(_lib, gdt, pyr, 2, ld_x=ge, ld_y=l.c_out, **fwd)
                            d.x_group_stride = 2 * l.t_in * P * ge
                            cases.append((tag + '/fwd-groups-' + gname, 'rows', d))
                            if gdt == BF16:
                                cases.append((tag + '/wgrad-groups', 'ws', d))
                        if l.taps == 9 and dname == 'bf16':   # e4m3 forward, level-major
                            cases.append((tag + '/fwd-e4m3', 'rows', _desc(_lib, FP8, pyr, 2, ld_x=l.c_in,
                                                                           ld_y=l.c_out, **fwd)))
    return cases


def plan_values(_lib, lib):
    rows = (ctypes.c_int * _lib.MAX_LEVELS)()
    out = {}
    for label, kind, d in plan_cases(_lib):
        if kind == 'rows':
            for i in range(_lib.MAX_LEVELS):
                rows[i] = -7
            total = lib.sfvos_conv3d_stat_rows(ctypes.byref(d), rows)
            out[label] = [total] + [rows[i] for i in range(d.pyr.n_levels)] if total >= 0 else [total]
        else:
            out[label] = int(lib.sfvos_conv3d_wgrad_workspace_bytes(ctypes.byref(d)))
    return out


def test_stat_rows_and_wgrad_workspace_match_recorded():
    _lib, lib = _load()
    with open(GOLDEN) as f:
        want = json.load(f)
    got = plan_values(_lib, lib)
    assert sorted(got) == sorted(want)
    bad = [(k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]]
    assert not bad, bad[:10]
    # every kind of descriptor is covered by accepted cases
    assert all(v[0] > 0 for k, v in want.items() if isinstance(v, list))
    assert all(v > 0 for k, v in want.items() if not isinstance(v, list))


def _base(_lib, dt=None):
    from sfvos_amd import davis_pyramid
    return _desc(_lib, BF16 if dt is None else dt, _pyr(_lib, davis_pyramid()), 2, 3, 9, 64, 64, 5, 64, 64)


def _set(**kw):
    def f(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return f


def _level(i, h, w):
    def f(d):
        d.pyr.h[i], d.pyr.w[i] = h, w
    return f


# one malformed descriptor per check every conv entry point shares; `both`: the weight gradient refuses it too
REFUSALS = [
    ('struct_size', _set(struct_size=8), True),
    ('dtype', _set(dtype=7), True),
    ('taps', _set(taps=3), True),
    ('c_in', _set(c_in=48), True),
    ('c_out', _set(c_out=0), True),
    ('batch', _set(batch=0), True),
    ('t_in', _set(t_in=0), True),
    ('kt', _set(kt=0), False),
    ('t_alloc', _set(t_alloc=0), True),
    ('t_offset', _set(t_offset=1 << 20), True),
    ('t_offset_neg', _set(t_offset=-(1 << 20)), True),
    ('n_levels_0', lambda d: setattr(d.pyr, 'n_levels', 0), True),
    ('n_levels_9', lambda d: setattr(d.pyr, 'n_levels', 9), True),
    ('level_h', _level(2, 0, 84), True),
    ('level_w', _level(4, 12, -1), True),
    ('frame_2gib', lambda d: (_level(0, 4096, 4096)(d), _set(ld_x=64, ld_y=64)(d)), False),
]


@pytest.mark.parametrize('name,mutate,both', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_malformed_descriptor_is_refused(name, mutate, both):
    _lib, lib = _load()
    ok = _base(_lib)
    assert lib.sfvos_conv3d_stat_rows(ctypes.byref(ok), None) > 0
    assert lib.sfvos_conv3d_wgrad_workspace_bytes(ctypes.byref(ok)) > 0
    d = _base(_lib)
    mutate(d)
    # the planners refuse before any pointer is looked at or any kernel is launched
    assert lib.sfvos_conv3d_stat_rows(ctypes.byref(d), None) == -1
    assert lib.sfvos_last_error().decode().startswith('conv:')
    assert lib.sfvos_conv3d(ctypes.byref(d), None, None, None, None, None, None) == -1
    assert lib.sfvos_last_error().decode().startswith('conv:')
    if both:
        assert lib.sfvos_conv3d_wgrad_workspace_bytes(ctypes.byref(d)) == 0
        assert lib.sfvos_last_error().decode().startswith('wgrad:')
        assert lib.sfvos_conv3d_wgrad(ctypes.byref(d), None, None, None, 0, None, None) == -1
        assert lib.sfvos_last_error().decode().startswith('wgrad:')


def test_null_descriptor_is_refused():
    _lib, lib = _load()
    assert lib.sfvos_conv3d_stat_rows(None, None) == -1
    assert lib.sfvos_last_error().decode().startswith('conv:')
    assert lib.sfvos_conv3d_wgrad_workspace_bytes(None) == 0
    assert lib.sfvos_last_error().decode().startswith('wgrad:')
