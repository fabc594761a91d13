"""Training windows of a resident video with first-layer reuse (extended to training).

The reference trains SlowFastLayers one centre frame at a time (code/helpers/model.py:316-374): for centre frame i it
takes the window of fp frames around i (zero frames beyond the ends of the video, model.py:215-225), runs forward, loss
and backward(), and steps the optimiser after every second frame.  Inside such a pair the weights are the same and the
second window is the first one shifted by one frame.  fast_conv1 and slow_conv1 read the raw input features, so their
outputs BEFORE BatchNorm depend only on the weights and the input frames: the second window's pre-BN buffers are the
first window's frames s .. t_out-1 followed by s new frames.  `SlowFastWindows.enhance` computes only those s frames
(sfvos_conv3d over s + kt - 1 input frames) and shifts the rest over (sfvos_shift_frames, which also writes the
BatchNorm statistics rows).  Everything after the first layers' BatchNorm runs as in the plain path: train-mode
BatchNorm normalises with per-window statistics, so nothing later is shift-invariant.

Statistics difference: with reuse, BatchNorm of fast_conv1 / slow_conv1 sums the STORED pre-BN values (rounded to bf16
in bf16 mode); the plain path sums the conv's f32 accumulators.  In fp32 the two agree to rounding.

Every window is a view of the resident sequence: sfvos_conv_desc.t_alloc / t_offset address it inside the sequence's
buffer, and the frames beyond the ends are zero frames that are never read -- no per-window copy of the input."""
from collections import OrderedDict

from . import _lib
from ._lib import _DT
from .module import RawReuse

REUSED_LAYERS = ('f1', 's1')


def window_tag(seq, conv, precision):
    """Everything a layer's pre-BN frames depend on besides the centre frame: the sequence (storage, _version,
    pyramid), the precision and the weights (_lib.weight_tag of weight and bias)."""
    d = seq.data
    return (d.untyped_storage().data_ptr(), d.storage_offset(), d._version, tuple(d.shape), d.dtype,
            tuple(seq.shapes), precision, _lib.weight_tag((conv.weight, conv.bias)))


def reuse_shift(prev_centre, centre, t_out, prev_tag, tag):
    """Frames s the window at `centre` shifts its layer's pre-BN buffer by to reuse the window at `prev_centre`:
    1 <= s < t_out when the new centre is s frames later and nothing the frames depend on changed; 0 = recompute."""
    if prev_centre is None or prev_tag is None or prev_tag != tag:
        return 0
    s = centre - prev_centre
    return s if 1 <= s < t_out else 0


class SlowFastWindows(object):
    def __init__(self, module, seq, reuse=True):
        """module: a sfvos_amd.SlowFastLayers on the GPU (fp32 or bf16); seq: PackedClip of the whole video's
        features (B = 1, frames = N, every frame stored); reuse=False: every window runs the plain path (A/B)."""
        self.m = module
        self.seq = seq
        self.reuse = bool(reuse)
        plan = module.plan
        if module.precision not in ('fp32', 'bf16'):
            raise RuntimeError("SlowFastWindows trains in fp32 or bf16; precision=%r is inference-only"
                               % (module.precision,))
        _, tdt = _DT[module.precision]
        d = seq.data
        module._check_ready(d)
        if d.requires_grad:
            raise RuntimeError('SlowFastWindows: the sequence must not require grad (the reference computes the '
                               'backbone features under no_grad; input gradients are not built here)')
        if seq.batch != 1 or seq.pad != (0, 0):
            raise RuntimeError('SlowFastWindows takes one video (B = 1) with every frame stored, got B=%d pad=%s'
                               % (seq.batch, seq.pad))
        if seq.channels != plan.input_size or d.dtype != tdt or not d.is_contiguous() or seq.layout == 'grouped8':
            raise RuntimeError('SlowFastWindows: the sequence must be contiguous %s with %d channels, got %s %s x %d'
                               % (tdt, plan.input_size, seq.layout, d.dtype, seq.channels))
        if len(seq.shapes) > _lib.MAX_LEVELS:
            raise RuntimeError('at most %d pyramid levels' % _lib.MAX_LEVELS)
        self.reset()

    @property
    def frames(self):
        return self.seq.frames

    def reset(self):
        """Drop the cache: the next window is computed whole."""
        self._centre = None
        self._raw = {}
        self._tags = {}
        self.reused = {n: 0 for n in REUSED_LAYERS}

    def _layer_conv(self, name):
        return getattr(self.m, self.m.plan.layer(name).conv)

    def enhance(self, i):
        """Fused features of the window of fp frames around centre frame i (zero frames beyond the ends):
        OrderedDict level -> [1,256,H,W] fp32, = module.enhance_packed of that window.  Autograd flows into the
        module's parameters."""
        m, plan, seq = self.m, self.m.plan, self.seq
        N = seq.frames
        if not 0 <= int(i) < N:
            raise IndexError('centre frame %d outside the sequence [0, %d)' % (i, N))
        i = int(i)
        if m.precision not in ('fp32', 'bf16') or seq.data.requires_grad:
            raise RuntimeError('SlowFastWindows: precision must stay fp32 / bf16 and the sequence must not require grad')
        tags = {n: window_tag(seq, self._layer_conv(n), m.precision) for n in REUSED_LAYERS}
        prev = {}
        for n in REUSED_LAYERS:
            s = reuse_shift(self._centre, i, plan.layer(n).t_out, self._tags.get(n), tags[n]) if self.reuse else 0
            if s and n in self._raw:
                prev[n] = (self._raw[n], s)
        hook = RawReuse(prev) if self.reuse else None
        # the window is frames [i - fp//2, i - fp//2 + fp) of the sequence; the slow pathway reads its centre frames
        # (enhance_packed's default slow_offset)
        merged = m._enhance([seq.data], mode='packed', L=len(seq.shapes), shapes=seq.shapes, B=1,
                            slow_offset=plan.fp // 2 - plan.sp // 2, x_frames=N, x_pad=plan.fp // 2 - i, reuse=hook)
        self.reused = {n: (plan.layer(n).t_out - prev[n][1]) if n in prev else 0 for n in REUSED_LAYERS}
        if hook is not None:
            self._centre, self._raw, self._tags = i, dict(hook.raw), tags
        return OrderedDict(zip(seq.keys, merged))
