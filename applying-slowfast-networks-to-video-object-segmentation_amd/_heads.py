"""What the two branches of roi_heads (mask_head.py, box_head.py) share on the host: the precision check, layout
changes, the packer call, and the two backward steps both branches take: ReLU backward with its bias gradient, and the
backward of the class projection they end with."""
import torch

from . import _lib
from ._lib import _f32, _ptr, _stream


def _check_precision(precision):
    if precision not in ('fp32', 'bf16'):
        raise ValueError("precision must be 'fp32' or 'bf16'")
    return precision


def _to_nhwc(x, dt_id, tdt):
    """[N,C,H,W] fp32 (any strides) -> NHWC [N,H,W,C] in the compute dtype (sfvos_frames_to_ndhwc with T = N)."""
    N, C, H, W = x.shape
    s = x if x.dtype == torch.float32 else x.float()
    out = torch.empty((N, H, W, C), dtype=tdt, device=x.device)
    _lib.call('sfvos_frames_to_ndhwc', _ptr(s), s.stride(0), s.stride(1), s.stride(2), s.stride(3), _ptr(out), dt_id,
              N, C, H, W, C, _stream())
    return out


def _to_nchw(x_nhwc, dt_id):
    N, H, W, C = x_nhwc.shape
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=x_nhwc.device)
    _lib.call('sfvos_ndhwc_to_frames', _ptr(x_nhwc), dt_id, _ptr(out), out.stride(0), out.stride(1), out.stride(2),
              out.stride(3), N, C, H, W, C, 0, _stream())
    return out


def _pack(fn, w, dt_id, tdt, *shape):
    """Packed image of weight w (fp32 copy) by the libsfvos packer fn (shape: its size arguments)."""
    wc = _f32(w)
    packed = torch.empty(wc.numel(), dtype=tdt, device=w.device)
    _lib.call(fn, _ptr(wc), _ptr(packed), dt_id, *(shape + (_stream(),)))
    return packed


def _reduce_rows(part):
    """Column sums of the partial rows a kernel left: [rows, n] -> [n] fp32."""
    out = torch.empty(part.shape[1], dtype=torch.float32, device=part.device)
    _lib.call('sfvos_reduce_rows', _ptr(part), part.shape[0], part.shape[1], _ptr(out), 0, _stream())
    return out


def _relu_bwd(dy, a, dt_id):
    """ReLU backward in place, dy [..., C] = a > 0 ? dy : 0, and the gradient [C] of the bias of the layer that produced
    a: the column sums of the new dy, from the partial rows sfvos_relu_bwd leaves."""
    C = dy.shape[-1]
    M = dy.numel() // C
    part = torch.empty((_lib.load().sfvos_relu_bwd_rows(M), C), dtype=torch.float32, device=dy.device)
    _lib.call('sfvos_relu_bwd', _ptr(dy), _ptr(a), _ptr(dy), dt_id, M, C, _ptr(part), _stream())
    return _reduce_rows(part)


def _project_bwd(fn, x, dt_id, operands, dims, rows, J):
    """Backward of a class projection onto J outputs and of the ReLU that produced its input x [..., C]:
    fn(x, dtype, *operands, *dims, relu = 1, dz, part) with `rows` partial rows, then their sum ->
    (dz like x, gradient of the weights [J, C], of the biases [J], column sums of dz [C])."""
    C = x.shape[-1]
    part = torch.empty((rows, J * C + J + C), dtype=torch.float32, device=x.device)
    dz = torch.empty_like(x)
    _lib.call(fn, _ptr(x), dt_id, *([_ptr(t) for t in operands] + list(dims) + [1, _ptr(dz), _ptr(part), _stream()]))
    comb = _reduce_rows(part)
    return dz, comb[:J * C].view(J, C), comb[J * C:J * C + J], comb[J * C + J:]
