"""The scale discriminator's HIP entry points (include/vmasr_hip.h, csrc/gconv1d.hip, csrc/stem1d.hip, csrc/dconv1d.hip), one Python
function each — the companion of mpd_ops.py.

Every function takes tensors and plain numbers, allocates its outputs and launches through _lib.call.  No autograd and no switches here:
vm_asr_amd/msd.py decides what runs.  Layout: channel-first fp32, x (B, Cin, L), w (Cout, Cin / groups, k), y (B, Cout, T); the stem has Cin = groups = stride = 1."""
import torch

from . import _lib
from .mpd_ops import _call, _new


def out_len(L, k, stride, pad):
    return (L + 2 * pad - k) // stride + 1


def gconv1d_supported(Cin, Cout, groups, k, stride):
    return bool(_lib.lib().vmasr_gconv1d_supported(int(Cin), int(Cout), int(groups), int(k), int(stride)))


def gconv1d_supported_launch(Cin, Cout, groups, k, stride, pad, B, L):
    """What the three launchers accept (the same predicate they check): the shape, 0 <= pad < k, B and L within one launch."""
    return bool(_lib.lib().vmasr_gconv1d_supported_launch(int(Cin), int(Cout), int(groups), int(k), int(stride), int(pad), int(B), int(L)))


def gconv1d_fwd(x, w, bias, groups, stride, pad, act):
    """-> (y, pre): y = GELU(pre), pre = conv + bias if act, else y = conv + bias and pre None.  bias may be None."""
    B, Cin, L = x.shape
    Cout, _, k = w.shape
    y = _new(x, (B, Cout, out_len(L, k, stride, pad)))
    pre = torch.empty_like(y) if act else None
    _call(_lib.lib().vmasr_gconv1d_fwd, x, w, bias, y, pre, B, Cin, Cout, groups, L, k, stride, pad, int(bool(act)))
    return y, pre


def gconv1d_dgrad(gy, pre, w, x_shape, groups, stride, pad):
    """-> dx of x_shape from gy (times GELU'(pre) if pre is given)."""
    B, Cin, L = x_shape
    Cout, _, k = w.shape
    dx = _new(gy, x_shape)
    _call(_lib.lib().vmasr_gconv1d_dgrad, gy, pre, w, dx, B, Cin, Cout, groups, L, k, stride, pad)
    return dx


def gconv1d_wgrad(x, gy, pre, w_shape, groups, stride, pad, want_dw=True, want_db=True):
    """-> (dw of w_shape, db (Cout,)), each None unless wanted; split-K partials in a workspace, summed in a fixed order."""
    B, Cin, L = x.shape
    Cout, _, k = w_shape
    if not (want_dw or want_db):
        return None, None
    nbytes = _lib.lib().vmasr_gconv1d_wgrad_workspace(Cin, Cout, groups, k, stride, pad, B, L)
    if nbytes == 0:
        raise RuntimeError(f"gconv1d_wgrad: unsupported shape (Cin={Cin} Cout={Cout} groups={groups} k={k} stride={stride} pad={pad} B={B} L={L})")
    ws = _new(x, (nbytes // 4,))
    dw = _new(x, tuple(w_shape)) if want_dw else None
    db = _new(x, (Cout,)) if want_db else None
    _call(_lib.lib().vmasr_gconv1d_wgrad, x, gy, pre, dw, db, ws, nbytes, B, Cin, Cout, groups, L, k, stride, pad)
    return dw, db


def dconv1d_tiles():
    """(largest position tile, channels of an M tile, channels of a staged K chunk, most taps) of csrc/dconv1d.hip (the tests size their
    edge cases by them)."""
    l = _lib.lib()
    return int(l.vmasr_dconv1d_pos_tile()), int(l.vmasr_dconv1d_m_tile()), int(l.vmasr_dconv1d_k_chunk()), int(l.vmasr_dconv1d_max_taps())


def dconv1d_supported(Cin, Cout, groups, k, stride):
    return bool(_lib.lib().vmasr_dconv1d_supported(int(Cin), int(Cout), int(groups), int(k), int(stride)))


def dconv1d_supported_launch(Cin, Cout, groups, k, stride, pad, B, L):
    """What the three dense launchers accept (the same predicate they check): groups 1, stride 1, k <= 8, 0 <= pad < k, B and L within
    one launch."""
    return bool(_lib.lib().vmasr_dconv1d_supported_launch(int(Cin), int(Cout), int(groups), int(k), int(stride), int(pad), int(B), int(L)))


def dconv1d_fwd_slabs(Cin, Cout, groups, k, stride, pad, B, L):
    """K slabs of the forward at this shape (1: the epilogue in the GEMM's own launch; 0: a refused shape)."""
    return int(_lib.lib().vmasr_dconv1d_fwd_slabs(int(Cin), int(Cout), int(groups), int(k), int(stride), int(pad), int(B), int(L)))


def _dconv1d_ws(query, like, Cin, Cout, groups, k, stride, pad, B, L):
    """(workspace or None, its bytes): 0 bytes for one slab, and for a refused shape, which the launcher then names."""
    nbytes = query(Cin, Cout, groups, k, stride, pad, B, L)
    return (_new(like, (nbytes // 4,)) if nbytes else None), nbytes


def dconv1d_fwd(x, w, bias, stride, pad, act, groups=1):
    """-> (y, pre) of the dense stride-1 convolution: y = GELU(pre), pre = conv + bias if act, else y = conv + bias and pre None."""
    B, Cin, L = x.shape
    Cout, _, k = w.shape
    y = _new(x, (B, Cout, max(out_len(L, k, 1, pad), 0)))
    pre = torch.empty_like(y) if act else None
    ws, nbytes = _dconv1d_ws(_lib.lib().vmasr_dconv1d_fwd_workspace, x, Cin, Cout, groups, k, stride, pad, B, L)
    _call(_lib.lib().vmasr_dconv1d_fwd, x, w, bias, y, pre, ws, nbytes, B, Cin, Cout, groups, L, k, stride, pad, int(bool(act)))
    return y, pre


def dconv1d_dgrad(gy, pre, w, x_shape, stride, pad, groups=1):
    """-> dx of x_shape from gy (times GELU'(pre) if pre is given)."""
    B, Cin, L = x_shape
    Cout, _, k = w.shape
    dx = _new(gy, tuple(x_shape))
    ws, nbytes = _dconv1d_ws(_lib.lib().vmasr_dconv1d_dgrad_workspace, gy, Cin, Cout, groups, k, stride, pad, B, L)
    _call(_lib.lib().vmasr_dconv1d_dgrad, gy, pre, w, dx, ws, nbytes, B, Cin, Cout, groups, L, k, stride, pad)
    return dx


def dconv1d_wgrad(x, gy, pre, w_shape, stride, pad, want_dw=True, want_db=True, groups=1):
    """-> (dw of w_shape, db (Cout,)), each None unless wanted; sums in a fixed order (whole-K tiles or slab partials in a workspace)."""
    B, Cin, L = x.shape
    Cout, _, k = w_shape
    if not (want_dw or want_db):
        return None, None
    ws, nbytes = _dconv1d_ws(_lib.lib().vmasr_dconv1d_wgrad_workspace, x, Cin, Cout, groups, k, stride, pad, B, L)
    dw = _new(x, tuple(w_shape)) if want_dw else None
    db = _new(x, (Cout,)) if want_db else None
    _call(_lib.lib().vmasr_dconv1d_wgrad, x, gy, pre, dw, db, ws, nbytes, B, Cin, Cout, groups, L, k, stride, pad)
    return dw, db


def stem1d_time_tile():
    """Positions of one workgroup pass of the stem kernels (the tests size their edge cases by it)."""
    return int(_lib.lib().vmasr_stem1d_time_tile())


def stem1d_channel_group():
    """Output channels of one workgroup of the stem's forward."""
    return int(_lib.lib().vmasr_stem1d_channel_group())


def stem1d_supported_launch(Cout, k, stride, pad, B, L):
    """What vmasr_stem1d_fwd / _bwd accept (the same predicate they check)."""
    return bool(_lib.lib().vmasr_stem1d_supported_launch(int(Cout), int(k), int(stride), int(pad), int(B), int(L)))


def stem1d_fwd(x, w, bias, pad, act):
    """-> y = GELU(conv1d(x, w, bias, 1, pad)) if act, else the convolution + bias; x (B, 1, L), w (Cout, 1, k).  No pre-activation."""
    B, _, L = x.shape
    Cout, _, k = w.shape
    y = _new(x, (B, Cout, out_len(L, k, 1, pad)))
    _call(_lib.lib().vmasr_stem1d_fwd, x, w, bias, y, B, Cout, L, k, 1, pad, int(bool(act)))
    return y


def stem1d_bwd(gy, x, w, bias, pad, act, want_dx=True, want_dw=True, want_db=True):
    """-> (dx (B, 1, L), dw (Cout, 1, k), db (Cout,)), each None unless wanted, from gy and the forward's operands (the pre-activation
    is rebuilt in registers).  dw / db: per-slab partials in a workspace, summed in a fixed order."""
    B, _, L = x.shape
    Cout, _, k = w.shape
    if not (want_dx or want_dw or want_db):
        return None, None, None
    ws, nbytes = None, 0
    if want_dw or want_db:
        nbytes = _lib.lib().vmasr_stem1d_bwd_workspace(Cout, k, 1, pad, B, L)
        if nbytes == 0:
            raise RuntimeError(f"stem1d_bwd: unsupported shape (Cout={Cout} k={k} pad={pad} B={B} L={L})")
        ws = _new(x, (nbytes // 4,))
    dx = _new(x, tuple(x.shape)) if want_dx else None
    dw = _new(x, tuple(w.shape)) if want_dw else None
    db = _new(x, (Cout,)) if want_db else None
    _call(_lib.lib().vmasr_stem1d_bwd, gy, x, w, bias, dx, dw, db, ws, nbytes, B, Cout, L, k, 1, pad, int(bool(act)))
    return dx, dw, db


def stem1d_fm_supported_launch(Cout, k, stride, pad, B, L):
    """What vmasr_stem1d_fm_fwd / _fm_bwd accept (the same predicate they check): the stem's own set, GELU on."""
    return bool(_lib.lib().vmasr_stem1d_fm_supported_launch(int(Cout), int(k), int(stride), int(pad), int(B), int(L)))


def stem1d_fm_fwd(x, w, bias, y_real, pad):
    """-> (y, partials): y = GELU(conv1d(x, w, bias, 1, pad)), bit-equal to stem1d_fwd's, and the float64 per-workgroup sums of
    |y - y_real| (the caller adds them); y_real: y's shape.  Neither a sign nor a difference tensor is written."""
    B, _, L = x.shape
    Cout, _, k = w.shape
    y = _new(x, (B, Cout, out_len(L, k, 1, pad)))
    if tuple(y_real.shape) != tuple(y.shape):
        raise RuntimeError(f"stem1d_fm_fwd: y_real {tuple(y_real.shape)} is not the map's shape {tuple(y.shape)}")
    nbytes = _lib.lib().vmasr_stem1d_fm_workspace(Cout, k, 1, pad, B, L)       # (0: a refused shape; the launcher says which)
    partials = _new(x, (max(nbytes // 8, 1),), torch.float64)
    _call(_lib.lib().vmasr_stem1d_fm_fwd, x, w, bias, y_real, y, partials, nbytes, B, Cout, L, k, 1, pad)
    return y, partials


def stem1d_fm_bwd(gy, x, w, bias, y_real, gterm, coef, pad):
    """-> dx (B, 1, L) from g = gy + coef * gterm * sgn(y - y_real) with y and the pre-activation rebuilt in registers.  gy (the map's
    upstream gradient) or gterm (the loss term's, ONE fp32 element on the device) may be None, not both; coef: a Python float."""
    B, _, L = x.shape
    Cout, _, k = w.shape
    T = out_len(L, k, 1, pad)
    for name, t in (("gy", gy), ("y_real", y_real)):
        if t is not None and tuple(t.shape) != (B, Cout, T):
            raise RuntimeError(f"stem1d_fm_bwd: {name} {tuple(t.shape)} is not the map's shape {(B, Cout, T)}")
    if gterm is not None and gterm.numel() != 1:
        raise RuntimeError("stem1d_fm_bwd: gterm must have one element")
    dx = _new(x, tuple(x.shape))
    _call(_lib.lib().vmasr_stem1d_fm_bwd, gy, x, w, bias, y_real, gterm, float(coef), dx, B, Cout, L, k, 1, pad)
    return dx
