"""The period discriminator's HIP entry points (include/vmasr_hip.h), one Python function each — the companion of convgemm.py.

Every function takes tensors and plain numbers, allocates its outputs and launches through _call.  No autograd and no switches here:
vm_asr_amd/discriminator.py decides what runs.  Stacked layout as in convgemm.py: (n slots, rows, C) channel-last, geom =
((nseq_i, H_i), ...); "xs" is a list of per-slot tensors (None = absent) or ONE stacked tensor whose slot i is xs[i]."""
import ctypes

import torch

from . import _lib
from ._lib import ptr as _p

_F32, _BF16 = torch.float32, torch.bfloat16


def need(*ts):
    for t in ts:
        if t is not None and not (t.is_cuda and t.is_contiguous()):
            raise RuntimeError("vm_asr_amd: tensors must be contiguous CUDA tensors (there is no CPU path)")


def _call(fn, *args):
    """_lib.call for tensors that must also be contiguous."""
    need(*[a for a in args if torch.is_tensor(a)])
    _lib.call(fn, *args)


def _new(like, shape, dtype=None):
    return torch.empty(shape, dtype=dtype or like.dtype, device=like.device)


def geom_of(xs):
    """geom of channel-last (B, P, H, C) tensors (or their shapes): slot i = B*P_i sequences of H_i positions."""
    return tuple((s[0] * s[1], s[2]) for s in (getattr(x, "shape", x) for x in xs))


def _slot_arrays(ptrs, Ns, Hs=None):
    """ctypes host arrays (device pointers, per-slot sizes) of the multi-slot entry points (include/vmasr_hip.h)."""
    n = len(ptrs)
    a = (ctypes.c_void_p * n)(*[ctypes.c_void_p(p) if p else None for p in ptrs])
    return a, (ctypes.c_int64 * n)(*Ns), (ctypes.c_int32 * n)(*Hs) if Hs is not None else None


def _ptrs(xs, n):
    """Device addresses of the n slots of xs: a list of tensors (None = absent, 0) or ONE stacked tensor (slot i = xs[i])."""
    if torch.is_tensor(xs):
        need(xs)
        return [xs.data_ptr() + i * xs.stride(0) * xs.element_size() for i in range(n)]
    need(*xs)
    return [x.data_ptr() if x is not None else 0 for x in xs]


def _slots(xs, geom):
    return _slot_arrays(_ptrs(xs, len(geom)), [g[0] for g in geom], [g[1] for g in geom])


def _ptr_array(tensors):
    need(*tensors)
    return (ctypes.c_void_p * len(tensors))(*[_p(t) for t in tensors])


def im2col_kx1(xs, geom, C, k, stride, pad, rows=0):
    """-> cols (n, rows, k*C), (tap, channel) column order, zero rows below each slot's data (rows = 0, one slot: none); a launch per slot."""
    x0, (nseq0, H0), src = xs[0], geom[0], _ptrs(xs, len(geom))
    cols = _new(x0, (len(geom), rows or nseq0 * ((H0 + 2 * pad - k) // stride + 1), k * C))
    for i, (nseq, H) in enumerate(geom):
        _lib.call(_lib.lib().vmasr_im2col_kx1, src[i], cols[i], nseq, H, C, k, stride, pad, rows, _lib.torch_dtype_code(x0.dtype))
    return cols


def col2im_kx1(g, shape, k, stride, pad):
    """Adjoint of im2col_kx1 for one slot: g (B, P, H1, k*C) -> dx of `shape` = (B, P, H, C)."""
    B, P, H, C = shape
    dx = _new(g, shape)
    _call(_lib.lib().vmasr_col2im_kx1, g, dx, B * P, H, C, k, stride, pad, _lib.torch_dtype_code(g.dtype))
    return dx


def im2col_kx1_split(xs, geom, C, k, stride, pad, rows, cat3=False):
    """im2col of all fp32 slots in one launch as the bf16 pair (hi, lo), each (n, rows, k*C); cat3: as ONE operand [hi | lo | hi] instead."""
    n, x0 = len(geom), xs[0]
    ptrs, Ns, Hs = _slots(xs, geom)
    if cat3:
        acat = _new(x0, (n, rows, 3 * k * C), _BF16)
        _call(_lib.lib().vmasr_im2col_kx1_split3_multi, ptrs, Ns, Hs, n, acat, C, k, stride, pad, rows)
        return acat
    ch, cl = _new(x0, (n, rows, k * C), _BF16), _new(x0, (n, rows, k * C), _BF16)
    _call(_lib.lib().vmasr_im2col_kx1_split_multi, ptrs, Ns, Hs, n, ch, cl, C, k, stride, pad, rows)
    return ch, cl


def col2im_kx1_multi(dcols, shapes, k, stride, pad, want=None):
    """dcols (n, rows, k*C) -> one dx of shapes[i] = (B, P_i, H_i, C) per slot (None where want[i] is false), one launch."""
    dxs = [_new(dcols, shp) if want is None or want[i] else None for i, shp in enumerate(shapes)]
    ptrs, Ns, Hs = _slots(dxs, geom_of(shapes))
    _call(_lib.lib().vmasr_col2im_kx1_multi, dcols, ptrs, Ns, Hs, len(shapes), shapes[0][3], k, stride, pad, dcols.shape[1],
          _lib.torch_dtype_code(dcols.dtype))
    return dxs


def col2im_kx1_stacked(dcols, geom, shape, k, stride, pad):
    """dcols (n, rows, k*C) -> the STACKED dx of `shape` = (n, rows_in, C), zero rows below each slot's data, one launch."""
    n, rows_in, C = shape
    dx = _new(dcols, shape)
    _, Ns, Hs = _slot_arrays([0] * n, [g[0] for g in geom], [g[1] for g in geom])
    _call(_lib.lib().vmasr_col2im_kx1_stacked, dcols, dx, Ns, Hs, n, C, k, stride, pad, dcols.shape[1], rows_in,
          _lib.torch_dtype_code(dcols.dtype))
    return dx


def stack_rows(gs, Ms, shape, like):
    """Row blocks gs[i] (M_i, width; None = zero block) -> one (n, rows, width) tensor of `shape`, zero rows below each block."""
    full = _new(like, shape)
    gc = [g.contiguous() if g is not None else None for g in gs]      # (copies after `full`: the allocation order the step's graph has)
    ptrs, Ms, _ = _slot_arrays([g.data_ptr() if g is not None else 0 for g in gc], list(Ms))
    _call(_lib.lib().vmasr_stack_rows, ptrs, Ms, len(gs), full, shape[1], shape[2] * like.element_size())
    return full


def split_bf16(x):
    """fp32 tensor -> (hi, lo) bf16 with x = hi + lo up to 2^-17 |x| (vm_asr_amd/csrc/split.hip)."""
    x = x.contiguous()
    hi, lo = _new(x, x.shape, _BF16), _new(x, x.shape, _BF16)
    _call(_lib.lib().vmasr_split_bf16, x, hi, lo, x.numel())
    return hi, lo


def weight_prep_split(w):
    """w (n, N, K) fp32 -> (n, K, 3N) bf16 [hi^T | hi^T | lo^T] in one pass (csrc/split.hip)."""
    n, N, K = w.shape
    wcat = _new(w, (n, K, 3 * N), _BF16)
    _call(_lib.lib().vmasr_weight_prep_split, w, wcat, n, N, K)
    return wcat


def bias_gelu_fwd(pre, bias, nparts=1):
    """y = GELU(pre + bias), pre (n, M, N) fp32, bias (n, N); nparts = 3: pre is (3, n, M, N) partial products, summed in place into pre[0]."""
    n, M, N = pre.shape[-3:]
    y = _new(pre, (n, M, N))
    _call(_lib.lib().vmasr_bias_gelu_fwd, pre, bias, y, n, M, N, nparts)
    return y


def gelu_bwd(pre, gy, db=None, want_db=None):
    """gx = gy * GELU'(pre), all (n, M, N) fp32; the column sums of gx are added to db (n, N) fp32: zeroed by the caller, or (want_db
    given) made here after gx, only wanted if want_db.  -> (gx, db)"""
    gx = torch.empty_like(gy)
    if want_db is not None:
        db, = _lib.zeros_f32(gy.device, (gy.shape[0], gy.shape[2]) if want_db else None)
    _call(_lib.lib().vmasr_gelu_bwd, pre, gy, gx, db, *gy.shape)
    return gx, db


def gelu_bwd_split(pre, gy, db=None, cat=False):
    """The bf16 pair (gh, gl) of gy * GELU'(pre) (pre None: of gy itself) in one pass, the fp32 product is never written; db as in
    gelu_bwd.  cat: the pair as column blocks of ONE (n, M, 3N) operand [gh | gl | gh], returned third (else None)."""
    n, M, N = gy.shape
    gcat = _new(gy, (n, M, 3 * N), _BF16) if cat else None
    gh, gl = (gcat[:, :, :N], gcat[:, :, N:2 * N]) if cat else (_new(gy, (n, M, N), _BF16), _new(gy, (n, M, N), _BF16))
    _call(_lib.lib().vmasr_gelu_bwd_split, pre, gy, None if cat else gh, None if cat else gl, gcat, db, n, M, N)
    return gh, gl, gcat


def sum_parts(parts, nparts, n, S, shape):
    """parts fp32, nparts * n * S blocks of `shape` in that order -> their sum over nparts and S, (n, *shape)."""
    out = _new(parts, (n, *shape))
    _call(_lib.lib().vmasr_sum_parts, parts, out, nparts, n, S, parts.numel() // (nparts * n * S))
    return out


def conv_first_fwd(xs, geom, w, bias, rows):
    """Conv2d(1, 32, (5,1), (3,1), padding 2) + GELU of the folded fp32 signals xs[i] (B, p_i, H_i, 1): -> (pre, act), each (n, rows, 32)."""
    n, (ptrs, Ns, Hs) = len(xs), _slots(xs, geom)
    pre, act = _new(w, (n, rows, 32)), _new(w, (n, rows, 32))
    _call(_lib.lib().vmasr_conv_first_fwd, ptrs, Ns, Hs, n, w, bias, pre, act, rows)
    return pre, act


def conv_first_bwd(xs, geom, w, pre, gy, want_dx, want_dw, want_db):
    """-> (dcols (n, rows, 5) for col2im_kx1_multi, dw (n, 32, 5), db (n, 32)), each None unless wanted."""
    n, rows, _ = pre.shape
    ptrs, Ns, Hs = _slots(xs, geom)
    dcols = _new(pre, (n, rows, 5)) if want_dx else None
    dw, db = _lib.zeros_f32(pre.device, (n, 32, 5) if want_dw else None, (n, 32) if want_db else None)
    _call(_lib.lib().vmasr_conv_first_bwd, ptrs, Ns, Hs, n, w, pre, gy, dcols, dw, db, rows)
    return dcols, dw, db


def conv_post_supported(C, k):
    return bool(_lib.lib().vmasr_conv_post_supported(int(C), int(k)))


def conv_post_fwd(x, w, bias, Ms, Hs):
    """Conv2d(C, 1, (3,1), 1, padding 1) on the stacked fp32 x (n, rows, C); w (n, 1, 3C), bias (n, 1); Ms[i] valid rows of Hs[i]-long sequences."""
    n, rows, C = x.shape
    ms, hs = (ctypes.c_int64 * n)(*Ms), (ctypes.c_int32 * n)(*Hs)
    y = _new(x, (n, rows, 1), _F32)
    _call(_lib.lib().vmasr_conv_post_fwd, x, w, bias, y, ms, hs, n, rows, C, 3)
    return y


def conv_post_bwd(x, w, gy, Ms, Hs, want_dx, want_dw, want_db):
    """-> (dx like x, dw (n, 1, 3C), db (n,)), each None unless wanted."""
    n, rows, C = x.shape
    ms, hs = (ctypes.c_int64 * n)(*Ms), (ctypes.c_int32 * n)(*Hs)
    dx = torch.empty_like(x) if want_dx else None
    dw, db = _lib.zeros_f32(x.device, (n, 1, 3 * C) if want_dw else None, (n,) if want_db else None)
    _call(_lib.lib().vmasr_conv_post_bwd, x, w, gy, dx, dw, db, ms, hs, n, rows, C, 3)
    return dx, dw, db


def conv_post_bwd_gelu(x, w, gy, pre, Ms, Hs, want_pair, want_f32, want_dw, want_db, want_dbcol, sgn=None, gtok=None, valid=None, scale=None):
    """conv_post_bwd with the activation backward of the layer below in it (csrc/convpost.hip): g = (dx + gtok * scale[s] * sgn) * GELU'(pre),
    the sign term (sgn int8, x's shape; gtok one fp32 element) on the rows < valid[s].  -> (g fp32 or None, (gh, gl) bf16 pair or None,
    dbcol (n, C) column sums of g or None, dw (n, 1, 3C) or None, db (n,) or None); dx itself is never written."""
    n, rows, C = x.shape
    ms, hs = (ctypes.c_int64 * n)(*Ms), (ctypes.c_int32 * n)(*Hs)
    v, sc = _valid_scale(valid, scale) if sgn is not None else (None, None)
    g32 = torch.empty_like(x) if want_f32 else None
    gh = _new(x, x.shape, _BF16) if want_pair else None
    gl = _new(x, x.shape, _BF16) if want_pair else None
    dw, db, dbcol = _lib.zeros_f32(x.device, (n, 1, 3 * C) if want_dw else None, (n,) if want_db else None, (n, C) if want_dbcol else None)
    _call(_lib.lib().vmasr_conv_post_bwd_gelu, x if want_dw else None, w, gy, pre, sgn, gtok if sgn is not None else None, v, sc, gh, gl, g32,
          dw, db, dbcol, ms, hs, n, rows, C, 3)
    return g32, ((gh, gl) if want_pair else None), dbcol, dw, db


def conv_mfma_supported_launch(Cin, Cout, k, stride, n, rows):
    return bool(_lib.lib().vmasr_conv_mfma_supported_launch(int(Cin), int(Cout), int(k), int(stride), int(n), int(rows)))


def _valid_scale(valid, scale):
    n = len(valid)
    return (ctypes.c_int64 * n)(*valid), (ctypes.c_float * n)(*scale)


def masked_l1_fwd(real, gen, valid, scale, want_sgn):
    """-> (float64 block partials of sum_s scale[s] * sum_{r < valid[s]} |gen[s, r] - real[s, r]|, sign(gen - real) int8 if want_sgn)."""
    n, rows_g, N = gen.shape
    v, sc = _valid_scale(valid, scale)
    partials = _new(gen, n * _lib.lib().vmasr_masked_l1_blocks(), torch.float64)
    sgn = _new(gen, (n, rows_g, N), torch.int8) if want_sgn else None
    _call(_lib.lib().vmasr_masked_l1_fwd, real, gen, sgn, partials, v, sc, n, real.shape[1], rows_g, N)
    return partials, sgn


def masked_l1_bwd(sgn, g, valid, scale, add=None, tap=False):
    """g * scale[s] * sgn on the valid rows (g: one fp32 element), zero below; tap: the kernel that adds `add` (fp32, sgn's shape, or None) too."""
    v, sc = _valid_scale(valid, scale)
    out = _new(sgn, sgn.shape, _F32)
    if tap:
        _call(_lib.lib().vmasr_masked_l1_bwd_add, sgn, g, add, out, v, sc, *sgn.shape)
    else:
        _call(_lib.lib().vmasr_masked_l1_bwd, sgn, g, out, v, sc, *sgn.shape)
    return out


def sn_stack_fwd(ws, sig, want_pair=False):
    """out[s] = permute(ws[s] / sig[s]): n weights (N, Cin, k, 1) -> one (n, N, k*Cin) operand in (tap, channel) column order.
    want_pair: -> (out, (hi, lo)), its bf16 pair (split_bf16's) written in the same pass."""
    n, (N, Cin, k) = len(ws), ws[0].shape[:3]
    out = _new(ws[0], (n, N, k * Cin), _F32)
    hi, lo = (_new(out, out.shape, _BF16), _new(out, out.shape, _BF16)) if want_pair else (None, None)
    _call(_lib.lib().vmasr_sn_stack_fwd, _ptr_array(ws), _ptr_array(sig), n, out, hi, lo, N, Cin, k)
    return (out, (hi, lo)) if want_pair else out


def weight_transpose_supported(N, Cin):
    return Cin % 4 == 0 and N % 8 == 0


def weight_transpose(w, k, pair):
    """w (n, N, k*Cin) fp32, (tap, channel) columns -> the input gradient's operand (n, Cin, k*N) in (tap, output channel) order, one pass
    (csrc/split.hip): its bf16 pair (hi, lo) if pair, else fp32.  == split_bf16 of / the permute(0, 3, 2, 1) copy of w.view(n, N, k, Cin)."""
    n, N, K = w.shape
    Cin = K // k
    if pair:
        hi, lo = _new(w, (n, Cin, k * N), _BF16), _new(w, (n, Cin, k * N), _BF16)
        _call(_lib.lib().vmasr_weight_transpose, w, hi, lo, None, n, N, Cin, k)
        return hi, lo
    out = _new(w, (n, Cin, k * N), _F32)
    _call(_lib.lib().vmasr_weight_transpose, w, None, None, out, n, N, Cin, k)
    return out


def sn_stack_bwd(dW, out, sig, us, vs, shapes):
    """Gradients of the n original weights (of `shapes`) from dW (n, N, k*Cin): (g - <g, W/sigma> u v^T) / sigma each."""
    n, (N, Cin, k) = len(shapes), shapes[0][:3]
    gws = [_new(dW, shp, _F32) for shp in shapes]
    partials = _new(dW, n * _lib.lib().vmasr_sn_dot_blocks(), torch.float64)
    _call(_lib.lib().vmasr_sn_stack_bwd, dW, out, _ptr_array(gws), _ptr_array(sig), _ptr_array(us), _ptr_array(vs), n,
          partials, N, Cin, k)
    return gws


def spectral_power_iter(w, u, v, n_iter, eps):
    """n_iter power iterations of the fp32 matrix w (R, C), in place on u (R) and v (C)."""
    R, C = w.shape
    ws = _new(w, R + C)
    _call(_lib.lib().vmasr_spectral_power_iter, w, u, v, ws, R, C, int(n_iter), float(eps))


class SpectralBatch:
    """Power iteration of MANY _SpectralNorm modules in one launch per phase (vmasr_spectral_power_iter_batched): the descriptor table
    (pointers to the fp32 weights, u, v and scratch) is built once on the device; the pointers are those of parameters and buffers,
    which live at fixed addresses for the life of the model on its device."""

    def __init__(self, modules, weights):
        import numpy as np
        assert 0 < len(modules) <= 64
        dev = weights[0].device
        self.modules, self.eps = list(modules), float(modules[0].eps)
        mats = [w.detach() for w in weights]
        assert all(w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() for w in mats)
        shapes = [(w.shape[0], w[0].numel()) for w in mats]
        self.ws = torch.zeros(sum(r + c for r, c in shapes), dtype=torch.float32, device=dev)
        item = np.dtype([("W", "u8"), ("u", "u8"), ("v", "u8"), ("t", "u8"), ("s", "u8"), ("R", "i4"), ("C", "i4"), ("rb", "i4"), ("ct", "i4")])
        tab = np.zeros(len(mats), dtype=item)
        off = rb = ct = 0
        for i, (m, w, (r, c)) in enumerate(zip(self.modules, mats, shapes)):
            tab[i] = (w.data_ptr(), m._u.data_ptr(), m._v.data_ptr(), self.ws.data_ptr() + 4 * off,
                      self.ws.data_ptr() + 4 * (off + r), r, c, rb, ct)
            off += r + c
            rb += -(-r // 4)
            ct += -(-c // 1024) * -(-r // 32)
        self.n, self.row_blocks, self.col_tiles = len(mats), rb, ct
        self.weight_bytes = sum(4 * r * c for r, c in shapes)
        self.ptrs = [(w.data_ptr(), m._u.data_ptr(), m._v.data_ptr()) for m, w in zip(self.modules, mats)]
        self.sigma = torch.ones(len(mats), dtype=torch.float32, device=dev)
        self.table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)

    def matches(self, weights):
        return len(weights) == self.n and all(
            (w.data_ptr(), m._u.data_ptr(), m._v.data_ptr()) == p for m, w, p in zip(self.modules, weights, self.ptrs))

    @torch.no_grad()
    def run(self, n_iter, with_sigma=False):
        """n_iter power iterations of every matrix; with_sigma: also sigma_m = u^T W v, handed to the modules
        (`_sigma_pre`, a view of self.sigma) until clear_sigma()."""
        _call(_lib.lib().vmasr_spectral_power_iter_batched, self.table, self.n, self.row_blocks, self.col_tiles, self.weight_bytes,
              int(n_iter), self.eps, self.sigma if with_sigma else None)
        if with_sigma:
            for i, m in enumerate(self.modules):
                object.__setattr__(m, "_sigma_pre", self.sigma[i])

    def clear_sigma(self):
        for m in self.modules:
            object.__setattr__(m, "_sigma_pre", None)
