"""The Mlp branch of a VSSBlock as one HIP operator on the matrix cores (vm_asr_amd/csrc/mlp.hip):

    fused_mlp_residual(x, norm2, mlp, scale=None)  ==  x + scale * mlp(norm2(x))

i.e. `x + self.drop_path(self.mlp(self.norm2(x)))` of VSSBlock._forward (model/vmamba.py:1832-1837; Mlp :483-509 with
exact-erf GELU; timm DropPath as a per-sample scale) under bf16 autocast, for the residual stream x (..., d) in fp32 or bf16,
d in {8, 16, 32, 64}, hidden = 4 d.  Forward: ONE kernel (LayerNorm, fc1, bias, GELU, fc2, bias, residual; bf16
MFMA 32x32x16, fp32 accumulation; the hidden activations never leave the register file).  Backward: one kernel that
recomputes the forward and produces dxn plus the bf16 operands of the weight-gradient GEMMs, then LayerNorm's backward
(with the residual gradient folded in) and two GEMMs whose ones-column carries the bias gradients.  No CPU fallback.
"""
import torch

from . import _lib, knobs
from . import layernorm as _ln
from .wgrad import weight_grad_finished
from .linear import bf16_shadow, bf16_shadow_t

__all__ = ["fused_mlp_residual", "supported"]


def amp_stream(*streams):
    """GPU tensors in fp32 / bf16 under bf16 autocast (this and the two below: shared with gmlp.py, inproj.py, outproj.py)."""
    return all(t.is_cuda and t.dtype in (torch.float32, torch.bfloat16) for t in streams) and _lib.bf16_autocast()


def row_linear(m, bias):
    """An nn.Linear over the last axis with / without a bias.  (Linear2d / LayerNorm2d act on axis 1: never a row kernel.)"""
    return isinstance(m, torch.nn.Linear) and type(m).__name__ != "Linear2d" and (m.bias is not None) == bias


def row_layernorm(m, d):
    """An affine nn.LayerNorm of width d over the last axis."""
    return (isinstance(m, torch.nn.LayerNorm) and type(m).__name__ != "LayerNorm2d" and tuple(m.normalized_shape) == (d,)
            and m.weight is not None and m.bias is not None)


def mlp_hidden(x, norm, mlp, gated):
    """-> the hidden width if x + mlp(norm(x)) is what the fused Mlp (gated: gMlp, fc1: d -> 2 * hidden) computes, else 0: channel-last
    stream, biased row Linears, exact GELU, no active dropout.  Knob and width rule are the callers'."""
    d, fc1, fc2 = x.shape[-1], getattr(mlp, "fc1", None), getattr(mlp, "fc2", None)
    if not (amp_stream(x) and row_linear(fc1, True) and row_linear(fc2, True) and row_layernorm(norm, d)):
        return 0
    if getattr(mlp, "channel_first", False) or not isinstance(mlp.act, torch.nn.GELU) or getattr(mlp.act, "approximate", "none") != "none":
        return 0
    if (mlp.drop.p != 0.0 and mlp.training) or fc1.in_features != d or fc2.out_features != d:
        return 0
    return fc2.in_features if fc1.out_features == (2 if gated else 1) * fc2.in_features else 0


def supported(x, norm, mlp):
    hidden = knobs.get("VMASR_FUSED_MLP") and mlp_hidden(x, norm, mlp, False)
    return bool(hidden and _lib.lib().vmasr_mlp_supported(int(x.shape[-1]), int(hidden)))


class _FusedMlpFn(torch.autograd.Function):
    """entry: "vmasr_mlp", or "vmasr_gmlp" for the gated form (gmlp.py: fc1 has 2 * hidden rows, the kernels' argument lists are
    the same) — the shapes below are read off the weights, so one function serves both."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w1, b1, w2, b2, scale, eps, entry="vmasr_mlp"):
        d = x.shape[-1]
        x2 = _lib.rows2d(x, d)
        rows = x2.shape[0]
        g32, be32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        b1f, b2f = b1.detach().float().contiguous(), b2.detach().float().contiguous()
        w1b, w2b = bf16_shadow(w1).contiguous(), bf16_shadow(w2).contiguous()
        rps = rows // scale.numel() if scale is not None else 0
        sc = None if scale is None else scale.detach().float().contiguous().view(-1)
        y = torch.empty_like(x2)
        _lib.call(getattr(_lib.lib(), entry + "_fwd"), x2, g32, be32, float(eps), w1b, b1f, w2b, b2f, sc, rps, y, rows, d, _lib.torch_dtype_code(x2.dtype))
        ctx.save_for_backward(x2, g32, be32, w1b, b1f, w2b, sc)
        ctx.wts = (bf16_shadow_t(w1, w1b), bf16_shadow_t(w2, w2b))
        ctx.meta = (x.shape, eps, rps, gamma.dtype, beta.dtype, w1.dtype, b1.dtype, w2.dtype, b2.dtype)
        ctx.entry = entry
        if any(ctx.needs_input_grad[1:3]):
            _ln.note_use(gamma, beta)
        ctx.fresh = lambda: gamma.grad is None and beta.grad is None and _ln.used_once(gamma, beta)
        ctx.params = (gamma, beta)
        if any(ctx.needs_input_grad[3:7]):
            _ln.note_use(w1, b1, w2, b2)
        ctx.wparams = (w1, b1, w2, b2)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, gy):
        x2, g32, be32, w1b, b1f, w2b, sc = ctx.saved_tensors
        shape, eps, rps, gdt, bedt, w1dt, b1dt, w2dt, b2dt = ctx.meta
        rows, d = x2.shape
        hd, h1 = w2b.shape[1], w1b.shape[0]             # hidden; fc1's rows (hidden, gated: 2 * hidden)
        gy2 = gy.reshape(rows, d).to(x2.dtype)
        if not gy2.is_contiguous():
            gy2 = gy2.contiguous()
        lib = _lib.lib()
        dev = x2.device
        bf = dict(dtype=torch.bfloat16, device=dev)
        w1t = ctx.wts[0] if ctx.wts[0] is not None else w1b.t().contiguous()
        w2t = ctx.wts[1] if ctx.wts[1] is not None else w2b.t().contiguous()
        dxn = torch.empty((rows, d), **bf)
        xn_aug = torch.empty((rows, d + 8), **bf)
        gys = torch.empty((rows, d), **bf)
        act_aug = torch.empty((rows, hd + 8), **bf)
        gpre = torch.empty((rows, h1), **bf)
        stats = torch.empty((2, rows), dtype=torch.float32, device=dev)
        _lib.call(getattr(lib, ctx.entry + "_bwd"), x2, gy2, g32, be32, float(eps), w1b, w1t, b1f, w2t, sc, rps, dxn, xn_aug, gys, act_aug, gpre,
                  stats[0], stats[1], rows, d, _lib.torch_dtype_code(x2.dtype))
        # dx = gy + LayerNorm'(dxn); dgamma, dbeta  (one launch: csrc/ln.hip with the residual gradient folded in)
        dx = torch.empty_like(x2)
        dg_ = torch.empty(d, dtype=torch.float32, device=dev)      # separate tensors: autograd adopts each as a .grad
        db_ = torch.empty(d, dtype=torch.float32, device=dev)
        ws = torch.empty(lib.vmasr_layer_norm_bwd_workspace(rows, d) // 4, dtype=torch.float32, device=dev)
        later = (gdt == torch.float32 and bedt == torch.float32 and ctx.fresh() and _ln.defer_reduction(ws, dg_, db_, rows, d, *ctx.params))
        _lib.call(lib.vmasr_layer_norm_bwd_res, x2, dxn, g32, stats[0], stats[1], gy2, dx, dg_ if not later else None,
                  db_ if not later else None, ws, rows, d, _lib.torch_dtype_code(x2.dtype), _lib.BF16)
        # [dW1 | db1 | 0] = gpre^T xn_aug,  [dW2 | db2 | 0] = gys^T act_aug  (fp32 accumulation, split over the rows when few tiles);
        # the sum over the slabs and the split into contiguous dW / db: one launch for ALL queued GEMMs of the pass (wgrad.py)
        fresh_w = _ln.fresh(*ctx.wparams)
        dw1, db1 = weight_grad_finished(gpre, xn_aug, d, ctx.wparams[0], ctx.wparams[1], fresh_w)
        dw2, db2 = weight_grad_finished(gys, act_aug, hd, ctx.wparams[2], ctx.wparams[3], fresh_w)
        return (dx.view(shape), dg_.to(gdt), db_.to(bedt), dw1.to(w1dt), db1.to(b1dt), dw2.to(w2dt), db2.to(b2dt), None, None, None)


def fused_mlp_residual(x, norm, mlp, scale=None):
    """x + scale * mlp(norm(x)); `scale`: None or a (B,) / (B,1,1,1) per-sample tensor (DropPath keep mask / keep)."""
    _lib.require_cuda("fused_mlp_residual", x)
    return _FusedMlpFn.apply(x, norm.weight, norm.bias, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias, scale, norm.eps)
