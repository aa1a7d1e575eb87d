"""The output side of SS2D.forwardv2 as one HIP operator on the matrix cores (vm_asr_amd/csrc/mlp.hip: outproj_kernel):

    fused_out_proj_residual(g, out_proj, x, scale=None)  ==  x + scale * out_proj(g)

i.e. `out = self.out_proj(y)` (model/vmamba.py:1551; no bias, dropout p = 0) followed by the VSSBlock's
`x = input + self.drop_path(...)` (:1826-1827) under bf16 autocast, for g (B, H, W, 2d) bf16 = the gated LayerNorm output of
`ss2d_glue.ln_gate`, the residual stream x (B, H, W, d) in fp32 or bf16 and d in {8, 16, 32, 64}.  Forward: one kernel instead of
GEMM + (DropPath multiply +) add.  Backward: one kernel (dg = scale * gy . W in bf16 for ln_gate's backward, gys = scale * gy as
the operand of the weight gradient) + one split-K GEMM; the stream's own gradient is gy itself.  No CPU fallback.
"""
import torch

from . import _lib, knobs
from .wgrad import weight_grad_finished
from . import layernorm as _ln
from .linear import bf16_shadow, bf16_shadow_t
from .mlp import amp_stream, row_linear

__all__ = ["fused_out_proj_residual", "supported"]


def supported(g, out_proj, x, dropout=None):
    """GPU, bf16 autocast, bf16 gate output, fp32 / bf16 stream, bias-free out_proj of a supported width, no active dropout."""
    if not knobs.get("VMASR_FUSED_OUTPROJ") or not amp_stream(g, x) or g.dtype != torch.bfloat16 or not row_linear(out_proj, False):
        return False
    if dropout is not None and not isinstance(dropout, torch.nn.Identity) and getattr(dropout, "p", 0.0) != 0.0 and dropout.training:
        return False
    d, di = x.shape[-1], g.shape[-1]
    if out_proj.in_features != di or out_proj.out_features != d or g.shape[:-1] != x.shape[:-1]:
        return False
    return bool(_lib.lib().vmasr_outproj_supported(int(d), int(di)))


class _OutProjFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, w, x, scale):
        d, di = x.shape[-1], g.shape[-1]
        g2, x2 = _lib.rows2d(g, di), _lib.rows2d(x, d)
        rows = x2.shape[0]
        wb = bf16_shadow(w).contiguous()
        rps = rows // scale.numel() if scale is not None else 0
        sc = None if scale is None else scale.detach().float().contiguous().view(-1)
        y = torch.empty_like(x2)
        _lib.call(_lib.lib().vmasr_outproj_fwd, g2, wb, x2, sc, rps, y, rows, d, _lib.torch_dtype_code(x2.dtype))
        ctx.save_for_backward(g2, wb, sc)
        ctx.wt = bf16_shadow_t(w, wb)
        ctx.meta = (g.shape, x.shape, x2.dtype, rps, w.dtype)
        if ctx.needs_input_grad[1]:
            _ln.note_use(w)
        ctx.wparam = w
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, gy):
        g2, wb, sc = ctx.saved_tensors
        gshape, xshape, xdt, rps, wdt = ctx.meta
        rows, di = g2.shape
        d = di // 2
        gy2 = gy.reshape(rows, d)
        if gy2.dtype not in (torch.float32, torch.bfloat16):
            gy2 = gy2.float()
        if not gy2.is_contiguous():
            gy2 = gy2.contiguous()
        dev = g2.device
        wt = ctx.wt if ctx.wt is not None else wb.t().contiguous()      # (2d, d)
        dg = torch.empty((rows, di), dtype=torch.bfloat16, device=dev)
        gys = torch.empty((rows, d), dtype=torch.bfloat16, device=dev)
        _lib.call(_lib.lib().vmasr_outproj_bwd, gy2, wt, sc, rps, dg, gys, rows, d, _lib.torch_dtype_code(gy2.dtype))
        dw = None
        if ctx.needs_input_grad[1]:                                          # (d, 2d) fp32; finished with the pass' other weight gradients
            dw, _ = weight_grad_finished(gys, g2, di, ctx.wparam, None, _ln.fresh(ctx.wparam))
        return dg.view(gshape), None if dw is None else dw.to(wdt), gy.to(xdt) if ctx.needs_input_grad[2] else None, None


def fused_out_proj_residual(g, out_proj, x, scale=None):
    """x + scale * out_proj(g); `scale`: None or a per-sample tensor (DropPath keep mask / keep)."""
    _lib.require_cuda("fused_out_proj_residual", x)
    return _OutProjFn.apply(g, out_proj.weight, x, scale)
