"""The input side of SS2D.forwardv2 as one HIP operator on the matrix cores (vm_asr_amd/csrc/mlp.hip: inproj_kernel):

    fused_in_proj(x, norm, in_proj) -> (xT (B, 2d, H, W), sz (B, H, W, 2d))
        == xz = in_proj(norm(x)); x', z = xz.chunk(2, -1); xT = x'.permute(0, 3, 1, 2).contiguous(); sz = SiLU(z)
           (model/vmamba.py:1826-1827 pre-norm of VSSBlock, :1535-1542 of SS2D.forwardv2)

under bf16 autocast, for the fp32 / bf16 residual stream x (B, H, W, d), d in {8, 16, 32, 64}, in_proj without bias, H*W a
multiple of 32; `norm` a LayerNorm or nn.Identity.  One launch instead of LayerNorm + GEMM + ss2d_pre; backward = one kernel
(recompute) + LayerNorm's backward + one weight-gradient GEMM.  No CPU fallback.
"""
import torch

from . import _lib, knobs
from . import layernorm as _ln
from .wgrad import weight_grad_finished
from .linear import bf16_shadow, bf16_shadow_t
from .mlp import amp_stream, row_layernorm, row_linear

__all__ = ["fused_in_proj", "supported"]


def supported(x, norm, in_proj):
    if not knobs.get("VMASR_FUSED_INPROJ") or x.dim() != 4 or not amp_stream(x) or not row_linear(in_proj, False):
        return False
    d = x.shape[-1]
    if not (row_layernorm(norm, d) or isinstance(norm, torch.nn.Identity)) or in_proj.in_features != d:
        return False
    return bool(_lib.lib().vmasr_inproj_supported(int(d), int(in_proj.out_features), int(x.shape[1] * x.shape[2])))


class _InProjFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, weight, eps):
        B, H, W, d = x.shape
        L = H * W
        x2 = _lib.rows2d(x, d)
        g32 = None if gamma is None else gamma.detach().float().contiguous()
        b32 = None if beta is None else beta.detach().float().contiguous()
        wb = bf16_shadow(weight).contiguous()
        xT = torch.empty((B, 2 * d, H, W), dtype=torch.bfloat16, device=x.device)
        sz = torch.empty((B, H, W, 2 * d), dtype=torch.bfloat16, device=x.device)
        _lib.call(_lib.lib().vmasr_inproj_fwd, x2, g32, b32, float(eps), wb, xT, sz, B * L, L, d, _lib.torch_dtype_code(x2.dtype))
        ctx.save_for_backward(x2, g32 if g32 is not None else torch.empty(0, device=x.device),
                              b32 if b32 is not None else torch.empty(0, device=x.device), wb)
        ctx.meta = (x.shape, eps, gamma is not None, None if gamma is None else gamma.dtype, None if beta is None else beta.dtype, weight.dtype)
        ctx.wt = bf16_shadow_t(weight, wb)
        if gamma is not None and any(ctx.needs_input_grad[1:3]):
            _ln.note_use(gamma, beta)
        ctx.fresh = lambda: gamma is not None and gamma.grad is None and beta.grad is None and _ln.used_once(gamma, beta)
        ctx.params = (gamma, beta)
        if ctx.needs_input_grad[3]:
            _ln.note_use(weight)
        ctx.wparam = weight
        return xT, sz

    @staticmethod
    def backward(ctx, dxT, dsz):
        x2, g32, b32, wb = ctx.saved_tensors
        shape, eps, has_norm, gdt, bedt, wdt = ctx.meta
        B, H, W, d = shape
        L, rows = H * W, x2.shape[0]
        dev = x2.device
        bf = dict(dtype=torch.bfloat16, device=dev)
        lib = _lib.lib()
        dxT = (torch.zeros((B, 2 * d, H, W), **bf) if dxT is None else dxT.to(torch.bfloat16)).contiguous()
        dsz = (torch.zeros((B, H, W, 2 * d), **bf) if dsz is None else dsz.to(torch.bfloat16)).contiguous()
        wt = ctx.wt if ctx.wt is not None else wb.t().contiguous()
        dxn = torch.empty((rows, d), **bf)
        xn = torch.empty((rows, d), **bf)
        gpre = torch.empty((rows, 4 * d), **bf)
        stats = torch.empty((2, rows), dtype=torch.float32, device=dev) if has_norm else None
        _lib.call(lib.vmasr_inproj_bwd, x2, g32 if has_norm else None, b32 if has_norm else None, float(eps), wb, wt, dxT, dsz, dxn, xn, gpre,
                  stats[0] if has_norm else None, stats[1] if has_norm else None, rows, L, d, _lib.torch_dtype_code(x2.dtype))
        dg = db = None
        if has_norm:
            dx = torch.empty_like(x2)
            dg = torch.empty(d, dtype=torch.float32, device=dev)
            db = torch.empty(d, dtype=torch.float32, device=dev)
            ws = torch.empty(lib.vmasr_layer_norm_bwd_workspace(rows, d) // 4, dtype=torch.float32, device=dev)
            later = (gdt == torch.float32 and bedt == torch.float32 and ctx.fresh() and _ln.defer_reduction(ws, dg, db, rows, d, *ctx.params))
            _lib.call(lib.vmasr_layer_norm_bwd, x2, dxn, g32, stats[0], stats[1], dx, dg if not later else None, db if not later else None, ws,
                      rows, d, _lib.torch_dtype_code(x2.dtype), _lib.BF16)
            dg, db = dg.to(gdt), db.to(bedt)
        else:
            dx = dxn.to(x2.dtype)
        # (4d, d) fp32, split over the rows when few tiles; finished together with the pass' other weight gradients (wgrad.py)
        dw, _ = weight_grad_finished(gpre, xn, d, ctx.wparam, None, _ln.fresh(ctx.wparam))
        return dx.view(shape), dg, db, dw.to(wdt), None


def fused_in_proj(x, norm, in_proj):
    _lib.require_cuda("fused_in_proj", x)
    ln = isinstance(norm, torch.nn.LayerNorm)
    return _InProjFn.apply(x, norm.weight if ln else None, norm.bias if ln else None, in_proj.weight, norm.eps if ln else 0.0)
