"""The gated Mlp branch of a VSSBlock (MODEL.VSSM.GMLP) as one HIP operator on the matrix cores (vm_asr_amd/csrc/gmlp.hip):

    fused_gmlp_residual(x, norm2, mlp, scale=None)  ==  x + scale * mlp(norm2(x))

with mlp = gMlp (model/vmamba.py:512-538): u, z = fc1(xn).chunk(2, -1); fc2(u * GELU(z)) — the branch VSSBlock._forward runs when
the block was built with gmlp=True (:1815, :1832-1837), under bf16 autocast, for the residual stream x (..., d) in fp32 or bf16,
d in {8, 16, 32, 64}, hidden = 4 d (fc1: d -> 8 d).  Forward: ONE kernel; backward: one kernel that recomputes the forward and
writes dxn plus the bf16 operands of the weight-gradient GEMMs (gpre = [du | dz] with 8 d columns), then LayerNorm's backward and
the two GEMMs — the autograd function is mlp.py's, with the gated entry points: same bf16 shadows and transposed shadows, same
deferred LayerNorm / weight-gradient reductions.  No CPU fallback.
"""
import torch

from . import _lib, knobs
from .mlp import _FusedMlpFn

__all__ = ["fused_gmlp_residual", "supported"]


def supported(x, norm, mlp):
    """GPU, bf16 autocast, fp32 or bf16 channel-last stream, a gMlp (fc1: d -> 2 * hidden, exact GELU, no active dropout) of a
    supported width.  (The channel-first form — Linear2d / LayerNorm2d, chunk on axis 1 — is never the row kernel.)"""
    if not knobs.get("VMASR_FUSED_GMLP") or not x.is_cuda or x.dtype not in (torch.float32, torch.bfloat16):
        return False
    if not _lib.bf16_autocast():
        return False
    fc1, fc2 = getattr(mlp, "fc1", None), getattr(mlp, "fc2", None)
    if not (isinstance(fc1, torch.nn.Linear) and isinstance(fc2, torch.nn.Linear) and isinstance(norm, torch.nn.LayerNorm)
            and all(type(m).__name__ not in ("Linear2d", "LayerNorm2d") for m in (fc1, fc2, norm))):
        return False
    if getattr(mlp, "channel_first", False) or not isinstance(mlp.act, torch.nn.GELU) or getattr(mlp.act, "approximate", "none") != "none":
        return False
    if (mlp.drop.p != 0.0 and mlp.training) or fc1.bias is None or fc2.bias is None or norm.weight is None or norm.bias is None:
        return False
    d = x.shape[-1]
    if tuple(norm.normalized_shape) != (d,) or fc1.in_features != d or fc2.out_features != d or fc1.out_features != 2 * fc2.in_features:
        return False
    return bool(_lib.lib().vmasr_gmlp_supported(int(d), int(fc2.in_features)))


def fused_gmlp_residual(x, norm, mlp, scale=None):
    """x + scale * mlp(norm(x)) for a gMlp; `scale`: None or a (B,) / (B,1,1,1) per-sample tensor (DropPath keep mask / keep)."""
    _lib.require_cuda("fused_gmlp_residual", x)
    return _FusedMlpFn.apply(x, norm.weight, norm.bias, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias, scale, norm.eps,
                             "vmasr_gmlp")
