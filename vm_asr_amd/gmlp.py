"""The gated Mlp branch of a VSSBlock (MODEL.VSSM.GMLP) as one HIP operator on the matrix cores (vm_asr_amd/csrc/mlp.hip, GATED):

    fused_gmlp_residual(x, norm2, mlp, scale=None)  ==  x + scale * mlp(norm2(x))

with mlp = gMlp (model/vmamba.py:512-538): u, z = fc1(xn).chunk(2, -1); fc2(u * GELU(z)) — the branch VSSBlock._forward runs when
the block was built with gmlp=True (:1815, :1832-1837), under bf16 autocast, for the residual stream x (..., d) in fp32 or bf16,
d in {8, 16, 32, 64}, hidden = 4 d (fc1: d -> 8 d).  Forward: ONE kernel; backward: one kernel that recomputes the forward and
writes dxn plus the bf16 operands of the weight-gradient GEMMs (gpre = [du | dz] with 8 d columns), then LayerNorm's backward and
the two GEMMs — the autograd function is mlp.py's, with the gated entry points: same bf16 shadows and transposed shadows, same
deferred LayerNorm / weight-gradient reductions.  No CPU fallback.
"""
from . import _lib, knobs
from .mlp import _FusedMlpFn, mlp_hidden

__all__ = ["fused_gmlp_residual", "supported"]


def supported(x, norm, mlp):
    hidden = knobs.get("VMASR_FUSED_GMLP") and mlp_hidden(x, norm, mlp, True)
    return bool(hidden and _lib.lib().vmasr_gmlp_supported(int(x.shape[-1]), int(hidden)))


def fused_gmlp_residual(x, norm, mlp, scale=None):
    """x + scale * mlp(norm(x)) for a gMlp; `scale`: None or a (B,) / (B,1,1,1) per-sample tensor (DropPath keep mask / keep)."""
    _lib.require_cuda("fused_gmlp_residual", x)
    return _FusedMlpFn.apply(x, norm.weight, norm.bias, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias, scale, norm.eps,
                             "vmasr_gmlp")
