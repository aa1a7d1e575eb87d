"""Multi-scale discriminator: the second adversary the reference can build from TRAIN.ADVERSARIAL.DISCRIMINATORS.

Re-statement of model/discriminator.py:174-313 (HiFi-GAN style: three ScaleDiscriminators, the second and third behind a cumulative
AvgPool1d(4, 2, padding=2); hidden 128).  As for the MPD, the reference's inverted ternary (`weight_norm if use_spectral_norm else
spectral_norm`, :177) means the default `use_spectral_norm=False` yields SPECTRAL norm; that is reproduced, so state_dicts
(`discriminators.{i}.convs.{j}.parametrizations.weight.original`, `....parametrizations.weight.0._u/_v`, `....bias`,
`discriminators.{i}.conv_post....`) load strict=True in both directions.

How it runs:

  * CPU tensors: plain torch (F.conv1d + F.gelu), like the MPD.
  * GPU: the five strided grouped convolutions (k 41, stride 4, pad 20, groups 4 / 16) run on csrc/gconv1d.hip — exact-fp32 MFMA
    forward with bias + GELU in the epilogue, input gradient by stride residue classes, weight gradient as split-K partials with an
    ordered sum (bit-identical from run to run).  The stem (1 -> h, k 15, stride 1: the one layer at the waveform rate, the largest
    map of the module) runs on csrc/stem1d.hip: convolution + bias + GELU in one pass that writes y only; its backward rebuilds the
    pre-activation in registers from x, w and bias, so nothing of the map's size is kept for it, and its dw / db are ordered sums too.
    The dense tail (8h -> 8h k 5 + GELU, conv_post 8h -> 1 k 3) has HIP kernels too, csrc/dconv1d.hip, selected by
    VMASR_MSD_TAIL=hip (the default is torch: the library's convolution is faster on the 8h -> 8h layer, profiles/msd_tail.md): the
    same exact-fp32 MFMA arithmetic on stride-1 windows, the summed channels cut into slabs whose partials are added in slab order (the maps are too short for output
    tiles alone to fill the device), the input gradient as the same GEMM on reversed taps, GELU' formed while the gradient is staged:
    bit-identical from run to run like the other layers, and no library algorithm search in the module.  The pools are ATen operators.
    VMASR_MSD_CONV=torch routes every layer through F.conv1d (A/B measurements; and what discriminator.plain_torch_ops selects: the
    HIP functions are differentiable once); VMASR_MSD_STEM=torch does that for the stem alone; VMASR_MSD_TAIL [torch] | hip selects
    the dense tail's route alone.
  * The generator's pass, forward_generator(x, f_real) -> (scores, feature-matching loss), forms the loss on the way on the GPU
    (msd_featmatch.py: the stem's share inside the stem kernels, the other maps in the one-pass L1 kernel); VMASR_MSD_FEAT=torch,
    CPU tensors and plain_torch_ops run forward_single and the reference's loop.
  * The module computes in fp32 with autocast disabled, so amp_scope="step" leaves the MSD in fp32.
  * Spectral norm follows the reference's schedule exactly: one power iteration per training forward of a ScaleDiscriminator, the
    weight normalised anew in every pass (the layers read their parametrization directly, so an enclosing
    torch.nn.utils.parametrize.cached() — the MPD's once-per-step weights — does not freeze them).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils import parametrize
from torch.nn.utils.parametrizations import weight_norm

from . import knobs, msd_ops as bind
from .discriminator import _PLAIN_OPS, _SpectralNorm, spectral_norm

__all__ = ["ScaleDiscriminator", "MultiScaleDiscriminator", "grouped_conv1d", "stem_conv1d", "dense_conv1d"]


class _GConv1dFn(torch.autograd.Function):
    """y = [GELU](conv1d(x, w, bias, stride, pad, groups)) on the HIP kernels; saves x, w and the pre-activation."""

    @staticmethod
    def forward(ctx, x, w, bias, groups, stride, pad, act):
        x, w = x.contiguous(), w.contiguous()
        y, pre = bind.gconv1d_fwd(x, w, None if bias is None else bias.contiguous(), groups, stride, pad, act)
        ctx.save_for_backward(x, w, pre)
        ctx.geom = (groups, stride, pad, bias is not None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, w, pre = ctx.saved_tensors
        groups, stride, pad, has_bias = ctx.geom
        gy = gy.contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2]
        dx = bind.gconv1d_dgrad(gy, pre, w, x.shape, groups, stride, pad) if need_x else None
        dw, db = bind.gconv1d_wgrad(x, gy, pre, w.shape, groups, stride, pad, need_w, need_b)
        return dx, dw, db, None, None, None, None


class _Stem1dFn(torch.autograd.Function):
    """y = [GELU](conv1d(x, w, bias, 1, pad)) for one input channel on csrc/stem1d.hip; saves x, w and bias: nothing of y's size."""

    @staticmethod
    def forward(ctx, x, w, bias, pad, act):
        x, w = x.contiguous(), w.contiguous()
        bias = None if bias is None else bias.contiguous()
        ctx.save_for_backward(x, w, bias)
        ctx.geom = (pad, act)
        return bind.stem1d_fwd(x, w, bias, pad, act)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, w, bias = ctx.saved_tensors
        pad, act = ctx.geom
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], bias is not None and ctx.needs_input_grad[2]
        dx, dw, db = bind.stem1d_bwd(gy.contiguous(), x, w, bias, pad, act, need_x, need_w, need_b)
        return dx, dw, db, None, None


class _DConv1dFn(torch.autograd.Function):
    """y = [GELU](conv1d(x, w, bias, 1, pad)) of a dense layer on csrc/dconv1d.hip; saves x, w and the pre-activation."""

    @staticmethod
    def forward(ctx, x, w, bias, pad, act):
        x, w = x.contiguous(), w.contiguous()
        y, pre = bind.dconv1d_fwd(x, w, None if bias is None else bias.contiguous(), 1, pad, act)
        ctx.save_for_backward(x, w, pre)
        ctx.geom = (pad, bias is not None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, w, pre = ctx.saved_tensors
        pad, has_bias = ctx.geom
        gy = gy.contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2]
        dx = bind.dconv1d_dgrad(gy, pre, w, x.shape, 1, pad) if need_x else None
        dw, db = bind.dconv1d_wgrad(x, gy, pre, w.shape, 1, pad, need_w, need_b)
        return dx, dw, db, None, None


def _stem_ok(x, w, bias, stride, pad):
    if not x.is_cuda or _PLAIN_OPS[0] or knobs.get("VMASR_MSD_CONV") != "hip" or knobs.get("VMASR_MSD_STEM") != "hip":
        return False
    if any(t.dtype != torch.float32 or not t.is_cuda for t in (x, w) + (() if bias is None else (bias,))):
        return False
    if x.dim() != 3 or w.dim() != 3 or x.shape[1] != 1 or w.shape[1] != 1:
        return False
    return bind.stem1d_supported_launch(w.shape[0], w.shape[2], stride, pad, x.shape[0], x.shape[2])


def stem_conv1d(x, w, bias, stride, pad, act):
    """[GELU](F.conv1d(x, w, bias, stride, pad)) of a one-channel x: the fused HIP pass where vmasr_stem1d_supported_launch accepts the
    call (fp32 on the GPU, VMASR_MSD_CONV=hip, VMASR_MSD_STEM=hip, plain_torch_ops off), torch's operators otherwise."""
    if _stem_ok(x, w, bias, stride, pad):
        return _Stem1dFn.apply(x, w, bias, pad, act)
    y = F.conv1d(x, w, bias, stride, pad)
    return F.gelu(y) if act else y


def _hip_ok(x, w, groups, stride, pad):
    if not x.is_cuda or _PLAIN_OPS[0] or knobs.get("VMASR_MSD_CONV") != "hip":
        return False
    if x.dtype != torch.float32 or w.dtype != torch.float32 or x.dim() != 3 or w.dim() != 3:
        return False
    if x.shape[1] % max(groups, 1) or w.shape[0] % max(groups, 1) or w.shape[1] * groups != x.shape[1]:
        return False
    return bind.gconv1d_supported_launch(x.shape[1], w.shape[0], groups, w.shape[2], stride, pad, x.shape[0], x.shape[2])


def grouped_conv1d(x, w, bias, groups, stride, pad, act):
    """[GELU](F.conv1d(x, w, bias, stride, pad, 1, groups)): the HIP kernels where vmasr_gconv1d_supported_launch accepts the call
    (fp32 on the GPU, VMASR_MSD_CONV=hip), torch's operators otherwise."""
    if _hip_ok(x, w, groups, stride, pad):
        return _GConv1dFn.apply(x, w, bias, groups, stride, pad, act)
    y = F.conv1d(x, w, bias, stride, pad, 1, groups)
    return F.gelu(y) if act else y


def _dense_ok(x, w, bias, stride, pad):
    if not x.is_cuda or _PLAIN_OPS[0] or knobs.get("VMASR_MSD_CONV") != "hip" or knobs.get("VMASR_MSD_TAIL") != "hip":
        return False
    if any(t.dtype != torch.float32 or not t.is_cuda for t in (x, w) + (() if bias is None else (bias,))):
        return False
    if x.dim() != 3 or w.dim() != 3 or w.shape[1] != x.shape[1]:
        return False
    return bind.dconv1d_supported_launch(x.shape[1], w.shape[0], 1, w.shape[2], stride, pad, x.shape[0], x.shape[2])


def dense_conv1d(x, w, bias, stride, pad, act):
    """[GELU](F.conv1d(x, w, bias, stride, pad)) of a dense (groups 1) layer: the HIP kernels where vmasr_dconv1d_supported_launch accepts
    the call (stride 1, k <= 8; fp32 on the GPU, VMASR_MSD_CONV=hip, VMASR_MSD_TAIL=hip, plain_torch_ops off), torch's operators
    otherwise."""
    if _dense_ok(x, w, bias, stride, pad):
        return _DConv1dFn.apply(x, w, bias, pad, act)
    y = F.conv1d(x, w, bias, stride, pad)
    return F.gelu(y) if act else y


def _weight(layer):
    """The layer's (normalised) weight, evaluated now: one power iteration in training mode, as every reference forward does."""
    if parametrize.is_parametrized(layer, "weight"):
        return layer.parametrizations.weight()
    return layer.weight


def is_stem(layer):
    return layer.groups == 1 and layer.in_channels == 1 and layer.stride[0] == 1


def conv_layer(x, layer, w, b, act):
    """One layer of a ScaleDiscriminator with the weight and bias given: the grouped kernels, the stem, or the dense kernels."""
    if layer.groups > 1:
        return grouped_conv1d(x, w, b, layer.groups, layer.stride[0], layer.padding[0], act)
    if is_stem(layer):
        return stem_conv1d(x, w, b, 1, layer.padding[0], act)
    return dense_conv1d(x, w, b, layer.stride[0], layer.padding[0], act)


class ScaleDiscriminator(nn.Module):
    def __init__(self, use_spectral_norm=False, hidden=128):
        super().__init__()
        norm = weight_norm if use_spectral_norm else spectral_norm  # sic
        h = hidden
        self.convs = nn.ModuleList([
            norm(nn.Conv1d(1, h, 15, 1, padding=7)),
            norm(nn.Conv1d(h, h, 41, 4, groups=4, padding=20)),
            norm(nn.Conv1d(h, h * 2, 41, 4, groups=16, padding=20)),
            norm(nn.Conv1d(h * 2, h * 4, 41, 4, groups=16, padding=20)),
            norm(nn.Conv1d(h * 4, h * 8, 41, 4, groups=16, padding=20)),
            norm(nn.Conv1d(h * 8, h * 8, 41, 4, groups=16, padding=20)),
            norm(nn.Conv1d(h * 8, h * 8, 5, 1, padding=2)),
        ])
        self.conv_post = norm(nn.Conv1d(h * 8, 1, 3, 1, padding=1))

    def forward(self, x, detach_weights=False):
        """-> (score (B, T'), the eight feature maps).  `detach_weights`: the weights as constants — the generator's pass through
        the discriminator, where no discriminator gradient is wanted."""
        fmap = []
        with torch.autocast(device_type=x.device.type, enabled=False):
            if x.dtype in (torch.float16, torch.bfloat16):
                x = x.float()
            for layer in list(self.convs) + [self.conv_post]:
                w, b = _weight(layer), layer.bias
                if detach_weights:
                    w, b = w.detach(), b.detach()
                x = conv_layer(x, layer, w, b, layer is not self.conv_post)
                fmap.append(x)
        return torch.flatten(x, 1, -1), fmap


class MultiScaleDiscriminator(nn.Module):
    def __init__(self, hidden=128):
        super().__init__()
        self.discriminators = nn.ModuleList([ScaleDiscriminator(hidden=hidden) for _ in range(3)])
        self.meanpools = nn.ModuleList([nn.AvgPool1d(4, 2, padding=2), nn.AvgPool1d(4, 2, padding=2)])

    def _scales(self, x):
        """x at the three scales: itself, pooled once, pooled twice."""
        xs = [x]
        for pool in self.meanpools:
            xs.append(pool(xs[-1]))
        return xs

    def forward(self, y, y_hat):
        """The reference's call: every scale on the real, then on the generated signal (two power iterations per weight in
        training mode).  y_hat None: zeros in the generated lists."""
        y_real, y_gen, fmap_real, fmap_gen = [], [], [], []
        ys = self._scales(y)
        hs = self._scales(y_hat) if y_hat is not None else [None] * len(ys)
        for disc, a, b in zip(self.discriminators, ys, hs):
            r, fr = disc(a)
            y_real.append(r)
            fmap_real.append(fr)
            if b is not None:
                g, fg = disc(b)
                y_gen.append(g)
                fmap_gen.append(fg)
            else:
                y_gen.append(0)
                fmap_gen.append(0)
        return y_real, y_gen, fmap_real, fmap_gen

    def forward_single(self, x, detach_weights=False):
        """Scores and feature maps of ONE signal batch (the generator's pass: detach_weights=True uses the weights as constants)."""
        res = [d(a, detach_weights) for d, a in zip(self.discriminators, self._scales(x))]
        return [r[0] for r in res], [r[1] for r in res]

    def forward_generator(self, x, f_real):
        """The generator's pass: -> (scores of x, the feature-matching loss against the real signal's maps f_real), the weights as
        constants, the same _weight calls in the same order as forward_single (one power iteration per weight in training mode).
        On the GPU the loss is formed on the way (msd_featmatch: the stem's share inside the stem kernels, the other maps in the
        one-pass L1 kernel); CPU tensors, plain_torch_ops and VMASR_MSD_FEAT=torch run forward_single and the reference's loop."""
        from . import msd_featmatch as fm          # (it imports this module)
        if fm.fused_ok(x):
            return fm.feature_matching(f_real, self._scales(x), self.discriminators)
        scores, fmaps = self.forward_single(x, detach_weights=True)
        return scores, fm.composed_feature_loss(f_real, fmaps)

    def forward_pair(self, y, y_hat):
        """Same results as forward(y, y_hat) from ONE pass over the stacked batch [y; y_hat] (same weights, identical per-sample
        arithmetic; ONE power iteration per weight instead of two)."""
        n = y.shape[0]
        scores, feats = self.forward_single(torch.cat((y, y_hat), dim=0))
        return ([s[:n] for s in scores], [s[n:] for s in scores],
                [[t[:n] for t in f] for f in feats], [[t[n:] for t in f] for f in feats])

    def spectral_norms(self):
        return [m for m in self.modules() if isinstance(m, _SpectralNorm)]
