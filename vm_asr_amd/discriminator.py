"""Multi-period discriminator: the adversary of the MPD configs.

Re-statement of model/discriminator.py:21-147 (HiFi-GAN style, periods 2,3,5,7,11, hidden 32
-> 41.09 M parameters).  The reference's inverted ternary (`weight_norm if use_spectral_norm
else spectral_norm`, :37) means the default `use_spectral_norm=False` yields SPECTRAL norm;
that is reproduced so state_dicts (parametrizations.weight.original + power-iteration
buffers) stay compatible.  The multi-scale discriminator (:174-337) is vm_asr_amd/msd.py.

How it runs on the GPU (MIOpen has only `naive_conv_*` fallbacks for these (k,1) convolutions):

  * signals folded to channel-last sequences (B, period, T/period, C); every convolution is
    `vmasr_im2col_kx1` (HIP gather) + a hipBLASLt GEMM + `vmasr_col2im_kx1` in the backward;
  * the five period discriminators run layer by layer on stacked operands — one batched GEMM per
    layer (`_forward_batched`); the one-by-one path (`PeriodDiscriminator.forward`) is the same
    arithmetic and is what `forward(y, y_hat)` (the reference's call) and the CPU use;
  * spectral norm: power iteration and sigma for all 30 weights in one launch per phase
    (`SpectralBatch` -> `vmasr_spectral_power_iter_batched`), W / sigma as one autograd function;
  * `_ConvKx1Fn` (GEMMs on shifted views, no im2col) is an exact alternative kept opt-in
    (`VMASR_MPD_CONV=gemm`): measured slower than im2col + one GEMM.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils import parametrize
from torch.nn.utils.parametrizations import weight_norm

from . import _lib, knobs, mpd_ops as bind
from .linear import linear as _linear, weight_grad as _weight_grad
from .mpd_featloss import StackedFeatures, _FeatTapFn, _MaskedL1Fn, _masked_l1_ok, feature_loss_stacked  # noqa: F401
from .mpd_layers import (_BatchedLinearFn, _BatchedLinearSplitFn, _StackedConvFirstFn, _StackedConvMfmaFn, _StackedConvPostFn,  # noqa: F401
                         _StackedConvSplitFn, _StackedIm2ColFn, _UnstackRowsFn, _bmm3, _dw3, _l1_mode, _poison, _round_up, _split_k,
                         _split_mode, scores_only, skip_weight_grads)
from .mpd_link import _Link, _Tap
from .mpd_ops import SpectralBatch, _slot_arrays, geom_of as _geom, split_bf16  # noqa: F401  (tests and tools import them from here)

__all__ = ["PeriodDiscriminator", "MultiPeriodDiscriminator", "spectral_norm", "plain_torch_ops"]

_PLAIN_OPS = [False]


class plain_torch_ops:
    """Inside this context the discriminator runs on plain torch operators (F.conv2d) on any device instead of the
    HIP im2col + GEMM functions.  Those launch raw kernels in their backward and are therefore differentiable
    ONCE; the WGAN-GP gradient penalty (model/loss.py:237-260) differentiates the discriminator TWICE
    (`autograd.grad(create_graph=True)`), which only the plain operators support."""

    def __enter__(self):
        self._saved = _PLAIN_OPS[0]
        _PLAIN_OPS[0] = True
        return self

    def __exit__(self, *exc):
        _PLAIN_OPS[0] = self._saved
        return False


class _SpectralNorm(nn.Module):
    """Spectral-norm parametrization with the state_dict layout of
    torch.nn.utils.parametrizations.spectral_norm (`parametrizations.weight.original`,
    `parametrizations.weight.0._u/_v`) and the same algorithm (one power iteration per training
    forward, sigma = u^T W v on cloned vectors).  The matrix-vector products are written as
    (N,1) matmuls in fp32: on ROCm 7.2 `torch.mv` (aten::addmv_ -> rocBLAS gemv) costs ~4 ms of
    HOST time per call, 1.1 s per training step for the 30 MPD layers (profiles/r01_*)."""

    def __init__(self, weight, n_power_iterations=1, eps=1e-12):
        super().__init__()
        self.n_power_iterations, self.eps = n_power_iterations, eps
        w = weight.detach().flatten(1)
        u = F.normalize(w.new_empty(w.size(0)).normal_(0, 1), dim=0, eps=eps)
        v = F.normalize(w.new_empty(w.size(1)).normal_(0, 1), dim=0, eps=eps)
        self.register_buffer("_u", u)
        self.register_buffer("_v", v)
        self._power_method(w, 15)

    @torch.autograd.no_grad()
    def _power_method(self, w, n):
        if w.is_cuda and n > 0 and w.dtype == torch.float32:
            bind.spectral_power_iter(w.contiguous(), self._u, self._v, n, self.eps)
            return
        for _ in range(n):
            self._u = F.normalize((w @ self._v.unsqueeze(1)).squeeze(1), dim=0, eps=self.eps, out=self._u)
            self._v = F.normalize((w.t() @ self._u.unsqueeze(1)).squeeze(1), dim=0, eps=self.eps, out=self._v)

    def forward(self, weight):
        with torch.autocast(device_type=weight.device.type, enabled=False):
            pre = getattr(self, "_sigma_pre", None)
            if pre is not None and self.training and self.n_power_iterations == 0 and weight.dtype == torch.float32:
                # u, v and sigma = u^T W v of this step come from the batched launch (SpectralBatch.run)
                return _SNDivFn.apply(weight, self._u, self._v, pre)
            w = (weight if weight.dtype == torch.float64 else weight.float()).flatten(1)   # float64: tests' adjudicator
            if self.training:
                self._power_method(w, self.n_power_iterations)
            u, v = self._u.clone(), self._v.clone()
            sigma = (u * (w @ v.unsqueeze(1)).squeeze(1)).sum()
            return weight / sigma


class _SNDivFn(torch.autograd.Function):
    """W / sigma with sigma = u^T W v precomputed (u, v constants, as in torch's spectral_norm):
    dL/dW = (g - <g, W/sigma> u v^T) / sigma  — two passes over the weight instead of the GEMV + outer-product
    GEMM + five elementwise kernels autograd needs for the same expression."""

    @staticmethod
    def forward(ctx, weight, u, v, sigma):
        out = weight / sigma
        ctx.save_for_backward(out, u, v, sigma)
        return out

    @staticmethod
    def backward(ctx, g):
        out, u, v, sigma = ctx.saved_tensors
        g2, o2 = g.reshape(u.numel(), -1), out.reshape(u.numel(), -1)
        s = torch.dot(g2.reshape(-1), o2.reshape(-1))
        gw = torch.addcmul(g2, (u * (-s)).unsqueeze(1), v.unsqueeze(0)) / sigma
        return gw.view_as(out), None, None, None


class _SNStackFn(torch.autograd.Function):
    """The spectrally normalised weights of one layer of all n period discriminators as ONE (n, N, k*Cin) GEMM operand in
    (tap, channel) column order: out[s] = permute(W_s / sigma_s) with sigma_s, u_s, v_s from the batched power iteration
    (constants, as in torch's spectral_norm).  One launch forward, two backward (csrc/spectral.hip) instead of n divisions +
    a stack and, per weight, a dot product, an outer-product update and a division.  An optional last argument, a dict, asks the forward
    launch for the bf16 pair of the operand too (the MFMA convolutions' weight operand, left in it as "w")."""

    @staticmethod
    def forward(ctx, n, *args):
        sig, us, vs, ws = args[:n], args[n:2 * n], args[2 * n:3 * n], args[3 * n:4 * n]
        pair_out = args[4 * n] if len(args) > 4 * n else None      # (stays a plain dict: one key, read by the caller right after apply())
        out = bind.sn_stack_fwd([w.detach().contiguous() for w in ws], sig, want_pair=pair_out is not None)
        if pair_out is not None:
            out, pair_out["w"] = out
        ctx.save_for_backward(out, *sig, *us, *vs)
        ctx.geom = (n, [w.shape for w in ws], len(args) - 4 * n)
        return out

    @staticmethod
    def backward(ctx, dW):
        n, shapes, extra = ctx.geom
        out, *rest = ctx.saved_tensors
        gws = bind.sn_stack_bwd(dW.float().contiguous(), out, rest[:n], rest[n:2 * n], rest[2 * n:3 * n], shapes)
        return (None, *([None] * (3 * n)), *gws, *([None] * extra))


def _sn_stack(layers, pair_out=None):
    """_SNStackFn over the n same-shaped spectrally normalised convolutions `layers`, or None when they do not qualify
    (sigmas not precomputed by SpectralBatch.run, eval mode, other dtypes / devices): the caller then stacks `l.weight`.
    pair_out: a dict that receives the operand's bf16 pair as "w", written by the same launch."""
    sns, origs = [], []
    for l in layers:
        if not (isinstance(l, nn.Conv2d) and parametrize.is_parametrized(l, "weight")):
            return None
        sn, w = l.parametrizations.weight[0], l.parametrizations.weight.original
        if not (isinstance(sn, _SpectralNorm) and getattr(sn, "_sigma_pre", None) is not None and sn.training and sn.n_power_iterations == 0
                and w.is_cuda and w.dtype == torch.float32 and w.dim() == 4 and w.shape[3] == 1):
            return None
        sns.append(sn); origs.append(w)
    n = len(layers)
    if n > 8 or any(w.shape != origs[0].shape for w in origs) or origs[0].shape[1] * origs[0].shape[2] * 4 > 60 * 1024:
        return None
    if n > 1 and (origs[0].numel() % 4):
        return None
    return _SNStackFn.apply(n, *[sn._sigma_pre for sn in sns], *[sn._u for sn in sns], *[sn._v for sn in sns], *origs,
                            *([pair_out] if pair_out is not None else []))


def spectral_norm(module, name="weight", n_power_iterations=1, eps=1e-12):
    parametrize.register_parametrization(module, name, _SpectralNorm(getattr(module, name), n_power_iterations, eps))
    return module


class _Im2ColFn(torch.autograd.Function):
    """x (B, P, H, C) channel-last -> columns (B, P, H1, k*C), (tap, channel) order, zero padding implicit:
    the HIP gather / adjoint-gather kernels of vm_asr_amd/csrc/im2col.hip."""

    @staticmethod
    def forward(ctx, x, k, stride, pad):
        B, P, H, C = x.shape
        cols = bind.im2col_kx1([x.contiguous()], _geom([x]), C, k, stride, pad)
        ctx.geom = (tuple(x.shape), k, stride, pad)
        return cols.view(B, P, -1, k * C)

    @staticmethod
    def backward(ctx, g):
        shape, k, stride, pad = ctx.geom
        return bind.col2im_kx1(g.contiguous(), shape, k, stride, pad), None, None, None


def _conv_kx1_cl(x, weight, bias, stride, pad):
    """Conv2d with a (k,1) kernel, stride (s,1), zero padding (pad,0) on CHANNEL-LAST input
    x (B, P, T, Cin) -> (B, P, T_out, Cout), evaluated as unfold + GEMM.  MIOpen runs these
    (5,1)/(3,1) bf16 convolutions with its `naive_conv_*` fallback (40+ ms per call on MI355X);
    as GEMMs (K = Cin*k up to 5120) they run on the MFMA pipes through hipBLASLt."""
    k = weight.shape[2]
    if x.is_cuda and x.dtype in (torch.float32, torch.float16, torch.bfloat16) and x.shape[2] + 2 * pad >= k:
        cols = _Im2ColFn.apply(x, k, stride, pad)      # (B, P, T_out, k*Cin), (tap, c) order, HIP gather
        w = weight[:, :, :, 0].permute(0, 2, 1).reshape(weight.shape[0], -1)
        return _linear(cols, w, bias)
    if pad:
        x = F.pad(x, (0, 0, pad, pad))
    cols = x.unfold(2, k, stride)                      # (B, P, T_out, Cin, k) view
    Bn, P, To, Cin, _ = cols.shape
    w = weight[:, :, :, 0].reshape(weight.shape[0], Cin * k)   # (Cout, Cin*k), (c,k) order; cast inside linear()
    y = _linear(cols.reshape(Bn, P, To, Cin * k), w, bias)
    return y


class _ConvKx1Fn(torch.autograd.Function):
    """The same convolution with NO im2col: on the (B*P sequences, T, C) channel-last layout the taps of a
    (k,1) kernel are row-shifted views of the zero-padded input, so the convolution is a few GEMMs on views.

      stride 3, k 5:  Xp (N, 3*Hq, C) viewed as V (N*Hq, 3C):   Y = V @ W[taps 0-2]^T ;  Y[:-1] += V[1:, :2C] @ W[taps 3-4]^T
      stride 1, k:    Xp (N*Hp, C):                              Y[:R] = sum_j Xp[j:j+R] @ W[tap j]^T,   R = N*Hp - (k-1)

    Rows that straddle two sequences are junk and lie exactly in the rows the valid-output view drops.
    unfold + GEMM reads and writes 5/3x (stride 3) or 5x (stride 1) the input as columns and scatters it back
    in the backward (`_unfold_backward`: 2.7 ms/step); here the only copy is the zero padding (1x).
    The backward is the same GEMMs transposed; dW is accumulated in fp32 (split over rows where it is one tile)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, cdt):
        B, P, H, C = x.shape
        Cout, _, k, _ = weight.shape
        N = B * P
        H1 = (H + 2 * pad - k) // stride + 1
        w = weight.detach()[:, :, :, 0].to(cdt)                       # (Cout, C, k)
        bc = None if bias is None else bias.detach().to(cdt)
        if stride == 3:
            Hq = H1 + 1
            Hp = 3 * Hq
            xp = F.pad(x.detach().reshape(N, H, C).to(cdt), (0, 0, pad, Hp - pad - H))   # negative = crop unused tail
            V = xp.view(N * Hq, 3 * C)
            Wa = w[:, :, 0:3].permute(0, 2, 1).reshape(Cout, 3 * C)   # (tap, c) order = V's column order
            Wb = w[:, :, 3:5].permute(0, 2, 1).reshape(Cout, 2 * C)
            Y = torch.addmm(bc, V, Wa.t()) if bc is not None else V @ Wa.t()
            Y[:-1].addmm_(V[1:, :2 * C], Wb.t())
            ctx.save_for_backward(xp, Wa, Wb)
            rows = Hq
        else:
            Hp = H + 2 * pad
            xp = F.pad(x.detach().reshape(N, H, C).to(cdt), (0, 0, pad, pad)).view(N * Hp, C)
            R = N * Hp - (k - 1)
            Wt = w.permute(2, 0, 1).contiguous()                       # (k, Cout, C)
            Y = torch.empty((N * Hp, Cout), dtype=cdt, device=x.device)
            Y[R:].zero_()
            if bc is not None:
                torch.addmm(bc, xp[0:R], Wt[0].t(), out=Y[:R])
            else:
                torch.mm(xp[0:R], Wt[0].t(), out=Y[:R])
            for j in range(1, k):
                Y[:R].addmm_(xp[j:j + R], Wt[j].t())
            ctx.save_for_backward(xp, Wt)
            rows = Hp
        ctx.meta = (x.shape, x.dtype, weight.dtype, None if bias is None else bias.dtype, stride, pad, k, H1, rows)
        return Y.view(B, P, rows, Cout)[:, :, :H1]

    @staticmethod
    def backward(ctx, gy):
        (B, P, H, C), xdt, wdt, bdt, stride, pad, k, H1, rows = ctx.meta
        N = B * P
        Cout = gy.shape[-1]
        cdt = ctx.saved_tensors[0].dtype
        g = F.pad(gy.reshape(N, H1, Cout).to(cdt), (0, 0, 0, rows - H1)).view(N * rows, Cout)   # junk rows: zero gradient
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dx = dw = db = None
        if stride == 3:
            xp, Wa, Wb = ctx.saved_tensors
            V = xp.view(N * rows, 3 * C)
            if need_x:
                dV = g @ Wa
                dV[1:, :2 * C].addmm_(g[:-1], Wb)
                dxp = dV.view(N, 3 * rows, C)
            if need_w:
                dWa = _weight_grad(g, V).view(Cout, 3, C)
                dWb = _weight_grad(g[:-1], V[1:, :2 * C]).view(Cout, 2, C)
                dw = torch.cat((dWa, dWb), dim=1).permute(0, 2, 1).unsqueeze(-1).to(wdt)
            Hp = 3 * rows
        else:
            xp, Wt = ctx.saved_tensors
            Hp = rows
            R = N * Hp - (k - 1)
            if need_x:
                dX = torch.zeros((N * Hp, C), dtype=cdt, device=gy.device)
                for j in range(k):
                    dX[j:j + R].addmm_(g[:R], Wt[j])
                dxp = dX.view(N, Hp, C)
            if need_w:
                dw = torch.stack([_weight_grad(g[:R], xp[j:j + R]) for j in range(k)], dim=2).unsqueeze(-1).to(wdt)
        if need_x:
            avail = min(H, Hp - pad)
            dx = dxp[:, pad:pad + avail]
            if avail < H:
                dx = F.pad(dx, (0, 0, 0, H - avail))
            dx = dx.reshape(B, P, H, C).to(xdt)
        if need_b and bdt is not None:
            db = g.sum(0, dtype=torch.float32 if cdt in (torch.float16, torch.bfloat16) else None).to(bdt)
        return dx, dw, db, None, None, None


def _kx1_mode():
    """VMASR_MPD_CONV as conv_kx1 reads it: gemm | s3 (stride-3 layers only) | unfold (default: measured fastest; mfma means the same here)"""
    return knobs.get("VMASR_MPD_CONV") or "unfold"


def _batched_conv_mode():
    """VMASR_MPD_CONV as the batched path reads it: mfma (default) = the implicit-GEMM kernels; any other value = not those"""
    return knobs.get("VMASR_MPD_CONV") or "mfma"


def conv_kx1(x, weight, bias, stride, pad):
    """(k,1) convolution of channel-last x (B, P, T, Cin) -> (B, P, T_out, Cout): the im2col-free GEMM form
    for the discriminator's two shapes (k 5 / stride 3, and stride 1), unfold + GEMM otherwise."""
    k = weight.shape[2]
    mode = _kx1_mode()
    ok = (stride == 3 and k == 5 and mode in ("gemm", "s3")) or (stride == 1 and mode == "gemm")
    if x.is_cuda and ok and x.shape[2] + 2 * pad >= k:
        cdt = _lib.autocast_dtype(x)
        return _ConvKx1Fn.apply(x, weight, bias, stride, pad, cdt)
    return _conv_kx1_cl(x, weight, bias, stride, pad)


def _layer_path(li, act, cdt, prev_dt, stacked, k, stride, pad, Cin, Cout, n, rows_out, rows_in):
    """Which implementation one stacked layer of _forward_batched takes: "post" | "first" | "mfma" | "split" | "gemm".
    act: GELU follows (every layer but conv_post); cdt: compute dtype; prev_dt: dtype of the previous layer's stacked output (None: first
    layer); stacked: the layer reads that output as it is; rows_out / rows_in: the largest slot's rows.  No tensor: runs without a GPU."""
    f32 = cdt == torch.float32
    if (not act and prev_dt is not None and f32 and k == 3 and stride == 1 and pad == 1 and Cout == 1
            and prev_dt == torch.float32 and knobs.get("VMASR_CONV_POST") and bind.conv_post_supported(Cin, k)):
        return "post"       # the 1-channel output convolution (csrc/convpost.hip)
    if (act and li == 0 and f32 and k == 5 and stride == 3 and pad == 2 and Cout == 32 and k * Cin == 5 and Cin == 1
            and knobs.get("VMASR_CONV_FIRST")):
        return "first"      # the 1 -> 32 channel input convolution + GELU (csrc/convfirst.hip)
    if (f32 and knobs.get("VMASR_MPD_GEMM") == "bf16x3" and act and stacked
            and _batched_conv_mode() == "mfma"
            and (Cin >= 128 or _l1_mode() != "0")
            # (shape, slot count and row count of the whole stacked launch: an MPD with more periods or a longer segment than
            #  the launchers address falls through to the split-GEMM path below)
            and bind.conv_mfma_supported_launch(Cin, Cout, k, stride, n, max(_round_up(rows_out, 256), rows_in))):
        # the three compute-bound layers (128 -> 512 -> 1024 -> 1024) as implicit GEMMs (csrc/convgemm.hip).  The 32 -> 128 layer takes the
        # same kernels in their EXACT-F32 form (VMASR_MPD_CONV_L1=f32, the default: fp32 operands, forward and input gradient; the weight
        # gradient as a bf16x3 triple): it is the first GEMM behind the signal, and with its forward at the pair's 16-17 bits (=1) the input
        # gradient d(loss)/d(wave) of an |f|-type loss moved to 2.5e-3 of its scale from float64 (fp32: 4e-4; gate 5e-4, tests/test_mpd.py).
        # =0: im2col + fp32 library GEMM + bias / GELU pass; GEMM + col2im
        return "mfma"
    if _split_mode(k * Cin, Cout, cdt) and Cin % 4 == 0:
        return "split"      # im2col as bf16 pairs + bf16x3 library GEMMs
    return "gemm"           # im2col + one batched library GEMM


class PeriodDiscriminator(nn.Module):
    def __init__(self, period, kernel_size=5, stride=3, use_spectral_norm=False, hidden=32):
        super().__init__()
        self.period = period
        norm = weight_norm if use_spectral_norm else spectral_norm  # sic
        pad = (kernel_size - 1) // 2
        chans = [1, hidden, hidden * 4, hidden * 16, hidden * 32]
        layers = [norm(nn.Conv2d(chans[i], chans[i + 1], (kernel_size, 1), (stride, 1), padding=(pad, 0)))
                  for i in range(4)]
        layers.append(norm(nn.Conv2d(hidden * 32, hidden * 32, (kernel_size, 1), 1, padding=(2, 0))))
        self.layers = nn.ModuleList(layers)
        self.conv_post = norm(nn.Conv2d(hidden * 32, 1, (3, 1), 1, padding=(1, 0)))

    def forward(self, x, detach_weights=False):
        """`detach_weights`: use the (spectrally normalised) weights as constants — the generator's pass
        through the discriminator, where no discriminator gradient is wanted.
        Feature maps are returned channel-last (B, period, T', C): the losses that consume them
        (L1 feature matching, LSGAN means) are layout-agnostic; the flattened score matches the
        reference's element set."""
        fmap = []
        b, c, t = x.shape
        if t % self.period != 0:
            n_pad = self.period - (t % self.period)
            x = F.pad(x, (0, n_pad), "reflect")
            t = t + n_pad
        wb = (lambda l: (l.weight.detach(), l.bias.detach())) if detach_weights else (lambda l: (l.weight, l.bias))
        if not x.is_cuda or _PLAIN_OPS[0]:  # host runs (tests, cpu_baseline) and double backward: plain convolutions
            x = x.view(b, c, t // self.period, self.period)
            for layer in list(self.layers) + [self.conv_post]:
                w, bias = wb(layer)
                x = F.conv2d(x, w, bias, layer.stride, layer.padding)
                if layer is not self.conv_post:
                    x = F.gelu(x)
                fmap.append(x)
            return torch.flatten(x, 1, -1), fmap
        x = x.view(b, c, t // self.period, self.period).permute(0, 3, 2, 1)  # (B, P, T', C=1)
        for layer in self.layers:
            w, bias = wb(layer)
            x = F.gelu(conv_kx1(x, w, bias, layer.stride[0], layer.padding[0]))
            fmap.append(x)
        w, bias = wb(self.conv_post)
        x = conv_kx1(x, w, bias, 1, self.conv_post.padding[0])
        fmap.append(x)
        return torch.flatten(x, 1, -1), fmap


class MultiPeriodDiscriminator(nn.Module):
    def __init__(self, hidden=32, periods=(2, 3, 5, 7, 11)):
        super().__init__()
        self.discriminators = nn.ModuleList([PeriodDiscriminator(p, hidden=hidden) for p in periods])
        self._frozen = None      # per-layer stacked weights while frozen_weights() is active

    def frozen_weights(self):
        """Context in which the caller guarantees that the (normalised) weights do not change — inside
        torch.nn.utils.parametrize.cached() within one training step: the batched passes then share the stacked
        weight of each layer instead of rebuilding it per pass."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            object.__setattr__(self, "_frozen", {})
            try:
                yield
            finally:
                object.__setattr__(self, "_frozen", None)
        return ctx()

    def _forward_batched(self, x, detach_weights=False):
        """All discriminators layer by layer on stacked GEMM operands (GPU path).  Same scores and feature maps
        (channel-last (B, p, T', C) views) as running the PeriodDiscriminators one by one."""
        discs = list(self.discriminators)
        n, (B, _, T) = len(discs), x.shape
        cdt = _lib.autocast_dtype(x)
        cur = []
        for d in discs:
            xp, p = x, d.period
            if T % p:
                xp = F.pad(xp, (0, p - T % p), "reflect")
            cur.append(xp.view(B, 1, -1, p).permute(0, 3, 2, 1).to(cdt))          # (B, p, T/p, 1)
        fmaps, stacks, valid, taps = [[] for _ in discs], [], [], []
        next_pair = this_link = None
        for li in range(len(discs[0].layers) + 1):
            layers = [d.layers[li] if li < len(d.layers) else d.conv_post for d in discs]
            k, stride, pad = layers[0].kernel_size[0], layers[0].stride[0], layers[0].padding[0]
            P = [c.shape[1] for c in cur]
            H1 = [(c.shape[2] + 2 * pad - k) // stride + 1 for c in cur]
            Ms = [B * p * h for p, h in zip(P, H1)]
            act = li < len(discs[0].layers)
            # from the second layer on the inputs are the slots of the previous layer's stacked output: hand that tensor over
            # (slot i = B*p_i sequences of H_i positions) so that its gradient comes back stacked, in one launch
            sgeom, src = None, cur
            pair, next_pair = next_pair, None     # the bf16 (hi, lo) pair of stacks[-1], if the previous layer's epilogue wrote it
            prev_link, this_link = this_link, None   # set by an MFMA layer: the layer above may finish its activation backward
            if stacks and stacks[-1].dtype == cdt and knobs.get("VMASR_STACK_INPUT"):
                sgeom, src = tuple((B * p, c.shape[2]) for c, p in zip(cur, P)), (stacks[-1],)
            rows = _round_up(max(Ms), 256)
            Cin = cur[0].shape[3]
            path = _layer_path(li, act, cdt, stacks[-1].dtype if stacks else None, sgeom is not None, k, stride, pad, Cin,
                               layers[0].out_channels, n, max(Ms), max(B * p * c.shape[2] for c, p in zip(cur, P)))
            wcache = wpair = None
            if path == "mfma" and self._frozen is not None:
                wcache = self._frozen.setdefault(("mfma_ops", li), {})
            W = None
            if knobs.get("VMASR_SN_STACK"):
                # normalisation, stack and (tap, c) permutation of the layer's n weights in one launch; while the trainer
                # holds the weights fixed for the step (frozen_weights()) the passes share it — one gradient path back
                key = (li, bool(detach_weights))
                W = self._frozen.get(key) if self._frozen is not None else None
                if W is None:
                    # an MFMA layer on bf16 pairs that has no weight operand yet: the same launch writes the pair of W
                    got = {} if (path == "mfma" and not (Cin < 128 and _l1_mode() == "f32")
                                 and (wcache is None or "ops" not in wcache)) else None
                    W = _sn_stack(layers, got)
                    wpair = got.get("w") if got is not None else None
                    if W is not None and detach_weights:
                        W = W.detach()
                    if W is not None and self._frozen is not None:
                        self._frozen[key] = W
            if W is not None:
                ws = [(None, l.bias.detach() if detach_weights else l.bias) for l in layers]
            else:
                ws = [(l.weight.detach(), l.bias.detach()) if detach_weights else (l.weight, l.bias) for l in layers]
                # (n, Cout, k, Cin) -> (n, Cout, k*Cin): (tap, c) column order, gathered by the stack's own copy
                W = torch.stack([w.squeeze(3).transpose(1, 2) for w, _ in ws])
                W = W.reshape(n, W.shape[1], -1)
            bstack = torch.stack([b for _, b in ws])
            if path == "post":      # straight on the previous layer's stacked maps (no column operand)
                y = _StackedConvPostFn.apply(tuple(valid[-1]), tuple(c.shape[2] for c in cur), W, bstack, stacks[-1], prev_link)
            elif path == "first":   # straight from the folded signals (no 5-column operand / K = 5 GEMM)
                y = _StackedConvFirstFn.apply(rows, W, bstack, *cur)
            elif path == "mfma":    # one implicit-GEMM launch each way; the epilogue leaves the bf16 pair of its activation for the next layer
                xh, xl = pair if pair is not None else (None, None)
                this_link = _Link()
                y = _StackedConvMfmaFn.apply(k, stride, pad, rows, sgeom, wcache, W, bstack, src[0], xh, xl, this_link, prev_link, wpair)
                next_pair, this_link.pair = this_link.pair, None      # (handed on, not held: the layer that reads it saves it)
            elif path == "split":
                y = _StackedConvSplitFn.apply(k, stride, pad, rows, act, sgeom, W, bstack, *src)
            else:
                cols = _StackedIm2ColFn.apply(k, stride, pad, rows, sgeom, *src)
                y = _BatchedLinearFn.apply(cols, W, bstack, cdt, act)
            tap = None
            if (act and y.requires_grad and y.dtype == torch.float32 and x.requires_grad
                    and knobs.get("VMASR_FEAT_TAP")):
                # generator phase: the map's gradient (next layer's + feature-matching loss's) is formed in one pass (_FeatTapFn)
                t = _Tap()
                y, token = _FeatTapFn.apply(y, t)
                tap = (token, t)
                if this_link is not None:
                    this_link.tap = t
            outs = _UnstackRowsFn.apply(y, *Ms)
            cur = [o.view(B, p, h, -1) for o, p, h in zip(outs, P, H1)]
            for f, c in zip(fmaps, cur):
                f.append(c)
            stacks.append(y)
            valid.append(tuple(Ms))
            taps.append(tap)
        return [torch.flatten(c, 1, -1) for c in cur], StackedFeatures(fmaps, stacks, valid, taps)

    def _use_batched(self, x):
        return (x.is_cuda and not _PLAIN_OPS[0] and knobs.get("VMASR_MPD_BATCHED")
                and len(self.discriminators) > 1)

    def forward_single(self, x, detach_weights=False):
        """scores and feature maps of ONE signal batch (used for the generator pass, where the
        real-signal features of the discriminator pass are reused instead of recomputed)."""
        if self._use_batched(x):
            return self._forward_batched(x, detach_weights)
        res = [d(x, detach_weights) for d in self.discriminators]
        return [r[0] for r in res], [r[1] for r in res]

    def forward_pair(self, y, y_hat):
        """Same results as forward(y, y_hat) from ONE pass over the stacked batch [y; y_hat] (same weights,
        identical per-sample arithmetic); on the GPU all discriminators advance layer by layer together
        (_forward_batched) and the real-signal features come back as StackedFeatures."""
        n = y.shape[0]
        y_real, y_gen, fmap_real, fmap_gen = [], [], [], []
        both = torch.cat((y, y_hat), dim=0)
        if self._use_batched(both):
            scores, feats = self._forward_batched(both)
            y_real, y_gen = [s[:n] for s in scores], [s[n:] for s in scores]
            # the real half of every slot is its leading rows (batch-major row order)
            fmap_real = StackedFeatures([[t[:n] for t in f] for f in feats], feats.stacks, [tuple(m // 2 for m in v) for v in feats.valid])
            return y_real, y_gen, fmap_real, [[t[n:] for t in f] for f in feats]
        else:
            res = [d(both) for d in self.discriminators]
        for s, f in res:
            y_real.append(s[:n]); y_gen.append(s[n:])
            fmap_real.append([t[:n] for t in f]); fmap_gen.append([t[n:] for t in f])
        return y_real, y_gen, fmap_real, fmap_gen

    def spectral_norms(self):
        return [m for m in self.modules() if isinstance(m, _SpectralNorm)]

    def power_iterate_all(self, n_iter, with_sigma=False):
        """n_iter power iterations of every spectrally normalised weight, batched into one launch per phase
        (with_sigma: the normalising sigmas too; call clear_sigmas() when the weights may change).
        Returns False (nothing done) when the model is not on the GPU in fp32."""
        pairs = [(mod.parametrizations.weight[0], mod.parametrizations.weight.original)
                 for mod in self.modules() if isinstance(mod, nn.Conv2d) and parametrize.is_parametrized(mod, "weight")
                 and isinstance(mod.parametrizations.weight[0], _SpectralNorm)]
        if not pairs or not all(w.is_cuda and w.dtype == torch.float32 for _, w in pairs) or len(pairs) > 64:
            return False
        weights = [w.detach() for _, w in pairs]
        batch = getattr(self, "_sn_batch", None)
        if batch is None or not batch.matches(weights):
            batch = SpectralBatch([m for m, _ in pairs], weights)
            object.__setattr__(self, "_sn_batch", batch)
        batch.run(n_iter, with_sigma)
        return True

    def clear_sigmas(self):
        batch = getattr(self, "_sn_batch", None)
        if batch is not None:
            batch.clear_sigma()

    def forward(self, y, y_hat):
        y_real, y_gen, fmap_real, fmap_gen = [], [], [], []
        for disc in self.discriminators:
            r, fr = disc(y)
            y_real.append(r)
            fmap_real.append(fr)
            if y_hat is not None:
                g, fg = disc(y_hat)
                y_gen.append(g)
                fmap_gen.append(fg)
            else:
                y_gen.append(0)
                fmap_gen.append(0)
        return y_real, y_gen, fmap_real, fmap_gen
