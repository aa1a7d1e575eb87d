"""The scale discriminator's generator pass with its feature-matching loss computed on the way (model/loss.py:227-235: the mean over all
24 feature maps of mean |real - generated|).

The stem's map — two thirds of the maps' bytes — never meets the loss as a tensor operation: _Stem1dFmFn is ONE autograd function with two
outputs, the map and its loss term, on csrc/stem1d.hip's fm kernels.  The forward reads the real signal's map beside the store of y and
leaves fp64 partial sums; the backward receives both incoming gradients from autograd and forms gy + coef * gterm * sgn(y - y_real) in
registers, y rebuilt like the pre-activation, so nothing of the map's size is kept or written between the two passes.  The other seven
maps of a scale go through the period discriminator's one-pass L1 kernel (mpd_featloss._MaskedL1Fn) as one slot each."""
import torch

from . import knobs, msd_ops as bind
from .mpd_featloss import _MaskedL1Fn, _masked_l1_ok
from .msd import _PLAIN_OPS, _stem_ok, _weight, conv_layer, is_stem


def composed_feature_loss(f_real, f_gen):
    """The reference's loop (what HiFiGANLoss.feature_loss evaluates for plain lists), operator for operator."""
    loss, n = 0, 0
    for dr, dg in zip(f_real, f_gen):
        for rl, gl in zip(dr, dg):
            n += 1
            loss = loss + torch.mean(torch.abs(rl - gl))
    return loss / n


class _Stem1dFmFn(torch.autograd.Function):
    """(y, term) = (GELU(conv1d(x, w, bias, 1, pad)), coef * sum |y - y_real|), term an fp32 scalar; w, bias and y_real are constants.
    Saves x, w, bias and y_real (the caller's tensor): nothing else of the map's size."""

    @staticmethod
    def forward(ctx, x, w, bias, y_real, pad, coef):
        x, w = x.contiguous(), w.contiguous()
        bias = None if bias is None else bias.contiguous()
        y, partials = bind.stem1d_fm_fwd(x, w, bias, y_real, pad)
        ctx.save_for_backward(x, w, bias, y_real)
        ctx.geom = (pad, coef)
        ctx.set_materialize_grads(False)
        return y, (partials.sum() * coef).float()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy, gterm):
        if not ctx.needs_input_grad[0] or (gy is None and gterm is None):
            return None, None, None, None, None, None
        x, w, bias, y_real = ctx.saved_tensors
        pad, coef = ctx.geom
        gy = None if gy is None else gy.float().contiguous()
        gterm = None if gterm is None else gterm.float().reshape(1).contiguous()
        return bind.stem1d_fm_bwd(gy, x, w, bias, y_real, gterm, coef, pad), None, None, None, None, None


def stem_fm_ok(x, w, bias, y_real, pad):
    """The fused stem applies: what stem_conv1d's HIP route needs, constant weights, and a real map that is a plain fp32 constant of
    the generated map's shape."""
    if w.requires_grad or (bias is not None and bias.requires_grad) or not _stem_ok(x, w, bias, 1, pad):
        return False
    shape = (x.shape[0], w.shape[0], bind.out_len(x.shape[2], w.shape[2], 1, pad))
    return (y_real.is_cuda and y_real.dtype == torch.float32 and tuple(y_real.shape) == shape and y_real.is_contiguous()
            and not y_real.requires_grad and bind.stem1d_fm_supported_launch(w.shape[0], w.shape[2], 1, pad, x.shape[0], x.shape[2]))


def _l1_term(r, g, n_maps):
    """mean |r - g| / n_maps of one (B, C, T) map: the one-pass kernel on the map as ONE slot of B C rows, torch's operators where it does
    not apply."""
    if r.shape == g.shape and r.dim() == 3:
        B, C, T = g.shape
        yr, yg = r.reshape(1, B * C, T), g.reshape(1, B * C, T)
        if _masked_l1_ok(yr, yg):
            return _MaskedL1Fn.apply(yr, yg, (B * C,), (1.0 / (B * C * T * n_maps),), None, None)
    return torch.mean(torch.abs(r - g)) / n_maps


def _scale(disc, x, f_real, n_maps):
    """One ScaleDiscriminator on x with constant weights -> (score, this scale's share of the loss).  The layers, and the order of their
    _weight calls, are forward()'s; a stem the fused operator refuses runs conv_layer and its term like the other maps."""
    total = None
    with torch.autocast(device_type=x.device.type, enabled=False):
        if x.dtype in (torch.float16, torch.bfloat16):
            x = x.float()
        for layer, r in zip(list(disc.convs) + [disc.conv_post], f_real):
            w, b = _weight(layer).detach(), layer.bias.detach()
            act = layer is not disc.conv_post
            if act and is_stem(layer) and stem_fm_ok(x, w, b, r, layer.padding[0]):
                x, term = _Stem1dFmFn.apply(x, w, b, r, layer.padding[0], 1.0 / (r.numel() * n_maps))
            else:
                x = conv_layer(x, layer, w, b, act)
                term = _l1_term(r, x, n_maps)
            total = term if total is None else total + term
    return torch.flatten(x, 1, -1), total


def fused_ok(x):
    return x.is_cuda and not _PLAIN_OPS[0] and knobs.get("VMASR_MSD_FEAT") == "hip"


def feature_matching(f_real, x_scales, discs):
    """-> (scores, loss) of the generated signal at its three scales `x_scales` through `discs` with constant weights; f_real: the real
    signal's maps (constants).  loss = the reference's value, the mean over all maps of mean |r - g|."""
    n_maps = sum(len(fs) for fs in f_real)
    scores, loss = [], None
    for disc, x, fr in zip(discs, x_scales, f_real):
        score, part = _scale(disc, x, fr, n_maps)
        scores.append(score)
        loss = part if loss is None else loss + part
    return scores, loss
