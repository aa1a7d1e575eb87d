"""The feature-matching loss of the batched period-discriminator pass on the stacked maps, and the tap that forms a map's gradient."""
import torch

from . import knobs, mpd_ops as bind


class StackedFeatures(list):
    """Feature maps of the batched discriminator pass: the usual list (per discriminator) of lists (per layer) of
    channel-last views, plus the stacked per-layer tensors they are views of — `stacks[l]` is (n, rows_l, N_l)
    and `valid[l][i]` says how many leading rows of slot i belong to this signal — so that losses over ALL
    discriminators can run as one kernel per layer (feature_loss_stacked) instead of one per feature map."""

    def __init__(self, per_disc, stacks, valid, taps=None):
        super().__init__(per_disc)
        self.stacks, self.valid = stacks, valid
        self.taps = taps if taps is not None else [None] * len(stacks)     # (token, _Tap) of _FeatTapFn per layer, or None

    def detach(self):
        return StackedFeatures([[f.detach() for f in fs] for fs in self], [y.detach() for y in self.stacks], self.valid)


class _FeatTapFn(torch.autograd.Function):
    """Identity on a stacked feature map that also hands out a one-element TOKEN.  The feature-matching loss takes the token —
    not the map — as its differentiable input (_MaskedL1Fn with `tap`) and leaves sign(gen - real) in `tap` (a _Tap); the map's
    gradient is then formed HERE as  gy + g_loss * scale[s] * sign  in one pass (vmasr_masked_l1_bwd_add: r 5 B, w 4 B per
    element) instead of the loss's own backward pass (r 1, w 4) + autograd's sum of the two gradients (r 8, w 4): the maps are
    0.8 GB per generator step.  A tap nobody feeds (the discriminator phase) passes gy through."""

    @staticmethod
    def forward(ctx, y, tap):
        ctx.tap = tap
        ctx.set_materialize_grads(False)
        return y.view_as(y), y.new_zeros(1)

    @staticmethod
    def backward(ctx, gy, gtok):
        t = ctx.tap
        sgn = t.sgn                 # (kept: with a shared discriminator pass the graph is walked once per loss phase)
        t.gtok = None               # (left by the loss' backward for the layer above: _Link.plan)
        consumed, t.consumed = t.consumed, False
        if consumed:                # the layer above has formed gy + g_loss * scale * sign (and GELU') in its epilogue
            return gy, None
        if gtok is None or sgn is None:
            return gy, None
        add = None if gy is None else gy.float().contiguous()
        return bind.masked_l1_bwd(sgn, gtok.float().contiguous(), t.valid, t.scale, add, tap=True), None


_FEAT_MASKS = {}


class _MaskedL1Fn(torch.autograd.Function):
    """sum_s scale[s] * sum_{r < valid[s]} |gen[s, r] - real[s, r]| over two stacked fp32 feature tensors in one pass
    (csrc/featloss.hip), gradient with respect to `gen` only (the real-signal features are constants of the
    generator phase); the forward leaves sign(gen - real) as int8 for the one-pass backward."""

    @staticmethod
    def forward(ctx, real, gen, valid, scale, token, tap):
        """token / tap: of the map's _FeatTapFn — then `gen` is the DETACHED map, the gradient goes to the token and the
        tap forms the map's gradient from the sign left in `tap`."""
        tapped = token is not None and ctx.needs_input_grad[4]
        partials, sgn = bind.masked_l1_fwd(real, gen, valid, scale, ctx.needs_input_grad[1] or tapped)
        ctx.meta = (valid, scale, gen.shape)
        ctx.tapped = tapped
        ctx.tap = tap if tapped else None
        if tapped:
            tap.offer(sgn, valid, scale)
        elif sgn is not None:
            ctx.save_for_backward(sgn)
        return partials.sum().float()

    @staticmethod
    def backward(ctx, g):
        if ctx.tapped:
            # this node runs before the discriminator's layers (it was created after them); the layer above the tapped map folds
            # g * scale * sign into its input-gradient epilogue when it finds the upstream gradient here (_Link.plan)
            ctx.tap.gtok = g.detach().reshape(1).float().contiguous()
            return None, None, None, None, g.reshape(1), None
        (sgn,) = ctx.saved_tensors
        valid, scale, _ = ctx.meta
        return None, bind.masked_l1_bwd(sgn, g.float().contiguous(), valid, scale), None, None, None, None


def _masked_l1_ok(yr, yg):
    return (yg.is_cuda and yr.is_cuda and yg.dtype == torch.float32 and yr.dtype == torch.float32 and yg.is_contiguous()
            and yr.is_contiguous() and not yr.requires_grad and yg.shape[0] <= 8 and yg.shape[0] == yr.shape[0]
            and (yg.shape[1] * yg.shape[2]) % 4 == 0 and (yr.shape[1] * yr.shape[2]) % 4 == 0
            and knobs.get("VMASR_FEAT_L1"))


def feature_loss_stacked(real, gen):
    """HiFi-GAN feature-matching loss (model/loss.py:227-235: mean over feature maps of mean |r - g|) from two
    StackedFeatures with the same per-slot row counts; None if the inputs do not qualify."""
    if not (isinstance(real, StackedFeatures) and isinstance(gen, StackedFeatures)) or real.valid != gen.valid:
        return None
    n_maps = sum(len(fs) for fs in gen)
    total = None
    for yr, yg, valid, tap in zip(real.stacks, gen.stacks, real.valid, gen.taps):
        R, N = min(yr.shape[1], yg.shape[1]), yg.shape[2]
        if max(valid) > R:
            return None
        if _masked_l1_ok(yr, yg):
            scale = tuple(1.0 / (m * N * n_maps) for m in valid)
            if tap is not None and tap[0].requires_grad and not tap[1].fed:
                term = _MaskedL1Fn.apply(yr, yg.detach(), tuple(valid), scale, *tap)
            else:
                term = _MaskedL1Fn.apply(yr, yg, tuple(valid), scale, None, None)
            total = term if total is None else total + term
            continue
        key = (yg.device, valid, R, N, n_maps)
        mask = _FEAT_MASKS.get(key)
        if mask is None:       # 1 / (elements of the feature map * number of maps) on its rows, 0 on padding rows
            rows = torch.arange(R, device=yg.device).unsqueeze(0)
            m = torch.tensor(valid, device=yg.device).unsqueeze(1)
            mask = ((rows < m).float() / (m.float() * N * n_maps)).unsqueeze(2)
            _FEAT_MASKS[key] = mask
        term = ((yg[:, :R] - yr[:, :R]).abs() * mask).sum()
        total = term if total is None else total + term
    return total
