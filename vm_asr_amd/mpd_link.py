"""What two stacked layers of the period discriminator share across their boundary (mpd_layers.py, mpd_featloss.py): the backward of the
layer ABOVE a feature map may finish the activation backward of the layer BELOW it — GELU', the feature-matching term, the bf16 split, the
bias gradient's column sums — in its own launch; `_Link.plan` is the one copy of that decision.  No torch import (like knobs.py)."""
from collections import namedtuple

Plan = namedtuple("Plan", "want_f32 want_pair want_db loss")


class _Tap:
    """Between a map's _FeatTapFn and its feature-matching loss (_MaskedL1Fn): the loss' forward offers sign(gen - real), its backward
    leaves the upstream gradient `gtok`; `consumed`: the layer above has folded the term into the map's gradient, the tap passes through."""
    __slots__ = ("sgn", "valid", "scale", "gtok", "consumed")

    def __init__(self):
        self.sgn = self.valid = self.scale = self.gtok = None
        self.consumed = False

    def offer(self, sgn, valid, scale):
        self.sgn, self.valid, self.scale = sgn, valid, scale

    @property
    def fed(self):
        return self.sgn is not None

    def loss_term(self):
        """The term's operands as the fused kernels' keyword arguments, once the sign map AND the upstream gradient are here; else None."""
        if self.sgn is None or self.gtok is None:
            return None
        return dict(sgn=self.sgn, gtok=self.gtok, scale=self.scale, valid=self.valid)


class _Link:
    """The boundary between a stacked MFMA layer (the producer: fill() in its forward) and the layer above it (the consumer).  pre: the
    producer's pre-activation; C: its input channels; x_req / w_req / b_req: which of its gradients are wanted; tap: the _Tap of the map
    between the two (None: untapped); pair: the bf16 (hi, lo) of the producer's activation on its way out of forward (the caller clears it)."""
    __slots__ = ("pre", "C", "x_req", "w_req", "b_req", "tap", "pair", "_stash")

    def __init__(self):
        self.pre = self.C = self.tap = self.pair = self._stash = None
        self.x_req = self.w_req = self.b_req = False

    def fill(self, pre, C, x_req, w_req, b_req, pair):
        self.pre, self.C, self.x_req, self.w_req, self.b_req, self.pair = pre, C, x_req, w_req, b_req, pair

    def put(self, g32, pair, db):
        """The consumer's backward leaves the producer's finished activation backward: fp32 gradient, its bf16 pair, bias column sums."""
        if self._stash is not None:
            raise RuntimeError("MPD: the fused activation backward of an earlier pass was never taken by the layer below")
        self._stash = (g32, pair, db)

    def take(self):
        stash, self._stash = self._stash, None
        return stash

    def plan(self, skip_w, scores_only, map_shape=None):
        """May the consumer finish the producer's activation backward in its own launch?  -> None (no) or a Plan: which outputs the
        producer's backward needs and the feature-matching term to fold in (None: none).  map_shape: the consumer's view of the map."""
        from . import _lib, knobs
        if (self.pre is None or not knobs.get("VMASR_MPD_FUSE_GELU_BWD") or _lib.det_mode()
                or (map_shape is not None and self.pre.shape != map_shape)):
            return None
        want_db = bool(self.b_req and not skip_w)
        want_f32 = bool(self.C < 128 and self.x_req)
        want_pair = bool((not want_f32 and self.x_req) or (self.w_req and not skip_w))
        if not (want_f32 or want_pair):
            return None
        # The map between the two layers must have no other consumer (it would receive the poisoned placeholder in autograd's sum):
        # (a) the generator-loss pass with the stacked feature-matching loss — the map's tap holds the sign map AND the loss' backward has
        #     left the upstream gradient: the term goes into the epilogue too; or
        # (b) a pass the caller declared to read scores only (scores_only(): the discriminator loss) — no term, taps pass through.
        loss = self.tap.loss_term() if self.tap is not None else None
        if loss is not None and map_shape is not None and self.tap.sgn.shape != map_shape:
            loss = None
        if loss is not None:
            self.tap.consumed = True
        elif not scores_only:
            return None
        return Plan(want_f32, want_pair, want_db, loss)
