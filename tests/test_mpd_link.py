"""vm_asr_amd/mpd_link.py: the typed hand-off between two stacked layers of the period discriminator.

CPU: the decision table of `_Link.plan` (expected column written down from the two `_fuse_below` bodies of the commit before the link
existed, one for the MFMA input gradient, one — with the map's shape — for conv_post), the stash, the two phase flags.
GPU: no pass leaves a stash, an upstream gradient or a `consumed` mark behind, and a second pass repeats the first."""
from types import SimpleNamespace as NS

import pytest
import torch

from vm_asr_amd.mpd_link import _Link, _Tap

MAP = (5, 256, 128)
OTHER = (5, 256, 512)


def _link(pre=MAP, C=128, x_req=True, w_req=False, b_req=False, tap=None):
    l = _Link()
    if pre is not None:
        l.fill(NS(shape=pre), C, x_req, w_req, b_req, pair=None)
    l.tap = tap
    return l


def _tap(sgn=MAP, gtok=True):
    t = _Tap()
    if sgn is not None:
        t.offer(NS(shape=sgn), (256,) * 5, (0.5,) * 5)
    if gtok:
        t.gtok = NS(shape=(1,))
    return t


# (id, link arguments, tap arguments or None, environment, skip_w, scores_only, map_shape,
#  expected: None or (want_f32, want_pair, want_db, carries the loss term))
PLAN_TABLE = [
    ("no pre", dict(pre=None), None, {}, False, True, None, None),
    ("knob 0", {}, None, {"VMASR_MPD_FUSE_GELU_BWD": "0"}, False, True, None, None),
    ("deterministic", {}, None, {"VMASR_DETERMINISTIC": "1"}, False, True, None, None),
    ("nothing wanted", dict(x_req=False, w_req=False, b_req=True), None, {}, False, True, None, None),
    ("w only, skipped", dict(x_req=False, w_req=True), None, {}, True, True, None, None),
    ("w only", dict(x_req=False, w_req=True), None, {}, False, True, None, (False, True, False, False)),
    ("C 32, x", dict(C=32), None, {}, False, True, None, (True, False, False, False)),
    ("C 32, x and w", dict(C=32, w_req=True), None, {}, False, True, None, (True, True, False, False)),
    ("C 32, x and w, skipped", dict(C=32, w_req=True), None, {}, True, True, None, (True, False, False, False)),
    ("C 128, x", dict(C=128), None, {}, False, True, None, (False, True, False, False)),
    ("C 128, x and w, skipped", dict(C=128, w_req=True), None, {}, True, True, None, (False, True, False, False)),
    ("bias", dict(b_req=True), None, {}, False, True, None, (False, True, True, False)),
    ("bias, skipped", dict(b_req=True), None, {}, True, True, None, (False, True, False, False)),
    ("knob 1 spelt out", {}, None, {"VMASR_MPD_FUSE_GELU_BWD": "1", "VMASR_DETERMINISTIC": "0"}, False, True, None, (False, True, False, False)),
    ("no tap, map consumed elsewhere", {}, None, {}, False, False, None, None),
    ("fed tap with gradient", {}, dict(), {}, True, False, None, (False, True, False, True)),
    ("fed tap with gradient, scores only", {}, dict(), {}, True, True, None, (False, True, False, True)),
    ("fed tap, no gradient", {}, dict(gtok=False), {}, True, False, None, None),
    ("fed tap, no gradient, scores only", {}, dict(gtok=False), {}, True, True, None, (False, True, False, False)),
    ("unfed tap", {}, dict(sgn=None, gtok=False), {}, False, False, None, None),
    ("unfed tap, scores only", {}, dict(sgn=None, gtok=False), {}, False, True, None, (False, True, False, False)),
    ("map shape, all equal", {}, dict(), {}, True, False, MAP, (False, True, False, True)),
    ("map shape, pre differs", dict(pre=OTHER), dict(), {}, True, True, MAP, None),
    ("map shape, sign differs", {}, dict(sgn=OTHER), {}, True, False, MAP, None),
    ("map shape, sign differs, scores only", {}, dict(sgn=OTHER), {}, True, True, MAP, (False, True, False, False)),
    ("no map shape, sign differs", {}, dict(sgn=OTHER), {}, True, False, None, (False, True, False, True)),
    ("nothing wanted, fed tap", dict(x_req=False), dict(), {}, True, False, None, None),
]


@pytest.mark.parametrize("name,largs,targs,env,skip_w,scores,map_shape,want", PLAN_TABLE, ids=[r[0] for r in PLAN_TABLE])
def test_link_plan_decision_table(monkeypatch, name, largs, targs, env, skip_w, scores, map_shape, want):
    for k in ("VMASR_MPD_FUSE_GELU_BWD", "VMASR_DETERMINISTIC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tap = _tap(**targs) if targs is not None else None
    link = _link(tap=tap, **largs)
    plan = link.plan(skip_w, scores, map_shape)
    if want is None:
        assert plan is None
    else:
        assert plan is not None and (plan.want_f32, plan.want_pair, plan.want_db) == want[:3]
        if want[3]:
            assert set(plan.loss) == {"sgn", "gtok", "scale", "valid"}
            assert plan.loss["sgn"] is tap.sgn and plan.loss["gtok"] is tap.gtok
            assert plan.loss["scale"] == tap.scale and plan.loss["valid"] == tap.valid
        else:
            assert plan.loss is None
    if tap is not None:      # marked exactly when a plan carries the term
        assert tap.consumed is bool(want is not None and want[3])
    assert link.take() is None      # deciding stores nothing


def test_tap_offer_and_loss_term():
    t = _Tap()
    assert not t.fed and t.loss_term() is None and t.consumed is False and t.gtok is None
    t.offer("s", (3,), (0.25,))
    assert t.fed and t.loss_term() is None
    t.gtok = "g"
    assert t.loss_term() == dict(sgn="s", gtok="g", scale=(0.25,), valid=(3,))
    with pytest.raises(AttributeError):
        t.gtoken = 1      # a misspelt field fails instead of travelling along


def test_link_stash():
    l = _Link()
    assert l.take() is None
    l.put("g32", ("hi", "lo"), "db")
    assert l.take() == ("g32", ("hi", "lo"), "db")
    assert l.take() is None
    l.put(None, ("hi", "lo"), None)
    with pytest.raises(RuntimeError):
        l.put("g32", None, None)      # the result of an earlier pass that nobody took
    assert l.take() == (None, ("hi", "lo"), None)
    with pytest.raises(AttributeError):
        l.stash = 1


@pytest.mark.parametrize("flag", ["skip_weight_grads", "scores_only"])
def test_phase_flags_restore_what_they_found(flag):
    from vm_asr_amd import discriminator
    cls = getattr(discriminator, flag)
    other = discriminator.scores_only if flag == "skip_weight_grads" else discriminator.skip_weight_grads
    assert cls.on is False
    with cls():
        assert cls.on is True and other.on is False
        with cls():
            assert cls.on is True
        assert cls.on is True      # still set until the outer block ends
    assert cls.on is False
    with pytest.raises(KeyError):
        with cls():
            with cls():
                raise KeyError("inside")
    assert cls.on is False
    with cls():
        with pytest.raises(KeyError):
            with cls():
                raise KeyError("inside")
        assert cls.on is True
    assert cls.on is False


@pytest.mark.gpu
def test_no_pass_leaves_anything_behind_and_a_second_pass_repeats_the_first(monkeypatch):
    """MultiPeriodDiscriminator(hidden=32) on (2, 1, 12000) signals (the 128 -> 512 -> 1024 -> 1024 layers on the MFMA kernels): after the
    fused generator-loss backward, the per-map (unfused) one and a scores_only() discriminator-loss backward every tap has
    `consumed == False` and `gtok is None` and every link of that forward an empty stash; a second backward through a fresh forward gives
    the first one's gradients: 2e-6 of the scale for d(loss)/d(signal), 2e-5 of its scale per parameter.  All three passes run in eval
    mode, the discriminator-loss pass with weights that want their gradients: in training mode every forward runs a power iteration of
    the spectral norm whose W^T u sums are unordered atomics (csrc/spectral.hip), so the two runs would not see the same weights
    (measured there: d(loss)/d(signal) 2.9e-6 of its scale apart, parameters up to 2.4e-6); the links, puts and taps are the same."""
    from vm_asr_amd import mpd_link
    from vm_asr_amd.discriminator import MultiPeriodDiscriminator, StackedFeatures, scores_only
    from vm_asr_amd.loss import HiFiGANLoss
    links, puts = [], []
    init, put = mpd_link._Link.__init__, mpd_link._Link.put
    monkeypatch.setattr(mpd_link._Link, "__init__", lambda self: (links.append(self), init(self))[1])
    monkeypatch.setattr(mpd_link._Link, "put", lambda self, *a: (puts.append(self), put(self, *a))[1])
    monkeypatch.delenv("VMASR_MPD_FUSE_GELU_BWD", raising=False)
    monkeypatch.delenv("VMASR_DETERMINISTIC", raising=False)
    torch.manual_seed(3)
    D = MultiPeriodDiscriminator(hidden=32).cuda()
    y = 0.3 * torch.randn(2, 1, 12000, device="cuda")
    y_hat0 = 0.3 * torch.randn(2, 1, 12000, device="cuda")
    L = HiFiGANLoss("lsgan")

    def clean(feats, n_puts):
        taps = [t for t in feats.taps if t is not None]
        assert len(taps) == 5      # the five maps behind a GELU
        for _, t in taps:
            assert t.consumed is False and t.gtok is None
        assert len(links) == 4 and len(puts) == n_puts, (len(links), len(puts))      # 32 -> 128 -> 512 -> 1024 -> 1024
        assert all(p in links for p in puts) and all(l.take() is None for l in links)

    def generator_pass(stacked):
        D.eval()
        y_hat = y_hat0.clone().requires_grad_()
        with torch.no_grad():
            _, real = D.forward_single(y)
        links.clear(); puts.clear()
        scores, gen = D.forward_single(y_hat, detach_weights=True)
        assert isinstance(real, StackedFeatures) and isinstance(gen, StackedFeatures)
        feats = (real, gen) if stacked else ([list(f) for f in real], [list(f) for f in gen])
        loss = 2.0 * L.feature_loss(*feats) + sum((1.0 - s).pow(2).mean() for s in scores)
        loss.backward()
        clean(gen, 4 if stacked else 0)      # three input-gradient epilogues and conv_post, or none: the maps have a second consumer
        return {"signal": y_hat.grad.clone()}

    def discriminator_pass():
        D.eval()                          # (same weights in both runs: no power iteration of the spectral norm)
        D.zero_grad(set_to_none=True)
        x = y_hat0.clone().requires_grad_()      # (as in the trainer's shared fake pass: taps exist, nobody feeds them)
        links.clear(); puts.clear()
        scores, feats = D.forward_single(x)
        loss = sum((1.0 - s).pow(2).mean() for s in scores)
        with scores_only():
            loss.backward()
        clean(feats, 4)
        grads = {n: p.grad.clone() for n, p in D.named_parameters() if p.grad is not None}
        assert len(grads) > 20
        return dict(grads, signal=x.grad.clone())

    bad = []
    for name, run in (("generator, stacked loss", lambda: generator_pass(True)), ("generator, per-map loss", lambda: generator_pass(False)),
                      ("discriminator, scores only", discriminator_pass)):
        first, second = run(), run()
        assert first.keys() == second.keys()
        for k in first:
            sc = max(first[k].abs().max().item(), 1e-12)
            err = (second[k] - first[k]).abs().max().item()
            print(f"{name}: {k}: {err:.3e} of scale {sc:.3e} = {err / sc:.2e}")
            if not (torch.isfinite(second[k]).all() and err <= (2e-6 if k == "signal" else 2e-5) * sc):
                bad.append((name, k, err, sc))
    assert not bad, bad
