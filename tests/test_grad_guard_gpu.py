"""The gradient guard on the GPU: csrc/gradnorm.hip against float64, the guarded AdamW launch (csrc/adamw.hip) against
torch.optim.AdamW, and the trainer's eager and captured steps with the guard on."""
import copy

import numpy as np
import pytest
import torch

from test_trainer import _batch, _tiny_config

pytestmark = pytest.mark.gpu

SHAPES = [(1024, 33), (7,), (4097,), (64, 5, 3, 1), (1,), (8192,), (3, 5)]        # tests/test_trainer.py's AdamW shapes
U = 2.0 ** -24

# Accuracy of state[0].  The kernel squares and sums in float64 (per thread, per chunk and across chunks: at most 17 + 8 + 40 + 8
# roundings of 2^-53 on the sum, nothing beside the next term) and rounds the root to fp32 ONCE: one rounding of 2^-24.  By the
# rule "(count + 1) * 2^-24" the tests allow relative 2 * 2^-24 = 1.2e-7 (the fp32-sum design's bound would have been 2e-6).
NORM_RTOL = 2 * U
# state[1] = max_norm / (norm + 1e-6) in fp32 from that norm: the norm's rounding, the sum's and the quotient's, 3 * 2^-24 = 1.8e-7 —
# inside the 4e-6 the tests allow
COEF_RTOL = 4e-6


def _dev():
    return torch.device("cuda", 0)


def _views(shapes, offset, dev):
    flat = torch.zeros(sum(int(np.prod(s)) for s in shapes) + offset, device=dev)
    out, off = [], offset
    for s in shapes:
        n = int(np.prod(s))
        out.append(flat[off:off + n].view(s))
        off += n
    return flat, out


LAYOUTS = {f"single{n}": ([(n,)], 0) for n in (1, 3, 4095, 4096, 4097)}
LAYOUTS["chunks300"] = ([(300 * 4096 + 5,)], 0)
LAYOUTS["views_unaligned"] = (SHAPES, 3)
LAYOUTS["views_aligned"] = (SHAPES, 0)


def _norm64(views):
    return float(torch.sqrt(sum((v.double() ** 2).sum() for v in views)))


@pytest.mark.parametrize("scale", [1.0, 1e-20, 1e15])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_norm_against_float64(layout, scale):
    from vm_asr_amd.grad_guard import GradGuard
    shapes, offset = LAYOUTS[layout]
    torch.manual_seed(11)
    flat, views = _views(shapes, offset, _dev())
    flat.normal_().mul_(scale)
    if offset:
        assert views[0].data_ptr() % 16 != 0
    guard = GradGuard(views, _dev())
    guard.measure()
    r, want = guard.read(), _norm64(views)
    err = abs(r["grad_norm"] - want) / want
    print(f"{layout} x {scale:g}: norm {r['grad_norm']:.9e}, float64 {want:.9e}, rel err {err:.2e} (allowed {NORM_RTOL:.2e})")
    assert err <= NORM_RTOL
    assert r["clip_coef"] == 1.0 and not r["found_inf"] and r["skipped"] == 0


@pytest.mark.parametrize("layout", ["single4097", "views_unaligned", "chunks300"])
def test_clip_coefficient(layout):
    from vm_asr_amd.grad_guard import GradGuard
    shapes, offset = LAYOUTS[layout]
    torch.manual_seed(12)
    flat, views = _views(shapes, offset, _dev())
    flat.normal_()
    n64 = _norm64(views)
    for max_norm in (0.5 * n64, 2 * n64, 0, None):
        guard = GradGuard(views, _dev(), max_norm=max_norm)
        guard.measure()
        got = guard.read()["clip_coef"]
        if not max_norm or max_norm >= n64:
            assert got == 1.0, (max_norm, got)
        else:
            want = min(1.0, max_norm / (n64 + 1e-6))
            assert abs(got - want) <= COEF_RTOL * want, (max_norm, got, want)


def _poison_cases():
    """(layout, index into the flat buffer) of: element 0, the scalar tail of a 4097-element segment, the last element of an
    unaligned segment, a middle chunk of the 300-chunk segment."""
    total = sum(int(np.prod(s)) for s in SHAPES)
    return [("single4097", 0), ("single4097", 4096), ("views_unaligned", 3 + total - 1), ("views_unaligned", 3 + 1024 * 33 + 6),
            ("chunks300", 150 * 4096 + 77)]


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("layout, index", _poison_cases())
def test_found_inf_per_element(layout, index, bad):
    from vm_asr_amd.grad_guard import GradGuard
    shapes, offset = LAYOUTS[layout]
    torch.manual_seed(13)
    flat, views = _views(shapes, offset, _dev())
    flat.normal_()
    guard = GradGuard(views, _dev(), max_norm=1.0)
    guard.measure()
    assert not guard.read()["found_inf"] and guard.read()["skipped"] == 0          # clean: flag 0, counter unchanged
    keep = flat[index].clone()
    flat[index] = bad
    for k in (1, 2):
        guard.measure()
        r = guard.read()
        assert r["found_inf"] and r["skipped"] == k and float(guard.state[2]) == 1.0
    flat[index] = keep
    guard.measure()
    assert not guard.read()["found_inf"] and guard.read()["skipped"] == 2


def test_finite_elements_with_overflowing_squares_are_not_found_inf():
    from vm_asr_amd.grad_guard import GradGuard
    flat, views = _views([(4097,), (5000,)], 3, _dev())
    flat.fill_(1e30)                                     # 1e60 is no fp32 number; every ELEMENT is finite
    guard = GradGuard(views, _dev(), max_norm=1.0)
    guard.measure()
    r = guard.read()
    assert not r["found_inf"] and r["skipped"] == 0
    want = float(torch.tensor(1e30, dtype=torch.float32).double()) * (4097 + 5000) ** 0.5
    assert abs(r["grad_norm"] - want) <= NORM_RTOL * want


def test_ten_calls_are_bit_identical():
    from vm_asr_amd.grad_guard import GradGuard
    torch.manual_seed(14)
    flat, views = _views(SHAPES + [(300 * 4096 + 5,)], 3, _dev())
    flat.normal_()
    guard = GradGuard(views, _dev(), max_norm=3.0)
    outs = []
    for _ in range(10):
        guard.measure()
        outs.append(guard.state[:3].clone())
    assert all(torch.equal(outs[0].view(torch.int32), o.view(torch.int32)) for o in outs[1:])
    assert 0 < float(outs[0][1]) < 1


def _adamw_pair(dev, flat_b):
    """Two identical parameter sets + AdamW(fused, capturable): `a` the twin with gradients of its own, `b` with views of flat_b at
    offset 3 (the set-up of test_hip_adamw_step_matches_torch_fused_adamw)."""
    def make(views):
        ps = [torch.nn.Parameter(torch.randn(*s, device=dev)) for s in SHAPES]
        off = 3
        for p in ps:
            p.grad = flat_b[off:off + p.numel()].view_as(p) if views else torch.zeros_like(p)
            off += p.numel()
        lr = torch.tensor(1e-3, device=dev)
        groups = [{"params": [p for p in ps if p.ndim > 1]}, {"params": [p for p in ps if p.ndim <= 1], "weight_decay": 0.0}]
        return ps, lr, torch.optim.AdamW(groups, lr=lr, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.05, capturable=True, fused=True)
    torch.manual_seed(4)
    a = make(False)
    torch.manual_seed(4)
    b = make(True)
    return a, b


def _set_twin_grads(pa, pb, coef):
    for x, y in zip(pa, pb):
        x.grad.copy_(y.grad * coef)


def _assert_adamw_close(pa, oa, pb, ob, step, tol):
    for x, y in zip(pa, pb):
        sa, sb = oa.state[x], ob.state[y]
        assert float(sa["step"]) == float(sb["step"]) == step, (float(sa["step"]), float(sb["step"]))
        for name, u, v in (("p", x, y), ("m", sa["exp_avg"], sb["exp_avg"]), ("v", sa["exp_avg_sq"], sb["exp_avg_sq"])):
            err = (u - v).abs().max().item()
            assert err <= tol * max(1e-3, u.abs().max().item()), (name, tuple(x.shape), err)


def test_guarded_adamw_clean_gradients_match_torch_on_clipped_copies():
    """Four steps, changing device learning rate, max_norm = half the measured norm.  Tolerance on p, m and v: that of
    test_hip_adamw_step_matches_torch_fused_adamw, 2e-6 * max(1e-3, max|x|), widened by the 4e-6 relative error the fp32
    coefficient may carry into the first-moment term: 2e-6 + 4e-6 = 6e-6.  (The second moment takes the coefficient squared: twice
    the 3 * 2^-24 = 1.8e-7 it really carries, 3.6e-7 — inside the same 6e-6.)"""
    from vm_asr_amd.fused_adamw import HipAdamWStep
    from vm_asr_amd.grad_guard import GradGuard
    dev = _dev()
    flat = torch.zeros(sum(int(np.prod(s)) for s in SHAPES) + 3, device=dev)
    (pa, lra, oa), (pb, lrb, ob) = _adamw_pair(dev, flat)
    torch.manual_seed(5)
    flat.normal_()
    _set_twin_grads(pa, pb, 1.0)
    oa.step(); ob.step()                                             # torch creates the state
    max_norm = 0.5 * _norm64([p.grad for p in pb])
    shadows = {id(p): p.detach().to(torch.bfloat16) for p in pb if p.ndim > 1}
    shadows_t = {id(p): p.detach().to(torch.bfloat16).t().contiguous() for p in pb if p.ndim == 2}
    guard = GradGuard(pb, dev, max_norm=max_norm, params=True)
    guard.rebuild()
    hip = HipAdamWStep(ob, shadows, shadows_t, guard=guard)
    for it in range(4):
        flat.normal_()
        g_before = flat.clone()
        coef = min(1.0, max_norm / (_norm64([p.grad for p in pb]) + 1e-6))
        assert coef < 1.0
        _set_twin_grads(pa, pb, coef)
        lra.fill_(1e-3 / (it + 1)); lrb.fill_(1e-3 / (it + 1))
        oa.step()
        guard.measure()
        hip.step()
        assert torch.equal(flat, g_before)                            # the gradient buffer itself is not modified
    assert hip.still_valid() and guard.still_valid() and guard.read()["skipped"] == 0
    _assert_adamw_close(pa, oa, pb, ob, 5.0, 2e-6 + 4e-6)
    for y in pb:
        if id(y) in shadows:
            assert torch.equal(shadows[id(y)], y.detach().to(torch.bfloat16))
        if id(y) in shadows_t:
            assert torch.equal(shadows_t[id(y)], y.detach().to(torch.bfloat16).t())


def test_guarded_adamw_skips_a_nonfinite_step_and_trains_on():
    from vm_asr_amd.fused_adamw import HipAdamWStep
    from vm_asr_amd.grad_guard import GradGuard
    dev = _dev()
    flat = torch.zeros(sum(int(np.prod(s)) for s in SHAPES) + 3, device=dev)
    (pa, lra, oa), (pb, lrb, ob) = _adamw_pair(dev, flat)
    torch.manual_seed(6)
    flat.normal_()
    _set_twin_grads(pa, pb, 1.0)
    oa.step(); ob.step()
    shadows = {id(p): p.detach().to(torch.bfloat16) for p in pb if p.ndim > 1}
    shadows_t = {id(p): p.detach().to(torch.bfloat16).t().contiguous() for p in pb if p.ndim == 2}
    guard = GradGuard([p.grad for p in pb], dev)
    hip = HipAdamWStep(ob, shadows, shadows_t, guard=guard)
    flat.normal_()
    flat[3 + 1024 * 33 + 2] = float("nan")                            # one element of the (7,) gradient
    everything = [t for y in pb for t in (y, ob.state[y]["exp_avg"], ob.state[y]["exp_avg_sq"], ob.state[y]["step"])]
    everything += list(shadows.values()) + list(shadows_t.values())
    before = [t.detach().clone() for t in everything]
    guard.measure()
    hip.step()
    assert all(torch.equal(t.detach(), c) for t, c in zip(everything, before))
    assert guard.read()["skipped"] == 1
    flat.normal_()                                                    # a clean step: the twin never took the bad one
    _set_twin_grads(pa, pb, 1.0)
    oa.step()
    guard.measure()
    hip.step()
    assert guard.read()["skipped"] == 1 and not guard.read()["found_inf"]
    _assert_adamw_close(pa, oa, pb, ob, 2.0, 2e-6)
    for y in pb:
        if id(y) in shadows:
            assert torch.equal(shadows[id(y)], y.detach().to(torch.bfloat16))


def test_without_a_guard_the_step_is_the_existing_entry_bit_for_bit():
    from vm_asr_amd import _lib
    from vm_asr_amd.fused_adamw import HipAdamWStep
    dev = _dev()
    flat = torch.zeros(sum(int(np.prod(s)) for s in SHAPES) + 3, device=dev)

    def make():
        torch.manual_seed(4)
        ps = [torch.nn.Parameter(torch.randn(*s, device=dev)) for s in SHAPES]
        off = 3
        for p in ps:
            p.grad = flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        lr = torch.tensor(1e-3, device=dev)
        opt = torch.optim.AdamW(ps, lr=lr, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.05, capturable=True, fused=True)
        return ps, opt
    (pa, oa), (pb, ob) = make(), make()
    torch.manual_seed(7)
    flat.normal_()
    oa.step(); ob.step()
    ha, hb = HipAdamWStep(oa, guard=None), HipAdamWStep(ob)
    assert ha.guard is None
    for _ in range(4):
        flat.normal_()
        ha.step()
        torch._foreach_add_(hb.steps, 1)                               # the existing entry, driven by hand
        _lib.call(_lib.lib().vmasr_adamw_step, hb.items, hb.chunks, hb.nchunks, hb.total, hb.lr, hb.steps[0], hb.betas[0], hb.betas[1],
                  hb.eps, device=dev)
    for x, y in zip(pa, pb):
        assert torch.equal(x, y) and float(oa.state[x]["step"]) == float(ob.state[y]["step"]) == 5.0
        assert torch.equal(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"]) and torch.equal(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"])


# ---- trainer -----------------------------------------------------------------------------------------------------------------------
def _trainer(cfg, capturable=False, **kw):
    import vm_asr_amd
    from vm_asr_amd.trainer import Trainer, build_optimizer
    torch.manual_seed(cfg.SEED)
    models = vm_asr_amd.get_model(cfg)
    opts = {"generator": build_optimizer(cfg, models["generator"], capturable=capturable),
            "discriminator": build_optimizer(cfg, [models["mpd"]], capturable=capturable)}
    tr = Trainer(models, [], opts, cfg, _dev(), None, None, {}, amp=False, gan=True, len_epoch=0, **kw)
    for m in tr.models.values():
        m.train()
    return tr


def _weights(tr):
    return [p.detach().clone() for k in ("generator", "mpd") for p in tr.models[k].parameters()]


def _trained_state(tr):
    out = _weights(tr)
    for o in (tr.optimizer_G, tr.optimizer_D):
        for g in o.param_groups:
            for p in g["params"]:
                out += [v.detach().clone() for v in o.state.get(p, {}).values() if torch.is_tensor(v)]
    return out


def _copy_into(dst, src):
    for k in ("generator", "mpd"):
        dst.models[k].load_state_dict(src.models[k].state_dict())
    dst.optimizer_G.load_state_dict(copy.deepcopy(src.optimizer_G.state_dict()))
    dst.optimizer_D.load_state_dict(copy.deepcopy(src.optimizer_D.state_dict()))
    dst.global_step = src.global_step


def _direct_bias(model):
    """A parameter whose gradient autograd delivers directly (not one filled by the deferred end-of-pass finishes, which run after a
    tensor hook would): the bias of a plain, ungrouped Conv2d that received a gradient in the step before."""
    return next(m.bias for m in model.modules() if isinstance(m, torch.nn.Conv2d) and m.groups == 1 and m.bias is not None
                and m.bias.grad is not None)


def _same_step(got, want, start, lr):
    """Two trainers took the same optimiser step from `start`: fp32 atomics in the backward make them differ at rounding level, which
    AdamW's normalised update can turn into a different step for single near-zero-gradient elements — so: no element further apart
    than one full update (2.5 lr), and the two results apart by less than 1 % of what the step moved."""
    diff = sum(float((a - b).abs().sum()) for a, b in zip(got, want))
    moved = sum(float((b - c).abs().sum()) for b, c in zip(want, start))
    assert all(float((a - b).abs().max()) <= 2.5 * lr for a, b in zip(got, want))
    assert moved > 0 and diff <= 1e-2 * moved, (diff, moved)


def test_eager_gpu_trainer_skips_and_clips():
    cfg = _tiny_config()
    batches = [[t.cuda() for t in _batch(cfg, 2, seed=s)] for s in range(4)]
    guarded, plain = _trainer(cfg, skip_nonfinite=True), _trainer(cfg)
    guarded.train_step(*batches[0])
    victims = [_direct_bias(guarded.models[k]) for k in ("generator", "mpd")]
    hooks = [v.register_hook(lambda g: g * float("inf")) for v in victims]
    before = _trained_state(guarded)
    guarded.train_step(*batches[1])
    for h in hooks:
        h.remove()
    after = _trained_state(guarded)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert [g.read()["skipped"] for g in guarded.grad_guards] == [1, 1]
    # the next clean step against an unguarded trainer from the same state (fp32 atomics in the backward: rounding-level differences)
    _copy_into(plain, guarded)
    guarded.train_step(*batches[2])
    plain.train_step(*batches[2])
    lr = float(guarded.optimizer_G.param_groups[0]["lr"])
    _same_step(_weights(guarded), _weights(plain), before, lr)
    assert sum(not torch.equal(a, c) for a, c in zip(_weights(guarded), before)) > 100
    # clip_grad below the measured norms == an unguarded step preceded by clip_grad_norm_
    norms = guarded.guard_report()
    max_norm = 0.5 * min(norms["grad_norm_G"], norms["grad_norm_D"])
    clipped = _trainer(cfg, clip_grad=max_norm)
    _copy_into(clipped, guarded)
    _copy_into(plain, guarded)
    start = _weights(guarded)
    plain_steps = plain._optimizer_steps

    def clip_then_step():
        for o in (plain.optimizer_G, plain.optimizer_D):
            torch.nn.utils.clip_grad_norm_([p for g in o.param_groups for p in g["params"]], max_norm)
        plain_steps()
    plain._optimizer_steps = clip_then_step
    clipped.train_step(*batches[3])
    plain.train_step(*batches[3])
    for guard in clipped.grad_guards:
        r = guard.read()
        assert r["grad_norm"] > max_norm and abs(r["clip_coef"] - max_norm / (r["grad_norm"] + 1e-6)) <= COEF_RTOL * r["clip_coef"]
    _same_step(_weights(clipped), _weights(plain), start, lr)


def test_captured_step_with_the_guard_matches_eager_and_skips_under_replay():
    cfg = _tiny_config()
    batches = [[t.cuda() for t in _batch(cfg, 2, seed=s)] for s in range(5)]
    probe = _trainer(cfg, capturable=True, skip_nonfinite=True)
    probe.train_step(*batches[0])
    norms = probe.guard_report()
    max_norm = 0.1 * min(norms["grad_norm_G"], norms["grad_norm_D"])      # well below: the clip stays active on the later batches
    del probe
    logs, trainers = {}, {}
    gates = {}
    for mode in ("eager", "graph"):
        tr = _trainer(cfg, capturable=True, skip_nonfinite=True, clip_grad=max_norm)
        gate = torch.ones(1, device=_dev())
        tr.train_step(*batches[0])
        for k in ("generator", "mpd"):
            _direct_bias(tr.models[k]).register_hook(lambda g, gate=gate: g * gate)      # before capture: the multiply is in the graph
        if mode == "graph":
            assert tr.enable_graphs(batches[0], warmup=2), tr.graph_error
            assert [g.read()["skipped"] for g in tr.grad_guards] == [0, 0]               # the warm-up steps are undone
        out = []
        for b in batches[1:3]:
            _, lg = tr.train_step(*b)
            out.append({k: float(v) for k, v in lg.items()})
        logs[mode], trainers[mode], gates[mode] = out, tr, gate
    # the tolerance of test_graph_replay_on_new_batches_matches_eager_training
    for i, (a, b) in enumerate(zip(logs["eager"], logs["graph"])):
        for k in a:
            assert abs(a[k] - b[k]) <= (2e-3 if i == 0 else 5e-2) * max(1.0, abs(a[k])), (i, k, a[k], b[k])
    tr, gate = trainers["graph"], gates["graph"]
    assert tr._graphed is not None
    assert all(0 < g.read()["clip_coef"] < 1 and not g.read()["found_inf"] for g in tr.grad_guards)
    # a poisoned replay: nothing moves, the counters advance
    gate.fill_(float("inf"))
    before = _trained_state(tr)
    tr.train_step(*batches[3])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, _trained_state(tr)))
    assert [g.read()["skipped"] for g in tr.grad_guards] == [1, 1]
    # the next clean replay trains
    gate.fill_(1.0)
    tr.train_step(*batches[4])
    torch.cuda.synchronize()
    assert sum(not torch.equal(a, b) for a, b in zip(before, _trained_state(tr))) > 100
    assert [g.read()["skipped"] for g in tr.grad_guards] == [1, 1] and not any(g.read()["found_inf"] for g in tr.grad_guards)
