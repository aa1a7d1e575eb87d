"""TRAIN.OPTIMIZER.NAME sgd in the trainer on the GPU: the one-launch HIP step against the optimizer.step() route, graph capture that
reads the learning rate from the device at every replay, and the refusal to capture torch's SGD."""
import numpy as np
import pytest
import torch

from test_trainer import _batch, _tiny_config

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _dev():
    return torch.device("cuda", 0)


def _config(**train):
    cfg = _tiny_config(gan=False, batch=2)
    cfg.defrost()
    cfg.TRAIN.OPTIMIZER.NAME = "sgd"
    cfg.TRAIN.WEIGHT_DECAY = 0.05
    for k, v in train.items():
        setattr(cfg.TRAIN, k, v)
    cfg.freeze()
    return cfg


def _trainer(cfg, **kw):
    import vm_asr_amd
    from vm_asr_amd.trainer import Trainer, build_optimizer
    torch.manual_seed(cfg.SEED)
    models = vm_asr_amd.get_model(cfg)
    opts = {"generator": build_optimizer(cfg, models["generator"], capturable=True)}
    tr = Trainer(models, [], opts, cfg, _dev(), None, None, {}, amp=False, gan=False, len_epoch=0, **kw)
    for m in tr.models.values():
        if m is not None:
            m.train()
    return tr


def _params(tr):
    return [p for g in tr.optimizer_G.param_groups for p in g["params"]]


def _first_step(tr):
    """The first step as enable_graphs' warm-up takes it: backward, the flat gradient buffer, then the optimiser half.  -> copies of the
    gradients the optimiser half was given (torch's multi-tensor Nesterov step adds momentum * buf INTO the gradient tensors of a group
    without weight decay, so they cannot be read afterwards; the HIP step leaves them alone)."""
    tr._forward_backward(*[t.cuda() for t in _batch(tr.config, 2)])
    tr.grads.setup("generator")
    grads = [None if p.grad is None else p.grad.clone() for p in _params(tr)]
    tr._reduce_and_step()
    torch.cuda.synchronize()
    return grads


def test_hip_route_matches_the_optimizer_step_route(monkeypatch):
    from vm_asr_amd import _lib
    from vm_asr_amd.fused_sgd import HipSgdStep
    cfg = _config()
    lib = _lib.lib()
    was = lib.vmasr_get_deterministic()
    monkeypatch.setenv("VMASR_DETERMINISTIC", "1")
    lib.vmasr_set_deterministic(1)
    try:
        trainers, grads, start = {}, {}, None
        for knob in ("1", "0"):
            monkeypatch.setenv("VMASR_HIP_SGD", knob)
            tr = trainers[knob] = _trainer(cfg)
            if start is None:
                start = [p.detach().clone() for p in _params(tr)]
            assert all(torch.equal(a, p.detach()) for a, p in zip(start, _params(tr)))      # the same seed: the same weights
            grads[knob] = _first_step(tr)
    finally:
        lib.vmasr_set_deterministic(was)
    hip, ref = trainers["1"], trainers["0"]
    assert hip._hip_sgd and all(isinstance(s, HipSgdStep) for s in hip._hip_sgd) and hip._hip_adamw is None      # the HIP route ran
    assert ref._hip_sgd is None
    opt = hip.optimizer_G
    lr, mu = float(opt.param_groups[0]["lr"]), float(np.float32(opt.param_groups[0]["momentum"]))
    assert opt.param_groups[0]["nesterov"] and lr == float(np.float32(cfg.TRAIN.BASE_LR))
    wds = [float(np.float32(g["weight_decay"])) for g in opt.param_groups for _ in g["params"]]
    assert set(wds) == {0.0, float(np.float32(0.05))}
    n = 0
    for p, q, g, gq, p0, wd in zip(_params(hip), _params(ref), grads["1"], grads["0"], start, wds):
        assert (g is None) == (gq is None) == (p.grad is None)
        if g is None:
            assert torch.equal(p.detach(), p0) and torch.equal(q.detach(), p0)
            continue
        n += 1
        assert torch.equal(g, gq) and torch.equal(p.grad, g)                     # deterministic mode: bit-identical gradients; the HIP step left them alone
        S = g.double().abs() + wd * p0.double().abs()                            # (the buffers start at zero)
        bp, bq = hip.optimizer_G.state[p]["momentum_buffer"], ref.optimizer_G.state[q]["momentum_buffer"]
        assert bool(((bp.double() - bq.double()).abs() <= 2 * 8 * U * S).all())
        assert bool(((p.detach().double() - q.detach().double()).abs() <= 2 * 8 * U * (p0.double().abs() + lr * (1 + mu) * S)).all())
    assert n > 100 and sum(not torch.equal(p.detach(), p0) for p, p0 in zip(_params(hip), start)) > 100


def test_guarded_trainer_takes_the_guarded_hip_step():
    tr = _trainer(_config(), skip_nonfinite=True)
    start = [p.detach().clone() for p in _params(tr)]
    _first_step(tr)
    assert tr._hip_sgd and tr._hip_sgd[0].guard is tr.grad_guards[0]
    r = tr.guard_report()
    assert r["skipped_G"] == 0 and r["grad_norm_G"] > 0
    assert sum(not torch.equal(p.detach(), p0) for p, p0 in zip(_params(tr), start)) > 100


def test_captured_step_reads_the_learning_rate_from_the_device(monkeypatch):
    from vm_asr_amd.optim import build_scheduler
    monkeypatch.setenv("VMASR_STEP_VARIANT", "one")
    # "step" schedule with MAX_LR 0: the warm-up's first value, lr_at(0), is 0, and lr_at(W) is BASE_LR
    cfg = _config(MAX_LR=0.0, EPOCHS=4, WARMUP_EPOCHS=1)
    cfg.defrost()
    cfg.TRAIN.LR_SCHEDULER.NAME = "step"
    cfg.freeze()
    tr = _trainer(cfg)
    batch = [t.cuda() for t in _batch(cfg, 2)]
    sched = build_scheduler(cfg, tr.optimizer_G, 5)
    lr = tr.optimizer_G.param_groups[0]["lr"]
    assert float(lr) == 0.0 and sched.lr_at(5) == cfg.TRAIN.BASE_LR
    sched.step_update(5)
    assert tr.enable_graphs(batch, warmup=2), tr.graph_error          # the very first optimiser step of this trainer is a warm-up step
    assert tr._graphed is not None and tr._hip_sgd and tr.optimizer_G.param_groups[0]["lr"] is lr
    params = [p for p in _params(tr) if p.grad is not None]
    bufs = [tr.optimizer_G.state[p]["momentum_buffer"] for p in params]
    assert len(params) > 100 and all(torch.count_nonzero(b) == 0 for b in bufs)      # the warm-up steps were undone
    # lr 0 through the schedule: a replayed step leaves every parameter bit-identical while the momentum buffers move
    sched.step_update(0)
    assert tr.optimizer_G.param_groups[0]["lr"] is lr and float(lr) == 0.0
    p0 = [p.detach().view(torch.int32).clone() for p in params]
    tr.train_step(*batch)
    torch.cuda.synchronize()
    assert all(torch.equal(a, p.detach().view(torch.int32)) for a, p in zip(p0, params))
    assert sum(int(torch.count_nonzero(b)) > 0 for b in bufs) > 100
    # lr restored: the next replay moves the parameters
    sched.step_update(5)
    assert float(lr) == float(np.float32(cfg.TRAIN.BASE_LR))
    tr.train_step(*batch)
    torch.cuda.synchronize()
    assert sum(not torch.equal(a, p.detach().view(torch.int32)) for a, p in zip(p0, params)) > 100
    assert tr._hip_sgd[0].still_valid()


def test_capture_is_refused_without_the_hip_step(monkeypatch):
    monkeypatch.setenv("VMASR_STEP_VARIANT", "one")
    monkeypatch.setenv("VMASR_HIP_SGD", "0")
    cfg = _config()
    tr = _trainer(cfg)
    with pytest.raises(RuntimeError, match="VMASR_HIP_SGD=0"):
        tr.enable_graphs([t.cuda() for t in _batch(cfg, 2)], warmup=2)
    assert tr._graphed is None
    # ... and an SGD with a host learning rate is refused with the wrapper's reason, not captured
    monkeypatch.setenv("VMASR_HIP_SGD", "1")
    for g in tr.optimizer_G.param_groups:
        g["lr"] = 1e-3
    with pytest.raises(RuntimeError, match="learning-rate tensor"):
        tr.enable_graphs([t.cuda() for t in _batch(cfg, 2)], warmup=2)
