"""The learning-rate schedules of optim.build_scheduler (TRAIN.LR_SCHEDULER.NAME: cosine | linear | step | multistep) against the
reference's formulas (utils/lr_scheduler.py:15-188, timm's StepLRScheduler), and the CPU half of the SGD optimiser: its state through
portable_optimizer_state / load_optimizer_state.  No GPU, no library."""
import bisect
import copy

import pytest
import torch

N = 7                       # updates per epoch
EPOCHS, WARMUP_EPOCHS = 50, 10
T, W = EPOCHS * N, WARMUP_EPOCHS * N          # 350, 70
REL = 1e-12                 # the test restates the formulas in float64 Python: differences come from the order of operations only


def _config(name, base=1e-3, max_lr=1e-3, multisteps=(), optimizer="adamw"):
    from vm_asr_amd.config import get_default_config
    c = get_default_config()
    c.TRAIN.EPOCHS, c.TRAIN.WARMUP_EPOCHS = EPOCHS, WARMUP_EPOCHS
    c.TRAIN.BASE_LR, c.TRAIN.MAX_LR, c.TRAIN.MIN_LR = base, max_lr, 1e-5
    c.TRAIN.LR_SCHEDULER.NAME = name
    c.TRAIN.LR_SCHEDULER.DECAY_EPOCHS, c.TRAIN.LR_SCHEDULER.DECAY_RATE = 30, 0.1
    c.TRAIN.LR_SCHEDULER.GAMMA, c.TRAIN.LR_SCHEDULER.MULTISTEPS = 0.1, list(multisteps)
    c.TRAIN.OPTIMIZER.NAME = optimizer
    return c


def _opt(lr=1e-3, tensor=False):
    p = torch.nn.Parameter(torch.zeros(3))
    return torch.optim.SGD([{"params": [p]}, {"params": [torch.nn.Parameter(torch.zeros(2))], "weight_decay": 0.0}],
                           lr=torch.tensor(lr) if tensor else lr, momentum=0.9)


def _warmup(t, base, max_lr):
    return max_lr + t * (base - max_lr) / W


def _expected(name, t, base, max_lr):
    if t < W:
        return _warmup(t, base, max_lr)
    if name == "linear":
        return base - (base - 0.01 * base) * (t - W) / (T - W)
    if name == "step":
        return base * 0.1 ** (t // (30 * N))
    return base * 0.1 ** bisect.bisect_right([20 * N, 40 * N], t)


# t = 0, W - 1, W, a decay boundary minus one, the boundary, T - 1 (linear has no boundary: the middle of the ramp instead)
POINTS = {"linear": (0, W - 1, W, (T + W) // 2 - 1, (T + W) // 2, T - 1),
          "step": (0, W - 1, W, 30 * N - 1, 30 * N, T - 1),
          "multistep": (0, W - 1, W, 20 * N - 1, 20 * N, 40 * N - 1, 40 * N, T - 1)}


@pytest.mark.parametrize("max_lr", [1e-3, 5e-3])       # MAX_LR == BASE_LR (the yaml default: a flat warm-up) and != (a ramp DOWN to BASE_LR)
@pytest.mark.parametrize("name", ["linear", "step", "multistep"])
def test_schedule_follows_the_reference_formula(name, max_lr):
    from vm_asr_amd.optim import build_scheduler
    base = 1e-3
    opt = _opt(base)
    s = build_scheduler(_config(name, base, max_lr, multisteps=(20, 40)), opt, N)
    assert all(g["lr"] == max_lr for g in opt.param_groups)          # constructed = step_update(0): the warm-up's first value
    for t in POINTS[name]:
        want = _expected(name, t, base, max_lr)
        assert abs(s.lr_at(t) - want) <= REL * want, (name, t, s.lr_at(t), want)
        s.step_update(t)
        assert all(g["lr"] == s.lr_at(t) for g in opt.param_groups)
    # the values themselves, so that a formula wrong in the test AND the code alike does not pass: the ends of each schedule
    assert s.lr_at(0) == max_lr and abs(s.lr_at(W) - base) <= REL
    if max_lr != base:
        assert s.lr_at(W - 1) > base and s.lr_at(1) < max_lr         # warm-up taken from MAX_LR towards BASE_LR, not the other way
    last = {"linear": base - 0.99 * base * (T - 1 - W) / (T - W), "step": base * 0.1, "multistep": base * 0.01}[name]
    assert abs(s.lr_at(T - 1) - last) <= 1e-9 * base
    if name == "step":
        assert abs(s.lr_at(30 * N - 1) - base) <= REL and abs(s.lr_at(30 * N) - 0.1 * base) <= REL * base
    if name == "multistep":
        assert abs(s.lr_at(20 * N - 1) - base) <= REL and abs(s.lr_at(20 * N) - 0.1 * base) <= REL * base
        assert abs(s.lr_at(40 * N) - 0.01 * base) <= REL * base


def test_cosine_through_build_scheduler_is_the_existing_class():
    from vm_asr_amd.optim import CosineWarmupScheduler, build_scheduler
    cfg = _config("cosine")
    a, b = _opt(), _opt()
    s = build_scheduler(cfg, a, N)
    d = CosineWarmupScheduler(b, cfg.TRAIN.EPOCHS * N, cfg.TRAIN.WARMUP_EPOCHS * N, cfg.TRAIN.BASE_LR, cfg.TRAIN.MIN_LR,
                              cfg.TRAIN.LR_SCHEDULER.WARMUP_PREFIX)
    assert type(s) is CosineWarmupScheduler
    for t in (0, 1, W - 1, W, W + 1, T // 2, T - 1, T, T + 5):
        assert s.lr_at(t) == d.lr_at(t)
    assert a.param_groups[0]["lr"] == b.param_groups[0]["lr"] == cfg.TRAIN.MIN_LR


@pytest.mark.parametrize("name", ["cosine", "linear", "step", "multistep"])
def test_step_update_fills_the_lr_tensor_in_place(name):
    from vm_asr_amd.optim import build_scheduler
    opt = _opt(tensor=True)
    lr = opt.param_groups[0]["lr"]
    opt.param_groups[1]["lr"] = lr                                     # one tensor shared by the groups, as lr_to_device leaves it
    ptr = lr.data_ptr()
    s = build_scheduler(_config(name, multisteps=(20, 40), max_lr=5e-3), opt, N)
    for t in (0, 3, W, 30 * N, T - 1):
        s.step_update(t)
        assert all(g["lr"] is lr for g in opt.param_groups) and lr.data_ptr() == ptr
        assert float(lr) == pytest.approx(s.lr_at(t), rel=1e-6)        # (an fp32 tensor)


def test_bad_schedules_raise():
    from vm_asr_amd.optim import build_scheduler
    with pytest.raises(NotImplementedError, match="plateau"):
        build_scheduler(_config("plateau"), _opt(), N)
    with pytest.raises(ValueError, match="MULTISTEPS"):
        build_scheduler(_config("multistep", multisteps=()), _opt(), N)
    with pytest.raises(ValueError, match="first milestone"):
        build_scheduler(_config("multistep", multisteps=(5, 40)), _opt(), N)      # W = 70 updates > 5 * 7
    build_scheduler(_config("multistep", multisteps=(10, 40)), _opt(), N)         # W == the first milestone: allowed (the reference's <=)


def test_main_builds_its_schedule_through_build_scheduler():
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "main.py")).read()
    assert "build_scheduler(config, o, steps)" in src and "CosineWarmupScheduler(" not in src


# ---- SGD, the CPU half ---------------------------------------------------------------------------------------------------------------
def _net(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.LayerNorm(4), torch.nn.Linear(4, 3))


def _backward(net, seed):
    g = torch.Generator().manual_seed(seed)
    net.zero_grad()
    net(torch.randn(6, 5, generator=g)).square().sum().backward()


def test_capturable_sgd_keeps_one_lr_tensor_and_follows_the_schedule_eagerly():
    """build_optimizer(capturable=True) for sgd: one fp32 lr tensor shared by the groups, and optimizer.step() reads it at every step
    (against a float-lr twin whose lr the same schedule sets)."""
    from vm_asr_amd.optim import build_optimizer, build_scheduler, lr_to_device
    cfg = _config("step", optimizer="sgd", max_lr=5e-3)
    cfg.TRAIN.WEIGHT_DECAY = 0.05
    a, b = _net(), _net()
    oa, ob = build_optimizer(cfg, a, capturable=True), build_optimizer(cfg, b, capturable=False)
    assert type(ob) is torch.optim.SGD and isinstance(ob.param_groups[0]["lr"], float) and ob.defaults["foreach"] is None
    assert ob.defaults["nesterov"] and ob.defaults["momentum"] == cfg.TRAIN.OPTIMIZER.MOMENTUM
    lr = oa.param_groups[0]["lr"]
    assert torch.is_tensor(lr) and lr.dtype == torch.float32 and all(g["lr"] is lr for g in oa.param_groups)
    lr_to_device(oa, torch.device("cpu"))
    lr = oa.param_groups[0]["lr"]
    assert torch.is_tensor(lr) and lr.dtype == torch.float32 and all(g["lr"] is lr for g in oa.param_groups)
    sa, sb = build_scheduler(cfg, oa, N), build_scheduler(cfg, ob, N)
    for i, t in enumerate((0, 40, W, 30 * N)):
        sa.step_update(t)
        sb.step_update(t)
        ob.param_groups[0]["lr"] = ob.param_groups[1]["lr"] = float(lr)      # the twin steps with the fp32 value the tensor holds
        _backward(a, i)
        _backward(b, i)
        oa.step()
        ob.step()
        for p, q in zip(a.parameters(), b.parameters()):
            assert torch.allclose(p, q, rtol=1e-6, atol=1e-8)
    assert oa.param_groups[0]["lr"] is lr


def test_sgd_state_round_trips_into_a_plain_sgd_and_back():
    from vm_asr_amd.optim import build_optimizer, load_optimizer_state, portable_optimizer_state, set_weight_decay
    cfg = _config("cosine", optimizer="sgd")
    cfg.TRAIN.WEIGHT_DECAY = 0.05
    a = _net()
    oa = build_optimizer(cfg, a, capturable=True)
    for i in range(2):
        _backward(a, i)
        oa.step()
    sd = portable_optimizer_state(oa)
    assert all(type(g["lr"]) is float and g["foreach"] is None and g.get("fused") is None for g in sd["param_groups"])
    assert all(set(st) == {"momentum_buffer"} for st in sd["state"].values()) and len(sd["state"]) == 6
    # the reference's optimiser (utils/optimizer.py:32-39) loads it and continues like ours
    b = copy.deepcopy(a)
    plain = torch.optim.SGD(set_weight_decay([b]), lr=cfg.TRAIN.BASE_LR, momentum=cfg.TRAIN.OPTIMIZER.MOMENTUM, nesterov=True,
                            weight_decay=cfg.TRAIN.WEIGHT_DECAY)
    plain.load_state_dict(copy.deepcopy(sd))
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(oa.state[p]["momentum_buffer"], plain.state[q]["momentum_buffer"])
    _backward(a, 7)
    _backward(b, 7)
    oa.step()
    plain.step()
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.allclose(p, q, rtol=1e-6, atol=1e-8)
        assert torch.allclose(oa.state[p]["momentum_buffer"], plain.state[q]["momentum_buffer"], rtol=1e-6, atol=1e-8)
    # and back: the plain optimiser's state into one of ours keeps OUR runtime flags and re-creates the shared lr tensor
    c = copy.deepcopy(b)
    oc = build_optimizer(cfg, c, capturable=True)
    load_optimizer_state(oc, plain.state_dict(), torch.device("cpu"))
    lr = oc.param_groups[0]["lr"]
    assert torch.is_tensor(lr) and lr.dtype == torch.float32 and all(g["lr"] is lr for g in oc.param_groups)
    assert float(lr) == pytest.approx(cfg.TRAIN.BASE_LR) and all(g["foreach"] is True for g in oc.param_groups)
    for q, r in zip(b.parameters(), c.parameters()):
        assert torch.equal(plain.state[q]["momentum_buffer"], oc.state[r]["momentum_buffer"])


def test_hip_sgd_knob(monkeypatch):
    from vm_asr_amd import knobs
    k = knobs.KNOBS["VMASR_HIP_SGD"]
    assert k.kind == "flag" and k.reader == "python:sgd"
    monkeypatch.delenv("VMASR_HIP_SGD", raising=False)
    assert knobs.get("VMASR_HIP_SGD") is True
    for raw, want in (("0", False), ("1", True)):
        monkeypatch.setenv("VMASR_HIP_SGD", raw)
        assert knobs.get("VMASR_HIP_SGD") is want
    monkeypatch.setenv("VMASR_HIP_SGD", "yes")
    with pytest.raises(ValueError, match="VMASR_HIP_SGD"):
        knobs.get("VMASR_HIP_SGD")
