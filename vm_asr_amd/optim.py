"""Optimisers, the learning-rate schedules and the optimiser half of a checkpoint, independent of any trainer:
the reference's utils/optimizer.py:16-77 and utils/lr_scheduler.py:15-188, plus what a HIP-graph replayed optimiser step
needs — one device learning-rate tensor, and optimiser state that any torch.optim.AdamW / SGD loads.
`unwrap` lives here because this module imports nothing of the package but `knobs` (trainer.py, grad_sync.py and
tester.py all need it)."""
import bisect
import math

import torch
from torch.nn.parallel import DistributedDataParallel as DDP

from . import knobs

__all__ = ["unwrap", "set_weight_decay", "build_optimizer", "CosineWarmupScheduler", "LinearWarmupScheduler", "StepWarmupScheduler",
           "MultiStepWarmupScheduler", "build_scheduler", "lr_to_device", "portable_optimizer_state", "load_optimizer_state"]


def unwrap(m):
    return m.module if isinstance(m, DDP) else m


def set_weight_decay(models):
    """1-D tensors, biases and `_no_weight_decay` params get weight_decay 0 (utils/optimizer.py:53-77)."""
    decay, no_decay = [], []
    for model in models:
        for name, p in unwrap(model).named_parameters():
            if not p.requires_grad:
                continue
            (no_decay if (p.ndim == 1 or name.endswith(".bias") or getattr(p, "_no_weight_decay", False))
             else decay).append(p)
    return [{"params": decay}, {"params": no_decay, "weight_decay": 0.0}]


def build_optimizer(config, models, capturable=False):
    if not isinstance(models, (list, tuple)):
        models = [models]
    groups = set_weight_decay(models)
    name = config.TRAIN.OPTIMIZER.NAME.lower()
    if name == "adamw":
        on_gpu = any(p.is_cuda for g in groups for p in g["params"])
        # capturable: the learning rate is a DEVICE tensor the fused kernel reads at run time, so the schedule keeps
        # working when the step is replayed from a HIP graph (a CPU tensor is read with .item() at capture and
        # frozen into the graph); lr_to_device() re-establishes this after .to(device) / load_state_dict
        dev = next((p.device for g in groups for p in g["params"]), torch.device("cpu"))
        lr = torch.tensor(float(config.TRAIN.BASE_LR), device=dev) if capturable else config.TRAIN.BASE_LR
        # fused: one multi-tensor kernel per step instead of ~10 foreach passes over 44 M parameters
        extra = dict(fused=True) if (capturable and on_gpu and knobs.get("VMASR_FUSED_ADAMW")) \
            else dict(foreach=True if capturable else None)
        return torch.optim.AdamW(groups, lr=lr, eps=config.TRAIN.OPTIMIZER.EPS,
                                 betas=tuple(config.TRAIN.OPTIMIZER.BETAS), weight_decay=config.TRAIN.WEIGHT_DECAY,
                                 capturable=capturable, **extra)
    if name == "sgd":
        if capturable:
            # torch's SGD has no capturable flag; the device lr tensor is the mark (_keeps_device_lr).  The one-launch HIP step
            # (fused_sgd.HipSgdStep) reads it on the device.  optimizer.step() stays correct with it through the multi-tensor
            # implementation, which reads the tensor with .item() at EVERY step (a schedule update is seen; one host sync per step,
            # which is why graph_step never captures it) and accepts a state in which only some parameters have a buffer yet —
            # the fused implementation decides "first step" for the whole list at once.
            dev = next((p.device for g in groups for p in g["params"]), torch.device("cpu"))
            return torch.optim.SGD(groups, lr=torch.tensor(float(config.TRAIN.BASE_LR), device=dev), momentum=config.TRAIN.OPTIMIZER.MOMENTUM,
                                   nesterov=True, weight_decay=config.TRAIN.WEIGHT_DECAY, foreach=True)
        return torch.optim.SGD(groups, lr=config.TRAIN.BASE_LR, momentum=config.TRAIN.OPTIMIZER.MOMENTUM,
                               nesterov=True, weight_decay=config.TRAIN.WEIGHT_DECAY)
    raise NotImplementedError(name)


class CosineWarmupScheduler:
    """Linear warm-up from MIN_LR then one cosine cycle to MIN_LR, stepped per update
    (`step_update`), like the timm scheduler the reference configures (utils/lr_scheduler.py:15-41)."""

    def __init__(self, optimizer, total_steps, warmup_steps, base_lr, min_lr, warmup_prefix=True):
        self.opt, self.base_lr, self.min_lr = optimizer, base_lr, min_lr
        self.warm = max(0, int(warmup_steps))
        self.t_initial = max(1, int(total_steps - self.warm if warmup_prefix else total_steps))
        self.prefix = warmup_prefix
        self.step_update(0)

    def lr_at(self, t):
        if t < self.warm:
            return self.min_lr + (self.base_lr - self.min_lr) * t / max(1, self.warm)
        tt = t - self.warm if self.prefix else t
        if tt >= self.t_initial:
            return self.min_lr
        return self.min_lr + 0.5 * (self.base_lr - self.min_lr) * (1 + math.cos(math.pi * tt / self.t_initial))

    def step_update(self, num_updates):
        lr, done = self.lr_at(num_updates), set()
        for g in self.opt.param_groups:
            if torch.is_tensor(g["lr"]):
                if g["lr"].data_ptr() not in done:      # capturable optimisers keep ONE lr tensor on the device
                    g["lr"].fill_(lr)
                    done.add(g["lr"].data_ptr())
            else:
                g["lr"] = lr


class _WarmupScheduler(CosineWarmupScheduler):
    """The reference's other three schedules (utils/lr_scheduler.py:52-188; timm's StepLRScheduler for "step"), stepped per update:
    a linear warm-up over `warmup_steps` updates from `warmup_lr` — the reference passes TRAIN.MAX_LR there — to `base_lr`, then
    `_after(t)`.  Same interface as the cosine schedule, and the same `step_update`: an existing lr tensor is filled, never replaced."""

    def __init__(self, optimizer, warmup_steps, base_lr, warmup_lr):
        self.opt, self.base_lr, self.warmup_lr = optimizer, float(base_lr), float(warmup_lr)
        self.warm = max(0, int(warmup_steps))
        self.step_update(0)

    def lr_at(self, t):
        if t < self.warm:
            return self.warmup_lr + t * (self.base_lr - self.warmup_lr) / self.warm
        return self._after(t)


class LinearWarmupScheduler(_WarmupScheduler):
    """t >= W: from base_lr down to 0.01 base_lr at t = total_steps, linear in t - W (LinearLRScheduler, lr_min_rate 0.01)."""

    def __init__(self, optimizer, total_steps, warmup_steps, base_lr, warmup_lr, min_rate=0.01):
        self.total, self.min_rate = int(total_steps), float(min_rate)
        super().__init__(optimizer, warmup_steps, base_lr, warmup_lr)

    def _after(self, t):
        b = self.base_lr
        return b - (b - b * self.min_rate) * (t - self.warm) / (self.total - self.warm)


class StepWarmupScheduler(_WarmupScheduler):
    """t >= W: base_lr * decay_rate ** (t // decay_steps); t is NOT shifted by the warm-up (timm's StepLRScheduler)."""

    def __init__(self, optimizer, decay_steps, decay_rate, warmup_steps, base_lr, warmup_lr):
        self.decay_steps, self.decay_rate = int(decay_steps), float(decay_rate)
        if self.decay_steps <= 0:
            raise ValueError(f"step schedule: DECAY_EPOCHS x updates per epoch = {decay_steps!r} is not a positive number of updates")
        super().__init__(optimizer, warmup_steps, base_lr, warmup_lr)

    def _after(self, t):
        return self.base_lr * self.decay_rate ** (t // self.decay_steps)


class MultiStepWarmupScheduler(_WarmupScheduler):
    """t >= W: base_lr * gamma ** (number of milestones <= t) (MultiStepLRScheduler).  No milestone, or a warm-up that ends behind the
    first one, raises ValueError (the reference asserts the latter and fails in min() on the former)."""

    def __init__(self, optimizer, milestones, gamma, warmup_steps, base_lr, warmup_lr):
        self.milestones, self.gamma = sorted(milestones), float(gamma)
        if not self.milestones:
            raise ValueError("multistep schedule: TRAIN.LR_SCHEDULER.MULTISTEPS is empty")
        if max(0, int(warmup_steps)) > self.milestones[0]:
            raise ValueError(f"multistep schedule: the warm-up ({int(warmup_steps)} updates) ends behind the first milestone "
                             f"({self.milestones[0]})")
        super().__init__(optimizer, warmup_steps, base_lr, warmup_lr)

    def _after(self, t):
        return self.base_lr * self.gamma ** bisect.bisect_right(self.milestones, t)


def build_scheduler(config, optimizer, n_iter_per_epoch):
    """The schedule TRAIN.LR_SCHEDULER.NAME asks for (utils/lr_scheduler.py:15-79), stepped per update: T = int(EPOCHS * n) updates in
    all, W = int(WARMUP_EPOCHS * n) of warm-up.  cosine warms up from MIN_LR, the other three from MAX_LR, as the reference does."""
    t, n = config.TRAIN, n_iter_per_epoch
    total, warm = int(t.EPOCHS * n), int(t.WARMUP_EPOCHS * n)
    name = t.LR_SCHEDULER.NAME
    if name == "cosine":
        return CosineWarmupScheduler(optimizer, t.EPOCHS * n, t.WARMUP_EPOCHS * n, t.BASE_LR, t.MIN_LR, t.LR_SCHEDULER.WARMUP_PREFIX)
    if name == "linear":
        return LinearWarmupScheduler(optimizer, total, warm, t.BASE_LR, t.MAX_LR)
    if name == "step":
        return StepWarmupScheduler(optimizer, int(t.LR_SCHEDULER.DECAY_EPOCHS * n), t.LR_SCHEDULER.DECAY_RATE, warm, t.BASE_LR, t.MAX_LR)
    if name == "multistep":
        return MultiStepWarmupScheduler(optimizer, [m * n for m in t.LR_SCHEDULER.MULTISTEPS], t.LR_SCHEDULER.GAMMA, warm, t.BASE_LR, t.MAX_LR)
    raise NotImplementedError(f"TRAIN.LR_SCHEDULER.NAME {name!r}: expected cosine, linear, step or multistep")


def _keeps_device_lr(optimizer):
    """Built by build_optimizer(..., capturable=True)?  AdamW says so itself; torch's SGD has no such flag, there the tensor lr it
    was constructed with is the mark (`defaults` survives load_state_dict, which turns the groups' lr back into floats)."""
    return bool(optimizer.defaults.get("capturable", False)
                or (isinstance(optimizer, torch.optim.SGD) and torch.is_tensor(optimizer.defaults.get("lr"))))


def lr_to_device(optimizer, device):
    """Capturable optimisers: every param group shares one lr tensor that lives on `device` (see build_optimizer).
    Needed after the models moved to the GPU and after `optimizer.load_state_dict` (which restores a CPU value)."""
    if optimizer is None or not _keeps_device_lr(optimizer):
        return
    shared = {}
    for g in optimizer.param_groups:
        v = float(g["lr"])
        if v not in shared:
            shared[v] = torch.tensor(v, dtype=torch.float32, device=device)
        g["lr"] = shared[v]


_RUNTIME_GROUP_KEYS = ("capturable", "fused", "foreach", "differentiable")


def portable_optimizer_state(optimizer):
    """optimizer.state_dict() in the form ANY torch.optim.AdamW (SGD for an SGD state) accepts — in particular the reference's plain
    one (main.py:168-201 builds it non-fused, non-capturable, float lr): `lr` as a Python float, the runtime flags of this
    package's optimisers (capturable / fused / foreach) reset to their defaults, `step` counters as CPU tensors.  An SGD state is
    torch's own already (`momentum_buffer` per parameter, which load_state_dict puts next to the parameters).
    `load_optimizer_state` below is the inverse for an optimiser built by build_optimizer()."""
    sd = optimizer.state_dict()
    groups = []
    for g in sd["param_groups"]:
        g = dict(g)
        g["lr"] = float(g["lr"])
        if "capturable" in g:
            g["capturable"] = False
        for k in ("fused", "foreach"):
            if k in g:
                g[k] = None
        groups.append(g)
    state = {pid: {k: (v.detach().cpu() if (k == "step" and torch.is_tensor(v)) else v) for k, v in st.items()}
             for pid, st in sd["state"].items()}
    return {"state": state, "param_groups": groups}


def load_optimizer_state(optimizer, state_dict, device):
    """optimizer.load_state_dict that keeps THIS optimiser's runtime flags (a checkpoint — ours or the reference's —
    carries its writer's), puts the step counters where a capturable optimiser needs them and re-creates the shared
    device learning-rate tensor."""
    keep = [{k: g[k] for k in _RUNTIME_GROUP_KEYS if k in g} for g in optimizer.param_groups]
    optimizer.load_state_dict(state_dict)
    for g, k in zip(optimizer.param_groups, keep):
        g.update(k)
    if optimizer.defaults.get("capturable", False):
        for st in optimizer.state.values():
            if "step" in st:
                st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).to(device)
    lr_to_device(optimizer, device)
