"""Optimisers, the learning-rate schedule and the optimiser half of a checkpoint, independent of any trainer:
the reference's utils/optimizer.py:16-77 and utils/lr_scheduler.py:15-41, plus what a capturable (HIP-graph replayed)
AdamW needs — one device learning-rate tensor, and optimiser state that any torch.optim.AdamW loads.
`unwrap` lives here because this module imports nothing of the package but `knobs` (trainer.py, grad_sync.py and
tester.py all need it)."""
import math

import torch
from torch.nn.parallel import DistributedDataParallel as DDP

from . import knobs

__all__ = ["unwrap", "set_weight_decay", "build_optimizer", "CosineWarmupScheduler", "lr_to_device",
           "portable_optimizer_state", "load_optimizer_state"]


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


def lr_to_device(optimizer, device):
    """Capturable optimisers: every param group shares one lr tensor that lives on `device` (see build_optimizer).
    Needed after the models moved to the GPU and after `optimizer.load_state_dict` (which restores a CPU value)."""
    if optimizer is None or not optimizer.defaults.get("capturable", False):
        return
    shared = {}
    for g in optimizer.param_groups:
        v = float(g["lr"])
        if v not in shared:
            shared[v] = torch.tensor(v, dtype=torch.float32, device=device)
        g["lr"] = shared[v]


_RUNTIME_GROUP_KEYS = ("capturable", "fused", "foreach", "differentiable")


def portable_optimizer_state(optimizer):
    """optimizer.state_dict() in the form ANY torch.optim.AdamW accepts — in particular the reference's plain one
    (main.py:168-201 builds it non-fused, non-capturable, float lr): `lr` as a Python float, the runtime flags of this
    package's optimisers (capturable / fused / foreach) reset to their defaults, `step` counters as CPU tensors.
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
