"""One-launch SGD (momentum / Nesterov) step on the HIP library (csrc/sgd.hip) over the state of an ordinary torch.optim.SGD.

The sibling of fused_adamw.HipAdamWStep.  The optimiser object stays the owner of its state (`momentum_buffer` per parameter):
checkpoints keep torch's `state_dict` layout, interchangeable with the reference's SGD runs (utils/optimizer.py:32-39,
base/base_trainer.py:130-179).  This class only replaces `optimizer.step()`: a device table of (param, grad, momentum_buffer, bf16
shadow) pointers built once, then one kernel per step that reads the learning rate from the device — which torch's own SGD
implementations do not: the multi-tensor one reads a tensor lr with `.item()`, so a captured torch step would freeze the schedule.
"""
import numpy as np
import torch

from . import _lib

__all__ = ["HipSgdStep"]

_ITEM = np.dtype([("p", "u8"), ("g", "u8"), ("buf", "u8"), ("lp", "u8"), ("lpt", "u8"), ("n", "i8"), ("wd", "f4"), ("vec", "i4"),
                  ("rows", "i4"), ("cols", "i4")])


class HipSgdStep:
    """step() == optimizer.step() for a torch.optim.SGD with dampening 0 and maximize off whose param groups share momentum, nesterov
    and ONE fp32 device learning-rate tensor (optim.build_optimizer(..., capturable=True) / optim.lr_to_device), and whose parameters'
    `.grad` are fixed tensors (the trainer's flat gradient buffers).  Raises ValueError if the optimiser does not qualify.

    A parameter that has a gradient and no `momentum_buffer` yet gets a ZERO buffer here, stored in
    `optimizer.state[p]["momentum_buffer"]`.  torch's first step sets buf = g' (= g + wd p) instead; with dampening 0 the kernel's
    buf = momentum * 0 + g' is the same float, so the first step needs no case of its own, no torch step has to run before a graph
    capture, and a state created here continues under torch's SGD (and the reverse) without a seam.

    `shadows`: {id(param): bf16 tensor} refreshed in the same pass; `shadows_t`: {id(2-D param): bf16 tensor of the transposed shape},
    likewise.  `guard`: a grad_guard.GradGuard measured over the same gradients just before step(): the launch then scales every
    gradient element by the guard's clip coefficient as it reads it, and takes no step at all — weights, buffers and shadows stay
    bit-identical — when the guard found a non-finite element, without a host read."""

    @staticmethod
    def check(optimizer):
        """The part of the admission that needs no gradient (graph_step asks before anything runs): -> (lr tensor, momentum, nesterov)."""
        if not isinstance(optimizer, torch.optim.SGD):
            raise ValueError("not an SGD")
        groups = optimizer.param_groups
        g0 = groups[0]
        if any(g["dampening"] != 0 or g["maximize"] for g in groups):
            raise ValueError("needs SGD with dampening 0 and maximize off")
        if any(g["momentum"] != g0["momentum"] or bool(g["nesterov"]) != bool(g0["nesterov"]) for g in groups):
            raise ValueError("param groups differ in momentum / nesterov")
        if not 0.0 <= float(g0["momentum"]) < 1.0:
            raise ValueError("momentum outside [0, 1)")
        lr = g0["lr"]
        if not (torch.is_tensor(lr) and lr.is_cuda and lr.numel() == 1 and all(g["lr"] is lr for g in groups)):
            raise ValueError("needs ONE device learning-rate tensor shared by the param groups (optim.lr_to_device)")
        if lr.dtype != torch.float32:
            raise ValueError("learning-rate tensor must be float32")
        for g in groups:
            for p in g["params"]:
                if not (p.is_cuda and p.device == lr.device and p.dtype == torch.float32 and p.is_contiguous()):
                    raise ValueError("a parameter does not qualify (dtype, device or layout)")
        return lr, float(g0["momentum"]), bool(g0["nesterov"])

    def __init__(self, optimizer, shadows=None, shadows_t=None, guard=None):
        self.lr, self.momentum, self.nesterov = self.check(optimizer)
        dev = self.lr.device
        if guard is not None and (guard.state.device != dev or guard.state.dtype != torch.float32):
            raise ValueError("the gradient guard's state is not an fp32 tensor on the optimiser's device")
        shadows, shadows_t = shadows or {}, shadows_t or {}
        chunk = _lib.lib().vmasr_adamw_chunk()
        items, chunks, keep, fresh = [], [], [], []
        for g in optimizer.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue                                   # never-used parameters: torch skips them too
                buf, lp, lpt = optimizer.state.get(p, {}).get("momentum_buffer"), shadows.get(id(p)), shadows_t.get(id(p))
                if buf is None:
                    buf = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    fresh.append((p, buf))
                ok = (p.grad.is_cuda and p.grad.device == dev and p.grad.dtype == torch.float32 and p.grad.is_contiguous()
                      and p.grad.shape == p.shape and torch.is_tensor(buf) and buf.device == dev and buf.dtype == torch.float32
                      and buf.is_contiguous() and buf.shape == p.shape
                      and (lp is None or (lp.is_contiguous() and lp.dtype == torch.bfloat16 and lp.shape == p.shape and lp.device == dev)))
                if not ok:
                    raise ValueError("a gradient / state / shadow tensor does not qualify (dtype, device or layout)")
                if lpt is not None and not (p.dim() == 2 and lpt.is_contiguous() and lpt.dtype == torch.bfloat16 and lpt.device == dev
                                            and tuple(lpt.shape) == (p.shape[1], p.shape[0])):
                    raise ValueError("a transposed shadow does not match its parameter")
                ptrs = (p.data_ptr(), p.grad.data_ptr(), buf.data_ptr())
                vec = all(q % 16 == 0 for q in ptrs) and (lp is None or lp.data_ptr() % 8 == 0)
                idx = len(items)
                items.append((*ptrs, lp.data_ptr() if lp is not None else 0, lpt.data_ptr() if lpt is not None else 0, p.numel(),
                              float(g["weight_decay"]), int(vec), p.shape[0] if lpt is not None else 0, p.shape[1] if lpt is not None else 0))
                chunks.extend((idx, c) for c in range(-(-p.numel() // chunk)))
                keep.append((p, p.grad, buf, (lp, lpt)))
        if not chunks:
            raise ValueError("no parameter with a gradient")
        for p, buf in fresh:                                   # only once every tensor qualified: a refused optimiser keeps its state
            optimizer.state[p]["momentum_buffer"] = buf
        self._skipped = [p for g in optimizer.param_groups for p in g["params"] if p.grad is None]
        self.items = torch.from_numpy(np.array(items, dtype=_ITEM).view(np.uint8).copy()).to(dev)
        self.chunks = torch.tensor(chunks, dtype=torch.int32, device=dev).contiguous()
        self.nchunks, self.total = len(chunks), sum(it[5] for it in items)
        self._keep, self._ptrs = keep, [it[:3] for it in items]
        self.optimizer, self.guard = optimizer, guard

    def still_valid(self):
        """The table holds raw pointers: it is stale once a parameter's .grad was re-bound (zero_grad(set_to_none), a new flat buffer),
        a momentum buffer was replaced (load_state_dict creates new tensors) or the learning-rate tensor was (lr_to_device)."""
        state = self.optimizer.state
        if any(g["lr"] is not self.lr for g in self.optimizer.param_groups):
            return False
        if any(p.grad is not None for p in self._skipped):
            return False                                  # a parameter that had no gradient at build time has one now
        for (p, _, _, _), (pp, gp, bp) in zip(self._keep, self._ptrs):
            buf = state.get(p, {}).get("momentum_buffer")
            if p.grad is None or buf is None or p.data_ptr() != pp or p.grad.data_ptr() != gp or buf.data_ptr() != bp:
                return False
        return True

    @torch.no_grad()
    def step(self):
        lib = _lib.lib()
        if self.guard is not None:
            _lib.call(lib.vmasr_sgd_step_guarded, self.items, self.chunks, self.nchunks, self.total, self.lr, self.momentum,
                      int(self.nesterov), self.guard.state, device=self.lr.device)
            return
        _lib.call(lib.vmasr_sgd_step, self.items, self.chunks, self.nchunks, self.total, self.lr, self.momentum, int(self.nesterov),
                  device=self.lr.device)
