"""Device-side gradient guard (csrc/gradnorm.hip): the global L2 norm of one optimiser's gradients, the clip coefficient of
torch.nn.utils.clip_grad_norm_ and a "some element is inf / NaN" flag, as device floats that the guarded AdamW launch
(fused_adamw.HipAdamWStep(guard=...)) reads.  It is the safety net the reference gets from its GradScaler (trainer/trainer.py:106-107,
428-438: `scaler.step()` leaves weights and moments alone when a gradient is not finite), without the loss scaling that bf16 does not
need: one guard per optimiser, as the reference has scaler_G and scaler_D.

Nothing here reads the device except `read()`: `measure()` is one library call and sits in the captured optimiser graph.
"""
import numpy as np
import torch

from . import _lib

__all__ = ["GradGuard"]

_SEG = np.dtype([("ptr", "u8"), ("n", "i8")])


class GradGuard:
    """tensors: the gradient tensors (fp32, contiguous; views into a flat buffer at any offset, or whole flat buffers) — or, with
    `params=True`, the parameters whose `.grad` they are: the table is then rebuilt from the current `.grad`s by `rebuild()` once
    `still_valid()` says they were re-bound.  `state` (fp32 on `device`) is created once and survives every rebuild:
    [0] norm, [1] clip coefficient min(1, max_norm / (norm + 1e-6)) (1 when max_norm is None or <= 0), [2] found_inf, [3] the running
    count of measure() calls that found a non-finite element (a float: exact up to 2^24), and [4] = 1 - found_inf, what the guarded
    AdamW step advances its counters by.  With an inf element the norm is inf and the coefficient 0: unused, the step is not taken.
    CPU tensors have no HIP path: measure() then forms the same values with torch, the norm from float64 sums of squares as the
    kernel does (the CPU trainer tests); GPU tensors go to the library only."""

    def __init__(self, tensors, device, max_norm=None, params=False):
        self.device = torch.device(device)
        self.max_norm = float(max_norm) if max_norm is not None and max_norm > 0 else 0.0
        self.state = torch.zeros(5, dtype=torch.float32, device=self.device)
        self._params = list(tensors) if params else None
        self._given = None if params else list(tensors)
        self._grads, self._ptrs = None, None
        if not params:
            self.rebuild()

    def _current(self):
        if self._params is None:
            return self._given
        return [p.grad for p in self._params if p.grad is not None]

    def rebuild(self):
        """(Re)build the segment and chunk tables from the gradient tensors as they are now (a host-to-device copy: outside any capture)."""
        grads = self._current()
        if not grads:
            raise ValueError("no gradient tensor to guard")
        for g in grads:
            if g.dtype != torch.float32 or not g.is_contiguous() or g.device.type != self.device.type:
                raise ValueError("a gradient tensor does not qualify (fp32, contiguous, on the guard's device)")
        self._grads = grads
        self._ptrs = [(g.data_ptr(), g.numel()) for g in grads]
        if self.device.type != "cuda":
            return
        lib = _lib.lib()
        chunk = lib.vmasr_adamw_chunk()
        segs = [(q, n) for q, n in self._ptrs if n > 0]
        chunks = [(i, c) for i, (_, n) in enumerate(segs) for c in range(-(-n // chunk))]
        if not chunks:
            raise ValueError("no gradient element to guard")
        self.nchunks, self.total = len(chunks), sum(n for _, n in segs)
        self.segments = torch.from_numpy(np.array(segs, dtype=_SEG).view(np.uint8).copy()).to(self.device)
        self.chunks = torch.tensor(chunks, dtype=torch.int32, device=self.device).contiguous()
        self.ws_bytes = int(lib.vmasr_grad_norm_workspace(self.nchunks))
        self.workspace = torch.empty(-(-self.ws_bytes // 8), dtype=torch.float64, device=self.device)

    def still_valid(self):
        """The table holds raw pointers: stale once a `.grad` was re-bound (a new flat buffer, zero_grad(set_to_none))."""
        if self._ptrs is None:
            return False
        cur = self._current()
        return len(cur) == len(self._ptrs) and all(g.data_ptr() == q and g.numel() == n for g, (q, n) in zip(cur, self._ptrs))

    @torch.no_grad()
    def measure(self):
        """Fill `state` from the gradients: one library call (two launches), no host read, capturable."""
        if self.device.type == "cuda":
            _lib.call(_lib.lib().vmasr_grad_norm, self.segments, self.chunks, self.nchunks, self.total, self.max_norm, self.state,
                      self.workspace, self.ws_bytes, device=self.device)
            return
        grads = self._grads
        norm = torch.sqrt(torch.stack([g.double().square().sum() for g in grads]).sum()).float()      # fp64 sums, one rounding
        found = torch.stack([(~torch.isfinite(g)).any() for g in grads]).any().float()      # per element, not from the norm
        coef = torch.ones(())
        if self.max_norm > 0:
            coef = torch.clamp(self.max_norm / (norm + 1e-6), max=1.0)
            coef = torch.where(torch.isnan(coef), torch.ones(()), coef)
        self.state[0], self.state[1], self.state[2], self.state[4] = norm, coef, found, 1.0 - found
        self.state[3] += found

    @torch.no_grad()
    def clip_(self):
        """The measured gradients times the device coefficient, in place (one multi-tensor multiply): the optimizer.step() route,
        which calls it only for a step it takes (with an inf element the coefficient is 0 and would turn that element into NaN).
        (The guarded AdamW launch applies the coefficient as it reads and leaves the gradients alone.)"""
        torch._foreach_mul_(self._grads, self.state[1])

    def found_inf(self):
        """ONE host read of the flag (what GradScaler's unfused route does before it decides to call optimizer.step())."""
        return bool(self.state[2].item() != 0.0)

    def read(self):
        """The one host read of all the values."""
        n, c, f, k, _ = self.state.tolist()
        return {"grad_norm": n, "clip_coef": c, "found_inf": bool(f), "skipped": int(k)}
