"""The data-parallel gradient transport of dp_mode "flat": every model's gradients live in ONE flat fp32 buffer, which one
collective per model per step all-reduces over RCCL / xGMI (few large messages suit the point-to-point links, and the step
stays HIP-graph capturable).  `FlatGrads` owns the buffers, the views the parameters' `.grad` point into, the optional
bf16 wire copies and the in-flight collectives; a Trainer holds one as `trainer.grads` and decides only WHEN to call it.
"""
import torch
import torch.distributed as dist

from . import knobs
from .optim import unwrap

__all__ = ["FlatGrads"]


class _StreamWork:
    """The join handle of a collective issued on a stream of ours: wait() = the current stream waits for its event."""

    def __init__(self, event, device):
        self.event, self.device = event, device

    def wait(self):
        torch.cuda.current_stream(self.device).wait_event(self.event)


class FlatGrads:
    def __init__(self, models, device, world, dp_mode, gather):
        """models: the trainer's own dict (it replaces entries in place: DDP wrapping, .to(device)); gather: fresh gradients
        are packed into the buffer after each backward (no gradient accumulation) instead of being accumulated in place."""
        self.models, self.device, self.world, self.dp_mode, self._gather = models, device, world, dp_mode, gather
        self.flat, self.params, self.views = {}, {}, {}
        self._lp = {}                   # bf16 wire buffers (comm_dtype)
        self._pending = []              # in-flight gradient all-reduces (async work handles)
        self.time_reduces, self._reduce_events = False, []
        self._comm_st = None            # created on first use: an earlier stream can change the queue assignment
        self._direct_rccl = None

    def setup(self, key):
        """After a first backward: give every parameter that received a gradient a view into one
        flat fp32 buffer (never-used parameters keep grad None, as in the reference)."""
        model = unwrap(self.models[key])
        used = [p for p in model.parameters() if p.requires_grad and p.grad is not None]
        flat = torch.zeros(sum(p.numel() for p in used), dtype=torch.float32, device=self.device)
        off = 0
        for p in used:
            n = p.numel()
            view = flat[off:off + n].view_as(p)
            view.copy_(p.grad)
            p.grad = view
            off += n
        self.flat[key] = flat
        self.params[key] = used
        self.views[key] = [p.grad for p in used]
        return flat

    def zero(self, key, optimizer):
        """Before a backward.  With a flat buffer and no gradient accumulation the parameters' grads are
        dropped so that autograd hands over each gradient tensor as produced (no `grad += g` kernel per
        parameter: 640 launches a step); gather() then packs them into the flat buffer."""
        if key in self.flat:
            if self._gather:
                for p in self.params[key]:
                    p.grad = None
            else:
                self.flat[key].zero_()
        else:
            optimizer.zero_grad(set_to_none=True)

    def gather(self, key):
        """After a backward: multi-tensor copy of the fresh gradients into the flat buffer's views, which
        become the parameters' .grad again (what the all-reduce and the fused AdamW read)."""
        if key not in self.flat or not self._gather:
            return
        params, views = self.params[key], self.views[key]
        src, dst = [], []
        for p, v in zip(params, views):
            if p.grad is None:
                v.zero_()
            else:
                src.append(p.grad)
                dst.append(v)
            p.grad = v
        torch._foreach_copy_(dst, src)

    def targets(self, key):
        """The parameters a backward of `key`'s loss produces gradients for (`backward(inputs=...)`)."""
        if key in self.params:
            return self.params[key]
        return [p for p in unwrap(self.models[key]).parameters() if p.requires_grad]

    def comm_dtype(self, key):
        """Wire dtype of `key`'s gradient all-reduce.  VMASR_GRAD_COMM: "fp32" (default: what the reference's DDP sends, so N-rank and
        1-rank training agree to fp32 rounding) | "mpd-bf16": the period discriminator's 164 MB buffer travels as bf16 (82 MB; the
        fp32 flat buffer stays the optimiser's input, AdamW's moments and the weights stay fp32 — DDP's bf16 compression hook,
        SURVEY.md 8(e)), the generator's 9 MB as fp32 | "bf16": both.  The 16-bit wire is a NUMERICS CHANGE (3e-4 ... 9e-4 on the
        losses of one step) and is opt-in until a multi-GPU run has shown loss parity with the fp32 wire.  RCCL only: gloo is
        the CPU test backend."""
        mode = knobs.get("VMASR_GRAD_COMM")
        if mode not in ("bf16", "mpd-bf16") or self.device.type != "cuda" or dist.get_backend() != "nccl":
            return torch.float32
        return torch.bfloat16 if (mode == "bf16" or key != "generator") else torch.float32

    def reduce(self, key, async_op=False):
        """ONE all-reduce (mean) per model per step over RCCL/xGMI (generator 9 MB fp32, MPD 82 MB bf16 / 164 MB fp32).
        async_op: the call returns at once and the collective runs on RCCL's own stream, ordered after the CURRENT stream's work so
        far — the caller overlaps it with further work and joins it with wait() before the optimiser reads the gradients.
        Capturable (RCCL): inside a stream capture the collective becomes a branch of the graph."""
        emu = knobs.get("VMASR_GRAD_COMM_EMULATE") if self.world == 1 else None
        if emu and key in self.flat and (emu == "bf16" or (emu == "mpd-bf16" and key != "generator")):
            # one rank, no wire: the 16-bit wire's ROUNDING applied to this rank's own gradient (tools/wire_dtype_run.py compares the
            # loss curves of 200 steps with and without it — the numerics question of the bf16 wire, answerable without a second GPU)
            flat = self.flat[key]
            flat.copy_(flat.to(torch.bfloat16))
            return
        if self.world > 1 and self.dp_mode == "flat":
            if key not in self.flat:
                self.setup(key)
            flat = self.flat[key]
            if not knobs.get("VMASR_OVERLAP_REDUCE"):
                async_op = False                    # escape hatch: collectives strictly between the graphs, no overlap
            avg = dist.get_backend() == "nccl"      # RCCL averages in the collective; gloo has no AVG
            buf = flat
            if self.comm_dtype(key) != flat.dtype:
                lp = self._lp.get(key)
                if lp is None:                      # (allocated before any capture: GraphedTrainStep's warm-up steps reduce too)
                    lp = self._lp[key] = torch.empty_like(flat, dtype=self.comm_dtype(key))
                lp.copy_(flat)
                buf = lp
            if self._direct_rccl is not None and (torch.cuda.is_current_stream_capturing() or knobs.get("VMASR_RCCL_DIRECT")):
                # RCCL's C API on a stream of its own, forked from the current one (vm_asr_amd/rccl.py: the process group's watchdog
                # cannot live with captured collectives): a branch of the graph being captured
                cs, cur = self._comm_stream(), torch.cuda.current_stream(self.device)
                cs.wait_stream(cur)
                self._direct_rccl.all_reduce_(buf, avg=True, stream=cs)
                done = torch.cuda.Event()
                done.record(cs)
                self._pending.append((_StreamWork(done, self.device), flat, buf, False))
                return
            work = dist.all_reduce(buf, op=dist.ReduceOp.AVG if avg else dist.ReduceOp.SUM, async_op=async_op)
            self._pending.append((work if async_op else None, flat, buf, not avg))
            if not async_op:
                self.wait()

    def _comm_stream(self):
        if self._comm_st is None:
            self._comm_st = torch.cuda.Stream(self.device)
        return self._comm_st

    def enable_direct_rccl(self):
        """Create this trainer's own RCCL communicator (collective over the process group: every rank calls it, outside any capture)."""
        if self._direct_rccl is None:
            from .rccl import RcclComm
            self._direct_rccl = RcclComm(self.device)
            self._comm_stream()
        return self._direct_rccl

    def wait(self):
        """Join the pending collectives.  With `time_reduces` (bench.py, N > 1, collectives between the graphs) an event pair
        brackets the join on the compute stream: the time between them is what the collectives cost the step AFTER the overlap
        — the EXPOSED all-reduce time (`reduce_exposed_ms()`).  Inside a capture nothing is timed."""
        capturing = self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()
        timed = self.time_reduces and self.device.type == "cuda" and bool(self._pending) and not capturing
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        for work, flat, buf, divide in self._pending:
            if work is not None:
                work.wait()                # the current stream waits for the collective (no host block on RCCL)
            if buf is not flat:
                flat.copy_(buf)            # bf16 wire buffer -> the optimiser's fp32 gradients
            if divide:
                flat.div_(self.world)
        if timed:
            e1.record()
            self._reduce_events.append((e0, e1))
        self._pending = []

    def reduce_exposed_ms(self):
        """Sum of the bracketed join times since the last call (synchronises)."""
        torch.cuda.synchronize(self.device)
        ms = sum(a.elapsed_time(b) for a, b in self._reduce_events)
        self._reduce_events = []
        return ms
