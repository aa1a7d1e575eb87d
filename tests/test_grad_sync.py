"""grad_sync.FlatGrads on the host (no GPU, no process group): the flat buffer's layout, the two ways gradients reach it (packed
after each backward / accumulated in place), the backward targets, and what a one-rank reduce does to the buffer."""
import pytest
import torch


class _Net(torch.nn.Module):
    """Three parameters; `unused` takes no part in the forward and never receives a gradient."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.w = torch.nn.Parameter(torch.randn(3, 4, generator=g))
        self.b = torch.nn.Parameter(torch.randn(3, generator=g))
        self.unused = torch.nn.Parameter(torch.randn(7, generator=g))

    def forward(self, x):
        return (x @ self.w.t() + self.b).square().sum()


def _x(seed):
    return torch.randn(5, 4, generator=torch.Generator().manual_seed(seed))


def _grads(gather=True, keys=("generator",), world=1):
    from vm_asr_amd.grad_sync import FlatGrads
    models = {k: _Net() for k in keys}
    return FlatGrads(models, torch.device("cpu"), world, "flat", gather), models


def _same(a, b):
    return len(a) == len(b) and all(x is y for x, y in zip(a, b))


def _is_view(p, flat, offset):
    g = p.grad
    return (g is not None and g.shape == p.shape and g.is_contiguous()
            and g.data_ptr() == flat.data_ptr() + 4 * offset and g.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr())


def test_setup_packs_the_used_parameters_only():
    fg, models = _grads()
    net = models["generator"]
    assert _same(fg.targets("generator"), [net.w, net.b, net.unused])         # before setup: everything that requires a gradient
    net(_x(1)).backward()
    want = torch.cat([net.w.grad.flatten(), net.b.grad.flatten()]).clone()
    flat = fg.setup("generator")
    assert flat is fg.flat["generator"] and flat.dtype == torch.float32 and flat.numel() == net.w.numel() + net.b.numel() == 15
    assert _is_view(net.w, flat, 0) and _is_view(net.b, flat, net.w.numel()) and net.unused.grad is None
    assert torch.equal(flat, want)
    assert _same(fg.params["generator"], [net.w, net.b]) and _same(fg.targets("generator"), [net.w, net.b])
    assert [v.data_ptr() for v in fg.views["generator"]] == [net.w.grad.data_ptr(), net.b.grad.data_ptr()]


def test_gather_mode_packs_fresh_gradients_into_the_views():
    fg, models = _grads(gather=True)
    net, opt = models["generator"], None
    net(_x(1)).backward()
    flat = fg.setup("generator")
    fg.zero("generator", opt)
    assert net.w.grad is None and net.b.grad is None
    net(_x(2)).backward()
    fresh = [net.w.grad.clone(), net.b.grad.clone()]
    assert not _is_view(net.w, flat, 0)                                    # autograd handed over tensors of its own
    fg.gather("generator")
    assert _is_view(net.w, flat, 0) and _is_view(net.b, flat, 12) and net.unused.grad is None
    assert torch.equal(net.w.grad, fresh[0]) and torch.equal(net.b.grad, fresh[1])
    assert torch.equal(flat, torch.cat([f.flatten() for f in fresh]))
    # a parameter whose gradient stayed None (no backward reached it): a zeroed view
    fg.zero("generator", opt)
    (net.w.sum() * 2.0).backward()
    fg.gather("generator")
    assert _is_view(net.b, flat, 12) and torch.equal(net.b.grad, torch.zeros(3)) and torch.equal(net.w.grad, torch.full((3, 4), 2.0))


def test_zero_before_setup_goes_through_the_optimizer():
    fg, models = _grads()
    net = models["generator"]
    calls = []

    class Opt:      # (stands in for torch.optim: importing an optimiser costs this file's whole run time again)
        def zero_grad(self, set_to_none):
            calls.append(set_to_none)
    net(_x(1)).backward()
    fg.zero("generator", Opt())
    assert calls == [True]
    fg.gather("generator")                                                 # no buffer yet: nothing to pack
    assert "generator" not in fg.flat


def test_accumulate_mode_sums_in_place():
    fg, models = _grads(gather=False)
    net = models["generator"]
    net(_x(1)).backward()
    first = torch.cat([net.w.grad.flatten(), net.b.grad.flatten()]).clone()
    flat = fg.setup("generator")
    fg.zero("generator", None)
    assert torch.equal(flat, torch.zeros(15)) and _is_view(net.w, flat, 0) and _is_view(net.b, flat, 12)
    net(_x(1)).backward()
    fg.gather("generator")                                                 # (nothing to pack in this mode)
    assert torch.equal(flat, first) and _is_view(net.w, flat, 0) and _is_view(net.b, flat, 12)
    ref = _Net()
    ref(_x(2)).backward()
    second = torch.cat([ref.w.grad.flatten(), ref.b.grad.flatten()])
    net(_x(2)).backward()
    assert torch.equal(flat, first + second) and _is_view(net.w, flat, 0) and _is_view(net.b, flat, 12)
    assert net.unused.grad is None


def _filled(keys):
    """Buffers holding values that bf16 cannot represent."""
    fg, models = _grads(keys=keys)
    for k in keys:
        models[k](_x(3)).backward()
        fg.setup(k).mul_(1.0 + 2.0 ** -12)
        assert not torch.equal(fg.flat[k], fg.flat[k].to(torch.bfloat16).float())
    return fg


def test_one_rank_reduce_leaves_the_buffer_alone(monkeypatch):
    monkeypatch.delenv("VMASR_GRAD_COMM_EMULATE", raising=False)
    monkeypatch.delenv("VMASR_GRAD_COMM", raising=False)
    fg = _filled(("generator", "mpd"))
    before = {k: v.clone() for k, v in fg.flat.items()}
    for k in ("mpd", "generator"):
        fg.reduce(k, async_op=True)
    fg.wait()
    assert fg._pending == [] and all(torch.equal(fg.flat[k], before[k]) for k in before)
    for mode in ("fp32", "mpd-bf16", "bf16"):
        monkeypatch.setenv("VMASR_GRAD_COMM", mode)
        assert fg.comm_dtype("generator") == torch.float32 and fg.comm_dtype("mpd") == torch.float32      # the 16-bit wire is RCCL's


@pytest.mark.parametrize("mode, rounded", [("bf16", ("generator", "mpd")), ("mpd-bf16", ("mpd",))])
def test_one_rank_reduce_emulates_the_bf16_wire(monkeypatch, mode, rounded):
    monkeypatch.setenv("VMASR_GRAD_COMM_EMULATE", mode)
    fg = _filled(("generator", "mpd"))
    before = {k: v.clone() for k, v in fg.flat.items()}
    for k in ("mpd", "generator"):
        fg.reduce(k, async_op=True)
    fg.wait()
    assert fg._pending == []
    for k in before:
        assert torch.equal(fg.flat[k], before[k].to(torch.bfloat16).float() if k in rounded else before[k]), k
