"""The one-launch SGD step (csrc/sgd.hip, fused_sgd.HipSgdStep) on the GPU: against a float64 evaluation of torch's SGD recurrence,
bit-reproducibility, the gradient guard's skip and clip, interchange of the optimiser state with a plain torch.optim.SGD, and the
refusals.

Bound (elementwise, u = 2^-24): with S = mu |buf| + |clip g| + wd |p| of the fp32 state BEFORE the step,
    |d buf| <= 8 u S        |d p| <= 8 u (|p| + lr (1 + mu) S)
Each quantity goes through at most six fp32 roundings of terms bounded by these sums (clip g, g', buf, mu buf, d, lr d, p - lr d).
The float64 side takes the hyper-parameters as the C ABI takes them: mu and wd rounded to fp32, lr the fp32 device value."""
import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MU = 0.9
SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 8193)
LRS = (1e-2, 3e-3, 0.25)          # the device lr of the three steps: changed between launches, no rebuild


def _dev():
    return torch.device("cuda", 0)


def _f32(x):
    return float(np.float32(x))


class _Case:
    """One optimiser over 1-D parameters of SIZES (weight decay 0.1), one view that starts one element into its storage (the scalar
    path for misaligned items), a 3 x 5 and a 64 x 65 weight with transposed shadows (weight decay 0; 64 x 65 = 4160 elements crosses
    a chunk boundary), every parameter with a bf16 shadow; lr one fp32 device tensor shared by the two groups."""

    def __init__(self, nesterov, seed=3, momentum=MU, guard_norm=None, with_guard=False):
        from vm_asr_amd.fused_sgd import HipSgdStep
        from vm_asr_amd.grad_guard import GradGuard
        dev = _dev()
        g = torch.Generator(device=dev).manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, device=dev, generator=g)      # noqa: E731
        flat = [torch.nn.Parameter(rnd(n)) for n in SIZES]
        off = torch.nn.Parameter(rnd(1001)[1:])
        assert off.data_ptr() % 16 == 4 and off.numel() == 1000
        mats = [torch.nn.Parameter(rnd(3, 5)), torch.nn.Parameter(rnd(64, 65))]
        self.params = flat + [off] + mats
        self.wd = {id(p): (0.1 if p.dim() == 1 else 0.0) for p in self.params}
        self.lr = torch.tensor(LRS[0], dtype=torch.float32, device=dev)
        self.opt = torch.optim.SGD([{"params": flat + [off], "weight_decay": 0.1}, {"params": mats, "weight_decay": 0.0}],
                                   lr=self.lr, momentum=momentum, nesterov=nesterov)
        for grp in self.opt.param_groups:
            grp["lr"] = self.lr
        for p in self.params:
            p.grad = rnd(*p.shape)
        self.shadows = {id(p): torch.zeros_like(p, dtype=torch.bfloat16) for p in self.params}
        self.shadows_t = {id(p): torch.zeros(p.shape[1], p.shape[0], dtype=torch.bfloat16, device=dev) for p in mats}
        self.gen, self.nesterov, self.momentum = g, nesterov, momentum
        self.guard = GradGuard([p.grad for p in self.params], dev, guard_norm) if with_guard else None
        self.hip = HipSgdStep(self.opt, self.shadows, self.shadows_t, guard=self.guard)

    def new_grads(self):
        for p in self.params:
            p.grad.copy_(torch.randn(p.shape, device=p.device, generator=self.gen))

    def bufs(self):
        return [self.opt.state[p]["momentum_buffer"] for p in self.params]

    def snapshot(self):
        return [p.detach().clone() for p in self.params], [b.clone() for b in self.bufs()]

    def everything(self):
        """Every tensor a step may write, as integer views (bit comparison)."""
        out = [p.detach().view(torch.int32).clone() for p in self.params] + [b.view(torch.int32).clone() for b in self.bufs()]
        out += [s.view(torch.int16).clone() for s in self.shadows.values()] + [s.view(torch.int16).clone() for s in self.shadows_t.values()]
        return out

    def check_step(self, before, clip=1.0, scale=1.0):
        """p and buf now against float64 from the fp32 state `before` = snapshot(); the shadows bit-equal to the stored p."""
        p0s, b0s = before
        lr, mu = float(self.lr), _f32(self.momentum)
        for p, p0, b0 in zip(self.params, p0s, b0s):
            wd = _f32(self.wd[id(p)])
            p64, b64, g64 = p0.double(), b0.double(), p.grad.double()
            gp = clip * g64 + wd * p64
            buf = mu * b64 + gp
            d = gp + mu * buf if self.nesterov else buf
            want = p64 - lr * d
            S = mu * b64.abs() + (clip * g64).abs() + wd * p64.abs()
            got_b = self.opt.state[p]["momentum_buffer"]
            eb = (got_b.double() - buf).abs()
            ep = (p.detach().double() - want).abs()
            assert bool((eb <= scale * 8 * U * S).all()), (tuple(p.shape), float((eb / (8 * U * S).clamp_min(1e-300)).max()))
            bound_p = scale * 8 * U * (p64.abs() + lr * (1 + mu) * S)
            assert bool((ep <= bound_p).all()), (tuple(p.shape), float((ep / bound_p.clamp_min(1e-300)).max()))
        self.check_shadows()

    def check_shadows(self):
        for p in self.params:
            lp = p.detach().to(torch.bfloat16)
            assert torch.equal(self.shadows[id(p)].view(torch.int16), lp.view(torch.int16)), tuple(p.shape)
            if id(p) in self.shadows_t:
                assert torch.equal(self.shadows_t[id(p)].view(torch.int16), lp.t().contiguous().view(torch.int16)), tuple(p.shape)


@pytest.mark.parametrize("nesterov", [True, False])
def test_three_steps_against_float64_with_a_changing_device_lr(nesterov):
    c = _Case(nesterov)
    # the wrapper created the buffers torch's first step would have created: zeros, owned by the optimiser
    assert all(torch.count_nonzero(b) == 0 and b.shape == p.shape for b, p in zip(c.bufs(), c.params))
    assert c.hip.nchunks == sum(-(-p.numel() // 4096) for p in c.params) and c.hip.total == sum(p.numel() for p in c.params)
    items = c.hip.items
    for i, lr in enumerate(LRS):
        if i:
            c.new_grads()
        c.lr.fill_(lr)
        before = c.snapshot()
        c.hip.step()
        torch.cuda.synchronize()
        assert c.hip.items is items and c.hip.still_valid()
        moved = [not torch.equal(p.detach(), p0) for p, p0 in zip(c.params, before[0])]
        assert all(moved)
        c.check_step(before)
    # after the first step buf == g' as floats (torch's first step): step 1 of a fresh case
    f = _Case(nesterov, seed=5)
    p0s, _ = f.snapshot()
    f.hip.step()
    for p, p0, b in zip(f.params, p0s, f.bufs()):
        wd = _f32(f.wd[id(p)])
        gp = p.grad.double() + wd * p0.double()
        assert bool(((b.double() - gp).abs() <= 2 * U * (p.grad.double().abs() + wd * p0.double().abs())).all())


def test_two_runs_are_bit_identical():
    runs = []
    for _ in range(2):
        c = _Case(True, seed=9)
        for lr in LRS[:2]:
            c.lr.fill_(lr)
            c.hip.step()
            c.new_grads()
        torch.cuda.synchronize()
        runs.append(c.everything())
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs))


def test_guard_skips_a_nonfinite_step_bit_exactly_and_clips_by_norm():
    c = _Case(True, seed=13, with_guard=True, guard_norm=None)
    c.guard.measure()
    c.hip.step()                                   # a clean guarded step first: buffers and shadows hold values
    c.new_grads()
    victim = c.params[7].grad                      # 8193 elements: the inf sits in the last chunk of a three-chunk item
    victim[8192] = float("inf")
    skipped = c.guard.read()["skipped"]
    before = c.everything()
    c.guard.measure()
    c.hip.step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, c.everything()))
    r = c.guard.read()
    assert r["skipped"] == skipped + 1 and r["found_inf"]
    # clean again: the step is taken, unclipped (max_norm None -> coefficient 1)
    victim[8192] = 0.5
    snap = c.snapshot()
    c.guard.measure()
    c.hip.step()
    assert c.guard.read()["skipped"] == skipped + 1 and c.guard.read()["clip_coef"] == 1.0
    c.check_step(snap)
    # clip_grad below the gradient norm: the bound holds with the clip coefficient the guard measured
    probe = c.guard.read()["grad_norm"]
    k = _Case(False, seed=13, with_guard=True, guard_norm=0.25 * probe)
    k.guard.measure()
    clip = k.guard.read()["clip_coef"]
    assert 0.0 < clip < 0.5 and k.guard.read()["grad_norm"] > 0.25 * probe
    grads = [p.grad.clone() for p in k.params]
    snap = k.snapshot()
    k.hip.step()
    torch.cuda.synchronize()
    assert all(torch.equal(p.grad, g) for p, g in zip(k.params, grads))          # the gradient buffer is not modified
    k.check_step(snap, clip=clip)
    assert any(not torch.equal(p.detach(), p0) for p, p0 in zip(k.params, snap[0]))


def test_state_loads_into_a_plain_cpu_sgd_that_takes_the_same_third_step():
    from vm_asr_amd.optim import portable_optimizer_state
    c = _Case(True, seed=17)
    for lr in LRS[:2]:
        c.lr.fill_(lr)
        c.hip.step()
        c.new_grads()
    c.lr.fill_(LRS[1])
    sd = portable_optimizer_state(c.opt)
    assert all(type(g["lr"]) is float for g in sd["param_groups"])
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in c.params]
    plain = torch.optim.SGD([{"params": cpu[:-2], "weight_decay": 0.1}, {"params": cpu[-2:], "weight_decay": 0.0}], lr=1.0,
                            momentum=MU, nesterov=True)
    plain.load_state_dict(copy.deepcopy(sd))
    assert all(g["lr"] == float(c.lr) for g in plain.param_groups)
    for q, p in zip(cpu, c.params):
        assert torch.equal(plain.state[q]["momentum_buffer"], c.opt.state[p]["momentum_buffer"].cpu())
        q.grad = p.grad.cpu().clone()
    before = c.snapshot()
    c.hip.step()
    plain.step()
    c.check_step(before)                            # the HIP side within one bound of float64 ...
    lr, mu = float(c.lr), _f32(MU)
    for q, p, p0, b0 in zip(cpu, c.params, *before):     # ... torch's side too, hence the two within twice the bound of each other
        wd = _f32(c.wd[id(p)])
        S = mu * b0.double().abs() + p.grad.double().abs() + wd * p0.double().abs()
        eb = (plain.state[q]["momentum_buffer"].double() - c.opt.state[p]["momentum_buffer"].cpu().double()).abs()
        ep = (q.detach().double() - p.detach().cpu().double()).abs()
        assert bool((eb <= 2 * 8 * U * S.cpu()).all()) and bool((ep <= 2 * 8 * U * (p0.double().abs() + lr * (1 + mu) * S).cpu()).all())


def test_still_valid_notices_new_grads_buffers_and_lr():
    from vm_asr_amd.optim import lr_to_device
    c = _Case(True, seed=19)
    c.hip.step()
    assert c.hip.still_valid()
    p = c.params[2]
    old = p.grad
    p.grad = old.clone()
    assert not c.hip.still_valid()
    p.grad = old
    assert c.hip.still_valid()
    buf = c.opt.state[p]["momentum_buffer"]
    c.opt.state[p]["momentum_buffer"] = buf.clone()
    assert not c.hip.still_valid()
    c.opt.state[p]["momentum_buffer"] = buf
    assert c.hip.still_valid()
    lr = c.lr
    c.opt.load_state_dict(copy.deepcopy(c.opt.state_dict()))      # what a resume does: new momentum buffers (and a new lr object)
    for g in c.opt.param_groups:
        g["lr"] = lr
    assert not c.hip.still_valid()
    c2 = _Case(True, seed=19)
    lr_to_device(c2.opt, _dev())                                   # a new shared lr tensor
    assert c2.opt.param_groups[0]["lr"] is not c2.lr and not c2.hip.still_valid()


def test_optimisers_that_do_not_qualify_raise_value_error():
    from vm_asr_amd.fused_sgd import HipSgdStep
    dev = _dev()

    def make(lr_tensor=True, groups=None, **kw):
        ps = [torch.nn.Parameter(torch.randn(7, device=dev)), torch.nn.Parameter(torch.randn(3, 5, device=dev))]
        lr = torch.tensor(1e-2, device=dev) if lr_tensor else 1e-2
        opt = torch.optim.SGD(groups(ps) if groups else ps, lr=lr, **{"momentum": MU, **kw})
        for g in opt.param_groups:
            g["lr"] = lr
        for p in ps:
            p.grad = torch.randn_like(p)
        return opt

    assert HipSgdStep(make()).nchunks == 2
    with pytest.raises(ValueError, match="dampening"):
        HipSgdStep(make(dampening=0.1))
    with pytest.raises(ValueError, match="dampening 0 and maximize off"):
        HipSgdStep(make(maximize=True))
    with pytest.raises(ValueError, match="learning-rate tensor"):
        HipSgdStep(make(lr_tensor=False))
    with pytest.raises(ValueError, match="momentum / nesterov"):
        HipSgdStep(make(groups=lambda ps: [{"params": ps[:1], "momentum": 0.8}, {"params": ps[1:]}]))
    with pytest.raises(ValueError, match="momentum / nesterov"):
        HipSgdStep(make(groups=lambda ps: [{"params": ps[:1], "nesterov": True}, {"params": ps[1:]}]))
    with pytest.raises(ValueError, match="not an SGD"):
        HipSgdStep(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(3, device=dev))], lr=1e-3))
    opt = make()
    opt.param_groups[0]["params"][1].grad = torch.randn(5, 3, device=dev).t()      # the right shape, not contiguous
    with pytest.raises(ValueError, match="does not qualify"):
        HipSgdStep(opt)
    assert not opt.state                      # a refused optimiser keeps its state: no buffer was created


def test_c_abi_refuses_a_null_pointer_and_momentum_one_without_a_launch():
    from vm_asr_amd import _lib
    c = _Case(True, seed=23)
    lib, h = _lib.lib(), c.hip
    torch.cuda.synchronize()
    before = c.everything()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    assert lib.vmasr_sgd_step(ptr(h.items), ptr(h.chunks), h.nchunks, h.total, None, MU, 1, None) == -1
    assert b"null" in lib.vmasr_last_error()
    assert lib.vmasr_sgd_step(ptr(h.items), ptr(h.chunks), h.nchunks, h.total, ptr(h.lr), 1.0, 1, None) == -1
    assert b"momentum" in lib.vmasr_last_error()
    with pytest.raises(RuntimeError, match=r"sgd_step failed \(-1\).*momentum"):
        _lib.call(lib.vmasr_sgd_step, h.items, h.chunks, h.nchunks, h.total, h.lr, 1.0, 1)
    with pytest.raises(RuntimeError, match=r"sgd_step_guarded failed \(-1\).*null"):
        _lib.call(lib.vmasr_sgd_step_guarded, h.items, h.chunks, h.nchunks, h.total, h.lr, MU, 1, None, device=_dev())
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, c.everything()))
