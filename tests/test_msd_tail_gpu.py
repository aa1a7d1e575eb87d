"""The scale discriminator's dense tail on the GPU: csrc/dconv1d.hip (forward, input gradient, weight / bias gradient) against float64
on the CPU at the 2e-5 gate, its optional outputs, run-to-run bit equality and capability query, and the hidden-128 module and its
generator pass under both values of VMASR_MSD_TAIL."""
import copy

import pytest
import torch
import torch.nn.functional as F

import msd_tail_cases as tc
from msd_common import close

pytestmark = pytest.mark.gpu

GATE = tc.GATE
_ID = lambda c: "x".join(map(str, c))


def _run(case, act):
    from vm_asr_amd import msd_ops
    from vm_asr_amd.msd import _DConv1dFn
    B, Cin, Cout, L, k, pad = case[:6]
    x, w, b, gy, y64, dx64, dw64, db64 = tc.problem(case, act)
    assert msd_ops.dconv1d_supported(Cin, Cout, 1, k, 1) and msd_ops.dconv1d_supported_launch(Cin, Cout, 1, k, 1, pad, B, L)
    xd, wd = x.cuda().requires_grad_(), w.cuda().requires_grad_()
    bd = None if b is None else b.cuda().requires_grad_()
    y = _DConv1dFn.apply(xd, wd, bd, pad, act)
    assert y.shape == y64.shape
    y.backward(gy.cuda())
    close(y, y64, GATE, f"tail y {case} act={act}")
    close(xd.grad, dx64, GATE, f"tail dx {case} act={act}")
    close(wd.grad, dw64, GATE, f"tail dW {case} act={act}")
    if b is not None:
        close(bd.grad, db64, GATE, f"tail db {case} act={act}")


@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("case", tc.CASES + [tc.NO_BIAS], ids=_ID)
def test_dconv1d_vs_float64(case, act):
    _run(case, act)


def test_dconv1d_conv_post_vs_float64():
    _run(tc.CONV_POST, False)


@pytest.mark.parametrize("case", [tc.CASES[3], tc.CASES[4], tc.CASES[6], tc.CASES[-1]], ids=_ID)
def test_dconv1d_optional_outputs(case):
    """need_x / need_w / need_b false in turn: the other gradients are bitwise those of the full backward (weight gradient with slabs,
    and, at (1, 3, 2, 4, 5, 4) with its single K unit, without)."""
    from vm_asr_amd.msd import _DConv1dFn
    B, Cin, Cout, L, k, pad = case
    x, w, b, gy = (t.cuda() for t in tc.problem(case, True)[:4])

    def grads(need):
        xs = [t.clone().requires_grad_(n) for t, n in zip((x, w, b), need)]
        _DConv1dFn.apply(*xs, pad, True).backward(gy)
        return [t.grad for t in xs]
    full = grads((True, True, True))
    assert all(g is not None for g in full)
    for off in range(3):
        need = tuple(i != off for i in range(3))
        for i, g in enumerate(grads(need)):
            assert (g is None and full[i] is not None) if i == off else torch.equal(g, full[i]), (case, off, i)


@pytest.mark.parametrize("case", [tc.WORKLOAD, tc.CONV_POST], ids=_ID)
def test_dconv1d_is_bit_reproducible(case):
    from vm_asr_amd import msd_ops
    B, Cin, Cout, L, k, pad = case
    act = case is tc.WORKLOAD
    x, w, b, gy = (t.cuda() for t in tc.problem(case, act)[:4])
    runs = []
    for _ in range(2):
        y, pre = msd_ops.dconv1d_fwd(x, w, b, 1, pad, act)
        dx = msd_ops.dconv1d_dgrad(gy, pre, w, x.shape, 1, pad)
        dw, db = msd_ops.dconv1d_wgrad(x, gy, pre, w.shape, 1, pad)
        runs.append((y, dx, dw, db) + ((pre,) if act else ()))
    for a, c in zip(*runs):
        assert torch.equal(a, c)


def test_supported_implies_every_launcher_accepts():
    """The query and the launchers must not disagree.  Over the cases: supported_launch is true and forward, dgrad and wgrad run; a
    shape the query refuses (stride 2) is refused by all three with the invalid-argument code, and dense_conv1d falls through to
    F.conv1d and still matches float64."""
    from vm_asr_amd import msd_ops
    from vm_asr_amd.msd import dense_conv1d
    for case in tc.CASES[1:] + [tc.CONV_POST]:
        B, Cin, Cout, L, k, pad = case
        assert msd_ops.dconv1d_supported_launch(Cin, Cout, 1, k, 1, pad, B, L)
        x, w, b, gy = (t.cuda() for t in tc.problem(case, False)[:4])
        msd_ops.dconv1d_fwd(x, w, b, 1, pad, False)
        msd_ops.dconv1d_dgrad(gy, None, w, x.shape, 1, pad)
        msd_ops.dconv1d_wgrad(x, gy, None, w.shape, 1, pad)
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(5)
    x, w, b = torch.randn(2, 24, 50, generator=g), torch.randn(16, 24, 5, generator=g) / 120 ** 0.5, torch.randn(16, generator=g)
    assert not msd_ops.dconv1d_supported(24, 16, 1, 5, 2) and not msd_ops.dconv1d_supported_launch(24, 16, 1, 5, 2, 2, 2, 50)
    gz = torch.zeros(2, 16, 25, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported shape"):
        msd_ops.dconv1d_fwd(x.cuda(), w.cuda(), b.cuda(), 2, 2, False)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        msd_ops.dconv1d_dgrad(gz, None, w.cuda(), x.shape, 2, 2)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        msd_ops.dconv1d_wgrad(x.cuda(), gz, None, w.shape, 2, 2)
    xd, wd, bd = (t.cuda().requires_grad_() for t in (x, w, b))
    y = dense_conv1d(xd, wd, bd, 2, 2, True)
    x64, w64, b64 = (t.double().requires_grad_() for t in (x, w, b))
    y64 = F.gelu(F.conv1d(x64, w64, b64, 2, 2))
    gy = torch.randn(y64.shape, generator=g)
    y.backward(gy.cuda())
    y64.backward(gy.double())
    close(y, y64.detach(), GATE, "tail fallback y")
    close(xd.grad, x64.grad, GATE, "tail fallback dx")
    close(wd.grad, w64.grad, GATE, "tail fallback dW")


def test_dense_conv1d_takes_the_hip_route(monkeypatch):
    """The switch selects the route: at hip the autograd node is _DConv1dFn's and pre-activations are bit-reproducible; at torch it is
    not (the library's convolution), whatever VMASR_MSD_CONV=hip says."""
    from vm_asr_amd.msd import dense_conv1d
    x, w, b = (t.cuda() for t in tc.problem(tc.CASES[2], True)[:3])
    for mode, want in (("hip", True), ("torch", False)):
        monkeypatch.setenv("VMASR_MSD_TAIL", mode)
        y = dense_conv1d(x.clone().requires_grad_(), w, b, 1, 2, True)
        assert ("_DConv1dFn" in type(y.grad_fn).__name__) == want, (mode, y.grad_fn)


NAMES = ["discriminators.0.convs.6.parametrizations.weight.original", "discriminators.2.conv_post.parametrizations.weight.original"]


@pytest.fixture(scope="module")
def wide():
    """hidden 128, B 1, T 8192, eval mode, seeded weights: the module, its float64 CPU evaluation (scores, maps, dW of the two tail
    layers) and the float64 composed generator pass (scores, loss, dx).  The real maps of the generator pass are built tie-free as in
    tests/test_msd_featmatch_gpu.py — float32(map64 + s u), s = +-1, u in [0.01, 1] — so fp32 and float64 agree on every sign of the
    L1 terms: one sign that sits on a rounding edge moves dx by 4e-4 of its maximum (measured with two random signals), which says
    nothing about the convolutions."""
    from vm_asr_amd.msd import MultiScaleDiscriminator
    from vm_asr_amd.msd_featmatch import composed_feature_loss
    torch.manual_seed(77)
    D = MultiScaleDiscriminator(hidden=128).eval()
    x = 0.3 * torch.randn(1, 1, 8192)
    D64 = copy.deepcopy(D).double()
    scores, fmaps = D64.forward_single(x.double())
    sum((s ** 2).sum() for s in scores).backward()
    p64 = dict(D64.named_parameters())
    single = ([s.detach() for s in scores], [[f.detach() for f in fs] for fs in fmaps], {n: p64[n].grad.clone() for n in NAMES})
    g = torch.Generator().manual_seed(78)
    f_real = [[(f + (2.0 * torch.randint(0, 2, f.shape, generator=g) - 1.0) * (0.01 + 0.99 * torch.rand(f.shape, generator=g))).float()
               for f in fs] for fs in single[1]]
    xg = x.double().requires_grad_()
    gs, gf = D64.forward_single(xg, detach_weights=True)
    assert min((r.double() - f).abs().min().item() for rs, fs in zip(f_real, gf) for r, f in zip(rs, fs)) > 5e-3
    loss = composed_feature_loss([[r.double() for r in rs] for rs in f_real], gf)
    (2.0 * loss + sum((s ** 2).mean() for s in gs)).backward()
    return D, x, f_real, single, ([s.detach() for s in gs], loss.detach(), xg.grad)


@pytest.mark.parametrize("mode", ["hip", "torch"])
def test_msd_hidden128_tail_vs_float64(wide, mode, monkeypatch):
    monkeypatch.setenv("VMASR_MSD_TAIL", mode)
    D, x, _, (s64, f64, g64), _ = wide
    D = copy.deepcopy(D).cuda()
    scores, fmaps = D.forward_single(x.cuda())
    sum((s ** 2).sum() for s in scores).backward()
    assert sum(len(f) for f in fmaps) == 24
    for i in range(3):
        close(scores[i], s64[i], GATE, f"tail {mode} score{i}")
        for j in range(8):
            close(fmaps[i][j], f64[i][j], GATE, f"tail {mode} fmap{i}_{j}")
    params = dict(D.named_parameters())
    for n, g in g64.items():
        close(params[n].grad, g, GATE, f"tail {mode} dW {n}")


@pytest.mark.parametrize("mode", ["hip", "torch"])
def test_msd_generator_pass_tail_vs_float64(wide, mode, monkeypatch):
    """forward_generator (constant weights, the feature-matching loss formed on the way) under both values of the switch: scores, loss
    and dx against the float64 composed loop."""
    monkeypatch.setenv("VMASR_MSD_TAIL", mode)
    D, x, f_real, _, (s64, loss64, dx64) = wide
    D = copy.deepcopy(D).cuda()
    f_real = [[r.cuda() for r in rs] for rs in f_real]
    xg = x.cuda().requires_grad_()
    scores, loss = D.forward_generator(xg, f_real)
    (2.0 * loss + sum((s ** 2).mean() for s in scores)).backward()
    for i in range(3):
        close(scores[i], s64[i], GATE, f"tail gen {mode} score{i}")
    close(loss, loss64, GATE, f"tail gen {mode} loss")
    close(xg.grad, dx64, GATE, f"tail gen {mode} dx")
    assert all(p.grad is None for p in D.parameters())
