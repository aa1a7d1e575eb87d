"""The fused stem of the scale discriminator on the GPU (csrc/stem1d.hip): forward and backward against F.conv1d (+ F.gelu) and autograd
in float64 on the CPU, the backward's subsets, run-to-run bit equality, the module with the switch in each position, what the autograd
node keeps, and one eager ["mpd", "msd"] trainer step per switch value.

Gate: max|got - ref| <= 2e-5 max|ref| per tensor, the one tests/test_msd_gpu.py holds the grouped layers to.  The achieved worst values
are in profiles/msd_stem.md."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from msd_common import close, make_trainer

pytestmark = pytest.mark.gpu

GATE = 2e-5


def _tiles():
    from vm_asr_amd import msd_ops
    return msd_ops.stem1d_time_tile(), msd_ops.stem1d_channel_group()


TT, CG = _tiles()
# (B, Cout, L, k, pad): single positions, a window that is all padding, lengths around one and two time tiles, one more channel than a
# workgroup's group, the 32-channel weight stages of the input gradient (128), outputs shorter than the input, k > 16 (the kernels'
# second tap width), and the input gradient's own tile of 256 - (k - 1) positions filled exactly and exceeded by one
CASES = [(1, 1, 1, 15, 7), (2, 3, 14, 15, 7), (2, 3, 15, 15, 7), (3, 16, 16, 15, 7), (1, 128, 1201, 15, 7),
         (2, 5, TT - 1, 15, 7), (2, 5, TT, 15, 7), (2, 5, TT + 1, 15, 7), (1, 7, 2 * TT + 3, 15, 7), (2, CG + 1, 70, 15, 7),
         (2, 6, 333, 5, 2), (2, 6, 333, 4, 0), (2, 5, TT + 40, 20, 3), (1, 3, 77, 32, 31), (2, 5, 242, 15, 7), (2, 5, 243, 15, 7)]

_REF = {}


def _problem(case, act, has_bias):
    """Inputs and the float64 CPU result of one case, computed once and shared (never modified)."""
    key = (case, act, has_bias)
    if key not in _REF:
        B, Cout, L, k, pad = case
        g = torch.Generator().manual_seed(2000 + CASES.index(case))
        x = torch.randn(B, 1, L, generator=g)
        w = torch.randn(Cout, 1, k, generator=g) / k ** 0.5
        b = torch.randn(Cout, generator=g) if has_bias else None
        gy = torch.randn(B, Cout, L + 2 * pad - k + 1, generator=g)
        x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
        b64 = b.double().requires_grad_() if has_bias else None
        y64 = F.conv1d(x64, w64, b64, 1, pad)
        if act:
            y64 = F.gelu(y64)
        y64.backward(gy.double())
        _REF[key] = (x, w, b, gy, y64.detach(), x64.grad, w64.grad, b64.grad if has_bias else None)
    return _REF[key]


@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", [True, False], ids=["gelu", "linear"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_stem1d_vs_float64(case, act, has_bias):
    from vm_asr_amd import msd_ops
    from vm_asr_amd.msd import _Stem1dFn
    B, Cout, L, k, pad = case
    x, w, b, gy, y64, dx64, dw64, db64 = _problem(case, act, has_bias)
    assert msd_ops.stem1d_supported_launch(Cout, k, 1, pad, B, L)
    xd, wd = x.cuda().requires_grad_(), w.cuda().requires_grad_()
    bd = b.cuda().requires_grad_() if has_bias else None
    y = _Stem1dFn.apply(xd, wd, bd, pad, act)
    assert y.shape == y64.shape
    y.backward(gy.cuda())
    what = f"{case} act={act} bias={has_bias}"
    close(y, y64, GATE, f"stem y {what}")
    close(xd.grad, dx64, GATE, f"stem dx {what}")
    close(wd.grad, dw64, GATE, f"stem dW {what}")
    if has_bias:
        close(bd.grad, db64, GATE, f"stem db {what}")


@pytest.mark.parametrize("case", [CASES[4], CASES[8], CASES[12]], ids=lambda c: "x".join(map(str, c)))
def test_stem1d_backward_subsets_are_bitwise_parts_of_the_full_call(case):
    from vm_asr_amd import msd_ops
    pad = case[4]
    x, w, b, gy = (t.cuda() for t in _problem(case, True, True)[:4])
    dx, dw, db = msd_ops.stem1d_bwd(gy, x, w, b, pad, True)
    a = msd_ops.stem1d_bwd(gy, x, w, b, pad, True, True, False, False)
    assert torch.equal(a[0], dx) and a[1] is None and a[2] is None
    a = msd_ops.stem1d_bwd(gy, x, w, b, pad, True, False, True, True)
    assert a[0] is None and torch.equal(a[1], dw) and torch.equal(a[2], db)
    a = msd_ops.stem1d_bwd(gy, x, w, b, pad, True, False, True, False)
    assert a[0] is None and torch.equal(a[1], dw) and a[2] is None
    assert msd_ops.stem1d_bwd(gy, x, w, b, pad, True, False, False, False) == (None, None, None)


def test_stem1d_is_bit_reproducible():
    from vm_asr_amd import msd_ops
    g = torch.Generator().manual_seed(11)
    B, Cout, L = 3, 128, 2 * TT + 3
    x, w, b = torch.randn(B, 1, L, generator=g).cuda(), (torch.randn(Cout, 1, 15, generator=g) / 15 ** 0.5).cuda(), torch.randn(Cout, generator=g).cuda()
    gy = torch.randn(B, Cout, L, generator=g).cuda()
    runs = [(msd_ops.stem1d_fwd(x, w, b, 7, True),) + msd_ops.stem1d_bwd(gy, x, w, b, 7, True) for _ in range(2)]
    for a, c in zip(*runs):
        assert torch.isfinite(a).all() and torch.equal(a, c)


def test_stem1d_refused_shape_raises_and_the_module_falls_through():
    from vm_asr_amd import msd_ops
    from vm_asr_amd.msd import stem_conv1d
    g = torch.Generator().manual_seed(5)
    x, w, b = torch.randn(2, 1, 50, generator=g), torch.randn(4, 1, 33, generator=g) / 33 ** 0.5, torch.randn(4, generator=g)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        msd_ops.stem1d_fwd(x.cuda(), w.cuda(), b.cuda(), 16, True)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        msd_ops.stem1d_bwd(torch.zeros(2, 4, 50, device="cuda"), x.cuda(), w.cuda(), b.cuda(), 16, True)
    xd, wd, bd = (t.cuda().requires_grad_() for t in (x, w, b))
    y = stem_conv1d(xd, wd, bd, 1, 16, True)                 # k 33: torch's operators
    assert "Stem1d" not in type(y.grad_fn).__name__
    x64, w64, b64 = (t.double() for t in (x, w, b))
    close(y, F.gelu(F.conv1d(x64, w64, b64, 1, 16)), GATE, "stem fallback y")


def _loss(scores):
    """A fixed weighted sum of the scores, scaled so that every gradient checked below is far above close()'s 1e-6 floor of the scale
    (the squared scores of a freshly initialised hidden-16 module give gradients of 1e-8)."""
    return 100.0 * sum((torch.cos(torch.arange(s.numel(), dtype=s.dtype, device=s.device)).view_as(s) * s).sum() for s in scores)


@pytest.fixture(scope="module")
def small():
    """hidden 16, B 2, T 1201, seeded weights, eval mode: the module and its float64 CPU evaluation."""
    from vm_asr_amd.msd import MultiScaleDiscriminator
    torch.manual_seed(78)
    D = MultiScaleDiscriminator(hidden=16).eval()
    x = 0.3 * torch.randn(2, 1, 1201)
    D64 = copy.deepcopy(D).double()
    x64 = x.double().requires_grad_()
    scores, fmaps = D64.forward_single(x64)
    _loss(scores).backward()
    p64 = dict(D64.named_parameters())
    names = [f"discriminators.{i}.convs.0.{n}" for i in range(3) for n in ("parametrizations.weight.original", "bias")]
    return D, x, [s.detach() for s in scores], [[f.detach() for f in fs] for fs in fmaps], x64.grad, {n: p64[n].grad for n in names}


def _env(monkeypatch, stem="hip", conv="hip"):
    monkeypatch.setenv("VMASR_MSD_STEM", stem)
    monkeypatch.setenv("VMASR_MSD_CONV", conv)


def test_msd_module_with_fused_stem_vs_float64(small, monkeypatch):
    _env(monkeypatch)
    D, x, s64, f64, dx64, g64 = small
    D = copy.deepcopy(D).cuda()
    xd = x.cuda().requires_grad_()
    scores, fmaps = D.forward_single(xd)
    assert all("Stem1d" in type(fmaps[i][0].grad_fn).__name__ for i in range(3))
    _loss(scores).backward()
    for i in range(3):
        close(scores[i], s64[i], GATE, f"stem module score{i}")
        assert len(fmaps[i]) == 8
        for j in range(8):
            close(fmaps[i][j], f64[i][j], GATE, f"stem module fmap{i}_{j}")
    close(xd.grad, dx64, GATE, "stem module dx")
    params = dict(D.named_parameters())
    for n, g in g64.items():
        close(params[n].grad, g, GATE, f"stem module grad {n}")


def test_msd_module_detached_weights_reach_the_kernel_as_dx_only(small, monkeypatch):
    _env(monkeypatch)
    D, x, _, _, dx64, _ = small
    D = copy.deepcopy(D).cuda()
    xd = x.cuda().requires_grad_()
    scores, fmaps = D.forward_single(xd, detach_weights=True)
    assert all("Stem1d" in type(fmaps[i][0].grad_fn).__name__ for i in range(3))
    _loss(scores).backward()
    assert all(p.grad is None for p in D.parameters())
    close(xd.grad, dx64, GATE, "stem module dx, weights detached")


@pytest.mark.parametrize("route", ["stem=torch", "conv=torch", "plain_torch_ops"])
def test_stem_off_is_the_torch_chain_bitwise(small, route, monkeypatch):
    from vm_asr_amd.discriminator import plain_torch_ops
    from vm_asr_amd.msd import _weight
    _env(monkeypatch, stem="torch" if route == "stem=torch" else "hip", conv="torch" if route == "conv=torch" else "hip")
    D = copy.deepcopy(small[0]).cuda().discriminators[0]
    xd = small[1].cuda().requires_grad_()
    if route == "plain_torch_ops":
        with plain_torch_ops():
            _, fmap = D(xd)
    else:
        _, fmap = D(xd)
    layer = D.convs[0]
    assert "Stem1d" not in type(fmap[0].grad_fn).__name__
    assert torch.equal(fmap[0], F.gelu(F.conv1d(xd, _weight(layer), layer.bias, 1, 7)))


def test_fused_stem_saves_nothing_of_the_maps_size(small, monkeypatch):
    _env(monkeypatch)
    D = copy.deepcopy(small[0]).cuda().discriminators[0]
    xd = small[1].cuda().requires_grad_()
    _, fmap = D(xd)
    y = fmap[0]
    assert y.shape == (2, 16, 1201) and "Stem1d" in type(y.grad_fn).__name__
    saved = [t for t in y.grad_fn.saved_tensors if t is not None]
    assert len(saved) == 3 and all(t.numel() < y.numel() for t in saved)
    assert sorted(t.numel() for t in saved) == sorted([2 * 1201, 16 * 15, 16])


def test_trainer_step_agrees_between_the_stem_routes(monkeypatch):
    """One eager ["mpd", "msd"] step per switch value from the same state and seed: the same losses to the gate, every MSD parameter moves."""
    logs = {}
    for mode in ("hip", "torch"):
        _env(monkeypatch, stem=mode)
        torch.manual_seed(0)
        z, tr = make_trainer("cuda:0")
        before = {n: p.detach().clone() for n, p in tr.models["msd"].named_parameters()}
        wave_target = torch.from_numpy(z["wave_target"]).cuda()
        hf = torch.full((wave_target.shape[0],), 171, dtype=torch.int64, device="cuda")
        _, lg = tr.train_step(wave_target, wave_target, hf)
        logs[mode] = {k: float(v) for k, v in lg.items()}
        for n, p in tr.models["msd"].named_parameters():
            assert torch.isfinite(p).all() and not torch.equal(p, before[n]), (mode, n)
    assert logs["hip"].keys() == logs["torch"].keys() and "generator/features_msd" in logs["hip"]
    for k, ref in logs["torch"].items():
        got = logs["hip"][k]
        print(f"{k}: hip {got:.8f} torch {ref:.8f}")
        assert np.isfinite(got) and abs(got - ref) <= GATE * abs(ref), (k, got, ref)
