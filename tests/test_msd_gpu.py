"""The multi-scale discriminator on the GPU: the grouped 1-D convolution kernels (csrc/gconv1d.hip) against float64 on the CPU, their
run-to-run bit equality and capability query, the module against the reference's goldens and against itself in float64, and one
eager trainer step with ["mpd", "msd"]."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from msd_common import check_trainstep, close, make_trainer, run_eval

pytestmark = pytest.mark.gpu

K, S, PAD = 41, 4, 20
# (B, Cin, Cout, groups, L): the hidden-128 layers, one input channel per group, windows that are mostly padding
CASES = [(2, 128, 128, 4, 1201), (2, 128, 256, 16, 301), (2, 256, 512, 16, 76), (1, 512, 1024, 16, 19), (1, 1024, 1024, 16, 19),
         (2, 16, 32, 16, 76), (2, 16, 16, 4, 5), (2, 16, 16, 4, 2), (2, 16, 16, 4, 1)]
GATE = 2e-5      # max|got - ref| <= 2e-5 max|ref| per tensor: the MPD convolutions' gate (tests/test_mpd.py)
# (B, Cin, Cout, groups, L, pad): what the launcher admits beyond the module's own layers (0 <= pad < 41, any per-group (Ci, Co)), at the
# smallest sizes that reach each path of csrc/gconv1d.hip.  Ci = Cin / groups walks the 4-channel LDS stage's remainders (2, 3 alone; 5,
# 6, 7, 9 behind full stages; 40: the input gradient's 64-row tile, 40 rows used), Co = Cout / groups the output-channel tiles (1, 3 of
# 16; 17, 24 of 32; 40 of 64; 72 = 64 + 8: a second, ragged tile).  T = outputs, nq = ceil((L + pad) / 4) = the input gradient's
# positions per residue; tiles: 128 outputs (forward), 64 outputs (weight gradient's K unit), 64 nq (input gradient).
EDGE_CASES = [
    (2, 6, 3, 3, 545, 0),          # pad 0, Ci 2, Co 1, T 127
    (2, 6, 6, 2, 543, 3),          # pad 3, Ci 3, Co 3, T 128
    (2, 10, 34, 2, 473, 40),       # pad 40, Ci 5, Co 17, T 129
    (2, 12, 48, 2, 249, 20),       # pad 20, Ci 6, Co 24, T 63
    (2, 7, 40, 1, 293, 0),         # pad 0, Ci 7, Co 40, T 64, groups 1
    (2, 18, 144, 2, 291, 3),       # pad 3, Ci 9, Co 72 (two output-channel tiles, the second of 8 rows), T 65
    (2, 80, 6, 2, 216, 40),        # pad 40, Ci 40 (input gradient: MT 4, 40 of 64 rows), Co 3, nq 64, T 64
    (2, 8, 16, 8, 257, 0),         # pad 0, groups = Cin (Ci 1, Co 2), nq 65
    (2, 5, 17, 1, 236, 20),        # pad 20, Ci 5, Co 17, groups 1, nq 64
    (2, 12, 80, 2, 255, 3),        # pad 3, Ci 6, Co 40, nq 65
    (2, 6, 6, 2, 41, 0),           # L + 2 pad == 41: T 1, no padding at all
    (2, 4, 34, 2, 36, 3),          # T 1, the one window padded on both ends; Ci 2, Co 17
    (2, 7, 1, 1, 10, 20),          # every window padded on both ends (L 10); Ci 7, Co 1, groups 1
    (2, 9, 9, 9, 10, 40),          # pad 40, L 10: most windows are all padding; groups = Cin
    (1, 18, 48, 2, 7, 40),         # one K unit in all (B 1, T 12): the weight gradient has ONE slab; Ci 9, Co 24
    (3, 128, 256, 16, 8231, 3),    # T 2050 -> 3 x 33 K units over 50 slabs of 2: the last slab has one
]

_REF = {}


def _problem(case, act):
    """Inputs and the float64 CPU result of one case, computed once and shared (never modified)."""
    key = (case, act)
    if key not in _REF:
        B, Cin, Cout, G, L, pad = case if len(case) == 6 else case + (PAD,)
        g = torch.Generator().manual_seed(1000 + CASES.index(case) if len(case) == 5 else 3000 + EDGE_CASES.index(case))
        x = torch.randn(B, Cin, L, generator=g)
        w = torch.randn(Cout, Cin // G, K, generator=g) / (Cin // G * K) ** 0.5
        b = torch.randn(Cout, generator=g)
        T = (L + 2 * pad - K) // S + 1
        gy = torch.randn(B, Cout, T, generator=g)
        x64, w64, b64 = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
        y64 = F.conv1d(x64, w64, b64, S, pad, 1, G)
        if act:
            y64 = F.gelu(y64)
        y64.backward(gy.double())
        _REF[key] = (x, w, b, gy, y64.detach(), x64.grad, w64.grad, b64.grad)
    return _REF[key]


@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_gconv1d_vs_float64(case, act):
    from vm_asr_amd import msd_ops
    from vm_asr_amd.msd import _GConv1dFn
    B, Cin, Cout, G, L = case
    x, w, b, gy, y64, dx64, dw64, db64 = _problem(case, act)
    assert msd_ops.gconv1d_supported(Cin, Cout, G, K, S) and msd_ops.gconv1d_supported_launch(Cin, Cout, G, K, S, PAD, B, L)
    xd, wd, bd = (t.cuda().requires_grad_() for t in (x, w, b))
    y = _GConv1dFn.apply(xd, wd, bd, G, S, PAD, act)
    y.backward(gy.cuda())
    close(y, y64, GATE, f"y {case} act={act}")
    close(xd.grad, dx64, GATE, f"dx {case} act={act}")
    close(wd.grad, dw64, GATE, f"dW {case} act={act}")
    close(bd.grad, db64, GATE, f"db {case} act={act}")


@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gconv1d_edges_vs_float64(case, act):
    """test_gconv1d_vs_float64 over EDGE_CASES: the same four comparisons at the same gate, the pad per case."""
    from vm_asr_amd import msd_ops
    from vm_asr_amd.msd import _GConv1dFn
    B, Cin, Cout, G, L, pad = case
    x, w, b, gy, y64, dx64, dw64, db64 = _problem(case, act)
    assert msd_ops.gconv1d_supported(Cin, Cout, G, K, S) and msd_ops.gconv1d_supported_launch(Cin, Cout, G, K, S, pad, B, L)
    xd, wd, bd = (t.cuda().requires_grad_() for t in (x, w, b))
    y = _GConv1dFn.apply(xd, wd, bd, G, S, pad, act)
    assert y.shape == y64.shape
    y.backward(gy.cuda())
    close(y, y64, GATE, f"y {case} act={act}")
    close(xd.grad, dx64, GATE, f"dx {case} act={act}")
    close(wd.grad, dw64, GATE, f"dW {case} act={act}")
    close(bd.grad, db64, GATE, f"db {case} act={act}")


def _slabs(case):
    """(slabs, K units) of the weight gradient: the slab count read back from the workspace size, S (Cout Ci 41 + Cout) floats."""
    from vm_asr_amd import _lib
    B, Cin, Cout, G, L, pad = case
    nbytes = _lib.lib().vmasr_gconv1d_wgrad_workspace(Cin, Cout, G, K, S, pad, B, L)
    per = 4 * (Cout * (Cin // G) * K + Cout)
    assert nbytes > 0 and nbytes % per == 0
    T = (L + 2 * pad - K) // S + 1
    return nbytes // per, B * -(-T // 64)


def test_edge_cases_reach_one_slab_and_a_short_last_slab():
    """What EDGE_CASES[-2] and [-1] are in the list for, asserted instead of trusted: one slab; several slabs whose last is short."""
    assert _slabs(EDGE_CASES[-2]) == (1, 1)
    slabs, units = _slabs(EDGE_CASES[-1])
    per = -(-units // slabs)
    assert slabs > 1 and per > 1 and (slabs - 1) * per < units < slabs * per, (slabs, units, per)
    # and the tile edges the comments name
    for case, T in zip(EDGE_CASES[:6], (127, 128, 129, 63, 64, 65)):
        assert (case[4] + 2 * case[5] - K) // S + 1 == T
    for case, nq in zip(EDGE_CASES[6:10], (64, 65, 64, 65)):
        assert -(-(case[4] + case[5]) // S) == nq
    assert sum(c[5] != PAD for c in EDGE_CASES[:10]) >= 5


@pytest.mark.parametrize("case", [EDGE_CASES[2], EDGE_CASES[5], EDGE_CASES[-2], EDGE_CASES[-1]], ids=lambda c: "x".join(map(str, c)))
def test_gconv1d_optional_outputs(case):
    """The weight gradient with only dw / only db is bitwise the matching output of the full call (one slab, many slabs, ragged tiles);
    the forward without a bias against float64, with and without the activation."""
    from vm_asr_amd import msd_ops
    B, Cin, Cout, G, L, pad = case
    x, w, b, gy = (t.cuda() for t in _problem(case, True)[:4])
    y, pre = msd_ops.gconv1d_fwd(x, w, b, G, S, pad, True)
    dw, db = msd_ops.gconv1d_wgrad(x, gy, pre, w.shape, G, S, pad)
    only_w = msd_ops.gconv1d_wgrad(x, gy, pre, w.shape, G, S, pad, want_dw=True, want_db=False)
    only_b = msd_ops.gconv1d_wgrad(x, gy, pre, w.shape, G, S, pad, want_dw=False, want_db=True)
    assert only_w[1] is None and torch.equal(only_w[0], dw)
    assert only_b[0] is None and torch.equal(only_b[1], db)
    pre64 = F.conv1d(x.cpu().double(), w.cpu().double(), None, S, pad, 1, G)
    y0, pre0 = msd_ops.gconv1d_fwd(x, w, None, G, S, pad, True)
    close(pre0, pre64, GATE, f"pre without bias {case}")
    close(y0, F.gelu(pre64), GATE, f"y without bias {case}")
    y1, none = msd_ops.gconv1d_fwd(x, w, None, G, S, pad, False)
    assert none is None
    close(y1, pre64, GATE, f"linear y without bias {case}")


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[6]], ids=lambda c: "x".join(map(str, c)))
def test_gconv1d_is_bit_reproducible(case):
    from vm_asr_amd import msd_ops
    B, Cin, Cout, G, L = case
    x, w, b, gy = (t.cuda() for t in _problem(case, True)[:4])
    runs = []
    for _ in range(2):
        y, pre = msd_ops.gconv1d_fwd(x, w, b, G, S, PAD, True)
        dx = msd_ops.gconv1d_dgrad(gy, pre, w, x.shape, G, S, PAD)
        dw, db = msd_ops.gconv1d_wgrad(x, gy, pre, w.shape, G, S, PAD)
        runs.append((y, pre, dx, dw, db))
    for a, c in zip(*runs):
        assert torch.equal(a, c)


def test_supported_implies_every_launcher_accepts():
    """ADVICE: the query and the launchers must not disagree.  Over the cases: supported_launch == 1 and forward, dgrad and wgrad run;
    a shape the query refuses (groups that do not divide Cin for the kernels' layout: here k 5) is refused by all three with
    the invalid-argument code, and grouped_conv1d falls through to F.conv1d and still matches float64."""
    from vm_asr_amd import msd_ops
    from vm_asr_amd.msd import grouped_conv1d
    for case in CASES:
        B, Cin, Cout, G, L = case
        assert msd_ops.gconv1d_supported(Cin, Cout, G, K, S) and msd_ops.gconv1d_supported_launch(Cin, Cout, G, K, S, PAD, B, L)
        x, w, b, gy = (t.cuda() for t in _problem(case, False)[:4])
        y, _ = msd_ops.gconv1d_fwd(x, w, b, G, S, PAD, False)
        msd_ops.gconv1d_dgrad(gy, None, w, x.shape, G, S, PAD)
        msd_ops.gconv1d_wgrad(x, gy, None, w.shape, G, S, PAD)
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(5)
    x, w, b = torch.randn(2, 24, 50, generator=g), torch.randn(16, 3, 5, generator=g) / 15 ** 0.5, torch.randn(16, generator=g)
    assert not msd_ops.gconv1d_supported(24, 16, 8, 5, 2) and not msd_ops.gconv1d_supported(20, 16, 8, K, S)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        msd_ops.gconv1d_fwd(x.cuda(), w.cuda(), b.cuda(), 8, 2, 2, False)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        msd_ops.gconv1d_dgrad(torch.zeros(2, 16, 25, device="cuda"), None, w.cuda(), x.shape, 8, 2, 2)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        msd_ops.gconv1d_wgrad(x.cuda(), torch.zeros(2, 16, 25, device="cuda"), None, w.shape, 8, 2, 2)
    xd, wd, bd = (t.cuda().requires_grad_() for t in (x, w, b))
    y = grouped_conv1d(xd, wd, bd, 8, 2, 2, True)
    x64, w64, b64 = (t.double().requires_grad_() for t in (x, w, b))
    y64 = F.gelu(F.conv1d(x64, w64, b64, 2, 2, 1, 8))
    gy = torch.randn(y64.shape, generator=g)
    y.backward(gy.cuda())
    y64.backward(gy.double())
    close(y, y64.detach(), GATE, "fallback y")
    close(xd.grad, x64.grad, GATE, "fallback dx")
    close(wd.grad, w64.grad, GATE, "fallback dW")


def test_msd_module_vs_golden_hip():
    """Scores, feature maps, losses, gradients, train-mode u / v on the device: the tolerance of tests/test_mpd.py::test_mpd_eval_hip."""
    run_eval("cuda:0", 1e-4)


@pytest.fixture(scope="module")
def wide():
    """hidden 128, B 1, T 8192, seeded weights: the module and its float64 CPU evaluation (scores, maps, dW of two grouped layers)."""
    from vm_asr_amd.msd import MultiScaleDiscriminator
    torch.manual_seed(77)
    D = MultiScaleDiscriminator(hidden=128).eval()
    x = 0.3 * torch.randn(1, 1, 8192)
    D64 = copy.deepcopy(D).double()
    names = ["discriminators.0.convs.1.parametrizations.weight.original", "discriminators.1.convs.4.parametrizations.weight.original"]
    scores, fmaps = D64.forward_single(x.double())
    sum((s ** 2).sum() for s in scores).backward()
    p64 = dict(D64.named_parameters())
    return D, x, [s.detach() for s in scores], [[f.detach() for f in fs] for fs in fmaps], {n: p64[n].grad for n in names}


@pytest.mark.parametrize("mode", ["hip", "torch"])
def test_msd_hidden128_vs_float64(wide, mode, monkeypatch):
    monkeypatch.setenv("VMASR_MSD_CONV", mode)
    D, x, s64, f64, g64 = wide
    D = copy.deepcopy(D).cuda()
    scores, fmaps = D.forward_single(x.cuda())
    sum((s ** 2).sum() for s in scores).backward()
    for i in range(3):
        close(scores[i], s64[i], GATE, f"{mode} score{i}")
        for j in range(8):
            close(fmaps[i][j], f64[i][j], GATE, f"{mode} fmap{i}_{j}")
    params = dict(D.named_parameters())
    for n, g in g64.items():
        close(params[n].grad, g, GATE, f"{mode} dW {n}")


def test_trainer_step_mpd_msd_hip():
    """Losses and gradients of one step against the reference's, then the eager optimiser step: parameters move and stay finite."""
    z, tr = check_trainstep("cuda:0")
    before = {k: {n: p.detach().clone() for n, p in tr.models[k].named_parameters()} for k in ("mpd", "msd")}
    wave_target = torch.from_numpy(z["wave_target"]).cuda()
    hf = torch.full((2,), 171, dtype=torch.int64, device="cuda")
    _, logs = tr.train_step(wave_target, wave_target, hf)
    assert all(np.isfinite(float(v)) for v in logs.values())
    for k in ("mpd", "msd"):
        for n, p in tr.models[k].named_parameters():
            assert torch.isfinite(p).all() and not torch.equal(p, before[k][n]), (k, n)
    with pytest.raises(NotImplementedError, match="MSD"):
        tr.enable_graphs(None)
