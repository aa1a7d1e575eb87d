"""The scale discriminator's generator pass with its feature-matching loss on the GPU (csrc/stem1d.hip's fm kernels, msd_featmatch.py):
the fused stem against F.conv1d + F.gelu + the L1 term in float64 on the CPU with autograd, bit equality with the plain stem, ties,
run-to-run equality, refused shapes, the module and one eager ["mpd", "msd"] trainer step per VMASR_MSD_FEAT value.

Gate: max|got - ref| <= 2e-5 max|ref| per tensor (tests/test_msd_stem_gpu.py's), relative 2e-5 for the scalar term.  y_real is built
tie-free — float32(y_ref64 + s u), s = +-1, u in [0.01, 1] — so fp32 and float64 agree on every sign.  Achieved errors:
profiles/msd_featmatch.md."""
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
# (B, Cout, L, k, pad, bias): L in {1, 15, tile - 1, tile, tile + 1, 2 tile + 3}, Cout in {1, 3, cg, cg + 1, 128}, (k, pad) in
# {(15, 7), (32, 31), (20, 3)}, B in {1, 3}, bias present and absent
CASES = [(1, 1, 1, 15, 7, True), (3, 3, 15, 15, 7, False), (1, CG, TT - 1, 15, 7, True), (3, CG + 1, TT, 15, 7, True),
         (1, 3, TT + 1, 15, 7, False), (1, 128, 2 * TT + 3, 15, 7, True), (3, 128, 15, 15, 7, False), (3, 1, TT + 1, 32, 31, True),
         (1, CG + 1, 15, 32, 31, False), (1, 3, 1, 32, 31, True), (3, CG, 2 * TT + 3, 32, 31, False), (1, 128, TT - 1, 32, 31, True),
         (3, 3, TT, 20, 3, True), (1, CG + 1, 2 * TT + 3, 20, 3, False), (3, 128, TT + 1, 20, 3, True), (1, 1, 15, 20, 3, False)]
COEF = 0.37 / 1000.0        # an arbitrary loss weight (the module's is 1 / (elements * maps))
GTERM = 1.7                 # the term's upstream gradient

_REF = {}


def _problem(case):
    """Inputs and the float64 CPU results of one case, computed once and shared (never modified): x, w, b, gy, y_real, y64, term64 and
    dx64 for the three gradient settings (both, gy alone, gterm alone)."""
    if case not in _REF:
        B, Cout, L, k, pad, has_bias = case
        g = torch.Generator().manual_seed(4000 + CASES.index(case))
        x = torch.randn(B, 1, L, generator=g)
        w = torch.randn(Cout, 1, k, generator=g) / k ** 0.5
        b = torch.randn(Cout, generator=g) if has_bias else None
        T = L + 2 * pad - k + 1
        gy = torch.randn(B, Cout, T, generator=g)
        x64 = x.double().requires_grad_()
        y64 = F.gelu(F.conv1d(x64, w.double(), None if b is None else b.double(), 1, pad))
        s = torch.randint(0, 2, y64.shape, generator=g).double() * 2 - 1
        u = 0.01 + 0.99 * torch.rand(y64.shape, generator=g).double()
        y_real = (y64.detach() + s * u).float()
        assert (y64.detach() - y_real.double()).abs().min().item() > 1e-3       # no sign sits on a rounding edge
        term64 = COEF * (y64 - y_real.double()).abs().sum()
        dx = {}
        dx["both"], = torch.autograd.grad((y64 * gy.double()).sum() + GTERM * term64, x64, retain_graph=True)
        dx["gy"], = torch.autograd.grad((y64 * gy.double()).sum(), x64, retain_graph=True)
        dx["gterm"], = torch.autograd.grad(GTERM * term64, x64)
        _REF[case] = (x, w, b, gy, y_real, y64.detach(), term64.detach(), dx)
    return _REF[case]


def _cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:5])) + ("b" if c[5] else ""))
def test_stem1d_fm_vs_float64(case):
    from vm_asr_amd import msd_ops
    from vm_asr_amd.msd_featmatch import _Stem1dFmFn
    B, Cout, L, k, pad, _ = case
    x, w, b, gy, y_real, y64, term64, dx64 = _problem(case)
    assert msd_ops.stem1d_fm_supported_launch(Cout, k, 1, pad, B, L)
    xd, wd, bd, gyd, yrd = _cuda(x, w, b, gy, y_real)
    xd.requires_grad_()
    y, term = _Stem1dFmFn.apply(xd, wd, bd, yrd, pad, COEF)
    assert y.shape == y64.shape and term.dim() == 0 and term.dtype == torch.float32
    close(y, y64, GATE, f"fm y {case}")
    print(f"fm term {case}: got {term.item():.9e} want {term64.item():.9e}")
    assert abs(term.item() - term64.item()) <= GATE * abs(term64.item())
    both, = torch.autograd.grad([y, term], xd, [gyd, torch.tensor(GTERM, device="cuda")], retain_graph=True)
    close(both, dx64["both"], GATE, f"fm dx gy+gterm {case}")
    only_gy, = torch.autograd.grad(y, xd, gyd, retain_graph=True)
    close(only_gy, dx64["gy"], GATE, f"fm dx gy {case}")
    plain = msd_ops.stem1d_bwd(gyd, xd.detach(), wd, bd, pad, True, True, False, False)[0]
    close(only_gy, plain.double().cpu(), GATE, f"fm dx gy vs stem1d_bwd {case}")
    only_term, = torch.autograd.grad(term, xd, torch.tensor(GTERM, device="cuda"))
    close(only_term, dx64["gterm"], GATE, f"fm dx gterm {case}")


@pytest.mark.parametrize("case", [CASES[3], CASES[5], CASES[10], CASES[14]], ids=lambda c: "x".join(map(str, c[:5])))
def test_fm_forward_is_the_plain_stem_bitwise_and_ties_have_no_sign(case):
    from vm_asr_amd import msd_ops
    pad = case[4]
    x, w, b, gy, y_real = _cuda(*_problem(case)[:5])
    y0 = msd_ops.stem1d_fwd(x, w, b, pad, True)
    y, partials = msd_ops.stem1d_fm_fwd(x, w, b, y_real, pad)
    assert torch.equal(y, y0) and partials.dtype == torch.float64 and torch.isfinite(partials).all()
    y, partials = msd_ops.stem1d_fm_fwd(x, w, b, y0, pad)             # the real map IS the generated one: every difference is 0
    assert torch.equal(y, y0) and partials.sum().item() == 0.0 and (partials == 0).all()
    dx0 = msd_ops.stem1d_bwd(gy, x, w, b, pad, True, True, False, False)[0]
    gterm = torch.tensor([GTERM], device="cuda")
    dx = msd_ops.stem1d_fm_bwd(gy, x, w, b, y0, gterm, 1.0, pad)      # every sign 0: the rebuilt y is the forward's
    assert torch.equal(dx, dx0)
    assert torch.equal(msd_ops.stem1d_fm_bwd(gy, x, w, b, y0, None, 1.0, pad), dx0)
    assert torch.count_nonzero(msd_ops.stem1d_fm_bwd(None, x, w, b, y0, gterm, 1.0, pad)).item() == 0


def test_fm_is_bit_reproducible():
    from vm_asr_amd import msd_ops
    g = torch.Generator().manual_seed(12)
    B, Cout, L = 3, 128, 2051
    x, w, b = torch.randn(B, 1, L, generator=g).cuda(), (torch.randn(Cout, 1, 15, generator=g) / 15 ** 0.5).cuda(), torch.randn(Cout, generator=g).cuda()
    gy, y_real = torch.randn(B, Cout, L, generator=g).cuda(), torch.randn(B, Cout, L, generator=g).cuda()
    gterm = torch.tensor([GTERM], device="cuda")
    runs = []
    for _ in range(2):
        y, partials = msd_ops.stem1d_fm_fwd(x, w, b, y_real, 7)
        runs.append((y, partials, (partials.sum() * COEF).float(), msd_ops.stem1d_fm_bwd(gy, x, w, b, y_real, gterm, COEF, 7)))
    for a, c in zip(*runs):
        assert torch.isfinite(a).all() and torch.equal(a, c)


def _fused_stems(loss):
    """How many _Stem1dFmFn nodes the autograd graph of `loss` holds."""
    seen, stack = set(), [loss.grad_fn]
    while stack:
        n = stack.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        stack.extend(f for f, _ in n.next_functions)
    return sum("Stem1dFm" in type(n).__name__ for n in seen)


def test_fm_refused_shapes_raise_and_the_module_takes_the_composed_route(monkeypatch):
    from vm_asr_amd import _lib, msd_ops
    from vm_asr_amd.mpd_ops import _call
    from vm_asr_amd.msd import MultiScaleDiscriminator
    from vm_asr_amd.msd_featmatch import composed_feature_loss
    g = torch.Generator().manual_seed(6)
    x, w, b = _cuda(torch.randn(2, 1, 50, generator=g), torch.randn(4, 1, 33, generator=g) / 33 ** 0.5, torch.randn(4, generator=g))
    y_real, gterm = torch.zeros(2, 4, 50, device="cuda"), torch.ones(1, device="cuda")
    assert not msd_ops.stem1d_fm_supported_launch(4, 33, 1, 16, 2, 50) and not msd_ops.stem1d_fm_supported_launch(4, 15, 2, 7, 2, 50)
    with pytest.raises(RuntimeError, match="unsupported shape"):                     # k 33
        msd_ops.stem1d_fm_fwd(x, w, b, y_real, 16)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        msd_ops.stem1d_fm_bwd(torch.zeros_like(y_real), x, w, b, y_real, gterm, 1.0, 16)
    w15, part = w[:, :, :15].contiguous(), torch.zeros(64, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported shape"):                     # stride 2 (the bindings always pass 1)
        _call(_lib.lib().vmasr_stem1d_fm_fwd, x, w15, b, y_real, torch.empty_like(y_real), part, part.numel() * 8, 2, 4, 50, 15, 2, 7)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        _call(_lib.lib().vmasr_stem1d_fm_bwd, None, x, w15, b, y_real, gterm, 1.0, torch.empty_like(x), 2, 4, 50, 15, 2, 7)
    torch.cuda.synchronize()
    # a module whose stems have k 33: forward_generator gives the composed route's values (the other maps still take the L1 kernel)
    monkeypatch.setenv("VMASR_MSD_FEAT", "hip")
    torch.manual_seed(9)
    D = MultiScaleDiscriminator(hidden=16)
    for d in D.discriminators:
        d.convs[0] = torch.nn.Conv1d(1, 16, 33, 1, padding=16)
    D = D.cuda().eval()
    real, xg = 0.3 * torch.randn(2, 1, 801, device="cuda"), (0.3 * torch.randn(2, 1, 801, device="cuda")).requires_grad_()
    with torch.no_grad():
        _, f_real = D.forward_single(real, detach_weights=True)
    scores, loss = D.forward_generator(xg, f_real)
    assert _fused_stems(loss) == 0
    dx, = torch.autograd.grad(loss, xg)
    ref_scores, fmaps = D.forward_single(xg, detach_weights=True)
    want = composed_feature_loss(f_real, fmaps)
    dx_ref, = torch.autograd.grad(want, xg)
    for i, (a, c) in enumerate(zip(scores, ref_scores)):      # (the k 33 stem is a library convolution here: values, not bits)
        close(a, c.detach().double().cpu(), GATE, f"fm refused stem: score{i}")
    print(f"fm refused stem loss: hip {loss.item():.9e} composed {want.item():.9e}")
    assert abs(loss.item() - want.item()) <= GATE * abs(want.item())
    close(dx, dx_ref.double().cpu(), GATE, "fm refused stem: dx")


def _spectral_state(D):
    return {k: v.clone() for k, v in D.state_dict().items() if k.endswith("._u") or k.endswith("._v")}


@pytest.fixture
def reproducible_library_ops(monkeypatch):
    """torch's library operators in their deterministic forms for one test (the dense 8h -> 8h k 5 layer and conv_post are library
    convolutions, whose default algorithms are not bit-reproducible from call to call)."""
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    torch.use_deterministic_algorithms(True, warn_only=True)
    yield
    torch.use_deterministic_algorithms(was, warn_only=warn)


def test_module_forward_generator_vs_the_composed_route(monkeypatch, reproducible_library_ops):
    """hidden 16, B 2, T 1201.  Identical weights in both routes: the spectrally normalised weights are baked in first
    (parametrizations removed, so there is no u / v left to snapshot) — on the GPU a training-mode pass does not reproduce its
    weights bit for bit even from restored u / v (the power iteration's column sums end in float atomics), and the scores are
    compared for equality; for the same reason the two library convolutions run in their deterministic forms (measured: without
    them maps 6 and 7 of a scale differ by an ulp between two identical calls).  The power-iteration schedule itself is pinned by
    tests/test_msd_featmatch.py and the trainer step below."""
    from torch.nn.utils import parametrize
    from vm_asr_amd.msd import MultiScaleDiscriminator
    from vm_asr_amd.msd_featmatch import composed_feature_loss
    torch.manual_seed(79)
    D = MultiScaleDiscriminator(hidden=16).cuda().train()
    assert len(_spectral_state(D)) == 48
    for m in list(D.modules()):
        if isinstance(m, torch.nn.Conv1d) and parametrize.is_parametrized(m, "weight"):
            parametrize.remove_parametrizations(m, "weight", leave_parametrized=True)
    real = 0.3 * torch.randn(2, 1, 1201, device="cuda")
    x = (0.3 * torch.randn(2, 1, 1201, device="cuda")).requires_grad_()
    with torch.no_grad():
        _, f_real = D.forward_single(real, detach_weights=True)
    assert len(_spectral_state(D)) == 0

    def total(scores, loss):
        return 2.0 * loss + sum((torch.cos(torch.arange(s.numel(), dtype=s.dtype, device=s.device)).view_as(s) * s).sum() for s in scores)

    monkeypatch.setenv("VMASR_MSD_FEAT", "hip")
    scores, loss = D.forward_generator(x, f_real)
    assert _fused_stems(loss) == 3
    dx, = torch.autograd.grad(total(scores, loss), x)
    assert all(p.grad is None for p in D.parameters())

    ref_scores, fmaps = D.forward_single(x, detach_weights=True)
    want = composed_feature_loss(f_real, fmaps)
    dx_ref, = torch.autograd.grad(total(ref_scores, want), x)
    assert all(p.grad is None for p in D.parameters())
    for i, (a, c) in enumerate(zip(scores, ref_scores)):
        print(f"fm module score{i}: max|hip - composed| {(a - c).abs().max().item():.3e} of {c.abs().max().item():.3e}")
    assert len(scores) == 3 and all(torch.equal(a, c) for a, c in zip(scores, ref_scores))
    print(f"fm module loss: hip {loss.item():.9e} composed {want.item():.9e}")
    assert abs(loss.item() - want.item()) <= GATE * abs(want.item())
    close(dx, dx_ref.double().cpu(), GATE, "fm module dx")

    monkeypatch.setenv("VMASR_MSD_FEAT", "torch")                                    # the switch: exactly the composed route
    scores_t, loss_t = D.forward_generator(x, f_real)
    assert torch.equal(loss_t, want) and all(torch.equal(a, c) for a, c in zip(scores_t, ref_scores))


def test_trainer_step_agrees_between_the_feature_loss_routes(monkeypatch):
    """One eager ["mpd", "msd"] step per switch value from the same state and seed: losses to 1e-5, generator parameters after the
    step within 2e-5 of the largest update."""
    logs, params = {}, {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("VMASR_MSD_FEAT", mode)
        torch.manual_seed(0)
        z, tr = make_trainer("cuda:0")
        before = {n: p.detach().clone() for n, p in tr.models["generator"].named_parameters()}
        wave_target = torch.from_numpy(z["wave_target"]).cuda()
        hf = torch.full((wave_target.shape[0],), 171, dtype=torch.int64, device="cuda")
        _, lg = tr.train_step(wave_target, wave_target, hf)
        logs[mode] = {k: float(v) for k, v in lg.items()}
        params[mode] = {n: p.detach().clone() for n, p in tr.models["generator"].named_parameters()}
    assert logs["hip"].keys() == logs["torch"].keys() and "generator/features_msd" in logs["hip"]
    for k, ref in logs["torch"].items():
        got = logs["hip"][k]
        print(f"{k}: hip {got:.8f} torch {ref:.8f}")
        assert np.isfinite(got) and abs(got - ref) <= 1e-5 * abs(ref), (k, got, ref)
    for n, ref in params["torch"].items():
        update = (ref - before[n]).abs().max().item()
        err = (params["hip"][n] - ref).abs().max().item()
        print(f"{n}: max update {update:.3e} err {err:.3e}")
        assert update > 0 and err <= GATE * update, (n, err, update)
