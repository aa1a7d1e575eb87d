"""Where a VSS block's operator path is chosen (vm_asr_amd/vmamba.py: product_ops_in_force, core_path, SS2D._glue_path; the module
checks the four MFMA wrappers share, vm_asr_amd/mlp.py).  CPU part: the choice functions touch no tensor, and the library's
`*_supported` queries are host code.  GPU part: small modules under spies — the exact multiset of operators each one calls, and the
same numbers as with every fusion knob off."""
import collections
import types
from functools import partial

import pytest
import torch

KNOBS_OFF = ("VMASR_SS2D_FUSED", "VMASR_SS2D_DEEP", "VMASR_SS2D_GLUE", "VMASR_SS2D_PAIRS", "VMASR_FUSED_MLP", "VMASR_FUSED_GMLP",
             "VMASR_FUSED_INPROJ", "VMASR_FUSED_OUTPROJ")
ORDER = ["pairs", "fused", "deep", "xproj", "chain"]
F32, BF16 = torch.float32, torch.bfloat16

# (d_state, dt_rank, d_inner, H, W, dtype) -> the path with every knob on and the pair form wanted.  The SS2D call shapes of the
# shipped configs at n_fft 1024 (DIMS 16: three fused stages, three deep stages of which 256 @ 16 x 16 is the bottleneck; DIMS 32:
# its bottleneck 512 @ 16 x 16 with dt_rank 16, and its d_inner-64 stage at 256 x 256, too long for the deep core), in the fp32 of
# the parity runs and the bf16 the fused in_proj hands over; one general-d_state shape (d_state 32) and one no fused operator takes
# (d_inner 1024 is beyond every kernel's widths and beyond VMASR_XPROJ_MAX_D).
TABLE = {
    (1, 1, 32, 128, 128, F32): "pairs", (1, 1, 16, 256, 256, BF16): "pairs", (1, 1, 2, 512, 512, BF16): "pairs",
    (1, 2, 64, 64, 64, F32): "deep", (1, 4, 128, 32, 32, BF16): "deep", (1, 8, 256, 16, 16, BF16): "deep", (1, 16, 512, 16, 16, BF16): "deep",
    (1, 2, 64, 256, 256, BF16): "xproj", (32, 4, 128, 64, 64, F32): "xproj", (1, 64, 1024, 8, 8, F32): "chain",
}
# ... and where each goes when no fused core may take it: the x_proj map, except where its weights do not fit the map's 64 KiB
# ((2 * 16 + 2) * 512 floats) or d_inner is beyond VMASR_XPROJ_MAX_D
UNFUSED = {k: ("chain" if k[2] >= 512 and k[1] >= 16 else "xproj") for k in TABLE}
KNOB_OF = {"pairs": "VMASR_SS2D_PAIRS", "fused": "VMASR_SS2D_FUSED", "deep": "VMASR_SS2D_DEEP"}


def _parent_path(N, R, D, H, W, dtype, hip_default, delta_softplus, K, pairs):
    """The parent commit's routing, restated from its four predicates in its order: SS2D.forward's pair test (reached only with
    the glue path in force, which implied hip_default and delta_softplus), then forward_corev2's if-chain."""
    from vm_asr_amd import knobs, ss2d_core, ss2d_deep, ss2d_glue, xproj
    if pairs and hip_default and delta_softplus and K == 4 and ss2d_core.supported(N, R, D, H, W) and ss2d_glue.pairs_supported(D, H, W, dtype):
        return "pairs"
    if hip_default and delta_softplus and K == 4 and ss2d_core.supported(N, R, D, H, W):
        return "fused"
    if hip_default and delta_softplus and K == 4 and ss2d_deep.supported(N, R, D, H, W, dtype):
        return "deep"
    if hip_default and xproj.supported(N, R, D) and D <= knobs.get("VMASR_XPROJ_MAX_D"):
        return "xproj"
    return "chain"


def test_core_path_truth_table(monkeypatch):
    """Every shape of TABLE with all knobs on, then with each of VMASR_SS2D_PAIRS / _FUSED / _DEEP off in turn, with and without
    the pair form wanted, with another k_group, without the product operators and without softplus.  The expected column is NOT
    core_path's own output: it is TABLE (written by hand from the kernels' admission rules) and, for every cell, _parent_path —
    the parent commit's four predicates evaluated in the parent's order.  Turning a path's knob off moves a shape to a later
    path of the priority order and never to an earlier one — pairs to fused; fused and deep stages to the x_proj map (the fused
    stages are too narrow for the deep core), the 512-wide bottleneck to the chain —; shapes on another path do not move.
    Without softplus the parent kept the x_proj map where it applies (only the fused cores are softplus-only) and took the generic
    chain otherwise; that is what is asserted, cell by cell — never one of the fused cores."""
    from vm_asr_amd.vmamba import core_path
    for k in KNOB_OF.values():
        monkeypatch.delenv(k, raising=False)
    on = {}
    for key, want in TABLE.items():
        on[key] = core_path(*key, True, True, 4, True)
        assert on[key] == want == _parent_path(*key, True, True, 4, True), key
        merged = core_path(*key, True, True, 4, False)                 # forward_corev2's own question: never the pair form
        assert merged == ("fused" if want == "pairs" else want) == _parent_path(*key, True, True, 4, False), key
        assert core_path(*key, False, True, 4, True) == "chain" == _parent_path(*key, False, True, 4, True), key
        for pairs in (True, False):
            soft = core_path(*key, True, False, 4, pairs)
            assert soft == _parent_path(*key, True, False, 4, pairs) and soft in ("xproj", "chain"), (key, soft)
            assert soft == UNFUSED[key], (key, soft)
            assert core_path(*key, True, True, 2, pairs) == soft, key       # the fused cores are four-direction operators
            assert core_path(*key, False, False, 4, pairs) == "chain", key
    for path, knob in KNOB_OF.items():
        monkeypatch.setenv(knob, "0")
        for key, want in on.items():
            got = core_path(*key, True, True, 4, True)
            assert got == _parent_path(*key, True, True, 4, True), (knob, key)
            if want == path or (path == "fused" and want == "pairs"):       # (no fused core: no pair outputs either)
                assert ORDER.index(got) > ORDER.index(want) and got == ("fused" if path == "pairs" else UNFUSED[key]), (knob, key, got)
            else:
                assert got == want, (knob, key, got)
        monkeypatch.delenv(knob)
    # a float64 module (the tests' adjudicator) never gets pair outputs or the deep core
    assert core_path(1, 4, 128, 32, 32, torch.float64, True, True, 4, True) == "xproj"


class _Stop(Exception):
    pass


def _forms(m, monkeypatch):
    """-> (keyword form, module form) of product_ops_in_force for module `m`, both asked for a GPU tensor: what forward_corev2
    computes from the arguments `m.forward_core` really hands it (observed at core_path, which is stopped there), and what
    SS2D.forward computes from m._core_kw()."""
    from vm_asr_amd import vmamba as vm
    real, seen = vm.product_ops_in_force, []

    def on_gpu(_, *a, **k):
        return real(True, *a, **k)

    def stop(*a, **k):
        seen.append(a[6])
        raise _Stop
    monkeypatch.setattr(vm, "product_ops_in_force", on_gpu)
    monkeypatch.setattr(vm, "core_path", stop)
    with pytest.raises(_Stop):
        m.forward_core(torch.zeros(1, m.d_inner, 4, 4))
    monkeypatch.undo()
    return seen[0], real(True, **m._core_kw())


def test_product_ops_predicate_agrees_in_both_forms(monkeypatch):
    """forward_corev2 (keyword form) and SS2D.forward (module form: the keywords forward_core was bound with) state the product
    operator set through ONE function and get the same answer for every way the repository binds forward_core."""
    from oracle.torch_backend import OracleCrossMerge, OracleCrossScan, OracleSelectiveScan
    from vm_asr_amd.vmamba import SS2D
    x = types.SimpleNamespace(is_cuda=True)
    mk = lambda **kw: SS2D(d_model=8, d_state=1, forward_type=kw.pop("forward_type", "v5"), **kw)      # noqa: E731
    m = mk()
    assert _forms(m, monkeypatch) == (True, True) and m._fused_glue_ok(x)
    m = mk(forward_type="v2no32")
    assert _forms(m, monkeypatch) == (False, False) and not m._fused_glue_ok(x)
    m = mk(channel_first=True)          # the operators are the product's; the glue kernels are channel-last only
    assert _forms(m, monkeypatch) == (True, True) and not m._fused_glue_ok(x)
    m = mk()
    m.forward_core = partial(m.forward_corev2, force_fp32=True, SelectiveScan=OracleSelectiveScan, CrossScan=OracleCrossScan,
                             CrossMerge=OracleCrossMerge)
    assert _forms(m, monkeypatch) == (False, False) and not m._fused_glue_ok(x)
    m = mk()
    m.forward_core = lambda x, **k: m.forward_corev2(x, force_fp32=True, SelectiveScan=OracleSelectiveScan, **k)
    assert _forms(m, monkeypatch) == (False, False) and not m._fused_glue_ok(x)
    m = mk()
    m.conv_act_fn = lambda x, w, b: x   # the core's operators are untouched; the glue path is off (its conv is a hook now)
    assert _forms(m, monkeypatch) == (True, True) and not m._fused_glue_ok(x)
    for kw in (dict(delta_softplus=False), dict(no_einsum=True)):
        m = mk()
        m.forward_core = partial(m.forward_corev2, **{**m.forward_core.keywords, **kw})
        assert _forms(m, monkeypatch) == ((True, True) if "delta_softplus" in kw else (False, False)) and not m._fused_glue_ok(x)
    assert not mk()._fused_glue_ok(types.SimpleNamespace(is_cuda=False))


def _stream(d, dtype=F32, cuda=True):
    """What the checks read of a GPU stream tensor (B, H, W, d)."""
    return types.SimpleNamespace(is_cuda=cuda, dtype=dtype, shape=(2, 16, 16, d), dim=lambda: 4)


def test_module_checks_refuse_what_the_row_kernels_cannot_take(monkeypatch):
    """mlp.supported / gmlp.supported (one body, `gated`), inproj.supported, outproj.supported and the helpers under them, on
    modules built on the CPU; only the stream tensor and the autocast state are stood in for.  Each accepts the block's own
    modules and refuses: Linear2d, LayerNorm2d, a missing (or, for the projections, a present) bias, a LayerNorm without
    affine, a wrong width, tanh-GELU, dropout that is active (training) — and accepts dropout that is idle (eval)."""
    from torch import nn
    from vm_asr_amd import _lib, gmlp as G, inproj, mlp as M, outproj
    from vm_asr_amd.layernorm import LayerNorm
    from vm_asr_amd.linear import Linear
    from vm_asr_amd.vmamba import LayerNorm2d, Linear2d, Mlp, gMlp
    for k in KNOBS_OFF:
        monkeypatch.delenv(k, raising=False)
    d, x = 16, _stream(16)
    assert not M.supported(x, LayerNorm(d), Mlp(d, 4 * d))                  # no autocast
    monkeypatch.setattr(_lib, "bf16_autocast", lambda: True)
    for sup, cls, other in ((M.supported, Mlp, gMlp), (G.supported, gMlp, Mlp)):
        ok = lambda norm=None, mlp=None, xx=x: sup(xx, norm or LayerNorm(d), mlp or cls(d, 4 * d))        # noqa: E731
        assert ok() and ok(xx=_stream(d, BF16)) and ok(norm=nn.LayerNorm(d))
        assert not ok(xx=_stream(d, cuda=False)) and not ok(xx=_stream(d, torch.float16)) and not ok(xx=_stream(d, torch.float64))
        assert not ok(mlp=other(d, 4 * d))                                  # fc1's width says which of the two it is
        assert not ok(mlp=cls(d, 4 * d, channels_first=True))               # Linear2d
        assert not ok(norm=LayerNorm2d(d))
        assert not ok(norm=nn.LayerNorm(d, elementwise_affine=False)) and not ok(norm=nn.LayerNorm(d, bias=False))
        assert not ok(norm=LayerNorm(2 * d)) and not ok(norm=nn.Identity())
        assert not ok(xx=_stream(2 * d)) and not ok(mlp=cls(d, 2 * d)) and not ok(mlp=cls(d, 4 * d, out_features=2 * d))
        for i in (1, 2):
            m = cls(d, 4 * d)
            setattr(m, f"fc{i}", Linear(getattr(m, f"fc{i}").in_features, getattr(m, f"fc{i}").out_features, bias=False))
            assert not ok(mlp=m)
        assert not ok(mlp=cls(d, 4 * d, act_layer=partial(nn.GELU, approximate="tanh"))) and not ok(mlp=cls(d, 4 * d, act_layer=nn.SiLU))
        m = cls(d, 4 * d, drop=0.1)
        assert m.training and not ok(mlp=m)
        assert ok(mlp=m.eval())
        monkeypatch.setenv("VMASR_FUSED_GMLP" if cls is gMlp else "VMASR_FUSED_MLP", "0")
        assert not ok()
        monkeypatch.delenv("VMASR_FUSED_GMLP" if cls is gMlp else "VMASR_FUSED_MLP")
    # the helpers themselves
    assert M.row_linear(Linear(d, d), True) and M.row_linear(Linear(d, d, bias=False), False) and M.row_linear(nn.Linear(d, d), True)
    assert not M.row_linear(Linear(d, d), False) and not M.row_linear(Linear(d, d, bias=False), True)
    assert not M.row_linear(Linear2d(d, d), True) and not M.row_linear(None, True) and not M.row_linear(nn.Identity(), False)
    assert M.row_layernorm(LayerNorm(d), d) and not M.row_layernorm(LayerNorm(d), d + 1) and not M.row_layernorm(LayerNorm2d(d), d)
    assert not M.row_layernorm(nn.LayerNorm(d, elementwise_affine=False), d) and not M.row_layernorm(nn.Identity(), d)
    assert M.amp_stream(x) and M.amp_stream(x, _stream(d, BF16)) and not M.amp_stream(x, _stream(d, cuda=False))
    assert not M.amp_stream(_stream(d, torch.float16))
    monkeypatch.setattr(_lib, "bf16_autocast", lambda: False)
    assert not M.amp_stream(x)
    monkeypatch.setattr(_lib, "bf16_autocast", lambda: True)
    # in_proj: bias-free row Linear d -> 4 d behind an affine LayerNorm of width d or nn.Identity
    inp = lambda norm=None, proj=None, xx=x: inproj.supported(xx, norm or LayerNorm(d), proj or Linear(d, 4 * d, bias=False))   # noqa: E731
    assert inp() and inp(norm=nn.Identity()) and inp(xx=_stream(d, BF16))
    assert not inp(proj=Linear(d, 4 * d)) and not inp(proj=Linear2d(d, 4 * d, bias=False)) and not inp(proj=Linear(2 * d, 4 * d, bias=False))
    assert not inp(norm=LayerNorm2d(d)) and not inp(norm=LayerNorm(2 * d)) and not inp(norm=nn.LayerNorm(d, elementwise_affine=False))
    assert not inp(norm=nn.GELU()) and not inp(xx=_stream(d, cuda=False)) and not inp(xx=_stream(d, torch.float16))
    flat = _stream(d)
    flat.dim = lambda: 3
    assert not inp(xx=flat)
    # out_proj: bf16 gate output (.., 2 d), bias-free row Linear 2 d -> d, no active dropout
    g = types.SimpleNamespace(is_cuda=True, dtype=BF16, shape=(2, 16, 16, 2 * d))
    out = lambda proj=None, gg=g, xx=x, drop=None: outproj.supported(gg, proj or Linear(2 * d, d, bias=False), xx, drop)    # noqa: E731
    assert out() and out(drop=nn.Identity()) and out(drop=nn.Dropout(0.0)) and out(drop=nn.Dropout(0.1).eval())
    assert not out(drop=nn.Dropout(0.1))
    assert not out(proj=Linear(2 * d, d)) and not out(proj=Linear2d(2 * d, d, bias=False)) and not out(proj=Linear(d, d, bias=False))
    assert not out(gg=types.SimpleNamespace(is_cuda=True, dtype=F32, shape=g.shape))
    assert not out(gg=types.SimpleNamespace(is_cuda=False, dtype=BF16, shape=g.shape))
    assert not out(gg=types.SimpleNamespace(is_cuda=True, dtype=BF16, shape=(2, 16, 8, 2 * d)))


# ---- GPU: the operators each module really calls ---------------------------------------------------------------------------------
def _spies(monkeypatch):
    """Every operator a VSS block can reach, wrapped at the module attribute the product looks it up through -> Counter of calls."""
    from vm_asr_amd import selective_scan, vmamba as vm
    calls = collections.Counter()

    def wrap(obj, attr, name=None):
        orig = getattr(obj, attr)

        def spy(*a, **k):
            calls[name or attr] += 1
            return orig(*a, **k)
        monkeypatch.setattr(obj, attr, spy)
    for obj, attrs in ((vm._glue, ("ss2d_pre", "ln_gate", "ln_gate_pairs")), (vm, ("dwconv3x3_silu",)), (vm._ss2d, ("ss2d_core", "ss2d_core_pairs")),
                       (vm._deep, ("ss2d_deep",)), (vm._xproj, ("x_proj_dt",)), (vm._inproj, ("fused_in_proj",)),
                       (vm._outproj, ("fused_out_proj_residual",)), (vm._mlp, ("fused_mlp_residual",)), (vm._gmlp, ("fused_gmlp_residual",))):
        for a in attrs:
            wrap(obj, a)
    wrap(selective_scan, "fwd", "scan")         # SelectiveScanCore.forward's launcher: one call = the four directions' scan
    return calls


def _run(m, x, amp):
    """One forward + backward from a fixed seed (the DropPath draws) -> [y, dx, every parameter gradient]."""
    torch.manual_seed(7)
    xi = x.clone().requires_grad_()
    m.zero_grad()
    with torch.autocast("cuda", dtype=BF16, enabled=amp):
        y = m(xi)
    y.float().square().mean().backward()
    return [y.detach(), xi.grad] + [p.grad.clone() for p in m.parameters()]


def _check(monkeypatch, m, x, want, amp=False, env=()):
    calls = _spies(monkeypatch)
    for k in KNOBS_OFF:
        monkeypatch.delenv(k, raising=False)
    for k in env:
        monkeypatch.setenv(k, "0")
    got = _run(m, x, amp)
    assert calls == collections.Counter(want), dict(calls)
    for k in KNOBS_OFF:
        monkeypatch.setenv(k, "0")
    calls.clear()
    ref = _run(m, x, amp)
    assert not set(calls) - {"dwconv3x3_silu", "x_proj_dt", "scan"}, dict(calls)      # no knob governs these three
    tol = 2e-2 if amp else 1e-3       # test_vssblock_uses_the_fused_mlp_under_autocast_only / test_ss2d_module_uses_deep_core
    assert len(got) == len(ref) and (ref[0].float() - x).abs().max() > 0
    for i, (a, b) in enumerate(zip(got, ref)):
        err, scale = (a.float() - b.float()).abs().max().item(), max(b.abs().max().item(), 1e-12)
        print(f"tensor {i} {tuple(a.shape)}: err {err:.3e} scale {scale:.3e}")
        assert a.dtype == b.dtype and err <= tol * scale, (i, err, scale)


GLUE = ["ss2d_pre", "dwconv3x3_silu"]
SS2D_CASES = {
    "pairs": (dict(d_model=8, d_state=1, forward_type="v5"), (), GLUE + ["ss2d_core_pairs", "ln_gate_pairs"]),
    "no-pairs": (dict(d_model=8, d_state=1, forward_type="v5"), ("VMASR_SS2D_PAIRS",), GLUE + ["ss2d_core", "ln_gate"]),
    "no-fused": (dict(d_model=8, d_state=1, forward_type="v5"), ("VMASR_SS2D_FUSED",), GLUE + ["x_proj_dt", "scan", "ln_gate"]),
    "deep": (dict(d_model=64, d_state=1), (), GLUE + ["ss2d_deep", "ln_gate"]),
    "d_state-8": (dict(d_model=8, d_state=8), (), GLUE + ["x_proj_dt", "scan", "ln_gate"]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(SS2D_CASES))
def test_ss2d_calls_exactly_its_path_operators(case, monkeypatch):
    """fp32, B = 2, 16 x 16 (the smallest image the fused core and the pair gate admit): the multiset of operators SS2D.forward
    calls, and output and every gradient against the same module with every fusion knob off (1e-3 of each tensor's scale)."""
    from vm_asr_amd.vmamba import SS2D
    kw, env, want = SS2D_CASES[case]
    torch.manual_seed(0)
    m = SS2D(**kw).cuda()
    x = torch.randn(2, 16, 16, kw["d_model"], device="cuda")
    _check(monkeypatch, m, x, want, env=env)


@pytest.mark.gpu
@pytest.mark.parametrize("train", [True, False], ids=["train-droppath", "eval"])
@pytest.mark.parametrize("gated", [False, True], ids=["mlp", "gmlp"])
def test_vssblock_under_autocast_calls_each_fused_operator_once(gated, train, monkeypatch):
    """VSSBlock(hidden_dim=16, ssm_d_state=1) under bf16 autocast, B = 2, 16 x 16, in training with drop_path > 0 and in eval:
    fused in_proj, conv, pair core, pair gate, fused out_proj + residual and the fused (gated) Mlp, each exactly once and nothing
    else; output and every gradient within 2e-2 of the same block with every fusion knob off, same DropPath draws."""
    from vm_asr_amd.vmamba import VSSBlock
    torch.manual_seed(0)
    blk = VSSBlock(hidden_dim=16, drop_path=0.3, ssm_d_state=1, ssm_dt_rank="auto", forward_type="v5", gmlp=gated).cuda()
    blk.train(train)
    x = torch.randn(2, 16, 16, 16, device="cuda")
    want = ["fused_in_proj", "dwconv3x3_silu", "ss2d_core_pairs", "ln_gate_pairs", "fused_out_proj_residual",
            "fused_gmlp_residual" if gated else "fused_mlp_residual"]
    _check(monkeypatch, blk, x, want, amp=True)
