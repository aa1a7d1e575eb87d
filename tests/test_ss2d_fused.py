"""The fused SS2D core (vm_asr_amd/csrc/ss2d.hip: cross-scan + x_proj + dt_proj + 4 selective scans + cross-merge as
one operator, forward and backward) against the oracle's composition of the SAME reference steps
(model/vmamba.py:1472-1497: CrossScan -> einsum x2 -> selective_scan_ref -> CrossMerge; each oracle piece is pinned
to reference goldens in tests/test_oracle.py), in fp32 and — as adjudicator — in float64."""
import numpy as np
import pytest
import torch

SHAPES = [(2, 32, 16, 16), (1, 16, 32, 32), (2, 8, 16, 32), (1, 4, 32, 32), (2, 2, 64, 64), (1, 32, 64, 128), (1, 16, 128, 64)]
# the three fused call shapes of vm_asr_48k at B = 1 (enc0/out0, out1, out2) — the oracle chain does them in seconds
BENCH_SHAPES = [(1, 32, 128, 128), (1, 16, 256, 256), (1, 2, 512, 512)]


def _params(D, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)      # noqa: E731
    Wx = ((2 * r(4, 3, D) - 1) / D ** 0.5)
    Wdt = (2 * r(4, D, 1) - 1)
    dt = torch.exp(r(4, D) * (np.log(0.1) - np.log(1e-3)) + np.log(1e-3))
    dtb = dt + torch.log(-torch.expm1(-dt))                                # softplus^-1 (model/vmamba.py:886-905)
    A_logs = 0.3 * (2 * r(4 * D, 1) - 1)
    Ds = 1 + 0.2 * (2 * r(4 * D) - 1)
    return [t.to(dtype) for t in (Wx, Wdt, dtb, A_logs, Ds)]


def _oracle_ys(x, Wx, Wdt, dtb, A_logs, Ds):
    """model/vmamba.py:1472-1496 on the oracle's kernels (dtype follows the active oracle build): the four directional scans'
    outputs (B, 4 D, L), before CrossMerge."""
    from oracle.torch_backend import OracleCrossScan, OracleSelectiveScan
    B, D, H, W = x.shape
    L = H * W
    xs = OracleCrossScan.apply(x)
    x_dbl = torch.einsum("b k d l, k c d -> b k c l", xs, Wx)
    dts, Bs, Cs = torch.split(x_dbl, [1, 1, 1], dim=2)
    dts = torch.einsum("b k r l, k d r -> b k d l", dts, Wdt)
    return OracleSelectiveScan.apply(xs.reshape(B, -1, L), dts.contiguous().view(B, -1, L), -torch.exp(A_logs), Bs.contiguous(),
                                     Cs.contiguous(), Ds, dtb.reshape(-1), True)


def _oracle_core(x, Wx, Wdt, dtb, A_logs, Ds):
    """model/vmamba.py:1472-1497 on the oracle's kernels (dtype follows the active oracle build)."""
    from oracle.torch_backend import OracleCrossMerge
    B, D, H, W = x.shape
    return OracleCrossMerge.apply(_oracle_ys(x, Wx, Wdt, dtb, A_logs, Ds).view(B, 4, D, H, W))


def _oracle_pairs(x, Wx, Wdt, dtb, A_logs, Ds):
    """The same steps stopped before CrossMerge's transposing add (model/csm_triton.py:82-154 without its last step), in plain torch:
    -> (y0 + flip(y2) in (h,w) order, y1 + flip(y3) in (w,h) order), what ss2d_core_pairs returns.  No HIP code."""
    B, D, H, W = x.shape
    ys = _oracle_ys(x, Wx, Wdt, dtb, A_logs, Ds).view(B, 4, D, H * W)
    return ys[:, 0] + torch.flip(ys[:, 2], dims=[-1]), ys[:, 1] + torch.flip(ys[:, 3], dims=[-1])


def _run(fn, x, params, gy):
    """-> [output(s)..., dx, dWx, dWdt, ddtb, dA_logs, dDs] of the loss sum_i <gy_i, output_i> (gy: one tensor, or one per output)."""
    x = x.clone().requires_grad_()
    ps = [p.clone().requires_grad_() for p in params]
    y = fn(x, *ps)
    ys, gys = (list(y), list(gy)) if isinstance(y, (tuple, list)) else ([y], [gy])
    torch.autograd.backward(ys, [g.to(o.dtype).to(o.device) for o, g in zip(ys, gys)])
    return [o.detach() for o in ys] + [t.grad.detach() for t in [x] + ps]


NAMES = ["y", "dx", "dWx", "dWdt", "ddtb", "dA_logs", "dDs"]
NAMES_PAIRS = ["out02", "out13"] + NAMES[1:]
U16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}       # unit roundoff of one round-to-nearest store


def _dx16_share(a, c, e_cpu, dtype):
    """Largest |dx_hip - dx64| / bound over the elements of a 16-bit dx, with
        bound = u |dx64| + (1 + u) (2.5 e_cpu + 2e-8) max|dx64|      (+ 2^-25 in fp16: half its subnormal spacing).
    Derived, not measured: the kernels compute dx in fp32, where the fp32 gate of _compare holds it within E = (2.5 e_cpu + 2e-8)
    max|dx64| of float64, and the ONLY rounding to T is the last store of merge_pairs_kernel<T>: |rn(v) - v| <= u |v| and
    |v| <= |dx64| + E."""
    u = U16[dtype]
    bound = u * c.abs() + (1 + u) * (2.5 * e_cpu + 2e-8) * c.abs().max()
    if dtype == torch.float16:
        bound = bound + 2.0 ** -25
    return ((a - c).abs() / bound).max().item()


def _compare(tag, names, got, ref, r64, dtype=torch.float32):
    """The gates of every oracle comparison in this file: got (HIP), ref (oracle fp32 chain) and r64 (its float64 build) hold the
    tensors called `names`; dtype is that of x and dx.  One line per tensor is printed (pytest -s: profiles/ss2d_fused_types.md)."""
    for n, a, b, c in zip(names, got, ref, r64):
        a, b = a.double().cpu(), b.double()
        assert a.shape == c.shape, n
        scale = max(c.abs().max().item(), 1e-12)
        e_hip, e_cpu = (a - c).abs().max().item() / scale, (b - c).abs().max().item() / scale
        r_hip, r_cpu = (a - c).pow(2).mean().sqrt().item() / scale, (b - c).pow(2).mean().sqrt().item() / scale
        print(f"{tag} {n}: |hip - f64| max {e_hip:.2e} rms {r_hip:.2e}  |oracle fp32 chain - f64| max {e_cpu:.2e} rms {r_cpu:.2e}")
        if n == "dx" and dtype != torch.float32:
            share = _dx16_share(a, c, e_cpu, dtype)
            print(f"{tag} dx: largest |hip - f64| / (fp32 gate + one store rounded to {str(dtype)[6:]}) {share:.3f}")
            assert share <= 1.0, (tag, n, share, e_hip, e_cpu)
        elif n in ("y", "out02", "out13", "dx"):
            k_max, k_rms = (2.5, 2.0) if n == "dx" else (1.5, 1.5)            # dx measured: 1.5-1.6x in RMS, <= 2.3x max
            assert e_hip <= 1e-4, (tag, n, e_hip, e_cpu)                      # north_star (fp32)
            assert e_hip <= k_max * e_cpu + 2e-8, (tag, n, e_hip, e_cpu)
            assert r_hip <= k_rms * r_cpu + 2e-9, (tag, n, r_hip, r_cpu)
        else:
            assert e_hip <= 6 * e_cpu + 2e-6, (tag, n, e_hip, e_cpu)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES + BENCH_SHAPES)
def test_fused_core_matches_oracle_chain_fp32(shape):
    """Fused HIP core vs the oracle's chain of the reference steps, adjudicated by the float64 build of the same chain —
    at small shapes AND at the benchmark call shapes.  Bounds (round 3, after the decay exp stopped being v_exp_f32 —
    csrc/scan_prims.h decay_f): the output and dx are as close to float64 as the sequential fp32 recurrence of
    selective_scan_ref (y: x1.5 in the max norm and in RMS, + 2e-8 of scale; dx: x2.5 / x2); parameter gradients (fp32 sums over up to
    262 144 positions per row) within 6x its distance + 2e-6 of scale.  Measured on MI355X
    (profiles/r03_accuracy_probe.log): y 8e-9 RMS / 8e-8..1.6e-7 max of scale for both; with v_exp_f32 the HIP output
    was 1.7x and d(A_logs), d(dt_bias) 10-40x further from float64 than the oracle chain."""
    import oracle
    from vm_asr_amd.ss2d_core import ss2d_core, supported
    B, D, H, W = shape
    assert supported(1, 1, D, H, W)
    g = torch.Generator().manual_seed(D * 7 + H)
    x = torch.randn(B, D, H, W, generator=g)
    gy = torch.randn(B, D, H * W, generator=g)
    params = _params(D, D + 1)
    got = _run(ss2d_core, x.cuda(), [p.cuda() for p in params], gy)
    ref = _run(_oracle_core, x, params, gy)
    with oracle.float64():
        r64 = _run(_oracle_core, x.double(), _params(D, D + 1, torch.float64), gy.double())
    _compare(shape, NAMES, got, ref, r64)


@pytest.mark.gpu
def test_fused_core_bf16_activations():
    """Under autocast x arrives in bf16 (the depthwise conv's output): values are converted on load, arithmetic stays
    fp32, dx leaves in bf16.  Against the oracle chain on the same bf16-rounded x: y to 1e-4; dx, element by element against the
    float64 chain, to the fp32 gate plus the one bf16 rounding of its store (_dx16_share)."""
    import oracle
    from vm_asr_amd.ss2d_core import ss2d_core
    B, D, H, W = 2, 32, 32, 32
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, D, H, W, generator=g).to(torch.bfloat16)
    gy = torch.randn(B, D, H * W, generator=g)
    params = _params(D, 9)
    got = _run(ss2d_core, x.cuda(), [p.cuda() for p in params], gy)
    ref = _run(_oracle_core, x.float(), params, gy)
    with oracle.float64():
        dx64 = _run(_oracle_core, x.double(), _params(D, 9, torch.float64), gy.double())[1]
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.bfloat16
    for n, a, b in zip(NAMES, got, ref):
        if n == "dx":
            e_cpu = (b.double() - dx64).abs().max().item() / dx64.abs().max().item()
            share = _dx16_share(a.double().cpu(), dx64, e_cpu, torch.bfloat16)
            print(f"{(B, D, H, W)} bfloat16 dx: largest |hip - f64| / (fp32 gate + one store rounded to bfloat16) {share:.3f}")
            assert share <= 1.0, (n, share, e_cpu)
            continue
        err, scale = (a.float().cpu() - b).abs().max().item(), b.abs().max().item()
        assert err <= 2e-4 * scale, (n, err, scale)


# ---- 16-bit activations, pair outputs and images that are no multiple of the 64-wide transpose tile -----------------------------------
# (B, D, H, W): per template instance of SS2D_DISPATCH / SS2D_DISPATCH_BWD (csrc/ss2d.hip, <T, rows per wave, waves per tile, tiles per
# workgroup>) the smallest image with more than one tile group per image; tiles = H W / 256 must be a multiple of the tiles per
# workgroup of forward AND backward (cfg_for): 4 for d_inner 2 and 4, 2 for d_inner 8, 1 for d_inner 16 and 32.
CASES = [(2, 2, 24, 128),     # 12 tiles: fwd and bwd <2,1,4>, three tile groups; H < 64, W = two transpose tiles
         (2, 4, 128, 24),     # 12 tiles: fwd <4,1,4>, bwd <2,2,2>; the transposed geometry
         (2, 8, 48, 32),      #  6 tiles: fwd <4,2,2>, bwd <2,4,1>
         (2, 16, 40, 96),     # 15 tiles: fwd <4,4,1>, bwd <2,8,1>; odd tile count, ragged second transpose tile
         (2, 32, 96, 40),     # 15 tiles: fwd and bwd <4,8,1>
         (1, 16, 4, 64),      #  1 tile, H shorter than the transpose kernels' 4-row stride
         (1, 32, 64, 4)]      #  1 tile, W shorter than it
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
_ids = dict(ids=lambda v: str(v).replace("torch.", "").replace(" ", ""))


def _transpose_hw(t, H, W):
    """(B, D, H W) in (h,w) order -> (B, D, W H) in (w,h) order."""
    B, D, _ = t.shape
    return t.view(B, D, H, W).transpose(-1, -2).reshape(B, D, W * H)


def _case_inputs(shape, dtype):
    """x rounded to dtype on the host (the references take it up-converted, which is exact), two independent fp32 gradients."""
    B, D, H, W = shape
    g = torch.Generator().manual_seed(D * 7 + H)
    x = torch.randn(B, D, H, W, generator=g).to(dtype)
    return x, torch.randn(B, D, H * W, generator=g), torch.randn(B, D, W * H, generator=g)


def _references(fn, x, D, gy):
    """(oracle fp32 chain, its float64 build) of `fn` on the exactly up-converted x."""
    import oracle
    ref = _run(fn, x.float(), _params(D, D + 1), gy)
    with oracle.float64():
        r64 = _run(fn, x.double(), _params(D, D + 1, torch.float64), [t.double() for t in gy] if isinstance(gy, list) else gy.double())
    return ref, r64


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape", CASES, **_ids)
def test_fused_core_merged_output_every_dtype_and_instance(shape, dtype):
    """ss2d_core with x in fp32 / bf16 / fp16 at CASES, against the oracle chain in fp32 and float64 on the same rounded x.  The
    kernels convert on load and compute in fp32, y and the parameter gradients are fp32: they keep the fp32 gates of
    test_fused_core_matches_oracle_chain_fp32 for all three types; dx in bf16 / fp16 is held, element by element, to the fp32 gate
    plus its one rounded store (_dx16_share)."""
    from vm_asr_amd.ss2d_core import ss2d_core, supported
    B, D, H, W = shape
    assert supported(1, 1, D, H, W)
    x, gy, _ = _case_inputs(shape, dtype)
    got = _run(ss2d_core, x.cuda(), [p.cuda() for p in _params(D, D + 1)], gy)
    assert got[0].dtype == torch.float32 and got[1].dtype == dtype
    ref, r64 = _references(_oracle_core, x, D, gy)
    _compare(f"{shape} {str(dtype)[6:]} merged", NAMES, got, ref, r64, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape", CASES, **_ids)
def test_fused_core_pair_outputs_every_dtype_and_instance(shape, dtype):
    """ss2d_core_pairs (what the trainer calls, VMASR_SS2D_PAIRS) against _oracle_pairs, a reference without HIP code, under the loss
    <g02, out02> + <g13, out13> with INDEPENDENT g02 and g13: a backward that derived one order's gradient from the other's would
    fail.  out02 and out13 keep the gates of y, the gradients those of the merged test."""
    from vm_asr_amd.ss2d_core import ss2d_core_pairs, supported
    B, D, H, W = shape
    assert supported(1, 1, D, H, W)
    x, g02, g13 = _case_inputs(shape, dtype)
    got = _run(ss2d_core_pairs, x.cuda(), [p.cuda() for p in _params(D, D + 1)], [g02, g13])
    assert got[0].dtype == got[1].dtype == torch.float32 and got[2].dtype == dtype
    ref, r64 = _references(_oracle_pairs, x, D, [g02, g13])
    _compare(f"{shape} {str(dtype)[6:]} pairs", NAMES_PAIRS, got, ref, r64, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CASES, **_ids)
def test_fused_core_pair_outputs_bit_equal_merged_fp32(shape):
    """fp32: the merge kernel is ONE fp32 add per element, so out02 + transpose(out13) formed with torch is ss2d_core's y bit for
    bit; and with g13 = transpose(g02) the pair backward runs the kernels of the merged backward on the same inputs (no atomics):
    every gradient is bit-equal to the merged mode's for gy = g02."""
    from vm_asr_amd.ss2d_core import ss2d_core, ss2d_core_pairs
    B, D, H, W = shape
    x, g02, _ = _case_inputs(shape, torch.float32)
    params = [p.cuda() for p in _params(D, D + 1)]
    merged = _run(ss2d_core, x.cuda(), params, g02)
    pairs = _run(ss2d_core_pairs, x.cuda(), params, [g02, _transpose_hw(g02, H, W)])
    assert torch.equal(pairs[0] + _transpose_hw(pairs[1], W, H), merged[0]), shape
    for n, a, b in zip(NAMES[1:], pairs[2:], merged[1:]):
        assert torch.equal(a, b), (shape, n, (a - b).abs().max().item())


# ---- refused shapes ----------------------------------------------------------------------------------------------------------------------
# (d_state, dt_rank, d_inner, H, W) that vmasr_ss2d_supported must refuse
REFUSED = [(1, 1, 4, 16, 32),      # two tiles: the forward of d_inner 4 takes four per workgroup (its backward, two, would accept)
           (1, 1, 8, 16, 16),      # one tile: the forward of d_inner 8 takes two (its backward, one)
           (1, 1, 2, 24, 32),      # three tiles, four per workgroup
           (1, 1, 3, 32, 32), (1, 1, 64, 32, 32),
           (1, 1, 16, 20, 20),     # H W = 400: no whole number of 256-position tiles
           (2, 1, 16, 32, 32), (1, 2, 16, 32, 32)]


@pytest.mark.gpu
def test_supported_truth_table():
    """vmasr_ss2d_supported against the rule of cfg_for: d_state 1, dt_rank 1, d_inner in {2, 4, 8, 16, 32}, H W / 256 a whole
    number and a multiple of the tiles per workgroup of forward and backward."""
    from vm_asr_amd.ss2d_core import supported
    for B, D, H, W in CASES:
        assert supported(1, 1, D, H, W), (D, H, W)
    for q in REFUSED:
        assert not supported(*q), q


@pytest.mark.gpu
@pytest.mark.parametrize("case", [q for q in REFUSED if q[:2] == (1, 1) and q[2] in (2, 4, 8, 16, 32)], **_ids)
def test_fused_core_refuses_unsupported_shape(case):
    """The host-side checks of vmasr_ss2d_fwd turn a refused shape into a RuntimeError; they return before the first launch."""
    from vm_asr_amd.ss2d_core import ss2d_core
    _, _, D, H, W = case
    x = torch.randn(1, D, H, W, device="cuda")
    with pytest.raises(RuntimeError, match="ss2d_fwd.*multiple of"):
        ss2d_core(x, *[p.cuda() for p in _params(D, 1)])
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(4, 32, 128, 128), (4, 16, 256, 256), (4, 2, 512, 512)])
def test_fused_core_equals_unfused_hip_chain_at_benchmark_shapes(shape):
    """BASELINE sizes (B = 4, the three fused stages of vm_asr_48k): the fused operator against the unfused HIP chain
    of round 1 (CrossScanF32 -> xproj -> SelectiveScanCore -> CrossMerge, each oracle-checked in test_gpu_kernels.py):
    output and dx agree to 2e-4 of the tensor scale, parameter gradients (fp32 sums over B*L = 65 k .. 1 M positions
    in different orders) to 1e-3."""
    from vm_asr_amd import xproj
    from vm_asr_amd.csm import CrossMergeHIP, CrossScanF32
    from vm_asr_amd.selective_scan import SelectiveScanCore
    from vm_asr_amd.ss2d_core import ss2d_core
    B, D, H, W = shape
    L = H * W

    def chain(x, Wx, Wdt, dtb, A_logs, Ds):
        xs = CrossScanF32.apply(x)
        dts, Bs, Cs = xproj.x_proj_dt(xs, Wx, Wdt, 1)
        ys = SelectiveScanCore.apply(xs.view(B, -1, L), dts, -torch.exp(A_logs.float()), Bs, Cs, Ds.float(), dtb.view(-1).float(), True)
        return CrossMergeHIP.apply(ys.view(B, 4, D, H, W))
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, D, H, W, generator=g).cuda()
    gy = torch.randn(B, D, L, generator=g)
    params = [p.cuda() for p in _params(D, 5)]
    got, ref = _run(ss2d_core, x, params, gy), _run(chain, x, params, gy)
    for i, (n, a, b) in enumerate(zip(NAMES, got, ref)):
        err, scale = (a - b).abs().max().item(), max(b.abs().max().item(), 1e-12)
        assert err <= (2e-4 if i < 2 else 1e-3) * scale, (shape, n, err, scale)


@pytest.mark.gpu
def test_fused_core_scan_properties_full_size():
    """Size-independent properties at the largest fused call (d_inner 2, 512 x 512, B = 4): linear in Ds (y(Ds) -
    y(0) = sum_k Ds_k u exactly as cross-merge adds the four D*u terms), and zero input -> zero output."""
    from vm_asr_amd.ss2d_core import ss2d_core
    B, D, H, W = 4, 2, 512, 512
    x = torch.randn(B, D, H, W, device="cuda")
    params = [p.cuda() for p in _params(D, 4)]
    y1 = ss2d_core(x, *params)
    p0 = list(params)
    p0[4] = torch.zeros_like(params[4])
    y0 = ss2d_core(x, *p0)
    want = params[4].view(4, D).sum(0).view(1, D, 1) * x.view(B, D, -1)
    assert torch.allclose(y1 - y0, want, rtol=1e-4, atol=1e-4 * want.abs().max().item())
    assert float(ss2d_core(torch.zeros_like(x), *params).abs().max()) == 0.0
