"""The 16-bit and multi-pass paths of three generator operators against float64 (pytest -m gpu):

  * the small Linear row map (vm_asr_amd/csrc/linear.hip): all five (x, y) dtype pairs forward AND backward over all 15 admitted
    (in, out) shapes, row counts below one thread's four rows, the second grid-stride trip, null dx / null db;
  * depthwise 3x3 conv + bias + SiLU (csrc/dwconv.hip): the fp16 / bf16 instantiations of the scalar and the vectorised kernels,
    planes of more than one workgroup whose chunk boundary falls inside an image row, one-vector rows, one-row images;
  * x_proj / dt_proj (csrc/xproj.hip, csrc/xproj_n.hip) with 16-bit xs: one shape per kernel family.

Reference: the activations are rounded to the dtype under test first, then plain torch ops + autograd in float64 on the CPU (weights
stay fp32).  The kernels accumulate in fp32 and round once on store, so
  fp32 outputs   : the fp32 tolerances of the operator's existing test in tests/test_gpu_kernels.py (rtol 1e-4, atol below);
  16-bit outputs : |got - want| <= u |want| + a,  u the type's unit roundoff (2^-8 bf16, 2^-11 fp16) WITHOUT a multiplier (a kernel
                   that truncates errs by up to 2u), a the same fp32 atol (+ 2^-25 in fp16: half the smallest subnormal).
Before anything is launched every case asserts on the CPU that the same expression evaluated in fp32 and rounded once to the output type
meets these bounds (they are attainable for these inputs) and that max|want| < 1e3 (nothing near fp16's overflow).  Every element is
compared; nothing is masked."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
UNIT = {BF16: 2.0 ** -8, F16: 2.0 ** -11}
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
SCALED = "scaled"     # atol = 1e-4 max(1, max|want|), test_gpu_kernels._scaled


def _leaf(t, prec, grad=True):
    """A fresh leaf in `prec` (never the input itself: .to() of a tensor already in `prec` returns that tensor)."""
    return t.detach().to(prec, copy=True).requires_grad_(grad)


def _np64(t):
    return t.detach().cpu().to(torch.float64).numpy()


def _allowed(want, dtype, atol):
    """Per-element bound for an output stored as `dtype` (module docstring)."""
    a = 1e-4 * max(1.0, float(np.abs(want).max()) if want.size else 0.0) if atol == SCALED else atol
    if dtype == F32:
        return a + 1e-4 * np.abs(want)
    return UNIT[dtype] * np.abs(want) + a + (2.0 ** -25 if dtype == F16 else 0.0)


def _check(what, got, want, dtype, atol, record=True):
    assert got.dtype == dtype, (what, got.dtype, dtype)
    got, want = _np64(got), _np64(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    diff, lim = np.abs(got - want), _allowed(want, dtype, atol)
    if record and got.size:
        import errtable
        errtable.record(what, got, want, float(lim.flat[int(np.argmax(diff))]))
    bad = int(np.argmax(diff - lim))
    assert (diff <= lim).all(), (f"{what} [{NAME[dtype]}]: {int((diff > lim).sum())} of {diff.size} elements out of bound; worst at flat "
                                 f"index {bad}: got {got.flat[bad]!r}, want {want.flat[bad]!r}, allowed {lim.flat[bad]:.3e}")


def _attainable(spec, want, ref32):
    """spec: name -> (output dtype, atol).  The float64 reference evaluated in fp32 and rounded to the output type meets the bound."""
    for name, (dtype, atol) in spec.items():
        assert float(want[name].abs().max()) < 1e3, (name, float(want[name].abs().max()))
        _check(f"cpu-fp32 {name}", ref32[name].to(dtype), want[name], dtype, atol, record=False)


def _compare(spec, got, want, tag):
    for name, (dtype, atol) in spec.items():
        _check(f"{tag} {name}", got[name], want[name], dtype, atol)


@pytest.mark.parametrize("dt,drop", [(BF16, 16), (F16, 13)], ids=["bf16", "f16"])
def test_16bit_bound_rejects_a_store_that_truncates(dt, drop):
    """The bound has teeth (CPU only): the fp32 evaluation rounded to nearest passes, the same values with the mantissa bits below
    the 16-bit type's cut off (what a kernel storing the upper half of the fp32 word would write) do not."""
    (x, w, b, gy), _, want = _linear_case(4099, (8, 4), (F32, dt))
    y32 = _linear_ref(x, w, b, gy, F32, True)["y"]
    _check("nearest y", y32.to(dt), want["y"], dt, 1e-4, record=False)
    cut = (y32.view(torch.int32) & ~((1 << drop) - 1)).view(F32)
    assert torch.equal(cut.to(dt).float(), cut)                       # representable: .to(dt) adds no rounding of its own
    with pytest.raises(AssertionError, match="out of bound"):
        _check("truncated y", cut.to(dt), want["y"], dt, 1e-4, record=False)


# ------------------------------------------------------------------------------------------
# small Linear
# ------------------------------------------------------------------------------------------
SL_SHAPES = [(1, 1), (1, 2), (1, 4), (1, 8), (2, 1), (2, 2), (2, 4), (2, 8), (4, 1), (4, 2), (4, 4), (4, 8), (8, 1), (8, 2), (8, 4)]
SL_PAIRS = [(F32, F32), (BF16, BF16), (F32, BF16), (F16, F16), (F32, F16)]     # dispatch<KIND> of csrc/linear.hip: (x, y / gy)
_io_id = lambda io: f"{io[0]}to{io[1]}"                          # noqa: E731
_pair_id = lambda p: f"{NAME[p[0]]}-{NAME[p[1]]}"                # noqa: E731


def _linear_ref(x, w, b, gy, prec, need_dx):
    xr, wr = _leaf(x, prec, need_dx), _leaf(w, prec)
    br = None if b is None else _leaf(b, prec)
    y = F.linear(xr, wr, br)
    y.backward(gy.to(prec))
    out = dict(y=y.detach(), dW=wr.grad)
    if need_dx:
        out["dx"] = xr.grad
    if b is not None:
        out["db"] = br.grad
    return out


def _linear_case(rows, io, pair, bias=True, need_dx=True, xscale=1.0, gscale=1.0):
    """-> inputs (x and gy rounded to their dtypes), what to compare, the float64 expectation (attainability asserted)."""
    (IN, OUT), (tx, ty) = io, pair
    g = torch.Generator().manual_seed(1000 * IN + 10 * OUT + rows % 97)
    x = (xscale * torch.randn(rows, IN, generator=g)).to(tx)
    w = torch.randn(OUT, IN, generator=g)
    b = torch.randn(OUT, generator=g) if bias else None
    gy = (gscale * torch.randn(rows, OUT, generator=g)).to(ty)
    spec = dict(y=(ty, 1e-4), dW=(F32, SCALED))
    if need_dx:
        spec["dx"] = (tx, 1e-4)
    if bias:
        spec["db"] = (F32, SCALED)
    want = _linear_ref(x, w, b, gy, torch.float64, need_dx)
    _attainable(spec, want, _linear_ref(x, w, b, gy, F32, need_dx))
    return (x, w, b, gy), spec, want


def _linear_gpu(inputs, pair, need_dx=True):
    from vm_asr_amd.linear import _SmallLinearFn
    x, w, b, gy = inputs
    xd = x.to(DEV).requires_grad_(need_dx)
    wd = w.to(DEV).requires_grad_()
    bd = None if b is None else b.to(DEV).requires_grad_()
    y = _SmallLinearFn.apply(xd, wd, bd, pair[1])
    y.backward(gy.to(DEV))
    assert (xd.grad is not None) == need_dx
    got = dict(y=y.detach(), dW=wd.grad)
    if need_dx:
        got["dx"] = xd.grad
    if b is not None:
        got["db"] = bd.grad
    return got


def _linear_run(tag, rows, io, pair, **kw):
    need_dx = kw.get("need_dx", True)
    inputs, spec, want = _linear_case(rows, io, pair, **kw)
    _compare(spec, _linear_gpu(inputs, pair, need_dx), want, tag)


@pytest.mark.parametrize("pair", SL_PAIRS, ids=_pair_id)
@pytest.mark.parametrize("io", SL_SHAPES, ids=_io_id)
def test_small_linear_all_shapes_all_dtype_pairs(io, pair):
    """Every (in, out) instantiation of launch_io's shape table x every dtype pair, forward and backward (gy arrives in y's dtype: the mixed f32/16-bit
    backward is the one an autocast step takes), at a ragged row count (4099 % 4 == 3)."""
    _linear_run("linear", 4099, io, pair)


@pytest.mark.parametrize("pair", [(F32, F32), (BF16, BF16), (F32, BF16)], ids=_pair_id)
@pytest.mark.parametrize("io", [(1, 4), (8, 4), (4, 8)], ids=_io_id)
@pytest.mark.parametrize("rows", [1, 2, 3, 5])
def test_small_linear_fewer_rows_than_one_thread_owns(rows, io, pair):
    """Row counts the Python gate (_MIN_ROWS) never lets through: the vector load's `i0 + 3 < len` fallback and the 4-row tail are the
    whole launch."""
    _linear_run("linear-tiny", rows, io, pair)


@pytest.mark.parametrize("pair", [(F32, F32), (F32, BF16)], ids=_pair_id)
@pytest.mark.parametrize("io", [(1, 4), (4, 1), (8, 4)], ids=_io_id)
def test_small_linear_second_grid_stride_trip(io, pair):
    """rows = 1024 workgroups x 256 threads x 4 rows + 2049: grid_for caps the grid, the second trip is partly populated and
    rows % 4 == 1.  (x, gy scaled so that the 10^6-term sums dW, db stay below 1e3.)"""
    _linear_run("linear-2trips", 1024 * 256 * 4 + 2049, io, pair, xscale=0.5, gscale=0.125)


@pytest.mark.parametrize("pair", SL_PAIRS, ids=_pair_id)
@pytest.mark.parametrize("io", [(1, 4), (4, 1), (8, 4)], ids=_io_id)
@pytest.mark.parametrize("null", ["dx", "db"])
def test_small_linear_null_outputs(null, io, pair):
    """x.requires_grad = False -> dx == nullptr (dW, db still right); bias = None -> db == nullptr (dW, dx still right)."""
    _linear_run(f"linear-no-{null}", 4099, io, pair, bias=null != "db", need_dx=null != "dx")


# ------------------------------------------------------------------------------------------
# depthwise 3x3 conv + bias + SiLU
# ------------------------------------------------------------------------------------------
# fp32 atol of y / dx: 1e-5, what test_dwconv_silu_golden_and_oracle holds them to (tighter than the Linear's 1e-4)
DW_CASES = {
    # id: (B, C, H, W, bias, dtypes)
    "48x48-vec-2-workgroups-boundary-in-row-42": (2, 3, 48, 48, True, (F16, BF16, F32)),
    "45x47-scalar-boundary-mid-row": (2, 3, 45, 47, True, (F16, BF16, F32)),
    "5x4-one-vector-per-row": (2, 3, 5, 4, True, (F16, BF16, F32)),
    "1x8-no-row-above-or-below": (2, 3, 1, 8, True, (F16, BF16, F32)),
    "1x1": (2, 3, 1, 1, True, (F16, BF16, F32)),
    "7x130-ragged-scalar": (2, 3, 7, 130, True, (F16, BF16)),                       # fp32: test_dwconv_silu_golden_and_oracle
    "384x384-pass-a-chunk-3072": (1, 1, 384, 384, True, (BF16, F32)),
    "48x48-no-bias": (2, 3, 48, 48, False, (BF16,)),
    "45x47-no-bias": (2, 3, 45, 47, False, (F16,)),
}
DW_PARAMS = [pytest.param(k, dt, id=f"{k}-{NAME[dt]}") for k, v in DW_CASES.items() for dt in v[5]]


def _dwconv_ref(x, w, b, gy, prec):
    xr, wr = _leaf(x, prec), _leaf(w, prec)
    br = None if b is None else _leaf(b, prec)
    y = F.silu(F.conv2d(xr, wr, br, padding=1, groups=x.shape[1]))
    y.backward(gy.to(prec))
    out = dict(y=y.detach(), dx=xr.grad, dw=wr.grad)
    if b is not None:
        out["db"] = br.grad
    return out


def _dwconv_case(case, dt):
    B, C, H, W, bias, _ = DW_CASES[case]
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.randn(B, C, H, W, generator=g).to(dt)
    w = 0.3 * torch.randn(C, 1, 3, 3, generator=g)
    b = 0.1 * torch.randn(C, generator=g) if bias else None
    gy = torch.randn(B, C, H, W, generator=g).to(dt)
    spec = dict(y=(dt, 1e-5), dx=(dt, 1e-5), dw=(F32, SCALED))
    if bias:
        spec["db"] = (F32, SCALED)
    want = _dwconv_ref(x, w, b, gy, torch.float64)
    _attainable(spec, want, _dwconv_ref(x, w, b, gy, F32))
    return (x, w, b, gy), spec, want


@pytest.mark.parametrize("case,dt", DW_PARAMS)
def test_dwconv_silu_16bit_and_chunk_boundaries(case, dt):
    from vm_asr_amd import dwconv
    (x, w, b, gy), spec, want = _dwconv_case(case, dt)
    xd, wd = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    bd = None if b is None else b.to(DEV).requires_grad_()
    y = dwconv.dwconv3x3_silu(xd, wd, bd)
    y.backward(gy.to(DEV))
    got = dict(y=y.detach(), dx=xd.grad, dw=wd.grad)
    if b is not None:
        got["db"] = bd.grad
    _compare(spec, got, want, "dwconv")


# ------------------------------------------------------------------------------------------
# x_proj / dt_proj with 16-bit xs
# ------------------------------------------------------------------------------------------
XP_CASES = {
    # id: (B, D, N, R, L) as in test_xproj_vs_einsum
    "position-parallel-vec": (1, 2, 1, 1, 1024),
    "position-parallel-nonvec-L77": (2, 6, 2, 1, 77),
    "row-parallel-full-tiles": (1, 64, 1, 2, 256),
    "row-parallel-ragged-odd-D": (1, 100, 2, 3, 200),
    "weight-grad-five-position-chunks": (1, 16, 1, 1, 5000),
    "general-d_state-xproj_n": (1, 34, 8, 3, 300),       # csrc/xproj_n.hip admits 16-bit xs (its check() takes fp32 / fp16 / bf16)
}


def _xproj_ref(xs, Wx, Wdt, gd, gB, gC, N, prec):
    Bn, _, _, L = xs.shape
    R = Wdt.shape[2]
    xr, wxr, wdr = (_leaf(t, prec) for t in (xs, Wx, Wdt))
    x_dbl = torch.einsum("b k d l, k c d -> b k c l", xr, wxr)
    dts, Bs, Cs = torch.split(x_dbl, [R, N, N], dim=2)
    dts = torch.einsum("b k r l, k d r -> b k d l", dts, wdr).reshape(Bn, -1, L)
    ((dts * gd.to(prec)).sum() + (Bs * gB.to(prec)).sum() + (Cs * gC.to(prec)).sum()).backward()
    return dict(dts=dts.detach(), Bs=Bs.detach(), Cs=Cs.detach(), dxs=xr.grad, dWx=wxr.grad, dWdt=wdr.grad)


def _xproj_case(case, dt):
    Bn, D, N, R, L = XP_CASES[case]
    K, C = 4, R + 2 * N
    g = torch.Generator().manual_seed(D + L)
    xs = torch.randn(Bn, K, D, L, generator=g).to(dt)
    Wx = torch.randn(K, C, D, generator=g) / D ** 0.5
    Wdt = torch.randn(K, D, R, generator=g)
    gd, gB, gC = torch.randn(Bn, K * D, L, generator=g), torch.randn(Bn, K, N, L, generator=g), torch.randn(Bn, K, N, L, generator=g)
    spec = dict(dts=(F32, SCALED), Bs=(F32, 1e-4), Cs=(F32, 1e-4), dxs=(dt, SCALED), dWx=(F32, SCALED), dWdt=(F32, SCALED))
    want = _xproj_ref(xs, Wx, Wdt, gd, gB, gC, N, torch.float64)
    _attainable(spec, want, _xproj_ref(xs, Wx, Wdt, gd, gB, gC, N, F32))
    return (xs, Wx, Wdt, gd, gB, gC, N), spec, want


@pytest.mark.parametrize("dt", [BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("case", list(XP_CASES))
def test_xproj_16bit_xs(case, dt):
    from vm_asr_amd.xproj import x_proj_dt
    (xs, Wx, Wdt, gd, gB, gC, N), spec, want = _xproj_case(case, dt)
    xd, wxd, wdd = (t.to(DEV).requires_grad_() for t in (xs, Wx, Wdt))
    dts, Bs, Cs = x_proj_dt(xd, wxd, wdd, N)
    ((dts * gd.to(DEV)).sum() + (Bs * gB.to(DEV)).sum() + (Cs * gC.to(DEV)).sum()).backward()
    got = dict(dts=dts.detach(), Bs=Bs.detach(), Cs=Cs.detach(), dxs=xd.grad, dWx=wxd.grad, dWdt=wdd.grad)
    _compare(spec, got, want, "xproj")
