"""The fused Mlp branch (vm_asr_amd/csrc/mlp.hip: LayerNorm + fc1 + GELU + fc2 + residual as one MFMA kernel, and its
backward) against the reference's composition of the same steps (model/vmamba.py:1832-1837, 483-509) — evaluated in
float64 as the adjudicator and, as the yardstick for "bf16 accuracy", by torch's own bf16 autocast on the GPU."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F


def _ref(x, norm, mlp, scale, dtype):
    """x + scale * fc2(GELU(fc1(LN(x)))) in `dtype` (float64: the exact answer)."""
    c = lambda t: t.detach().to(dtype).requires_grad_()      # noqa: E731
    p = [c(t) for t in (x, norm.weight, norm.bias, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias)]
    xn = F.layer_norm(p[0], (x.shape[-1],), p[1], p[2], norm.eps)
    y = F.linear(F.gelu(F.linear(xn, p[3], p[4])), p[5], p[6])
    if scale is not None:
        y = y * scale.to(dtype).view(-1, *([1] * (x.dim() - 1)))
    return p[0] + y, p


NAMES = ["y", "dx", "dgamma", "dbeta", "dW1", "db1", "dW2", "db2"]


def _setup(d, shape, xdt, use_scale, seed=None):
    from vm_asr_amd.layernorm import LayerNorm
    from vm_asr_amd.vmamba import Mlp
    torch.manual_seed(d + shape[1] if seed is None else seed)
    dev = "cuda"
    norm, mlp = LayerNorm(d).to(dev), Mlp(d, 4 * d).to(dev)
    with torch.no_grad():
        norm.weight.add_(0.1 * torch.randn_like(norm.weight)); norm.bias.add_(0.1 * torch.randn_like(norm.bias))
        mlp.fc1.bias.add_(0.1 * torch.randn_like(mlp.fc1.bias)); mlp.fc2.bias.add_(0.1 * torch.randn_like(mlp.fc2.bias))
    x = torch.randn(*shape, d, device=dev).to(xdt)
    gy = torch.randn(*shape, d, device=dev).to(xdt)
    scale = (torch.tensor([0.0, 1.0 / 0.9, 1.0 / 0.9][: shape[0]], device=dev) if use_scale else None)
    return norm, mlp, x, gy, scale


def _run(fn, norm, mlp, x, gy):
    """forward + backward of fn(x) under bf16 autocast -> [y, dx, dgamma, dbeta, dW1, db1, dW2, db2] in float64"""
    params = [norm.weight, norm.bias, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias]
    xi = x.clone().requires_grad_()
    for p in params:
        p.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = fn(xi)
    y.backward(gy)
    return [y.detach().double(), xi.grad.double()] + [p.grad.double() for p in params]


def _fused_fn(norm, mlp, scale):
    from vm_asr_amd.mlp import fused_mlp_residual, supported

    def fused(xi):
        assert supported(xi, norm, mlp)
        return fused_mlp_residual(xi, norm, mlp, None if scale is None else scale.view(-1, 1, 1, 1))
    return fused


def _check_against_float64(d, shape, use_scale, xdt):
    norm, mlp, x, gy, scale = _setup(d, shape, xdt, use_scale)
    y64, p64 = _ref(x, norm, mlp, scale, torch.float64)
    y64.backward(gy.double())
    tol = 1e-2 if xdt == torch.float32 else 1.6e-2       # bf16 outputs: + half an ulp (2^-8) of the value itself
    want = [y64.detach()] + [t.grad for t in p64]

    def plain(xi):
        y = mlp(norm(xi))
        return xi + (y if scale is None else y * scale.view(-1, 1, 1, 1))
    got, auto = _run(_fused_fn(norm, mlp, scale), norm, mlp, x, gy), _run(plain, norm, mlp, x, gy)
    for n, a, b, c in zip(NAMES, got, auto, want):
        sc = max(c.abs().max().item(), 1e-12)
        e_f, e_a = (a - c).abs().max().item() / sc, (b - c).abs().max().item() / sc
        print(f"d={d} {shape} {n}: fused {e_f:.2e}  torch autocast {e_a:.2e}")
        assert a.shape == c.shape and torch.isfinite(a).all(), n
        # north_star: 1e-2 for bf16; and no worse than torch's own bf16 autocast of the same lines (x1.5 + a floor)
        assert e_f <= tol, (n, e_f)
        assert e_f <= 1.5 * e_a + 2e-3, (n, e_f, e_a)
    return got, x, gy


@pytest.mark.gpu
@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d,shape,use_scale", [(8, (2, 16, 16), True), (16, (2, 5, 7), True), (16, (1, 64, 64), False), (32, (3, 8, 8), True),
                                               (64, (2, 9, 5), False), (64, (2, 32, 32), True)])
def test_fused_mlp_matches_float64_as_well_as_torch_autocast(d, shape, use_scale, xdt):
    """xdt: dtype of the residual stream (fp32 in the first stage and behind every LayerNorm-ended sampler, bf16 behind a
    PatchMerging / skip convolution under autocast); y, dx come back in it."""
    got, x, gy = _check_against_float64(d, shape, use_scale, xdt)
    if use_scale:       # a dropped sample (scale 0) passes through untouched, forward and backward
        assert torch.equal(got[0][0].float(), x[0].float()) and torch.equal(got[1][0].float(), gy[0].float())


# The plain and the gated form are one kernel body (csrc/mlp.hip, template flag GATED): the cases below are the plain twins of
# tests/test_gmlp_gpu.py's, at the same shapes.
@pytest.mark.gpu
@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", [16, 64])
def test_dropped_sample_returns_x_and_gy_bit_exactly(d, xdt):
    norm, mlp, x, gy, _ = _setup(d, (3, 6, 7), xdt, False, seed=5)
    scale = torch.tensor([1.0 / 0.8, 0.0, 1.0 / 0.8], device="cuda")
    xi = x.clone().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = _fused_fn(norm, mlp, scale)(xi)
    y.backward(gy)
    assert y.dtype == xdt and torch.equal(y[1], x[1]) and torch.equal(xi.grad[1], gy[1])
    assert not torch.equal(y[0], x[0]) and not torch.equal(y[2], x[2])


@pytest.mark.gpu
@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16])
def test_fewer_rows_than_one_tile_through_the_hidden_split_path(xdt):
    """d = 64, 15 rows: one partial row tile, four waves each with their share of the hidden tiles."""
    _check_against_float64(64, (1, 3, 5), False, xdt)


@pytest.mark.gpu
def test_deterministic_mode_is_bit_reproducible_at_d64_and_the_narrow_forward_always():
    from vm_asr_amd import _lib
    lib = _lib.lib()

    def both(d, shape):
        norm, mlp, x, gy, scale = _setup(d, shape, torch.float32, True, seed=11)
        out = _run(_fused_fn(norm, mlp, scale), norm, mlp, x, gy)
        torch.cuda.synchronize()
        return out
    was = lib.vmasr_get_deterministic()
    try:
        lib.vmasr_set_deterministic(1)
        a, b = both(64, (2, 32, 32)), both(64, (2, 32, 32))
        assert lib.vmasr_det_timeouts() == 0
    finally:
        lib.vmasr_set_deterministic(was)
    for n, u, v in zip(NAMES, a, b):
        assert torch.equal(u, v), n
    # default mode: one wave per row tile at d <= 32, no cross-wave sums in the forward
    for d in (8, 16, 32):
        norm, mlp, x, _, scale = _setup(d, (2, 9, 5), torch.float32, True, seed=12)
        with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
            y1, y2 = _fused_fn(norm, mlp, scale)(x), _fused_fn(norm, mlp, scale)(x)
        assert torch.equal(y1, y2), d


EINVAL = -1           # include/vmasr_hip.h: contract violated


@pytest.mark.gpu
def test_c_entry_points_refuse_a_bad_width_and_no_rows_without_launching():
    from vm_asr_amd import _lib
    lib = _lib.lib()
    buf = torch.full((4096,), 7.0, device="cuda")
    torch.cuda.synchronize()
    p = ctypes.c_void_p(buf.data_ptr())
    code = _lib.torch_dtype_code(torch.float32)
    for d, rows in ((24, 64), (16, 0)):
        assert lib.vmasr_mlp_fwd(p, p, p, 1e-5, p, p, p, p, None, 0, p, rows, d, code, None) == EINVAL
        assert lib.vmasr_last_error().decode().startswith("mlp_fwd:")
        assert lib.vmasr_mlp_bwd(p, p, p, p, 1e-5, p, p, p, p, None, 0, p, p, p, p, p, p, p, rows, d, code, None) == EINVAL
        assert lib.vmasr_last_error().decode().startswith("mlp_bwd:")
        with pytest.raises(RuntimeError, match="mlp_fwd"):
            _lib.call(lib.vmasr_mlp_fwd, buf, buf, buf, 1e-5, buf, buf, buf, buf, None, 0, buf, rows, d, code)
    torch.cuda.synchronize()
    assert torch.equal(buf, torch.full_like(buf, 7.0))
    assert lib.vmasr_mlp_supported(24, 96) == 0 and lib.vmasr_mlp_supported(16, 64) == 1


def test_width_128_is_offered_by_neither_form_and_refused_by_all_four_entry_points():
    """No GPU needed: d = 128 has no kernel (csrc/mlp.hip: supported_d); the host checks refuse it before any launch and the (host)
    dummy operands are never touched."""
    from vm_asr_amd import _lib
    lib = _lib.lib()
    assert lib.vmasr_mlp_supported(128, 512) == 0 and lib.vmasr_gmlp_supported(128, 512) == 0
    buf = (ctypes.c_ubyte * 256)(*([0xA5] * 256))
    p = ctypes.cast(buf, ctypes.c_void_p)
    for code in (_lib.torch_dtype_code(torch.float32), _lib.torch_dtype_code(torch.bfloat16)):
        for form in ("mlp", "gmlp"):
            fwd, bwd = getattr(lib, f"vmasr_{form}_fwd"), getattr(lib, f"vmasr_{form}_bwd")
            assert fwd(p, p, p, 1e-5, p, p, p, p, None, 0, p, 64, 128, code, None) == EINVAL
            assert lib.vmasr_last_error().decode().startswith(f"{form}_fwd:")
            assert bwd(p, p, p, p, 1e-5, p, p, p, p, None, 0, p, p, p, p, p, p, p, 64, 128, code, None) == EINVAL
            assert lib.vmasr_last_error().decode().startswith(f"{form}_bwd:")
    assert bytes(buf) == b"\xa5" * len(buf)


@pytest.mark.gpu
def test_vssblock_uses_the_fused_mlp_under_autocast_only(monkeypatch):
    """Under bf16 autocast VSSBlock runs its Mlp branch through the fused kernel (same result as the unfused module path
    within bf16 accuracy); in fp32 it does not (the fused kernel is a bf16 operator)."""
    from vm_asr_amd import mlp as M
    from vm_asr_amd.vmamba import VSSBlock
    torch.manual_seed(0)
    blk = VSSBlock(hidden_dim=16, drop_path=0.0, ssm_d_state=1, ssm_dt_rank="auto", forward_type="v5").cuda()
    x = torch.randn(2, 32, 32, 16, device="cuda")
    assert not M.supported(x, blk.norm2, blk.mlp)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert M.supported(x, blk.norm2, blk.mlp)
        y1 = blk(x)
        monkeypatch.setenv("VMASR_FUSED_MLP", "0")
        y0 = blk(x)
    assert y1.dtype == torch.float32 and (y1 - y0).abs().max() <= 2e-2 * y0.abs().max()


@pytest.mark.gpu
@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d,shape,with_norm", [(8, (2, 16, 16), True), (16, (1, 32, 32), True), (16, (2, 8, 8), False), (32, (2, 8, 16), True),
                                               (64, (1, 16, 16), True), (64, (2, 8, 4), False)])
def test_fused_in_proj_matches_float64_as_well_as_torch_autocast(d, shape, with_norm, xdt):
    """LayerNorm -> in_proj -> chunk -> (channel-first x, SiLU(z)) as one MFMA kernel (vm_asr_amd/inproj.py; model/vmamba.py:
    1826-1827, 1535-1542) against float64, with torch's bf16 autocast of the same lines as the yardstick; with a LayerNorm and
    with nn.Identity (the output layers' blocks), fp32 and bf16 streams."""
    from vm_asr_amd.inproj import fused_in_proj, supported
    from vm_asr_amd.layernorm import LayerNorm
    from vm_asr_amd.linear import Linear
    torch.manual_seed(d + shape[1])
    dev = "cuda"
    norm = LayerNorm(d).to(dev) if with_norm else nn.Identity()
    proj = Linear(d, 4 * d, bias=False).to(dev)
    if with_norm:
        with torch.no_grad():
            norm.weight.add_(0.1 * torch.randn_like(norm.weight)); norm.bias.add_(0.1 * torch.randn_like(norm.bias))
    B, H, W = shape
    x = torch.randn(B, H, W, d, device=dev).to(xdt)
    gT, gz = torch.randn(B, 2 * d, H, W, device=dev).to(torch.bfloat16), torch.randn(B, H, W, 2 * d, device=dev).to(torch.bfloat16)
    params = ([norm.weight, norm.bias] if with_norm else []) + [proj.weight]

    def ref(dtype):
        c = lambda t: t.detach().to(dtype).requires_grad_()       # noqa: E731
        xi, ps = c(x), [c(p) for p in params]
        xn = F.layer_norm(xi, (d,), ps[0], ps[1], norm.eps) if with_norm else xi
        xz = F.linear(xn, ps[-1])
        xx, z = xz.chunk(2, -1)
        xT, sz = xx.permute(0, 3, 1, 2), F.silu(z)
        ((xT * gT.to(dtype)).sum() + (sz * gz.to(dtype)).sum()).backward()
        return [xT.detach(), sz.detach(), xi.grad] + [p.grad for p in ps]

    def run(fn):
        xi = x.clone().requires_grad_()
        for p in params:
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            xT, sz = fn(xi)
        ((xT.float() * gT.float()).sum() + (sz.float() * gz.float()).sum()).backward()
        return [xT.detach().double(), sz.detach().double(), xi.grad.double()] + [p.grad.double() for p in params]

    def plain(xi):
        xz = proj(norm(xi))
        xx, z = xz.chunk(2, -1)
        return xx.permute(0, 3, 1, 2).contiguous(), F.silu(z)

    def fused(xi):
        assert supported(xi, norm, proj)
        return fused_in_proj(xi, norm, proj)
    want, got, auto = ref(torch.float64), run(fused), run(plain)
    names = ["xT", "sz", "dx"] + (["dgamma", "dbeta"] if with_norm else []) + ["dW"]
    tol = 1.6e-2
    for n, a, b, c in zip(names, got, auto, want):
        sc = max(c.abs().max().item(), 1e-12)
        e_f, e_a = (a - c).abs().max().item() / sc, (b - c).abs().max().item() / sc
        print(f"d={d} {shape} norm={with_norm} {n}: fused {e_f:.2e}  torch autocast {e_a:.2e}")
        assert a.shape == c.shape and torch.isfinite(a).all(), n
        assert e_f <= tol and e_f <= 1.5 * e_a + 3e-3, (n, e_f, e_a)


@pytest.mark.gpu
@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d,shape,scaled", [(8, (2, 16, 16), True), (16, (1, 32, 32), False), (32, (2, 8, 16), True), (64, (1, 16, 16), False),
                                            (64, (3, 8, 4), True)])
def test_fused_out_proj_residual_matches_float64_as_well_as_torch_autocast(d, shape, scaled, xdt):
    """out_proj + DropPath scale + residual add as one MFMA kernel (vm_asr_amd/outproj.py; model/vmamba.py:1551, 1826-1827)
    against float64, with torch's bf16 autocast of the same lines as the yardstick; fp32 and bf16 streams, with and without the
    per-sample stochastic-depth scale, row counts that are not a multiple of the 32-row tile."""
    from vm_asr_amd.linear import Linear
    from vm_asr_amd.outproj import fused_out_proj_residual, supported
    torch.manual_seed(d + shape[1])
    dev = "cuda"
    proj = Linear(2 * d, d, bias=False).to(dev)
    B, H, W = shape
    g = torch.randn(B, H, W, 2 * d, device=dev).to(torch.bfloat16)
    x = torch.randn(B, H, W, d, device=dev).to(xdt)
    gy = torch.randn(B, H, W, d, device=dev)
    scale = (torch.rand(B, 1, 1, 1, device=dev) > 0.3).float() / 0.7 if scaled else None

    def ref(dtype):
        c = lambda t: t.detach().to(dtype).requires_grad_()       # noqa: E731
        gi, xi, w = c(g), c(x), c(proj.weight)
        y = xi + F.linear(gi, w) * (1.0 if scale is None else scale.to(dtype))
        (y * gy.to(dtype)).sum().backward()
        return [y.detach(), gi.grad, xi.grad, w.grad]

    def run(fn):
        gi, xi = g.clone().requires_grad_(), x.clone().requires_grad_()
        proj.weight.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = fn(gi, xi)
        assert y.dtype == xdt
        (y.float() * gy).sum().backward()
        return [y.detach().double(), gi.grad.double(), xi.grad.double(), proj.weight.grad.double()]

    def plain(gi, xi):
        out = proj(gi)
        return xi + out if scale is None else torch.addcmul(xi, out, scale.to(torch.promote_types(xi.dtype, out.dtype)))

    def fused(gi, xi):
        assert supported(gi, proj, xi)
        return fused_out_proj_residual(gi, proj, xi, scale)
    want, got, auto = ref(torch.float64), run(fused), run(plain)
    for n, a, b, c in zip(["y", "dg", "dx", "dW"], got, auto, want):
        sc = max(c.abs().max().item(), 1e-12)
        e_f, e_a = (a - c).abs().max().item() / sc, (b - c).abs().max().item() / sc
        print(f"d={d} {xdt} {n}: fused {e_f:.2e}  autocast {e_a:.2e}")
        assert e_f <= 1.5 * e_a + 2e-3, (n, e_f, e_a)
