"""The fused Mlp branch (vm_asr_amd/csrc/mlp.hip: LayerNorm + fc1 + GELU + fc2 + residual as one MFMA kernel, and its
backward) against the reference's composition of the same steps (model/vmamba.py:1832-1837, 483-509) — evaluated in
float64 as the adjudicator and, as the yardstick for "bf16 accuracy", by torch's own bf16 autocast on the GPU."""
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


@pytest.mark.gpu
@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d,shape,use_scale", [(8, (2, 16, 16), True), (16, (2, 5, 7), True), (16, (1, 64, 64), False), (32, (3, 8, 8), True),
                                               (64, (2, 9, 5), False), (64, (2, 32, 32), True)])
def test_fused_mlp_matches_float64_as_well_as_torch_autocast(d, shape, use_scale, xdt):
    """xdt: dtype of the residual stream (fp32 in the first stage and behind every LayerNorm-ended sampler, bf16 behind a
    PatchMerging / skip convolution under autocast); y, dx come back in it."""
    from vm_asr_amd.layernorm import LayerNorm
    from vm_asr_amd.mlp import fused_mlp_residual, supported
    from vm_asr_amd.vmamba import Mlp
    torch.manual_seed(d + shape[1])
    dev = "cuda"
    norm, mlp = LayerNorm(d).to(dev), Mlp(d, 4 * d).to(dev)
    with torch.no_grad():
        norm.weight.add_(0.1 * torch.randn_like(norm.weight)); norm.bias.add_(0.1 * torch.randn_like(norm.bias))
        mlp.fc1.bias.add_(0.1 * torch.randn_like(mlp.fc1.bias)); mlp.fc2.bias.add_(0.1 * torch.randn_like(mlp.fc2.bias))
    x = torch.randn(*shape, d, device=dev).to(xdt)
    gy = torch.randn(*shape, d, device=dev).to(xdt)
    scale = (torch.tensor([0.0, 1.0 / 0.9, 1.0 / 0.9][: shape[0]], device=dev) if use_scale else None)
    params = [norm.weight, norm.bias, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias]

    y64, p64 = _ref(x, norm, mlp, scale, torch.float64)
    y64.backward(gy.double())
    tol = 1e-2 if xdt == torch.float32 else 1.6e-2       # bf16 outputs: + half an ulp (2^-8) of the value itself
    want = [y64.detach()] + [t.grad for t in p64]

    def run(fn):
        xi = x.clone().requires_grad_()
        for p in params:
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = fn(xi)
        y.backward(gy)
        return [y.detach().double(), xi.grad.double()] + [p.grad.double() for p in params]

    def plain(xi):
        y = mlp(norm(xi))
        return xi + (y if scale is None else y * scale.view(-1, 1, 1, 1))

    def fused(xi):
        assert supported(xi, norm, mlp)
        return fused_mlp_residual(xi, norm, mlp, None if scale is None else scale.view(-1, 1, 1, 1))
    got, auto = run(fused), run(plain)
    names = ["y", "dx", "dgamma", "dbeta", "dW1", "db1", "dW2", "db2"]
    for n, a, b, c in zip(names, got, auto, want):
        sc = max(c.abs().max().item(), 1e-12)
        e_f, e_a = (a - c).abs().max().item() / sc, (b - c).abs().max().item() / sc
        print(f"d={d} {shape} {n}: fused {e_f:.2e}  torch autocast {e_a:.2e}")
        assert a.shape == c.shape and torch.isfinite(a).all(), n
        # north_star: 1e-2 for bf16; and no worse than torch's own bf16 autocast of the same lines (x1.5 + a floor)
        assert e_f <= tol, (n, e_f)
        assert e_f <= 1.5 * e_a + 2e-3, (n, e_f, e_a)
    if use_scale:       # a dropped sample (scale 0) passes through untouched, forward and backward
        assert torch.equal(got[0][0].float(), x[0].float()) and torch.equal(got[1][0].float(), gy[0].float())


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
