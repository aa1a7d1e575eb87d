"""ss2d_pre / ln_gate (vm_asr_amd/csrc/ss2d_glue.hip) against the torch expressions of SS2D.forwardv2 they replace
(model/vmamba.py:1537-1542 and :1528-1531,1550), forward and backward, fp32 (vs float64) and bf16 (vs the same
expression on the bf16-rounded inputs).  Further down: the multi-pass, ragged, fp16 and d_inner-1 paths, the C entry points on
guarded buffers, the workspace / deferred reduction of d_inner >= 64, and the admission rule."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

SHAPES = [(2, 8, 8, 2), (1, 16, 16, 16), (2, 16, 8, 32), (1, 8, 8, 64), (2, 8, 8, 128), (1, 8, 4, 256), (1, 4, 4, 512), (4, 128, 128, 32)]


def _ref_pre(xz):
    x, z = xz.chunk(2, dim=-1)
    return x.permute(0, 3, 1, 2).contiguous(), F.silu(z)


def _ref_ln_gate(y, sz, w, b, eps):
    B, H, W, D = sz.shape
    return F.layer_norm(y.transpose(1, 2).contiguous(), (D,), w, b, eps).view(B, H, W, D) * sz


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ss2d_pre(shape, dtype):
    from vm_asr_amd.ss2d_glue import ss2d_pre, supported
    B, H, W, D = shape
    if not supported(D, H * W, dtype):
        pytest.skip("shape not on the fused path")
    g = torch.Generator().manual_seed(D)
    xz = (2 * torch.randn(B, H, W, 2 * D, generator=g)).to(dtype)
    gx, gz = torch.randn(B, D, H, W, generator=g).to(dtype), torch.randn(B, H, W, D, generator=g).to(dtype)
    a = xz.cuda().requires_grad_()
    xT, sz = ss2d_pre(a)
    (xT.float() * gx.cuda().float()).sum().add((sz.float() * gz.cuda().float()).sum()).backward()
    r = xz.double().requires_grad_()
    rx, rz = _ref_pre(r)
    ((rx * gx.double()).sum() + (rz * gz.double()).sum()).backward()
    tol = 1e-6 if dtype == torch.float32 else 1e-2
    assert xT.dtype == sz.dtype == dtype and torch.equal(xT.cpu().double(), rx.detach().to(dtype).double())       # pure data movement
    assert torch.allclose(sz.cpu().double(), rz.detach(), rtol=tol, atol=tol)
    assert torch.allclose(a.grad.cpu().double(), r.grad, rtol=tol, atol=tol * r.grad.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ln_gate(shape, dtype):
    from vm_asr_amd.ss2d_glue import ln_gate, supported
    B, H, W, D = shape
    if not supported(D, H * W, dtype):
        pytest.skip("shape not on the fused path")
    g = torch.Generator().manual_seed(D + 1)
    y = 3 * torch.randn(B, D, H * W, generator=g) + 0.5
    sz = torch.randn(B, H, W, D, generator=g).to(dtype)
    w, b = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    go = torch.randn(B, H, W, D, generator=g).to(dtype)
    ins = [t.cuda().requires_grad_() for t in (y, sz, w, b)]
    out = ln_gate(*ins, 1e-5)
    (out.float() * go.cuda().float()).sum().backward()
    ref_in = [t.double().requires_grad_() for t in (y, sz, w, b)]
    ref = _ref_ln_gate(*ref_in, 1e-5)
    (ref * go.double()).sum().backward()
    assert out.dtype == dtype
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    # d_inner = 2: a LayerNorm over two channels amplifies rounding by up to 1/sqrt(eps) where they nearly coincide
    names = ["out", "dy", "dsz", "dgamma", "dbeta"]
    got = [out] + [t.grad for t in ins]
    want = [ref.detach()] + [t.grad for t in ref_in]
    for n, a, r in zip(names, got, want):
        scale = max(r.abs().max().item(), 1e-12)
        lim = tol * (50 if D == 2 and n == "dy" else 1)
        assert (a.cpu().double() - r).abs().max().item() <= lim * scale, (shape, dtype, n, (a.cpu().double() - r).abs().max().item(), scale)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 16, 32, 32), (1, 32, 16, 2), (2, 48, 16, 8), (1, 128, 128, 16)])
def test_ln_gate_pairs_equals_ln_gate_of_the_merged_tensor(shape, dtype):
    """ln_gate_pairs(y02, y13, ...) == ln_gate(y02 + transpose_hw(y13), ...) (what is left of CrossMerge,
    model/vmamba.py:50-73, formed on the fly), forward and every gradient — dy comes back in BOTH orders —, against float64."""
    from vm_asr_amd.ss2d_glue import ln_gate_pairs, pairs_supported
    B, H, W, D = shape
    assert pairs_supported(D, H, W, dtype)
    g = torch.Generator().manual_seed(D + H)
    y02 = 2 * torch.randn(B, D, H * W, generator=g) + 0.3
    y13 = 2 * torch.randn(B, D, W * H, generator=g)
    sz = torch.randn(B, H, W, D, generator=g).to(dtype)
    w, b = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    go = torch.randn(B, H, W, D, generator=g).to(dtype)
    ins = [t.cuda().requires_grad_() for t in (y02, y13, sz, w, b)]
    out = ln_gate_pairs(*ins, 1e-5)
    (out.float() * go.cuda().float()).sum().backward()
    r = [t.double().requires_grad_() for t in (y02, y13, sz, w, b)]
    ymerged = r[0] + r[1].view(B, D, W, H).transpose(2, 3).reshape(B, D, H * W)
    ref = _ref_ln_gate(ymerged, *r[2:], 1e-5)
    (ref * go.double()).sum().backward()
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    for n, a, q in zip(["out", "dy02", "dy13", "dsz", "dgamma", "dbeta"], [out] + [t.grad for t in ins], [ref.detach()] + [t.grad for t in r]):
        scale = max(q.abs().max().item(), 1e-12)
        lim = tol * (50 if D == 2 and n.startswith("dy") else 1)
        assert (a.cpu().double() - q).abs().max().item() <= lim * scale, (shape, dtype, n)


@pytest.mark.gpu
def test_ss2d_forward_with_pairs_equals_merged_path(monkeypatch):
    """SS2D.forward through (fused core -> pair outputs -> ln_gate_pairs) equals the path with the merged tensor
    (VMASR_SS2D_PAIRS=0), output and all gradients, fp32."""
    from vm_asr_amd.vmamba import SS2D
    torch.manual_seed(3)
    m = SS2D(d_model=8, d_state=1, ssm_ratio=2.0, dt_rank="auto", forward_type="v5").cuda()
    x = torch.randn(2, 32, 48, 8, device="cuda")
    gy = torch.randn(2, 32, 48, 8, device="cuda")
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("VMASR_SS2D_PAIRS", flag)
        xi = x.clone().requires_grad_()
        m.zero_grad()
        y = m(xi)
        y.backward(gy)
        res[flag] = [y.detach(), xi.grad] + [p.grad.clone() for p in m.parameters()]
    for a, b in zip(res["1"], res["0"]):
        assert (a - b).abs().max() <= 2e-5 * max(1e-6, b.abs().max().item()) + 1e-7


# ---- the multi-pass, ragged, fp16 and d_inner-1 paths, each at the smallest shape that takes it ----------------------------------------
# Error bound: |got - float64| <= tol * max|float64|.  fp16: the bf16 bound times the ratio of the unit roundoffs, 2^-11 / 2^-8.
TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 2.5e-3}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
EPS = 1e-5
EINVAL = -1           # include/vmasr_hip.h: contract violated
MAX_BLOCKS = 64       # csrc/ss2d_glue.hip: kGlueMaxBlocks, workgroups per batch element of the direct / pair backward
CHUNK = 256           # positions per workgroup and pass of the direct kernels
TILE = 16             # the pair kernels' (h, w) tile edge; also the positions per workgroup of the LDS-tile kernels for d_inner >= 64

# (B, H, W, D) -> passes the direct backward must take over its ceil(L / 256) chunks
DIRECT_SHAPES = {(2, 5, 64, 8): 1, (2, 5, 64, 2): 1,          # L = 320: two workgroups, the last with 64 of 256 positions
                 (1, 64, 257, 2): 2, (1, 64, 257, 16): 2,     # L = 16448 = 65 chunks: the 2nd pass is workgroup 0 alone, 64 live threads
                 (2, 192, 256, 4): 3}                          # L = 49152: three full passes
# (B, H, W, D) -> passes the pair backward must take over its (H / 16) (W / 16) tiles
PAIR_SHAPES = {(3, 16, 16, 32): 1,                             # one tile
               (1, 80, 208, 2): 2, (1, 80, 208, 32): 2,       # 5 x 13 = 65 tiles, H != W: the 2nd pass is workgroup 0 alone
               (2, 160, 208, 8): 3}                            # 130 tiles: the last pass has two workgroups
LDS_SHAPES = [(3, 4, 12, 64), (2, 4, 12, 256), (1, 4, 4, 512), (2, 8, 16, 1)]     # d_inner 512: 16-bit only; d_inner 1: P == 64, CH == 1


def _code(dtype):
    from vm_asr_amd import _lib
    return _lib.torch_dtype_code(dtype)


def _passes(units):
    nblk = min(units, MAX_BLOCKS)
    return (units + nblk - 1) // nblk


def _assert_direct_path(shape, dtype):
    """The shape still takes the path it is here for (a later change of kGlueMaxBlocks / the chunk must not make these single-pass)."""
    from vm_asr_amd import _lib
    from vm_asr_amd.ss2d_glue import supported
    B, H, W, D = shape
    L = H * W
    chunks = -(-L // CHUNK)
    assert supported(D, L, dtype), (shape, dtype)
    assert _passes(chunks) == DIRECT_SHAPES[shape]
    if DIRECT_SHAPES[shape] > 1:
        assert chunks > MAX_BLOCKS
    if shape[1:3] == (5, 64):
        assert L > CHUNK and L % CHUNK == 64                        # ragged last workgroup
    if shape[1:3] == (64, 257):
        assert chunks % MAX_BLOCKS == 1 and L % CHUNK == 64         # last pass: workgroup 0 only, ragged too
    assert _lib.lib().vmasr_ln_gate_bwd_workspace(B, D, L, _code(dtype)) == 0      # the direct backward folds per workgroup


def _assert_lds_path(shape, dtype):
    from vm_asr_amd import _lib
    from vm_asr_amd.ss2d_glue import supported
    B, H, W, D = shape
    L = H * W
    assert supported(D, L, dtype), (shape, dtype)
    P = TILE if D >= 64 else 64
    assert L % P == 0 and (L // P == 3 if D == 64 else True)         # (3, 4, 12, 64): three workgroups per sample
    assert _lib.lib().vmasr_ln_gate_bwd_workspace(B, D, L, _code(dtype)) == B * (L // P) * 2 * D


def _assert_pair_path(shape, dtype):
    from vm_asr_amd.ss2d_glue import pairs_supported
    B, H, W, D = shape
    assert pairs_supported(D, H, W, dtype)
    tiles = (H // TILE) * (W // TILE)
    assert _passes(tiles) == PAIR_SHAPES[shape]
    if PAIR_SHAPES[shape] > 1:
        assert tiles > MAX_BLOCKS and tiles % MAX_BLOCKS in (1, 2) and H != W and W // TILE == 13


def _lds_dtypes(shape):
    return [d for d in DTYPES if not (shape[3] == 512 and d == torch.float32)]


def _close(tag, names, got, want, tol, loose=()):
    """every got[i] within tol * max|want[i]| of want[i] (float64); prints the error as a fraction of that bound (headroom record)"""
    for n, a, r in zip(names, got, want):
        scale = max(r.abs().max().item(), 1e-12)
        lim = tol * (50 if n in loose else 1) * scale
        err = (a.detach().cpu().double() - r).abs().max().item()
        print(f"HEADROOM {tag} {n}: {err / lim:.4f} of the bound")
        assert err <= lim, (tag, n, err, lim)         # (a NaN anywhere fails this comparison too)


# The float64 references, computed once per (shape, dtype) on the CPU and shared (never modified) by the tests below.
@functools.lru_cache(maxsize=None)
def _pre_case(shape, dtype):
    B, H, W, D = shape
    g = torch.Generator().manual_seed(100 + D + H * W)
    xz = (2 * torch.randn(B, H, W, 2 * D, generator=g)).to(dtype)
    gx, gz = torch.randn(B, D, H, W, generator=g).to(dtype), torch.randn(B, H, W, D, generator=g).to(dtype)
    r = xz.double().requires_grad_()
    rx, rz = _ref_pre(r)
    ((rx * gx.double()).sum() + (rz * gz.double()).sum()).backward()
    return dict(ins=(xz, gx, gz), xT=rx.detach(), sz=rz.detach(), dxz=r.grad)


@functools.lru_cache(maxsize=None)
def _ln_case(shape, dtype):
    B, H, W, D = shape
    g = torch.Generator().manual_seed(200 + D + H * W)
    y = 3 * torch.randn(B, D, H * W, generator=g) + 0.5
    sz = torch.randn(B, H, W, D, generator=g).to(dtype)
    w, b = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    go = torch.randn(B, H, W, D, generator=g).to(dtype)
    r = [t.double().requires_grad_() for t in (y, sz, w, b)]
    ref = _ref_ln_gate(*r, EPS)
    (ref * go.double()).sum().backward()
    yt = y.double().transpose(1, 2)
    return dict(ins=(y, sz, w, b, go), out=ref.detach(), dy=r[0].grad, dsz=r[1].grad, dgamma=r[2].grad, dbeta=r[3].grad,
                mean=yt.mean(-1), rstd=1.0 / torch.sqrt(yt.var(-1, unbiased=False) + EPS))


@functools.lru_cache(maxsize=None)
def _pair_case(shape, dtype):
    B, H, W, D = shape
    g = torch.Generator().manual_seed(300 + D + H)
    y02 = 2 * torch.randn(B, D, H * W, generator=g) + 0.3
    y13 = 2 * torch.randn(B, D, W * H, generator=g)
    sz = torch.randn(B, H, W, D, generator=g).to(dtype)
    w, b = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    go = torch.randn(B, H, W, D, generator=g).to(dtype)
    r = [t.double().requires_grad_() for t in (y02, y13, sz, w, b)]
    merged = r[0] + r[1].view(B, D, W, H).transpose(2, 3).reshape(B, D, H * W)
    ref = _ref_ln_gate(merged, *r[2:], EPS)
    (ref * go.double()).sum().backward()
    yt = merged.detach().transpose(1, 2)
    return dict(ins=(y02, y13, sz, w, b, go), out=ref.detach(), dy02=r[0].grad, dy13=r[1].grad, dsz=r[2].grad, dgamma=r[3].grad,
                dbeta=r[4].grad, mean=yt.mean(-1), rstd=1.0 / torch.sqrt(yt.var(-1, unbiased=False) + EPS))


def _run_pre(shape, dtype):
    from vm_asr_amd.ss2d_glue import ss2d_pre
    c = _pre_case(shape, dtype)
    xz, gx, gz = c["ins"]
    a = xz.cuda().requires_grad_()
    xT, sz = ss2d_pre(a)
    (xT.float() * gx.cuda().float()).sum().add((sz.float() * gz.cuda().float()).sum()).backward()
    assert xT.dtype == sz.dtype == a.grad.dtype == dtype
    assert torch.equal(xT.cpu().double(), c["xT"])                                   # pure data movement: exact
    _close(f"ss2d_pre {shape} {dtype}", ["sz", "dxz"], [sz, a.grad], [c["sz"], c["dxz"]], TOL[dtype])
    # the x half of dxz is data movement as well
    assert torch.equal(a.grad[..., :shape[3]].cpu(), gx.permute(0, 2, 3, 1))


def _run_ln_gate(shape, dtype):
    from vm_asr_amd.ss2d_glue import ln_gate
    c = _ln_case(shape, dtype)
    ins = [t.cuda().requires_grad_() for t in c["ins"][:4]]
    out = ln_gate(*ins, EPS)
    (out.float() * c["ins"][4].cuda().float()).sum().backward()
    assert out.dtype == ins[1].grad.dtype == dtype
    names = ["out", "dy", "dsz", "dgamma", "dbeta"]
    got = dict(zip(names, [out] + [t.grad for t in ins]))
    if shape[3] == 1:
        # LayerNorm over ONE channel: xh == 0 exactly, so the output is beta * sz and neither y nor gamma receives a gradient.  These
        # two are held to the identity instead of to float64, whose own dy / dgamma here are rounding residue (~1e-13) around the true 0.
        y, sz, w, b = ins
        assert torch.equal(out, (b.detach() * sz.detach().float()).to(dtype))
        assert torch.equal(y.grad, torch.zeros_like(y.grad))
        assert torch.equal(w.grad, torch.zeros_like(w.grad))
        names = ["out", "dsz", "dbeta"]
    _close(f"ln_gate {shape} {dtype}", names, [got[n] for n in names], [c[n] for n in names], TOL[dtype],
           loose=("dy",) if shape[3] == 2 else ())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", list(DIRECT_SHAPES))
def test_ss2d_pre_direct_ragged_and_many_workgroups(shape, dtype):
    _assert_direct_path(shape, dtype)
    _run_pre(shape, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", list(DIRECT_SHAPES))
def test_ln_gate_direct_ragged_and_multi_pass(shape, dtype):
    """the direct backward walks `iters` chunks per workgroup: every position's dy / dsz written once, every pass' share of
    dgamma / dbeta kept, the ragged last chunk and the last pass' idle workgroups leave the wave reduction intact.
    (1, 64, 257, 2) fp32 found the one defect: centred on the rounded mean alone, dsz was 2.11x and out 0.82x the bound where the two
    channels nearly coincide; with the kernels' second centring step both are below 0.02x.)"""
    _assert_direct_path(shape, dtype)
    _run_ln_gate(shape, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtype", [(s, d) for s in LDS_SHAPES for d in _lds_dtypes(s)])
def test_ss2d_pre_lds_tile(shape, dtype):
    _assert_lds_path(shape, dtype)
    _run_pre(shape, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtype", [(s, d) for s in LDS_SHAPES for d in _lds_dtypes(s)])
def test_ln_gate_lds_tile(shape, dtype):
    """(d_inner 1: the exact identities out == round(beta * sz), dy == 0, dgamma == 0 are asserted in _run_ln_gate)"""
    _assert_lds_path(shape, dtype)
    _run_ln_gate(shape, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", list(PAIR_SHAPES))
def test_ln_gate_pairs_multi_pass(shape, dtype):
    from vm_asr_amd.ss2d_glue import ln_gate_pairs
    _assert_pair_path(shape, dtype)
    c = _pair_case(shape, dtype)
    ins = [t.cuda().requires_grad_() for t in c["ins"][:5]]
    out = ln_gate_pairs(*ins, EPS)
    (out.float() * c["ins"][5].cuda().float()).sum().backward()
    assert out.dtype == ins[2].grad.dtype == dtype
    names = ["out", "dy02", "dy13", "dsz", "dgamma", "dbeta"]
    _close(f"ln_gate_pairs {shape} {dtype}", names, [out] + [t.grad for t in ins], [c[n] for n in names], TOL[dtype],
           loose=("dy02", "dy13") if shape[3] == 2 else ())


# ---- the C entry points themselves, every output a NaN-filled slice between two guard bands -------------------------------------------
# (autograd hands the kernels torch.empty outputs: a position that is never written, or a write next to the tensor, can pass by luck)
_NAN_BITS = {4: 0x7FC00000, 2: 0x7FFF}      # a NaN in fp32 / in fp16 and bf16 alike
_GUARD_BITS = {4: 0x5A5A5A5A, 2: 0x5A5A}    # an ordinary finite number in every format


class _Guarded:
    """A (shape) payload carved from a larger buffer: guard | payload | guard, `guard` elements each side."""

    def __init__(self, shape, dtype, guard, zero=False):
        n = math.prod(shape)
        self.n, self.guard, esz = n, guard, dtype.itemsize
        self.buf = torch.empty(n + 2 * guard, dtype=dtype, device="cuda")
        self.bits = self.buf.view(torch.int32 if esz == 4 else torch.int16)
        self.bits.fill_(_GUARD_BITS[esz])
        self.t = self.buf[guard:guard + n].view(shape)
        if zero:
            self.t.zero_()                   # (dgamma / dbeta: the kernels add into them)
        else:
            self.bits[guard:guard + n].fill_(_NAN_BITS[esz])
            assert torch.isnan(self.t).all()
        self.sentinel = _GUARD_BITS[esz]

    def intact(self):
        g, n = self.guard, self.n
        return bool((self.bits[:g] == self.sentinel).all()) and bool((self.bits[g + n:] == self.sentinel).all())


def _assert_raw(tag, outs, c, dtype, stats=()):
    torch.cuda.synchronize()
    for n, o in outs.items():
        assert o.intact(), (tag, n, "guard band overwritten")
        assert not torch.isnan(o.t).any(), (tag, n, "unwritten position")
    names = [n for n in outs if n not in stats]
    _close(tag, names, [outs[n].t for n in names], [c[n].reshape(outs[n].t.shape) for n in names], TOL[dtype])
    _close(tag, list(stats), [outs[n].t for n in stats], [c[n] for n in stats], 2e-5)


RAW_DTYPES = [torch.float32, torch.float16]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", RAW_DTYPES)
@pytest.mark.parametrize("shape", [(2, 5, 64, 8), (1, 64, 257, 16), (3, 4, 12, 64)])
def test_raw_ss2d_pre_writes_every_position_and_nothing_else(shape, dtype):
    from vm_asr_amd import _lib
    lib, code = _lib.lib(), _code(dtype)
    B, H, W, D = shape
    L, G = H * W, CHUNK * D
    c = _pre_case(shape, dtype)
    xz, gx, gz = (t.cuda() for t in c["ins"])
    xT, sz, dxz = _Guarded((B, D, H, W), dtype, G), _Guarded((B, H, W, D), dtype, G), _Guarded((B, H, W, 2 * D), dtype, G)
    _lib.call(lib.vmasr_ss2d_pre_fwd, xz, xT.t, sz.t, B, D, L, code)
    _lib.call(lib.vmasr_ss2d_pre_bwd, xz, gx, gz, dxz.t, B, D, L, code)
    _assert_raw(f"raw ss2d_pre {shape} {dtype}", dict(xT=xT, sz=sz, dxz=dxz), c, dtype)
    assert torch.equal(xT.t.cpu().double(), c["xT"])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", RAW_DTYPES)
@pytest.mark.parametrize("shape", [(2, 5, 64, 8), (1, 64, 257, 16), (3, 4, 12, 64)])
def test_raw_ln_gate_writes_every_position_and_nothing_else(shape, dtype):
    """vmasr_ln_gate_fwd / _bwd (for d_inner 64 that is the LDS-tile backward with its closing global atomics, which autograd never
    takes), mean and rstd against float64 as well"""
    from vm_asr_amd import _lib
    lib, code = _lib.lib(), _code(dtype)
    B, H, W, D = shape
    L, G = H * W, CHUNK * D
    c = _ln_case(shape, dtype)
    y, sz, w, b, go = (t.cuda() for t in c["ins"])
    o = dict(out=_Guarded((B, H, W, D), dtype, G), mean=_Guarded((B, L), torch.float32, G), rstd=_Guarded((B, L), torch.float32, G))
    _lib.call(lib.vmasr_ln_gate_fwd, y, sz, w, b, o["out"].t, o["mean"].t, o["rstd"].t, B, D, L, EPS, code)
    o.update(dy=_Guarded((B, D, L), torch.float32, G), dsz=_Guarded((B, H, W, D), dtype, G),
             dgamma=_Guarded((D,), torch.float32, G, zero=True), dbeta=_Guarded((D,), torch.float32, G, zero=True))
    _lib.call(lib.vmasr_ln_gate_bwd, y, sz, go, w, b, o["mean"].t, o["rstd"].t, o["dy"].t, o["dsz"].t, o["dgamma"].t, o["dbeta"].t,
              B, D, L, code)
    _assert_raw(f"raw ln_gate {shape} {dtype}", o, c, dtype, stats=("mean", "rstd"))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", RAW_DTYPES)
@pytest.mark.parametrize("shape", [(1, 80, 208, 32), (2, 160, 208, 8)])
def test_raw_ln_gate_pair_writes_every_position_and_nothing_else(shape, dtype):
    """(the pair kernels have no ragged block: the 65-tile shape, whose last pass runs one workgroup, stands in for it)"""
    from vm_asr_amd import _lib
    lib, code = _lib.lib(), _code(dtype)
    B, H, W, D = shape
    L, G = H * W, CHUNK * D
    c = _pair_case(shape, dtype)
    y02, y13, sz, w, b, go = (t.cuda() for t in c["ins"])
    o = dict(out=_Guarded((B, H, W, D), dtype, G), mean=_Guarded((B, L), torch.float32, G), rstd=_Guarded((B, L), torch.float32, G))
    _lib.call(lib.vmasr_ln_gate_pair_fwd, y02, y13, sz, w, b, o["out"].t, o["mean"].t, o["rstd"].t, B, D, H, W, EPS, code)
    o.update(dy02=_Guarded((B, D, L), torch.float32, G), dy13=_Guarded((B, D, L), torch.float32, G), dsz=_Guarded((B, H, W, D), dtype, G),
             dgamma=_Guarded((D,), torch.float32, G, zero=True), dbeta=_Guarded((D,), torch.float32, G, zero=True))
    _lib.call(lib.vmasr_ln_gate_pair_bwd, y02, y13, sz, go, w, b, o["mean"].t, o["rstd"].t, o["dy02"].t, o["dy13"].t, o["dsz"].t,
              o["dgamma"].t, o["dbeta"].t, B, D, H, W, code)
    _assert_raw(f"raw ln_gate_pair {shape} {dtype}", o, c, dtype, stats=("mean", "rstd"))


# ---- d_inner >= 64: per-workgroup partials, reduced at once or at the end of the backward pass ------------------------------------------
def _reduce_multi(ws, dg, db, nblk, D):
    """vmasr_layer_norm_bwd_reduce_multi on one item (host tables of device addresses, as layernorm._flush_pending builds them)"""
    import numpy as np
    from vm_asr_amd import _lib
    tab = [np.array([t.data_ptr()], dtype=np.uint64) for t in (ws, dg, db)] + [np.array([v], dtype=np.int32) for v in (nblk, D)]
    _lib.call(_lib.lib().vmasr_layer_norm_bwd_reduce_multi, *[a.ctypes.data for a in tab], 1, device=ws.device)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(3, 4, 12, 64), (2, 4, 12, 256)])
def test_raw_ln_gate_bwd_ws_partials_and_reduction(shape, dtype):
    from vm_asr_amd import _lib
    lib, code = _lib.lib(), _code(dtype)
    B, H, W, D = shape
    L, G = H * W, CHUNK * D
    c = _ln_case(shape, dtype)
    y, sz, w, b, go = (t.cuda() for t in c["ins"])
    mean, rstd = c["mean"].float().cuda(), c["rstd"].float().cuda()
    nws = lib.vmasr_ln_gate_bwd_workspace(B, D, L, code)
    nblk = B * (L // TILE)
    assert nws == nblk * 2 * D

    def run(dg, db):
        o = dict(dy=_Guarded((B, D, L), torch.float32, G), dsz=_Guarded((B, H, W, D), dtype, G), ws=_Guarded((nblk, 2 * D), torch.float32, G))
        _lib.call(lib.vmasr_ln_gate_bwd_ws, y, sz, go, w, b, mean, rstd, o["dy"].t, o["dsz"].t, dg, db, o["ws"].t, B, D, L, code)
        return o
    # partials only: the rows of ws add up to dgamma | dbeta
    o = run(None, None)
    _assert_raw(f"raw ln_gate_bwd_ws {shape} {dtype}", dict(dy=o["dy"], dsz=o["dsz"]), c, dtype)
    assert o["ws"].intact() and not torch.isnan(o["ws"].t).any()
    sums = o["ws"].t.cpu().double().sum(0)
    _close(f"raw ln_gate_bwd_ws partials {shape} {dtype}", ["dgamma", "dbeta"], [sums[:D], sums[D:]], [c["dgamma"], c["dbeta"]],
           TOL[torch.float32])
    # with dgamma / dbeta: the same reduction as layer_norm_bwd_reduce_multi on these very partials
    dg, db = _Guarded((D,), torch.float32, G), _Guarded((D,), torch.float32, G)
    o = run(dg.t, db.t)
    dg2, db2 = _Guarded((D,), torch.float32, G), _Guarded((D,), torch.float32, G)
    _reduce_multi(o["ws"].t, dg2.t, db2.t, nblk, D)
    torch.cuda.synchronize()
    assert all(t.intact() for t in (dg, db, dg2, db2, o["ws"]))
    assert torch.equal(dg.t, dg2.t) and torch.equal(db.t, db2.t) and not torch.isnan(dg.t).any() and not torch.isnan(db.t).any()
    _close(f"raw ln_gate_bwd_ws reduced {shape} {dtype}", ["dgamma", "dbeta"], [dg.t, db.t], [c["dgamma"], c["dbeta"]], TOL[torch.float32])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 4, 12, 64), (2, 4, 12, 256)])
def test_ln_gate_deferred_reduction_matches_immediate(shape):
    """_LNGateFn.backward's `later` branch: under layernorm.deferred the call writes its partials only and queues ONE reduction, the
    end-of-pass flush fills .grad with the bits of the immediate run; parameters used twice in one graph reduce at once.
    Bit equality needs the deterministic mode: a workgroup's four waves add into its LDS partials with float atomics, in the order
    they arrive unless that mode fixes it (csrc/common.h: the wave-order macro of the deterministic mode)."""
    from vm_asr_amd import _lib
    from vm_asr_amd import layernorm as L
    from vm_asr_amd.ss2d_glue import ln_gate
    lib = _lib.lib()
    D = shape[3]
    c = _ln_case(shape, torch.float32)
    y, sz, w, b, go = (t.cuda() for t in c["ins"])

    def run(twice=False):
        ins = [t.clone().requires_grad_() for t in (y, sz, w, b)]
        out = ln_gate(*ins, EPS)
        if twice:
            out = out + ln_gate(-y, 0.5 * sz, ins[2], ins[3], EPS)
        (out * go).sum().backward()
        return [t.grad.clone() for t in ins]
    queued = []
    orig, was = L.defer_reduction, lib.vmasr_get_deterministic()

    def spy(*a, **k):
        queued.append(a[4])
        return orig(*a, **k)
    try:
        lib.vmasr_set_deterministic(1)
        L.reset_uses()
        L.defer_reduction = spy
        ref = run()
        assert queued == [] and L.DEFER_REDUCE is False                # the immediate run: not even asked
        with L.deferred(True):
            got = run()
            assert queued == [D] and not L._pending                    # queued exactly once, flushed when backward() returned
            got2 = run()                                               # (use counts were cleared by the flush)
            assert queued == [D, D] and not L._pending
            both = run(twice=True)
            assert queued == [D, D] and not L._pending                 # used twice in one graph: reduced at once, nothing queued
        assert L.DEFER_REDUCE is False
        assert lib.vmasr_det_timeouts() == 0
    finally:
        L.defer_reduction = orig
        lib.vmasr_set_deterministic(was)
        L.reset_uses()
    for a, p, q in zip(ref, got, got2):
        assert torch.equal(a, p) and torch.equal(a, q)
    r = [t.double().requires_grad_() for t in c["ins"][:4]]
    tot = _ref_ln_gate(*r, EPS) + _ref_ln_gate(-c["ins"][0].double(), 0.5 * c["ins"][1].double(), r[2], r[3], EPS)
    (tot * c["ins"][4].double()).sum().backward()
    _close(f"ln_gate twice {shape}", ["dy", "dsz", "dgamma", "dbeta"], both, [t.grad for t in r], TOL[torch.float32])


# ---- admission: one rule, stated three times (plan(), vmasr_ss2d_glue_supported, here) — and refusals come before any launch ------------
def _plan_admits(D, L, esz):
    """csrc/ss2d_glue.hip: plan(), restated line by line (B aside)"""
    if D <= 0 or L <= 0:
        return False
    V = 16 // esz
    CH = V if D % V == 0 else (4 if D % 4 == 0 else (2 if D % 2 == 0 else 1))
    if esz == 4 and CH > 4:
        CH = 4
    nch = D // CH
    if not (nch <= 64 and nch & (nch - 1) == 0):
        return False
    P = 64 if D <= 32 else 16
    return D <= 512 and L % P == 0


def _rule_admits(D, L, esz):
    """the same rule as a list: what the kernels are instantiated for"""
    ok = D in (1, 2, 4, 8, 16, 32, 64, 128, 256) or (D == 512 and esz == 2)
    return ok and L % (64 if D <= 32 else 16) == 0


def _host_buffer(nbytes=256):
    import ctypes
    buf = (ctypes.c_ubyte * nbytes)(*([0xA5] * nbytes))
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_glue_supported_is_plans_rule():
    """No GPU needed.  vmasr_ss2d_glue_supported re-derives plan()'s admission rule by hand; the two and the list of instantiated widths
    agree over d_inner 1..600 x six lengths x three dtypes.  plan() itself is probed without a launch: through
    vmasr_ln_gate_bwd_workspace (non-zero exactly for the admitted non-direct widths) and through the refusal of vmasr_ss2d_pre_fwd."""
    from vm_asr_amd import _lib
    lib = _lib.lib()
    buf, p = _host_buffer()
    direct = (2, 4, 8, 16, 32)
    for dtype in DTYPES:
        code, esz = _code(dtype), dtype.itemsize
        for L in (16, 48, 64, 100, 320, 16448):
            for D in range(1, 601):
                want = _plan_admits(D, L, esz)
                assert want == _rule_admits(D, L, esz), (D, L, dtype)
                assert lib.vmasr_ss2d_glue_supported(D, L, code) == int(want), (D, L, dtype)
                ws = lib.vmasr_ln_gate_bwd_workspace(2, D, L, code)
                assert ws == (2 * (L // (64 if D <= 32 else 16)) * 2 * D if want and D not in direct else 0), (D, L, dtype)
                if not want:
                    assert lib.vmasr_ss2d_pre_fwd(p, p, p, 1, D, L, code, None) == EINVAL, (D, L, dtype)
        assert lib.vmasr_ss2d_glue_supported(0, 64, code) == 0 and lib.vmasr_ss2d_glue_supported(8, 0, code) == 0
        assert lib.vmasr_ss2d_glue_supported(-8, 64, code) == 0 and lib.vmasr_ss2d_glue_supported(8, -64, code) == 0
    assert bytes(buf) == b"\xa5" * len(buf)
    for D in range(0, 70):
        for H in (0, 8, 16, 24, 32, 80, -16):
            for W in (0, 16, 24, 208, -16):
                want = D in direct and H > 0 and W > 0 and H % 16 == 0 and W % 16 == 0
                assert lib.vmasr_ln_gate_pair_supported(D, H, W) == int(want), (D, H, W)


# (d_inner, L, dtypes): shapes outside the rule, each refused for another reason
REFUSED = [(512, 64, [torch.float32]), (96, 64, DTYPES), (24, 64, DTYPES), (8, 100, DTYPES)]


def _glue_calls(lib, p, B, D, L, code):
    """every launching entry point of the two operators with `p` for each tensor"""
    return [("ss2d_pre_fwd", lib.vmasr_ss2d_pre_fwd, (p,) * 3 + (B, D, L, code)),
            ("ss2d_pre_bwd", lib.vmasr_ss2d_pre_bwd, (p,) * 4 + (B, D, L, code)),
            ("ln_gate_fwd", lib.vmasr_ln_gate_fwd, (p,) * 7 + (B, D, L, EPS, code)),
            ("ln_gate_bwd", lib.vmasr_ln_gate_bwd, (p,) * 11 + (B, D, L, code)),
            ("ln_gate_bwd_ws", lib.vmasr_ln_gate_bwd_ws, (p,) * 12 + (B, D, L, code))]


def _pair_calls(lib, p, B, D, H, W, code):
    return [("ln_gate_pair_fwd", lib.vmasr_ln_gate_pair_fwd, (p,) * 8 + (B, D, H, W, EPS, code)),
            ("ln_gate_pair_bwd", lib.vmasr_ln_gate_pair_bwd, (p,) * 13 + (B, D, H, W, code))]


def _refused_calls(lib, p):
    for D, L, dtypes in REFUSED:
        for dtype in dtypes:
            assert not _plan_admits(D, L, dtype.itemsize)
            yield from _glue_calls(lib, p, 2, D, L, _code(dtype))
    for dtype in DTYPES:
        yield from _pair_calls(lib, p, 2, 8, 24, 16, _code(dtype))
        yield from _pair_calls(lib, p, 2, 8, 16, 24, _code(dtype))


def test_glue_contract_violations_are_refused_before_any_launch():
    """No GPU needed: every check runs before the first launch, so the (host) dummy operands are never touched."""
    from vm_asr_amd import _lib
    lib = _lib.lib()
    buf, p = _host_buffer()
    n = 0
    for name, fn, args in _refused_calls(lib, p):
        code = fn(*args, None)
        assert code == EINVAL, (name, args[-4:])
        assert lib.vmasr_last_error().decode().startswith(name + ":"), (name, lib.vmasr_last_error())
        with pytest.raises(RuntimeError, match=rf"^{name} failed \(-1\): {name}:"):
            _lib.check(code, name)
        n += 1
    assert n == 10 * 5 + 6 * 2
    assert bytes(buf) == b"\xa5" * len(buf)


@pytest.mark.gpu
def test_glue_refusals_raise_and_leave_device_buffers_untouched():
    """the same refusals through _lib.call on device memory: RuntimeError naming the entry point with the EINVAL code, the poisoned
    buffer (every operand of the call) bit-identical afterwards"""
    from vm_asr_amd import _lib
    lib = _lib.lib()
    poison = torch.full((1 << 16,), _GUARD_BITS[4], dtype=torch.int32, device="cuda")
    p = poison.view(torch.float32)
    for name, fn, args in _refused_calls(lib, p):
        with pytest.raises(RuntimeError, match=rf"^{name} failed \(-1\): {name}:"):
            _lib.call(fn, *args)
    torch.cuda.synchronize()
    assert bool((poison == _GUARD_BITS[4]).all())
