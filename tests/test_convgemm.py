"""csrc/convgemm.hip — the period discriminator's (k,1) convolutions as implicit bf16x3 MFMA GEMMs, against a float64
evaluation of the reference's lines (model/discriminator.py:40-104: Conv2d (k,1) stride (s,1) padding (pad,0) -> GELU)
and against torch's own fp32 convolution's distance from float64.

Tolerance: north_star's fp32 bound, 1e-4 of the tensor scale; measured ~3e-6 (the triple carries 16-17 bits per product,
fp32 accumulation)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:      # (run as a module by the children of the switch test)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import errtable

gpu = pytest.mark.gpu


def _ref(xs, W, bias, k, stride, pad, act):
    """float64: per slot x (nseq, H, Cin), W (Cout, k*Cin) in (tap, channel) order -> pre, y (nseq*H1, Cout)"""
    pres, ys = [], []
    for x, w, b in zip(xs, W, bias):
        Cout, Cin = w.shape[0], x.shape[2]
        w4 = w.view(Cout, k, Cin).permute(0, 2, 1).unsqueeze(3)                     # (Cout, Cin, k, 1)
        o = F.conv2d(x.permute(0, 2, 1).unsqueeze(3), w4, b, (stride, 1), (pad, 0))  # (nseq, Cout, H1, 1)
        pre = o.squeeze(3).permute(0, 2, 1).reshape(-1, Cout)
        pres.append(pre)
        ys.append(F.gelu(pre) if act else pre)
    return pres, ys


def _stack(ts, rows):
    out = torch.zeros((len(ts), rows, ts[0].shape[-1]), dtype=ts[0].dtype, device=ts[0].device)
    for i, t in enumerate(ts):
        out[i, :t.shape[0]] = t
    return out


CASES = [
    # (Cin, Cout, k, stride, pad, geom [(nseq, H)])
    (128, 128, 5, 3, 2, [(3, 50), (2, 77)]),
    (128, 256, 5, 3, 2, [(4, 130), (6, 85), (10, 52)]),
    (256, 128, 5, 1, 2, [(2, 64), (3, 41)]),
    (128, 128, 3, 2, 1, [(5, 33)]),
    (128, 128, 5, 3, 2, [(7, 3)]),               # sequences shorter than the kernel
    (32, 128, 5, 3, 2, [(5, 61), (3, 100)]),     # the 32 -> 128 layer: 256 x 128 forward, 256 x 32 dgrad, 128 x 32 wgrad tiles
    (128, 256, 5, 3, 2, [(9, 200)]),             # several 256-row tiles
    (256, 256, 5, 1, 2, [(6, 90), (4, 131)]),    # 256 x 256 tiles everywhere
    # what vmasr_conv_mfma_supported admits beyond the discriminator's own layers (achieved errors: profiles/conv_shape_space.md)
    # (seventh field: the second forward gate's floor where torch's fp32 error is no yardstick, see _check_case)
    (128, 128, 1, 3, 0, [(3, 50), (2, 77)], 2 ** -16),       # k < stride: residue classes 1 and 2 of the input gradient have no tap
    (128, 128, 2, 3, 0, [(4, 61), (2, 100), (5, 32)]),       # k < stride: residue class 2 has none; pad 0
    (128, 128, 8, 2, 7, [(3, 40), (2, 77)]),                 # k 8, pad = k - 1 >= stride
    (128, 256, 4, 1, 0, [(3, 70), (2, 131)]),                # even k, stride 1, pad 0
    (256, 128, 3, 3, 4, [(3, 50), (4, 77), (2, 101)]),       # pad > stride: outputs whose window is all padding
    (128, 128, 5, 3, 2, [(300, 3), (2, 40)]),                # H1 == 1 with more sequences than a tile has rows
    (128, 128, 3, 2, 1, [(2, 9), (1, 30), (3, 5), (2, 14), (1, 7), (4, 4), (1, 21), (2, 3)]),   # 8 slots: the most a launch takes (24 dgrad problems)
    (128, 128, 5, 3, 2, [(2, 7), (1, 20), (3, 5), (2, 11), (1, 4), (2, 9)]),                      # 6 slots at stride 3: 24 dgrad problems
]


def _read_rows(H, k, stride, pad):
    """mask (H,) of the input positions that some output's window covers: the others get no gradient at all"""
    H1 = (H + 2 * pad - k) // stride + 1
    m = torch.zeros(H, dtype=torch.bool)
    for q in range(H1):
        lo, hi = max(q * stride - pad, 0), min(q * stride - pad + k, H)
        if hi > lo:
            m[lo:hi] = True
    return m


def _check_case(case):
    """One CASES entry: forward, input gradient and weight gradient against float64.  Prints every figure before it asserts it (the
    children of the switch test and profiles/conv_shape_space.md read them)."""
    from vm_asr_amd import convgemm as cg, mpd_ops
    from vm_asr_amd.discriminator import split_bf16
    Cin, Cout, k, stride, pad, geom = case[:6]
    # The second forward gate, e <= 20 e32 + floor * scale, measures the kernel by torch's own fp32 error e32.  With K = k Cin = 128
    # products per output torch's fp32 sum is nearly exact (e32 ~ 1e-7 of the scale), while the bf16 triple's error does not shrink with
    # K: each product drops lo * lo and the two split residuals, (2^-18 + 2 * 2^-17) |a b| = 1.25 * 2^-16 |a b|.  Such a case names
    # one such unit, 2^-16, as its floor in place of 1e-6; the form of the gate and every other case's floor stay.
    floor = case[6] if len(case) > 6 else 1e-6
    assert cg.supported(Cin, Cout, k, stride)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(7)
    n = len(geom)
    xs = [torch.randn(ns, H, Cin, generator=g).to(dev) for ns, H in geom]
    W = (torch.randn(n, Cout, k * Cin, generator=g) / (k * Cin) ** 0.5).to(dev)
    bias = torch.randn(n, Cout, generator=g).to(dev)
    H1 = [cg.out_positions(H, k, stride, pad) for _, H in geom]
    Ms = [ns * h1 for (ns, _), h1 in zip(geom, H1)]
    rows_in = -(-max(ns * H for ns, H in geom) // 256) * 256 + 256        # some zero rows below every slot
    rows_out = -(-max(Ms) // 256) * 256
    assert mpd_ops.conv_mfma_supported_launch(Cin, Cout, k, stride, n, max(rows_in, rows_out))
    x = _stack([t.reshape(-1, Cin) for t in xs], rows_in)
    xh, xl = split_bf16(x)
    wh, wl = split_bf16(W)
    pre, y, yh, yl = cg.conv_fwd(xh, xl, wh, wl, bias, geom, k, stride, pad, rows_out, act=True)
    xs64 = [t.double().requires_grad_(True) for t in xs]
    W64 = W.double().requires_grad_(True)
    pres64, ys64 = _ref(xs64, W64, bias.double(), k, stride, pad, True)
    # torch's fp32 evaluation of the same lines, for scale
    pres32, _ = _ref(xs, W, bias, k, stride, pad, True)
    for i, M in enumerate(Ms):
        sc = pres64[i].abs().max().item()
        e = (pre[i, :M].double() - pres64[i]).abs().max().item()
        e32 = (pres32[i].double() - pres64[i]).abs().max().item()
        print(f"case {case[:5]} slot {i}: pre e {e:.3e} e32 {e32:.3e} scale {sc:.3e} used {e / (1e-4 * sc):.3f} / {e / (20 * e32 + floor * sc):.3f}")
        errtable.record("pre", pre[i, :M].double().cpu().numpy(), pres64[i].detach().cpu().numpy(), min(1e-4 * sc, 20 * e32 + floor * sc))
        assert e <= 1e-4 * sc, (i, e, sc)
        assert e <= 20 * e32 + floor * sc, (i, e, e32)
        assert (y[i, :M].double() - ys64[i]).abs().max().item() <= 1e-4 * max(1.0, ys64[i].abs().max().item())
        pair = yh[i, :M].float() + yl[i, :M].float()
        assert (pair - y[i, :M]).abs().max().item() <= 2 ** -16 * y[i, :M].abs().max().item()
        for t in (pre, y, yh, yl):
            assert not t[i, M:].any(), "padding rows must be zero"
    # backward: a random output gradient (zero on padding rows), its pair
    gy = [torch.randn(M, Cout, generator=g).to(dev) for M in Ms]
    gst = _stack(gy, rows_out)
    gh, gl = split_bf16(gst)
    loss = sum((p * gg.double()).sum() for p, gg in zip(pres64, gy))
    loss.backward()
    Wt = W.view(n, Cout, k, Cin).permute(0, 3, 2, 1).reshape(n, Cin, k * Cout).contiguous()
    wth, wtl = split_bf16(Wt)
    dx = cg.conv_dgrad(gh, gl, wth, wtl, geom, k, stride, pad, rows_in)
    for i, (ns, H) in enumerate(geom):
        want = xs64[i].grad.reshape(-1, Cin)
        sc = max(want.abs().max().item(), 1e-30)
        e = (dx[i, :ns * H].double() - want).abs().max().item()
        print(f"case {case[:5]} slot {i}: dx e {e:.3e} scale {sc:.3e} used {e / (1e-4 * sc):.3f}")
        errtable.record("dx", dx[i, :ns * H].double().cpu().numpy(), want.cpu().numpy(), 1e-4 * sc)
        assert e <= 1e-4 * sc
        assert not dx[i, ns * H:].any(), "rows below the slot's data must be zero"
        unread = ~_read_rows(H, k, stride, pad)             # (k < stride: whole residue classes; pad 0: a tail the last window misses)
        assert not dx[i, :ns * H].view(ns, H, Cin)[:, unread.to(dev)].any(), "input rows that no output reads must get an exact zero"
        assert not want.view(ns, H, Cin)[:, unread.to(dev)].any()
    for splits in (None, 1, 3):
        dw = cg.conv_wgrad(gh, gl, xh, xl, geom, k, stride, pad, splits=splits)
        sc = W64.grad.abs().max().item()
        e = (dw.double() - W64.grad).abs().max().item()
        print(f"case {case[:5]} splits {splits}: dW e {e:.3e} scale {sc:.3e} used {e / (1e-4 * sc):.3f}")
        errtable.record("dW", dw.double().cpu().numpy(), W64.grad.cpu().numpy(), 1e-4 * sc)
        assert e <= 1e-4 * sc, splits


@gpu
@pytest.mark.parametrize("case", CASES)
def test_conv_mfma_fwd_dgrad_wgrad_match_float64(case):
    _check_case(case)


@gpu
def test_conv_mfma_full_size_layer_matches_float64_on_sampled_rows():
    """configs[2]'s last hidden layer (1024 -> 1024 channels, k 5, stride 1) at the size of one period discriminator's pair
    pass: sampled output rows against float64 (the whole convolution in float64 would take minutes)."""
    from vm_asr_amd import convgemm as cg
    from vm_asr_amd.discriminator import split_bf16
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(3)
    Cin = Cout = 1024
    k, stride, pad = 5, 1, 2
    geom = [(16, 758)]
    M = 16 * 758
    rows = -(-M // 256) * 256
    x = torch.zeros(1, rows, Cin, device=dev)
    x[0, :M] = torch.randn(M, Cin, generator=g).to(dev)
    W = (torch.randn(1, Cout, k * Cin, generator=g) / (k * Cin) ** 0.5).to(dev)
    bias = torch.randn(1, Cout, generator=g).to(dev)
    xh, xl = split_bf16(x)
    wh, wl = split_bf16(W)
    pre, y, _, _ = cg.conv_fwd(xh, xl, wh, wl, bias, geom, k, stride, pad, rows, act=True)
    rows_chk = torch.tensor([0, 1, 2, 757, 758, 759, 5000, 9093, M - 3, M - 1], device=dev)
    x64 = x[0, :M].double().view(16, 758, Cin)
    xp = F.pad(x64, (0, 0, pad, pad))                                   # (16, 762, Cin)
    cols = torch.stack([xp[r // 758, (r % 758):(r % 758) + k].reshape(-1) for r in rows_chk.tolist()])
    want = cols @ W[0].double().t() + bias[0].double()
    got = pre[0, rows_chk].double()
    assert (got - want).abs().max().item() <= 1e-4 * want.abs().max().item()
    assert (y[0, rows_chk].double() - F.gelu(want)).abs().max().item() <= 1e-4 * want.abs().max().item()


@gpu
def test_conv_mfma_cu_limit_changes_nothing_but_the_grid():
    """vmasr_conv_set_cu_limit: fewer workgroups than tiles, each looping over several — bit-identical outputs."""
    from vm_asr_amd import convgemm as cg
    from vm_asr_amd.discriminator import split_bf16
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(11)
    Cin, Cout, k, stride, pad = 256, 256, 5, 3, 2
    geom = [(6, 700), (4, 1001), (9, 333)]
    n = len(geom)
    H1 = [cg.out_positions(H, k, stride, pad) for _, H in geom]
    Ms = [ns * h1 for (ns, _), h1 in zip(geom, H1)]
    rows_in = -(-max(ns * H for ns, H in geom) // 256) * 256
    rows_out = -(-max(Ms) // 256) * 256
    x = _stack([torch.randn(ns * H, Cin, generator=g).to(dev) for ns, H in geom], rows_in)
    W = (torch.randn(n, Cout, k * Cin, generator=g) / (k * Cin) ** 0.5).to(dev)
    bias = torch.randn(n, Cout, generator=g).to(dev)
    gy = _stack([torch.randn(M, Cout, generator=g).to(dev) for M in Ms], rows_out)
    xh, xl = split_bf16(x)
    wh, wl = split_bf16(W)
    gh, gl = split_bf16(gy)
    wth, wtl = split_bf16(W.view(n, Cout, k, Cin).permute(0, 3, 2, 1).reshape(n, Cin, k * Cout).contiguous())

    def run():
        f = cg.conv_fwd(xh, xl, wh, wl, bias, geom, k, stride, pad, rows_out, act=True)
        d = cg.conv_dgrad(gh, gl, wth, wtl, geom, k, stride, pad, rows_in)
        w = cg.conv_wgrad(gh, gl, xh, xl, geom, k, stride, pad, splits=2)
        torch.cuda.synchronize()
        return list(f) + [d, w]

    ref = run()
    for cus in (8, 24, 200):
        with cg.cu_limit(cus):
            got = run()
        assert int(cg._lib.lib().vmasr_conv_get_cu_limit()) == 0 and cg._LIMIT["cus"] == 0
        for a, b in zip(ref, got):
            assert torch.equal(a, b), cus


@gpu
@pytest.mark.parametrize("case", [c for c in CASES if c[0] % 128 == 0])
def test_conv_mfma_dgrad_with_the_activation_backward_in_its_epilogue(case):
    """vmasr_conv_mfma_dgrad_gelu == vmasr_conv_mfma_dgrad -> vmasr_masked_l1_bwd_add -> vmasr_gelu_bwd_split / vmasr_gelu_bwd, the three
    passes it replaces (the reference's autograd: conv backward, + the feature-matching gradient, GELU backward): BIT-EXACT — the same fp32
    tile, the same fused multiply-add of the sign term, the same GELU' expression, the same split; with and without the sign term, fp32
    output and pair."""
    import ctypes
    from vm_asr_amd import _lib, convgemm as cg
    from vm_asr_amd.discriminator import split_bf16
    Cin, Cout, k, stride, pad, geom = case[:6]
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(11)
    n = len(geom)
    H1 = [cg.out_positions(H, k, stride, pad) for _, H in geom]
    Ms = [ns * h1 for (ns, _), h1 in zip(geom, H1)]
    rows_in = -(-max(ns * H for ns, H in geom) // 256) * 256 + 256
    rows_out = -(-max(Ms) // 256) * 256
    W = (torch.randn(n, Cout, k * Cin, generator=g) / (k * Cin) ** 0.5).to(dev)
    Wt = W.view(n, Cout, k, Cin).permute(0, 3, 2, 1).reshape(n, Cin, k * Cout).contiguous()
    wth, wtl = split_bf16(Wt)
    gh, gl = split_bf16(_stack([torch.randn(M, Cout, generator=g).to(dev) for M in Ms], rows_out))
    pre = (2.0 * torch.randn(n, rows_in, Cin, generator=g)).to(dev)
    sgn = torch.randint(-1, 2, (n, rows_in, Cin), generator=g, dtype=torch.int8).to(dev)
    gtok = torch.tensor([0.37], device=dev)
    valid = [max(ns * H - 5 * i, 0) for i, (ns, H) in enumerate(geom)]
    scale = [0.5 + 0.25 * i for i in range(n)]
    lib = _lib.lib()
    dx = cg.conv_dgrad(gh, gl, wth, wtl, geom, k, stride, pad, rows_in)
    for with_sgn in (False, True):
        t = dx
        if with_sgn:
            t = torch.empty_like(dx)
            v = (ctypes.c_int64 * n)(*valid)
            sc = (ctypes.c_float * n)(*scale)
            _lib.check(lib.vmasr_masked_l1_bwd_add(sgn.data_ptr(), gtok.data_ptr(), dx.data_ptr(), t.data_ptr(), v, sc, n, rows_in, Cin,
                                                   _lib.current_stream(dev)), "masked_l1_bwd_add")
        rh, rl, r32 = torch.empty_like(gh[:, :0]).new_empty((n, rows_in, Cin)), None, torch.empty_like(t)
        rl = torch.empty_like(rh)
        _lib.check(lib.vmasr_gelu_bwd_split(pre.data_ptr(), t.data_ptr(), rh.data_ptr(), rl.data_ptr(), None, None, n, rows_in, Cin,
                                            _lib.current_stream(dev)), "gelu_bwd_split")
        _lib.check(lib.vmasr_gelu_bwd(pre.data_ptr(), t.data_ptr(), r32.data_ptr(), None, n, rows_in, Cin, _lib.current_stream(dev)), "gelu_bwd")
        kw = dict(sgn=sgn, gtok=gtok, scale=scale, valid=valid) if with_sgn else {}
        g32, pair = cg.conv_dgrad_gelu(gh, gl, wth, wtl, geom, k, stride, pad, rows_in, pre, want_f32=True, want_pair=True, **kw)
        assert torch.equal(g32, r32), (with_sgn, (g32 - r32).abs().max().item())
        assert torch.equal(pair[0], rh) and torch.equal(pair[1], rl), with_sgn
        g32b, pairb = cg.conv_dgrad_gelu(gh, gl, wth, wtl, geom, k, stride, pad, rows_in, pre, want_f32=False, want_pair=True, **kw)
        assert g32b is None and torch.equal(pairb[0], rh) and torch.equal(pairb[1], rl)
        g32c, pairc = cg.conv_dgrad_gelu(gh, gl, wth, wtl, geom, k, stride, pad, rows_in, pre, want_f32=True, want_pair=False, **kw)
        assert pairc is None and torch.equal(g32c, r32)
        for i, (ns, H) in enumerate(geom):
            assert not g32[i, ns * H:].any() and not pair[0][i, ns * H:].any(), "rows below the slot's data must be zero"
        # the bias gradient's column sums from the same epilogue == gelu_bwd_split's (fp32 atomics in another order: 1e-5 of the scale)
        db_ref = torch.zeros(n, Cin, device=dev)
        _lib.check(lib.vmasr_gelu_bwd_split(pre.data_ptr(), t.data_ptr(), rh.data_ptr(), rl.data_ptr(), None, db_ref.data_ptr(), n, rows_in, Cin,
                                            _lib.current_stream(dev)), "gelu_bwd_split")
        db = torch.zeros(n, Cin, device=dev)
        _, paird = cg.conv_dgrad_gelu(gh, gl, wth, wtl, geom, k, stride, pad, rows_in, pre, want_f32=False, want_pair=True, db=db, **kw)
        assert torch.equal(paird[0], rh) and torch.equal(paird[1], rl)
        want = r32.double().sum(1)
        sc = want.abs().max().item()
        assert (db.double() - want).abs().max().item() <= 1e-5 * sc and (db_ref.double() - want).abs().max().item() <= 1e-5 * sc


F32_CASES = [
    # (Cin, Cout, k, stride, pad, geom): the 32 -> 128 layer's geometry (ragged sequences, several tiles, sequences shorter than the kernel)
    (32, 128, 5, 3, 2, [(5, 61), (3, 100)]),
    (32, 128, 5, 3, 2, [(9, 333), (4, 517), (2, 1031)]),
    (32, 128, 5, 3, 2, [(7, 3)]),
    (32, 256, 5, 3, 2, [(6, 200)]),
    (32, 128, 1, 3, 0, [(5, 61), (3, 100)]),     # k < stride, pad 0: one K step per output
    (32, 128, 8, 1, 3, [(5, 61), (3, 100)]),     # the longest kernel the shape query admits
]


@gpu
@pytest.mark.parametrize("case", F32_CASES)
def test_conv_f32_fwd_dgrad_match_float64_at_fp32_accuracy(case):
    _check_f32_case(case)


def _check_f32_case(case):
    """The exact-f32 form (csrc/convgemm.hip OPS 1: fp32 operands, v_mfma_f32_32x32x2_f32) of the 32 -> 128 layer's forward and input
    gradient against float64 — held to what an fp32 evaluation of the same lines achieves (torch's own fp32 convolution x 4), two orders
    tighter than the bf16x3 form's 16-17 bits; epilogue (bias, GELU, bf16 pair, zero padding rows) as the pair form."""
    from vm_asr_amd import convgemm as cg
    Cin, Cout, k, stride, pad, geom = case
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(11)
    n = len(geom)
    xs = [torch.randn(ns, H, Cin, generator=g).to(dev) for ns, H in geom]
    W = (torch.randn(n, Cout, k * Cin, generator=g) / (k * Cin) ** 0.5).to(dev)
    bias = torch.randn(n, Cout, generator=g).to(dev)
    H1 = [cg.out_positions(H, k, stride, pad) for _, H in geom]
    Ms = [ns * h1 for (ns, _), h1 in zip(geom, H1)]
    rows_in = -(-max(ns * H for ns, H in geom) // 256) * 256 + 256
    rows_out = -(-max(Ms) // 256) * 256
    x = _stack([t.reshape(-1, Cin) for t in xs], rows_in)
    pre, y, yh, yl = cg.conv_fwd_f32(x, W, bias, geom, k, stride, pad, rows_out, act=True)
    xs64 = [t.double().requires_grad_(True) for t in xs]
    W64 = W.double().requires_grad_(True)
    pres64, ys64 = _ref(xs64, W64, bias.double(), k, stride, pad, True)
    pres32, _ = _ref(xs, W, bias, k, stride, pad, True)
    for i, M in enumerate(Ms):
        sc = pres64[i].abs().max().item()
        e = (pre[i, :M].double() - pres64[i]).abs().max().item()
        e32 = (pres32[i].double() - pres64[i]).abs().max().item()
        print(f"f32 case {case[:5]} slot {i}: pre e {e:.3e} e32 {e32:.3e} scale {sc:.3e} used {e / (4 * e32 + 1e-7 * sc):.3f}")
        errtable.record("pre", pre[i, :M].double().cpu().numpy(), pres64[i].detach().cpu().numpy(), 4 * e32 + 1e-7 * sc)
        assert e <= 4 * e32 + 1e-7 * sc, (i, e, e32, sc)          # fp32 accuracy (measured: at or below torch's fp32 convolution)
        assert (y[i, :M].double() - ys64[i]).abs().max().item() <= 4 * e32 + 1e-6 * max(1.0, ys64[i].abs().max().item())
        pair = yh[i, :M].float() + yl[i, :M].float()
        assert (pair - y[i, :M]).abs().max().item() <= 2 ** -16 * y[i, :M].abs().max().item()
        for t in (pre, y, yh, yl):
            assert not t[i, M:].any(), "padding rows must be zero"
    gy = [torch.randn(M, Cout, generator=g).to(dev) for M in Ms]
    gst = _stack(gy, rows_out)
    sum((p * gg.double()).sum() for p, gg in zip(pres64, gy)).backward()
    xs32 = [t.clone().requires_grad_(True) for t in xs]
    p32, _ = _ref(xs32, W, bias, k, stride, pad, True)
    sum((p * gg).sum() for p, gg in zip(p32, gy)).backward()
    Wt = W.view(n, Cout, k, Cin).permute(0, 3, 2, 1).reshape(n, Cin, k * Cout).contiguous()
    dx = cg.conv_dgrad_f32(gst, Wt, geom, k, stride, pad, rows_in)
    for i, (ns, H) in enumerate(geom):
        want = xs64[i].grad.reshape(-1, Cin)
        sc = max(want.abs().max().item(), 1e-30)
        e32 = (xs32[i].grad.reshape(-1, Cin).double() - want).abs().max().item()
        e = (dx[i, :ns * H].double() - want).abs().max().item()
        print(f"f32 case {case[:5]} slot {i}: dx e {e:.3e} e32 {e32:.3e} scale {sc:.3e} used {e / (4 * e32 + 1e-7 * sc):.3f}")
        errtable.record("dx", dx[i, :ns * H].double().cpu().numpy(), want.cpu().numpy(), 4 * e32 + 1e-7 * sc)
        assert e <= 4 * e32 + 1e-7 * sc, (i, e, e32, sc)
        assert not dx[i, ns * H:].any(), "rows below the slot's data must be zero"


# ---- the launch query against the launchers' own row bounds (no GPU: every call below is refused before anything is launched) ----------
_DUMMY = 0x10000      # a non-null, 16-byte-aligned address that is never dereferenced


def _two_slots(nseq, H):
    """Slot 0 complete (dummy addresses), slot 1 without tensors: a launcher whose checks slot 0 passes stops at slot 1 with "null tensor
    in slot 1" — still before any launch —, one whose row bound refuses slot 0 says so.  The message tells the two apart."""
    from vm_asr_amd import _lib
    sl = (_lib.CgSlot * 2)()
    for f in ("ah", "al", "bh", "bl", "c0"):
        setattr(sl[0], f, _DUMMY)
    sl[0].nseq, sl[0].H = nseq, H
    sl[1].nseq, sl[1].H = 1, H
    return sl


def _accepts(launcher, Cin, Cout, k, stride, pad, rows):
    """Does `launcher` accept a slot of `rows` rows (fwd / f32: rows_out; dgrad: rows_in; wgrad: one sequence of `rows` positions)?"""
    from vm_asr_amd import _lib
    lib = _lib.lib()
    small = _two_slots(1, max(k, 1))
    if launcher == "fwd":
        code = lib.vmasr_conv_mfma_fwd(small, 2, Cin, Cout, k, stride, pad, rows, 1, None)
    elif launcher == "f32":
        code = lib.vmasr_conv_f32_fwd(small, 2, Cin, Cout, k, stride, pad, rows, 1, None)
    elif launcher == "dgrad":
        code = lib.vmasr_conv_mfma_dgrad(small, 2, Cin, Cout, k, stride, pad, rows, None)
    else:
        code = lib.vmasr_conv_mfma_wgrad(_two_slots(1, rows), 2, Cin, Cout, k, stride, pad, 1, None)
    msg = lib.vmasr_last_error().decode()
    assert code == -1, (launcher, code, msg)                    # the invalid-argument code either way: nothing was launched
    if "null tensor in slot 1" in msg:
        return True
    assert "do not fit" in msg or "too large" in msg, (launcher, msg)
    return False


def _frontier(ok):
    """Largest multiple of 256 in [256, 2^31) for which the monotone predicate ok holds (it must hold at 256)."""
    assert ok(256)
    lo, hi = 1, (1 << 31) // 256          # ok(256 lo), not ok(256 hi)
    assert not ok(256 * hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(256 * mid) else (lo, mid)
    return 256 * lo


BOUND_SHAPES = [(128, 128, 8, 1, 3), (1024, 1024, 5, 1, 2), (128, 512, 5, 3, 2), (512, 128, 5, 3, 2), (32, 128, 5, 3, 2), (32, 128, 1, 1, 0),
                (256, 128, 3, 3, 4), (128, 256, 1, 3, 0)]


@pytest.mark.parametrize("shape", BOUND_SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_launch_query_is_the_conjunction_of_the_launchers_row_bounds(shape):
    """ADVICE r06, first finding: vmasr_conv_mfma_supported_launch == 1 must imply that forward, input gradient and weight gradient all
    accept (and the exact-f32 forward where Cin = 32 can take it), and a 0 must name rows that at least one of them refuses.  Each
    launcher's own frontier is found by bisection and the query compared on both sides of every one of them.  (The bounds differ between
    launchers when Cin != Cout, so "the query refuses" means SOME launcher refuses, not each.)"""
    from vm_asr_amd import mpd_ops
    Cin, Cout, k, stride, pad = shape
    launchers = ["fwd", "dgrad", "wgrad"] + (["f32"] if Cin == 32 else [])
    top = {name: _frontier(lambda r, name=name: _accepts(name, Cin, Cout, k, stride, pad, r)) for name in launchers}
    q_top = _frontier(lambda r: mpd_ops.conv_mfma_supported_launch(Cin, Cout, k, stride, 1, r))
    assert q_top == min(top.values()), (q_top, top)
    for rows in sorted({r + d for r in list(top.values()) + [q_top] for d in (-256, 0, 256)}):
        if not 256 <= rows < 1 << 31:
            continue
        each = {name: _accepts(name, Cin, Cout, k, stride, pad, rows) for name in launchers}
        assert {name: rows <= top[name] for name in launchers} == each, (rows, each, top)
        assert mpd_ops.conv_mfma_supported_launch(Cin, Cout, k, stride, 1, rows) == all(each.values()), (rows, each)
    # the pair form's forward addresses what its input gradient does: rows * (widest operand row) < 2^31 elements (it stopped at 2^30)
    assert top["fwd"] == ((1 << 31) // max(Cout, k * Cin) - 1) // 256 * 256
    assert _accepts("fwd", Cin, Cout, k, stride, pad, -(-((1 << 30) // max(Cout, k * Cin)) // 256) * 256)


def test_conv_mfma_config_is_what_the_switches_say():
    """vmasr_conv_mfma_config, the function the launchers ask: the default choice per shape (this process set no tuning switch)."""
    from vm_asr_amd import _lib, convgemm as cg, knobs
    if any(os.environ.get(n) for n in ("VMASR_CONV_TILE", "VMASR_CONV_MFMA", "VMASR_CONV_F32_TILE")):
        pytest.skip("a tuning switch is set: the defaults are not in force")
    assert cg.config("fwd", 256, 256) == cg.config("dgrad", 256, 256) == cg.config("wgrad", 256, 256) == (256, 256, 16)
    assert cg.config("fwd", 128, 128) == cg.config("dgrad", 128, 128) == cg.config("wgrad", 128, 128) == (128, 128, 16)
    assert cg.config("fwd", 128, 256) == (256, 256, 16) and cg.config("dgrad", 128, 256) == (128, 128, 16) and cg.config("wgrad", 128, 256) == (128, 128, 16)
    assert cg.config("fwd", 32, 128) == (256, 128, 16) and cg.config("dgrad", 32, 128) == (256, 32, 16) and cg.config("wgrad", 32, 128) == (128, 32, 16)
    assert cg.config("fwd", 32, 128, f32=True) == (128, 128, 32) and cg.config("dgrad", 32, 128, f32=True) == (256, 32, 32)
    out = (ctypes.c_int32 * 3)()
    lib = _lib.lib()
    assert lib.vmasr_conv_mfma_config(3, 128, 128, 0, out) == -1 and lib.vmasr_conv_mfma_config(0, 128, 128, 1, out) == -1
    assert lib.vmasr_conv_mfma_config(2, 32, 128, 1, out) == -1 and lib.vmasr_conv_mfma_config(0, 100, 128, 0, out) == -1
    assert lib.vmasr_conv_mfma_config(0, 128, 128, 0, None) == -1


# ---- the instantiations behind the tuning switches: read once per process, so each runs in a child ----------------------------------------
SWITCHES = {
    # name: (variable, value, what vmasr_conv_mfma_config must answer in the child, the cases it runs)
    "tile128": ("VMASR_CONV_TILE", "128", {("fwd", 256, 256): (128, 128, 16), ("dgrad", 256, 256): (128, 128, 16), ("wgrad", 256, 256): (128, 128, 16),
                                           ("fwd", 128, 256): (128, 128, 16), ("fwd", 32, 128): (128, 128, 16)}),
    "mfma32": ("VMASR_CONV_MFMA", "32", {("fwd", 256, 256): (256, 256, 32), ("dgrad", 256, 256): (256, 256, 32), ("fwd", 128, 128): (128, 128, 32),
                                         ("dgrad", 128, 128): (128, 128, 32), ("wgrad", 128, 128): (128, 128, 32), ("wgrad", 128, 256): (128, 128, 32)}),
    "f32tile256": ("VMASR_CONV_F32_TILE", "256", {("fwd", 32, 128, True): (256, 128, 32), ("fwd", 32, 256, True): (256, 128, 32)}),
}
SWITCH_CASES = [(256, 256, 5, 1, 2), (128, 256, 5, 3, 2), (128, 128, 3, 2, 1)]


def _child(name):
    """One switch setting, in a process of its own: first the proof that the library is on the non-default instantiation, then the cases."""
    from vm_asr_amd import convgemm as cg
    var, val, want = SWITCHES[name]
    assert os.environ.get(var) == val, f"{var} must be {val} in this process"
    for key, cfg in want.items():
        assert cg.config(*key) == cfg, (name, key, cg.config(*key), cfg)
    if name == "f32tile256":
        for case in F32_CASES[:2]:
            _check_f32_case(case)
    else:
        for case in [c for c in CASES if c[:5] in SWITCH_CASES]:
            _check_case(case)
    torch.cuda.synchronize()
    print(f"CHILD-OK {name}")


@gpu
def test_conv_kernels_behind_the_tuning_switches_match_float64():
    """VMASR_CONV_TILE=128 (128 x 128 tiles on 256-wide outputs), VMASR_CONV_MFMA=32 (the 32x32x16 MFMA form: forward, input gradient and
    the 128 x 128 weight gradient) and VMASR_CONV_F32_TILE=256 (the 256 x 128 exact-f32 tile) pick template instantiations that the
    default process never launches.  One fresh child per setting, one after another, each under its own time limit; the first failure
    stops the test and shows that child's output."""
    for name, (var, val, _) in SWITCHES.items():
        env = {k: v for k, v in os.environ.items() if k not in ("VMASR_CONV_TILE", "VMASR_CONV_MFMA", "VMASR_CONV_F32_TILE")}
        env[var] = val
        r = subprocess.run([sys.executable, "-m", "tests.test_convgemm", name], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0 and f"CHILD-OK {name}" in r.stdout, (name, r.returncode, r.stdout[-3000:], r.stderr[-3000:])


@gpu
def test_conv_mfma_at_the_row_frontier_matches_float64_on_sampled_rows():
    """The largest stacked launch the query admits for (128 -> 128, k 8, stride 1, pad 3): rows * 1024 just below 2^31 elements, where a
    32-bit element offset would wrap.  rows_out comes from the query by bisection.  Forward and input gradient on the first and last
    valid rows (and a few between) against float64, the weight gradient on 64 sampled columns against a float64 contraction over all rows."""
    from vm_asr_amd import convgemm as cg, mpd_ops
    from vm_asr_amd.discriminator import split_bf16
    dev = torch.device("cuda:0")
    Cin, Cout, k, stride, pad = 128, 128, 8, 1, 3
    rows = _frontier(lambda r: mpd_ops.conv_mfma_supported_launch(Cin, Cout, k, stride, 1, r))
    assert rows * k * max(Cin, Cout) < 1 << 31 <= (rows + 256) * k * max(Cin, Cout)
    nseq = 64
    H = rows // nseq                       # the input fills rows_in = rows exactly; H1 = H - 1, so 64 zero rows end the output
    H1 = cg.out_positions(H, k, stride, pad)
    M, geom = nseq * H1, [(nseq, H)]
    assert nseq * H == rows and rows - 256 < M < rows
    torch.manual_seed(5)
    x = torch.randn(1, rows, Cin, device=dev)
    W = torch.randn(1, Cout, k * Cin, device=dev) / (k * Cin) ** 0.5
    bias = torch.randn(1, Cout, device=dev)
    xh, xl = split_bf16(x)
    wh, wl = split_bf16(W)
    pre, y, _, _ = cg.conv_fwd(xh, xl, wh, wl, bias, geom, k, stride, pad, rows, act=True, want_pair=False)
    chk = [0, 1, 2, H1 - 1, H1, 1000003, M // 2, M - H1, M - 3, M - 2, M - 1]
    xp = F.pad(x[0].view(nseq, H, Cin), (0, 0, pad, pad))                              # (nseq, H + 2 pad, Cin) fp32
    cols = torch.stack([xp[r // H1, (r % H1):(r % H1) + k].reshape(-1) for r in chk]).double()
    want = cols @ W[0].double().t() + bias[0].double()
    got = pre[0, chk].double()
    e, sc = (got - want).abs().max().item(), want.abs().max().item()
    print(f"frontier rows {rows}: pre e {e:.3e} scale {sc:.3e} used {e / (1e-4 * sc):.3f}")
    assert e <= 1e-4 * sc
    assert (y[0, chk].double() - F.gelu(want)).abs().max().item() <= 1e-4 * sc
    assert not pre[0, M:].any() and not y[0, M:].any(), "padding rows must be zero"
    del xp, y
    # backward: the output gradient lives on the M valid rows
    g = torch.randn(1, rows, Cout, device=dev)
    g[0, M:] = 0
    gh, gl = split_bf16(g)
    Wt = W.view(1, Cout, k, Cin).permute(0, 3, 2, 1).reshape(1, Cin, k * Cout).contiguous()
    wth, wtl = split_bf16(Wt)
    dx = cg.conv_dgrad(gh, gl, wth, wtl, geom, k, stride, pad, rows)
    gp = F.pad(g[0, :M].view(nseq, H1, Cout), (0, 0, k - 1 - pad, H + pad - H1))       # dx[h] = sum_t g[h + pad - t] W[:, t, :]
    hs = [0, 1, 2, H - 1, H, 777777, rows // 2, rows - H, rows - 3, rows - 2, rows - 1]
    gcols = torch.stack([gp[r // H, (r % H):(r % H) + k].flip(0).reshape(-1) for r in hs]).double()      # (tap t, output channel)
    want = gcols @ Wt[0].double().t()
    e, sc = (dx[0, hs].double() - want).abs().max().item(), want.abs().max().item()
    print(f"frontier rows {rows}: dx e {e:.3e} scale {sc:.3e} used {e / (1e-4 * sc):.3f}")
    assert e <= 1e-4 * sc
    del gp, dx
    dw = cg.conv_wgrad(gh, gl, xh, xl, geom, k, stride, pad)
    csel = torch.tensor([0, 1, 31, 32, 63, 64, 126, 127], device=dev)                  # 8 taps x 8 channels = 64 columns of dW
    xs = F.pad(x[0].view(nseq, H, Cin)[:, :, csel], (0, 0, pad, pad)).double()         # (nseq, H + 2 pad, 8)
    xc = torch.stack([xs[:, t:t + H1] for t in range(k)], 2).reshape(M, k * len(csel))  # row m, column (t, c)
    want = torch.zeros(Cout, k * len(csel), dtype=torch.float64, device=dev)
    for m0 in range(0, M, 1 << 18):
        m1 = min(m0 + (1 << 18), M)
        want += g[0, m0:m1].double().t() @ xc[m0:m1]
    got = dw.view(Cout, k, Cin)[:, :, csel].reshape(Cout, -1).double()
    e, sc = (got - want).abs().max().item(), want.abs().max().item()
    print(f"frontier rows {rows}: dW e {e:.3e} scale {sc:.3e} used {e / (1e-4 * sc):.3f}")
    assert e <= 1e-4 * sc


if __name__ == "__main__":
    _child(sys.argv[1])
