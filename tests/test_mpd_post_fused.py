"""The period discriminator's top boundary and weight operands (csrc/convpost.hip, csrc/spectral.hip, csrc/split.hip):

  * vmasr_conv_post_bwd_gelu — conv_post's backward with the activation backward of the 1024 -> 1024 layer in it — against the chain it
    replaces (vmasr_conv_post_bwd -> vmasr_masked_l1_bwd_add -> vmasr_gelu_bwd_split / vmasr_gelu_bwd) and a float64 restatement;
  * the bf16 pair written by vmasr_sn_stack_fwd and the transposed operands of vmasr_weight_transpose: bit-equal to split_bf16 /
    permute().contiguous();
  * the module: the fused launch runs once per backward pass under the conditions of _fuse_below and nowhere else, same losses and gradients.
"""
import math

import pytest
import torch

gpu = pytest.mark.gpu

# (sequences, positions) per slot: H = 1, H = 7 and H = 13 (no multiple of the 8-row run); 150 / 140 / 143 valid rows of 160: two
# workgroups of the 32-row runs (dw / column sums wanted: 128 rows each), five of the 8-row runs (32 rows each), the last one ragged
_GEOMS = [(150, 1), (20, 7), (11, 13)]
_ROWS = 160


def _gelu_grad64(p):
    return 0.5 * (1.0 + torch.erf(p / math.sqrt(2.0))) + p * torch.exp(-0.5 * p * p) / math.sqrt(2.0 * math.pi)


def _dx64(gy, w, geoms, rows, C):
    """dx[s, q, c] = sum_j gy[s, q - j + 1] w[s, j, c] within each sequence, float64, zero on the padding rows."""
    n = len(geoms)
    dx = torch.zeros(n, rows, C, dtype=torch.float64, device=gy.device)
    for s, (N, H) in enumerate(geoms):
        M = N * H
        g = gy[s, :M].double().view(N, H)
        gp = torch.nn.functional.pad(g, (1, 1))                  # gp[:, h + 1] = g[:, h]
        w64 = w[s].double().view(3, C)
        # tap 0 reads output q + 1, tap 1 output q, tap 2 output q - 1
        d = gp[:, 2:, None] * w64[0] + gp[:, 1:-1, None] * w64[1] + gp[:, :-2, None] * w64[2]
        dx[s, :M] = d.reshape(M, C)
    return dx


@gpu
@pytest.mark.parametrize("C", [256, 1024])
def test_conv_post_bwd_gelu_against_the_chain_and_float64(C):
    """Every combination of sign term / column sums / dw / (pair, fp32, both).  From float64 the fused result is no farther than the chain's
    plus one ulp of the tensor's scale; hi + lo reproduces the fp32 g to 2^-16 relative; the column sums (atomics reorder them) and
    conv_post's own dw / db within 2e-5 of their scale (the bound of tests/test_mpd.py); padding rows exactly zero."""
    from vm_asr_amd import mpd_ops as bind
    torch.manual_seed(C)
    dev = "cuda"
    n, rows = len(_GEOMS), _ROWS
    Ms, Hs = tuple(N * H for N, H in _GEOMS), tuple(H for _, H in _GEOMS)
    assert max(Ms) < rows
    x = torch.randn(n, rows, C, device=dev)                       # padding rows hold garbage on purpose
    pre = 2.0 * torch.randn(n, rows, C, device=dev)
    gy = torch.randn(n, rows, 1, device=dev)
    w = torch.randn(n, 1, 3 * C, device=dev) / (3 * C) ** 0.5
    sgn = torch.randint(-1, 2, (n, rows, C), dtype=torch.int8, device=dev)
    gtok = torch.tensor([0.37], device=dev)
    valid = (Ms[0] - 3, Ms[1], Ms[2] - 13)                        # below M_s, equal to it, a whole sequence short
    scale = (0.5, 0.75, 1.0)
    dx64 = _dx64(gy[..., 0], w, _GEOMS, rows, C)
    dx_ref, dw_ref, db_ref = bind.conv_post_bwd(x, w, gy, Ms, Hs, True, True, True)
    ulp = 2.0 ** -23
    for with_sgn in (False, True):
        t64 = dx64.clone()
        t = dx_ref
        kw = {}
        if with_sgn:
            for s in range(n):
                t64[s, :valid[s]] += float(gtok.item()) * float(torch.tensor(scale[s], dtype=torch.float32)) * sgn[s, :valid[s]].double()
            t = bind.masked_l1_bwd(sgn, gtok, valid, scale, dx_ref, tap=True)
            kw = dict(sgn=sgn, gtok=gtok, valid=valid, scale=scale)
        g64 = t64 * _gelu_grad64(pre.double())
        for s, m in enumerate(Ms):
            g64[s, m:] = 0
        sc = g64.abs().max().item()
        dbc64 = g64.sum(1)
        dbc_ref = torch.zeros(n, C, device=dev)
        rh, rl, _ = bind.gelu_bwd_split(pre, t, dbc_ref)
        r32, _ = bind.gelu_bwd(pre, t)
        chain_err32 = (r32.double() - g64).abs().max().item()
        chain_errp = ((rh.float() + rl.float()).double() - g64).abs().max().item()
        gfull, _, _, _, _ = bind.conv_post_bwd_gelu(x, w, gy, pre, Ms, Hs, False, True, False, False, False, **kw)      # the fused fp32 g
        print(f"C={C} sgn={with_sgn}: chain from float64 {chain_err32:.3e} (fp32) {chain_errp:.3e} (pair), scale {sc:.3e}")
        for want_dbcol in (False, True):
            for want_dw in (False, True):
                for want_pair, want_f32 in ((True, False), (False, True), (True, True)):
                    tag = (with_sgn, want_dbcol, want_dw, want_pair, want_f32)
                    g32, pair, dbcol, dw, db = bind.conv_post_bwd_gelu(x, w, gy, pre, Ms, Hs, want_pair, want_f32, want_dw, True, want_dbcol, **kw)
                    assert (g32 is not None) == want_f32 and (pair is not None) == want_pair, tag
                    assert (dbcol is not None) == want_dbcol and (dw is not None) == want_dw, tag
                    if want_f32:
                        err = (g32.double() - g64).abs().max().item()
                        print(f"  {tag}: fused fp32 from float64 {err:.3e}, bit-equal to the chain: {torch.equal(g32, r32)}")
                        assert err <= chain_err32 + ulp * sc, (tag, err, chain_err32)
                        for s, m in enumerate(Ms):
                            assert not g32[s, m:].any(), (tag, s)
                    if want_pair:
                        hl = pair[0].float() + pair[1].float()
                        err = (hl.double() - g64).abs().max().item()
                        print(f"  {tag}: fused pair from float64 {err:.3e}, bit-equal to the chain: {torch.equal(pair[0], rh) and torch.equal(pair[1], rl)}")
                        assert err <= chain_errp + ulp * sc, (tag, err, chain_errp)
                        assert ((hl - gfull).abs() <= 2.0 ** -16 * gfull.abs()).all(), tag
                        for s, m in enumerate(Ms):
                            assert not pair[0][s, m:].any() and not pair[1][s, m:].any(), (tag, s)
                    if want_dbcol:
                        dsc = dbc64.abs().max().item()
                        err = (dbcol.double() - dbc64).abs().max().item()
                        print(f"  {tag}: column sums from float64 {err:.3e} of scale {dsc:.3e} (gelu_bwd_split: {(dbc_ref.double() - dbc64).abs().max().item():.3e})")
                        assert err <= 2e-5 * dsc, (tag, err, dsc)
                    if want_dw:
                        assert (dw - dw_ref).abs().max().item() <= 2e-5 * dw_ref.abs().max().item(), tag
                    assert (db - db_ref).abs().max().item() <= 2e-5 * db_ref.abs().max().item(), tag


@gpu
@pytest.mark.parametrize("Cout,Cin,k", [(512, 128, 5), (128, 32, 5), (256, 128, 3)])
def test_weight_operands_written_once_are_bit_equal(Cout, Cin, k):
    """The pair from the stack kernel == split_bf16 of its fp32 operand (which is unchanged); the transposed operands of
    vmasr_weight_transpose == split_bf16(permute().contiguous()) and the fp32 permute.  Two slots."""
    from vm_asr_amd import mpd_ops as bind
    torch.manual_seed(Cout + Cin + k)
    dev, n = "cuda", 2
    ws = [torch.randn(Cout, Cin, k, 1, device=dev) for _ in range(n)]
    sig = [torch.tensor([1.3 + 0.4 * s], device=dev) for s in range(n)]
    plain = bind.sn_stack_fwd(ws, sig)
    out, (hi, lo) = bind.sn_stack_fwd(ws, sig, want_pair=True)
    assert torch.equal(out, plain)
    rh, rl = bind.split_bf16(plain)
    assert hi.shape == plain.shape and torch.equal(hi, rh) and torch.equal(lo, rl)
    assert bind.weight_transpose_supported(Cout, Cin)
    wt = plain.view(n, Cout, k, Cin).permute(0, 3, 2, 1).reshape(n, Cin, k * Cout).contiguous()
    assert torch.equal(bind.weight_transpose(plain, k, pair=False), wt)
    th, tl = bind.weight_transpose(plain, k, pair=True)
    wh, wl = bind.split_bf16(wt)
    assert th.shape == wt.shape and torch.equal(th, wh) and torch.equal(tl, wl)


def _counted(monkeypatch):
    """The new binding and gelu_bwd_split of vm_asr_amd.mpd_ops, logged: -> (fused calls, gelu_bwd_split's gradient shapes)."""
    from vm_asr_amd import mpd_ops as bind
    fused, splits = [], []
    o1, o2 = bind.conv_post_bwd_gelu, bind.gelu_bwd_split
    monkeypatch.setattr(bind, "conv_post_bwd_gelu", lambda *a, **k: (fused.append(1), o1(*a, **k))[1])
    monkeypatch.setattr(bind, "gelu_bwd_split", lambda pre, gy, *a, **k: (splits.append(tuple(gy.shape)), o2(pre, gy, *a, **k))[1])
    return fused, splits


@gpu
def test_generator_loss_pass_finishes_the_top_activation_backward_in_conv_post(monkeypatch):
    """Generator-loss pass with the stacked feature-matching loss: the top map's tap carries the sign map and the upstream gradient, so
    conv_post's backward forms (dx + sign term) GELU' and its pair in one launch; gelu_bwd_split does not run for the top map.  Equal
    losses, d(loss)/d(signal) within 2e-6 of its scale of VMASR_MPD_FUSE_GELU_BWD=0."""
    from vm_asr_amd.discriminator import MultiPeriodDiscriminator, StackedFeatures
    from vm_asr_amd.loss import HiFiGANLoss
    torch.manual_seed(3)
    D = MultiPeriodDiscriminator(hidden=32).cuda().eval()
    y = 0.3 * torch.randn(2, 1, 12000, device="cuda")
    y_hat0 = 0.3 * torch.randn(2, 1, 12000, device="cuda")
    L = HiFiGANLoss("lsgan")
    fused, splits = _counted(monkeypatch)

    def run(fuse):
        monkeypatch.setenv("VMASR_MPD_FUSE_GELU_BWD", fuse)
        y_hat = y_hat0.clone().requires_grad_()
        with torch.no_grad():
            _, real = D.forward_single(y)
        scores, gen = D.forward_single(y_hat, detach_weights=True)
        assert isinstance(real, StackedFeatures) and isinstance(gen, StackedFeatures)
        top = tuple(gen.stacks[-2].shape)
        loss = 2.0 * L.feature_loss(real, gen) + sum((1.0 - s).pow(2).mean() for s in scores)
        fused.clear(); splits.clear()
        loss.backward()
        return loss.item(), y_hat.grad.clone(), len(fused), splits.count(top)
    l0, g0, f0, s0 = run("0")
    l1, g1, f1, s1 = run("1")
    # (the 512 -> 1024 layer's map has the top map's shape: with the fusion on no gelu_bwd_split of that shape runs at all, the inner
    #  boundaries being finished by the input-gradient epilogues; with it off both layers call it)
    assert (f0, s0) == (0, 2) and (f1, s1) == (1, 0), (f0, s0, f1, s1)
    assert l0 == l1
    sc = g0.abs().max().item()
    err = (g1 - g0).abs().max().item()
    print(f"d(loss)/d(signal): {err:.3e} of scale {sc:.3e}")
    assert torch.isfinite(g1).all() and err <= 2e-6 * sc, (err, sc)


@gpu
def test_discriminator_loss_pass_finishes_the_top_activation_backward_in_conv_post(monkeypatch):
    """Discriminator-loss pass inside scores_only(): one fused launch (bias-gradient column sums of the 1024 -> 1024 layer included), no
    gelu_bwd_split for the top map; equal losses, every parameter gradient within 2e-5 of its scale of VMASR_MPD_FUSE_GELU_BWD=0;
    VMASR_DETERMINISTIC=1 takes the unfused chain."""
    from vm_asr_amd.discriminator import MultiPeriodDiscriminator, scores_only
    torch.manual_seed(4)
    D = MultiPeriodDiscriminator(hidden=32).cuda().train()
    x = 0.3 * torch.randn(2, 1, 12000, device="cuda")
    fused, splits = _counted(monkeypatch)
    state = {k: v.clone() for k, v in D.state_dict().items()}

    def run(fuse, det=False):
        monkeypatch.setenv("VMASR_MPD_FUSE_GELU_BWD", fuse)
        if det:
            monkeypatch.setenv("VMASR_DETERMINISTIC", "1")
        else:
            monkeypatch.delenv("VMASR_DETERMINISTIC", raising=False)
        D.load_state_dict(state)          # (the power iteration of the spectral norm advances per training-mode forward)
        D.zero_grad(set_to_none=True)
        scores, feats = D.forward_single(x)
        top = tuple(feats.stacks[-2].shape)
        loss = sum((1.0 - s).pow(2).mean() for s in scores)
        fused.clear(); splits.clear()
        with scores_only():
            loss.backward()
        return loss.item(), {n: p.grad.clone() for n, p in D.named_parameters() if p.grad is not None}, len(fused), splits.count(top)
    l0, g0, f0, s0 = run("0")
    l1, g1, f1, s1 = run("1")
    l2, g2, f2, s2 = run("1", det=True)
    monkeypatch.delenv("VMASR_DETERMINISTIC", raising=False)
    # (the 512 -> 1024 layer's map has the top map's shape: both layers call gelu_bwd_split in the unfused chain, neither with the fusion on)
    assert (f0, s0) == (0, 2) and (f1, s1) == (1, 0) and (f2, s2) == (0, 2), (f0, s0, f1, s1, f2, s2)
    assert l0 == l1 == l2
    assert g0.keys() == g1.keys() == g2.keys() and len(g0) > 20
    worst = 0.0
    for k in g0:
        sc = max(g0[k].abs().max().item(), 1e-12)
        for g in (g1, g2):
            err = (g[k] - g0[k]).abs().max().item()
            worst = max(worst, err / sc)
            assert torch.isfinite(g[k]).all() and err <= 2e-5 * sc, (k, err, sc)
    print(f"worst parameter-gradient distance: {worst:.3e} of its scale")
