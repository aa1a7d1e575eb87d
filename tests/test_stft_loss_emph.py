"""EMPHASIZE_HIGH_FREQ on the fused MR-STFT loss kernels (csrc/stftloss.hip: vmasr_stft_loss_w_fwd / _w_bwd).

The reference (model/loss.py:37-43) multiplies the (B, frames, bins) magnitudes by linspace(1, 2, frames) along dim 1 — the
frame axis — so on the (B, bins, frames) spectra the kernels read, the weight goes with the LAST index.  Checked here: the C ABI
(no GPU), the kernels against the float64 torch expression, the module's dispatch, its parity with the composed ATen path, bit
reproducibility and graph capture."""
import ctypes

import pytest
import torch

W_SYMBOLS = ("vmasr_stft_loss_w_fwd", "vmasr_stft_loss_w_bwd")


# ---- 1. C ABI (CPU) -------------------------------------------------------------------------------------------------------------

def test_w_entry_points_exported_and_declared():
    from vm_asr_amd import _lib
    lib = _lib.lib()
    for name in W_SYMBOLS:
        assert name in _lib.SYMBOLS, f"{name} has no ctypes prototype"
        assert hasattr(lib, name), f"{name} is not exported"
    assert len(_lib.SYMBOLS["vmasr_stft_loss_w_fwd"][1]) == 11 and len(_lib.SYMBOLS["vmasr_stft_loss_w_bwd"][1]) == 14


def test_w_entry_points_reject_invalid_arguments():
    """rows = 0, frames = 0, a null pointer and a pointer off the 16-byte grid come back as the ABI's invalid-argument code
    before anything is launched (no GPU needed); _lib.check turns it into the RuntimeError the wrappers raise."""
    from vm_asr_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(1 << 20)            # never dereferenced: every call below is refused on the host
    odd = ctypes.c_void_p((1 << 20) + 4)

    def fwd(rx=p, ix=p, ry=p, iy=p, rows=3, frames=5, partials=p, out=p):
        return lib.vmasr_stft_loss_w_fwd(rx, ix, ry, iy, rows, frames, 1.0, 2.0, partials, out, None)

    def bwd(rx=p, ix=p, ry=p, iy=p, rows=3, frames=5, fin=p, d_re=p, d_im=p):
        return lib.vmasr_stft_loss_w_bwd(rx, ix, ry, iy, rows, frames, 1.0, 2.0, fin, None, None, d_re, d_im, None)

    bad_fwd = [dict(rows=0), dict(frames=0), dict(rows=-1), dict(rx=None), dict(iy=None), dict(partials=None), dict(out=None),
               dict(ry=odd), dict(rows=1 << 40, frames=1 << 40)]
    bad_bwd = [dict(rows=0), dict(frames=0), dict(frames=-2), dict(ix=None), dict(fin=None), dict(d_re=None), dict(d_im=None),
               dict(d_im=odd), dict(rx=odd)]
    for fn, what, cases in ((fwd, "stft_loss_w_fwd", bad_fwd), (bwd, "stft_loss_w_bwd", bad_bwd)):
        for kw in cases:
            code = fn(**kw)
            assert code == -1, (what, kw, code)
            assert what.encode() in lib.vmasr_last_error(), (what, kw, lib.vmasr_last_error())
            with pytest.raises(RuntimeError, match=what):
                _lib.check(code, what)


# ---- 2. kernels against float64 -------------------------------------------------------------------------------------------------

def _float64_terms(rx, ix, ry, iy, emphasize=True):
    """model/loss.py:17-45,137-184 in float64 on (B, bins, frames) spectra; rx / ix may require grad."""
    def mag(re, im):
        m = torch.sqrt(torch.clamp(re ** 2 + im ** 2, min=1e-7)).transpose(2, 1)
        if emphasize:
            m = m * torch.linspace(1.0, 2.0, m.size(1), dtype=torch.float64, device=m.device).view(1, -1, 1)
        return m
    mx, my = mag(rx, ix), mag(ry.double(), iy.double())
    return torch.norm(my - mx, p="fro") / torch.norm(my, p="fro"), torch.nn.functional.l1_loss(torch.log(my), torch.log(mx))


def _spectra(shape):
    torch.manual_seed(shape[1])
    rx, ix, ry, iy = (torch.randn(shape, device="cuda:0") for _ in range(4))
    rx[0, :3, 0] = 1e-5; ix[0, :3, 0] = -2e-5                                   # below the clamp: re^2 + im^2 < 1e-7
    f, m = min(5, shape[1] - 1), min(1, shape[2] - 1)
    ry[0, f, m] = 0.0; iy[0, f, m] = 0.0
    return rx, ix, ry, iy


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 513, 37), (1, 257, 5), (3, 1025, 64), (2, 9, 1), (1, 3, 2), (4, 1025, 259), (5, 1025, 1023)])
def test_weighted_kernels_match_float64(shape):
    """The weighted forward / finish / backward against the float64 expression with emphasize_high_freq=True: rows that
    straddle a float4 (frames % 4 != 0), an aligned shape, one frame (w = 1: the unweighted kernels' bits) and six elements
    (one float4 + the scalar tail); bins below the clamp get exact zeros; each upstream weighting on its own and both.
    The last two are there for the column's step from one grid-stride sweep to the next (frames % 4 != 0 in both): the forward's
    1024 x 256 threads cover 1 048 576 elements per sweep (1 061 900 here, and every workload resolution is larger), the backward's
    at most 4096 x 256 threads 4 194 304 (5 242 875 here); a wrong step shows in sc and, with g_ml = 0, in the gradient."""
    from vm_asr_amd.loss import _STFTLossFn
    rx, ix, ry, iy = _spectra(shape)
    for wsc, wml in ((0.7, 1.3), (1.0, 0.0), (0.0, 2.0)):
        a, b = rx.clone().requires_grad_(), ix.clone().requires_grad_()
        sc, ml = _STFTLossFn.apply(a, b, ry, iy, True)
        terms = ([wsc * sc] if wsc else []) + ([wml * ml] if wml else [])
        sum(terms).backward()
        a64, b64 = rx.double().requires_grad_(), ix.double().requires_grad_()
        sc64, ml64 = _float64_terms(a64, b64, ry, iy)
        (wsc * sc64 + wml * ml64).backward()
        print(shape, wsc, wml, "sc", sc.item(), sc64.item(), "ml", ml.item(), ml64.item())
        assert abs(sc.item() - sc64.item()) <= 2e-6 * abs(sc64.item()) and abs(ml.item() - ml64.item()) <= 2e-6 * abs(ml64.item())
        for got, want in ((a.grad, a64.grad), (b.grad, b64.grad)):
            err = (got.double() - want).abs().max().item()
            print("  grad err", err, "of", want.abs().max().item())
            assert err <= 2e-5 * want.abs().max().item(), (shape, wsc, wml, err, want.abs().max().item())
        assert not a.grad[0, :3, 0].any() and not b.grad[0, :3, 0].any()
        if shape[2] == 1:                                                        # w = 1: the unweighted pair, bit for bit
            a1, b1 = rx.clone().requires_grad_(), ix.clone().requires_grad_()
            sc1, ml1 = _STFTLossFn.apply(a1, b1, ry, iy)
            sum(([wsc * sc1] if wsc else []) + ([wml * ml1] if wml else [])).backward()
            assert torch.equal(sc, sc1) and torch.equal(ml, ml1) and torch.equal(a.grad, a1.grad) and torch.equal(b.grad, b1.grad)


# ---- 3.-6. the module -----------------------------------------------------------------------------------------------------------

def _clip(seed, shape=(2, 4000)):
    g = torch.Generator().manual_seed(seed)
    y = 0.1 * torch.randn(shape, generator=g)
    x = y + 0.03 * torch.randn(shape, generator=g)
    return x.to("cuda:0"), y.to("cuda:0")


def _loss_and_grad(L, x, y):
    x = x.detach().clone().requires_grad_()
    sc, mag = L(x, y)
    (sc + mag).backward()
    return sc.detach(), mag.detach(), x.grad


def _close(got, want):
    """The bounds of tests/test_loss.py::_run, relative to the value itself: 1e-4 on sc and mag, 1e-4 max|grad| + 1e-7."""
    for name, g, w in zip(("sc", "mag"), got[:2], want[:2]):
        print(name, g.item(), w.item())
        assert abs(g.item() - w.item()) <= 1e-4 * abs(w.item()), (name, g.item(), w.item())
    err, top = (got[2] - want[2]).abs().max().item(), want[2].abs().max().item()
    print("grad err", err, "of", top)
    assert top > 0 and err <= 1e-4 * top + 1e-7, (err, top)


@pytest.mark.gpu
def test_emphasised_module_takes_the_fused_path(monkeypatch):
    import vm_asr_amd.loss as loss

    def boom(*a, **k):
        raise RuntimeError("composed path taken")

    monkeypatch.setattr(loss, "stft_magnitude", boom)
    L = loss.MultiResolutionSTFTLoss(emphasize_high_freq=True).to("cuda:0")
    x, y = _clip(0)
    sc, mag, gx = _loss_and_grad(L, x, y)
    assert torch.isfinite(sc) and torch.isfinite(mag) and sc > 0 and mag > 0
    assert torch.isfinite(gx).all() and gx.abs().max() > 0
    monkeypatch.setenv("VMASR_STFT_LOSS", "0")
    with pytest.raises(RuntimeError, match="composed path taken"):
        L(x, y)


@pytest.mark.gpu
def test_emphasised_module_matches_the_composed_path(monkeypatch):
    from vm_asr_amd.loss import MultiResolutionSTFTLoss
    L = MultiResolutionSTFTLoss(emphasize_high_freq=True).to("cuda:0")
    x, y = _clip(1)
    fused = _loss_and_grad(L, x, y)
    monkeypatch.setenv("VMASR_STFT_LOSS", "0")
    composed = _loss_and_grad(L, x, y)
    _close(fused, composed)


@pytest.mark.gpu
def test_emphasised_loss_is_bit_reproducible():
    from vm_asr_amd.loss import MultiResolutionSTFTLoss, _STFTLossFn
    L = MultiResolutionSTFTLoss(emphasize_high_freq=True).to("cuda:0")
    x, y = _clip(2)
    first, second = _loss_and_grad(L, x, y), _loss_and_grad(L, x, y)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    rx, ix, ry, iy = _spectra((3, 1025, 63))                                     # every workgroup of the forward has work
    runs = []
    for _ in range(2):
        a, b = rx.clone().requires_grad_(), ix.clone().requires_grad_()
        sc, ml = _STFTLossFn.apply(a, b, ry, iy, True)
        (sc + ml).backward()
        runs.append((sc.detach(), ml.detach(), a.grad, b.grad))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.gpu
def test_emphasised_loss_captures_into_a_graph():
    """One forward + backward captured (a host read or a synchronise inside would raise), replayed on two new inputs."""
    from vm_asr_amd import graph_step
    from vm_asr_amd.loss import MultiResolutionSTFTLoss
    dev = torch.device("cuda:0")
    if not graph_step.replay_selftest(dev):
        pytest.skip("this runtime does not replay captured graphs faithfully")
    L = MultiResolutionSTFTLoss(emphasize_high_freq=True).to(dev)
    xs, ys = _clip(3)
    xs.requires_grad_()

    def step():
        sc, mag = L(xs, ys)
        gx, = torch.autograd.grad(sc + mag, xs)
        return sc, mag, gx

    cur, side = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    cur.wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        outs = step()
    for seed in (4, 5):
        x, y = _clip(seed)
        with torch.no_grad():
            xs.copy_(x)
            ys.copy_(y)
        g.replay()
        torch.cuda.synchronize(dev)
        _close([t.detach().clone() for t in outs], _loss_and_grad(L, x, y))
    del g
