"""The polyphase resampler (csrc/resample.hip, vm_asr_amd/resample.py): C ABI contract, filter design, host logic of the
on-device degradation, and the kernel against scipy.signal.resample_poly.

The expected values are scipy's, stored by tests/golden/make_resample_golden.py in tests/golden/resample.npz (scipy need not be
installed where the GPU tests run).  Tolerance of every kernel comparison:

    max|hip - y64| <= max(4 * max|y32 - y64|, 2^-23 * max|y64|)

y64 = scipy on the input widened to float64, y32 = scipy on the fp32 input (scipy then filters in fp32).  The factor 4 covers
a different summation order over the 20 to 120 fp32 terms of an output (600 to 10 000 for the strong decimations, where
scipy's own fp32 error grows with them); the floor is one fp32 ulp of the tensor's largest value.  Achieved:
profiles/resample.md.
"""
import ctypes
import math
import os
import random
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vmasr_hip.h")

CASES = [(48000, 16000, 1000), (16000, 48000, 1000), (8000, 48000, 333), (48000, 8000, 1001), (48000, 44100, 700),
         (44100, 48000, 700), (12345, 48000, 500), (48000, 12345, 2000), (16000, 48000, 7), (48000, 16000, 7), (48000, 24000, 65)]
LONG = (48000, 47999, 50000)
# strong decimations, the launcher's other staging choices: 1/30 tile 128, 1/74 tile 64, 1/100 input from global memory (window
# too large for any tile; taps in LDS), 1/500 input and the 10 001 taps from global memory.  Inputs: stored periods, tiled.
STEEP = [(48000, 1600, 10000), (7400, 100, 20000), (48000, 480, 30000), (48000, 96, 60000)]
DEGRADE = [(48000, 16000, 2000), (48000, 12345, 2000)]


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "resample.npz")) as z:
        return {k: z[k] for k in z.files}


def _tolerance(y32, y64):
    return max(4.0 * float(np.abs(y32.astype(np.float64) - y64).max()), 2.0 ** -23 * float(np.abs(y64).max()))


def _check(what, got, y32, y64):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == y64.shape, (what, got.shape, y64.shape)
    tol = _tolerance(y32, y64)
    err = float(np.abs(got - y64).max())
    import errtable
    errtable.record(what, got, y64, tol)
    print(f"{what}: max|hip - y64| = {err:.3e}, allowed {tol:.3e}, used {err / tol:.2f}")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


# ---- CPU: C ABI -----------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_prototyped():
    from vm_asr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+vmasr_resample_poly\s*\(", src)
    assert hasattr(_lib.lib(), "vmasr_resample_poly")
    res, args = _lib.SYMBOLS["vmasr_resample_poly"]
    assert res is ctypes.c_int and len(args) == 10 and args[4] is ctypes.c_int64 and args[5] is ctypes.c_int64
    assert _lib.lib().vmasr_prof_name(_lib.K_COUNT - 1) == b"resample_poly"


_P = 64   # any non-null address: a refused call dereferences nothing
#                 x   h   y   B  n_in n_out up down half_len
_GOOD = dict(x=_P, h=_P, y=_P, B=2, n_in=10, n_out=30, up=3, down=1, half_len=30)


@pytest.mark.parametrize("change, message", [
    (dict(x=None), b"null"), (dict(h=None), b"null"), (dict(y=None), b"null"),
    (dict(B=0), b"non-positive"), (dict(B=-1), b"non-positive"), (dict(n_in=0, n_out=0), b"non-positive"),
    (dict(up=0), b"non-positive"), (dict(down=0), b"non-positive"), (dict(up=-3), b"non-positive"), (dict(down=-1), b"non-positive"),
    (dict(up=6, down=2), b"lowest terms"), (dict(up=3, down=3, n_out=10), b"lowest terms"),
    (dict(n_out=29), b"n_out"), (dict(n_out=31), b"n_out"), (dict(up=3, down=2, n_out=14), b"n_out"),
    (dict(half_len=-1), b"half_len"),
])
def test_contract_violations_return_einval_before_any_launch(change, message):
    from vm_asr_amd import _lib
    lib = _lib.lib()
    a = dict(_GOOD, **change)
    code = lib.vmasr_resample_poly(a["x"], a["h"], a["y"], a["B"], a["n_in"], a["n_out"], a["up"], a["down"], a["half_len"], None)
    assert code == -1
    assert message in lib.vmasr_last_error(), lib.vmasr_last_error()


# ---- CPU: filter design and host logic ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up, down", [(3, 1), (1, 6), (147, 160), (3200, 823)])
def test_design_matches_scipys_taps(golden, up, down):
    from vm_asr_amd import resample
    h, half_len = resample.design(up, down)
    assert half_len == 10 * max(up, down) and h.dtype == np.float64 and h.shape == (2 * half_len + 1,)
    want = golden[f"h_{up}_{down}"]
    got = h if want.size == h.size else h[:half_len + 1:7]      # the 64 001-tap filter is stored sampled (make_resample_golden.py)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max()
    assert np.array_equal(h, h[::-1])
    assert resample.design(2 * up, 2 * down)[0] is h            # reduced by the gcd, designed once


def test_filter_caches_stay_bounded_over_many_ratios():
    """DegradeOnDevice's training branch draws a new rate per clip: neither cache may grow with the number of distinct ratios."""
    from vm_asr_amd import resample
    cap = resample.CACHE_RATIOS
    cpu = torch.device("cpu")
    first = resample._taps(3, 1, cpu)
    assert resample._taps(3, 1, cpu) is first                              # kept while it is in use
    for down in range(2, 2 + 4 * cap):
        up = down + 1                                                      # coprime, small filters
        t = resample._taps(up, down, cpu)
        assert t.dtype == torch.float32 and t.numel() == 20 * up + 1
        assert np.array_equal(t.numpy(), resample.design(up, down)[0].astype(np.float32))
        assert len(resample._device_taps) <= cap and resample._design.cache_info().currsize <= cap
    assert resample._design.cache_info().maxsize == cap
    assert (3, 1, cpu) not in resample._device_taps                        # pushed out ...
    again = resample._taps(3, 1, cpu)
    assert again is not first and torch.equal(again, first)                # ... and designed again on the next use


def test_cpu_tensors_raise_runtime_error():
    from vm_asr_amd import resample
    x = torch.randn(2, 100)
    with pytest.raises(RuntimeError, match="no CPU path"):
        resample.resample_poly(x, 3, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        resample.resample_poly(x, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        resample.degrade(x, 48000, 16000)
    with pytest.raises(RuntimeError, match="no CPU path"):
        resample.degrade(x, 48000, 48000)
    with pytest.raises(RuntimeError):
        resample.resample_poly(x, 0, 1)


class _Cfg:
    """the three fields DegradeOnDevice reads"""
    class DATA:
        TARGET_SR = 48000
        RANDOM_RESAMPLE = [8000, 48000]

        class STFT:
            N_FFT = 2048


def _fake_loader(n_batches, batch, T=64):
    g = torch.Generator().manual_seed(5)
    return [(torch.zeros(batch, 1, T), torch.randn(batch, 1, T, generator=g), torch.zeros(batch, dtype=torch.int64),
             [f"clip{i}_{j}" for j in range(batch)], torch.zeros(batch, dtype=torch.int64)) for i in range(n_batches)]


def test_degrade_on_device_highcut_and_seeded_rates(monkeypatch):
    """Host logic only: the degradation itself is replaced by a marker that records the rate it was asked for."""
    from vm_asr_amd import resample
    asked = []

    def fake_degrade(wave, sr, sr_input):
        asked.append((sr, sr_input))
        return wave + 1.0
    monkeypatch.setattr(resample, "degrade", fake_degrade)
    loader = _fake_loader(3, 2)
    # evaluation: the fixed rate, highcut = int(1025 * 16000 / 48000)
    fixed = resample.DegradeOnDevice(loader, _Cfg, "cpu", sr_input=16000)
    assert len(fixed) == 3
    out = list(fixed)
    assert asked == [(48000, 16000)] * 6
    for (win, tgt, hc, name, pad), src in zip(out, loader):
        assert torch.equal(tgt, src[1]) and torch.equal(win, src[1] + 1.0) and name == src[3] and pad is src[4]
        assert hc.dtype == torch.int64 and hc.tolist() == [341, 341]
    assert resample.highcut_bin(_Cfg, 24000) == 512 and resample.highcut_bin(_Cfg, 48000) == 1025
    assert resample.highcut_bin(_Cfg, 8000) == 170 and resample.highcut_bin(_Cfg, 12345) == int(1025 * 12345 / 48000)
    # training: one seeded integer of [first, last] per clip, in clip order
    asked.clear()
    out = list(resample.DegradeOnDevice(loader, _Cfg, "cpu", seed=7))
    rng = random.Random(7)
    want = [rng.randint(8000, 48000) for _ in range(6)]
    assert [r for _, r in asked] == want and len(set(want)) > 1
    assert [h for b in out for h in b[2].tolist()] == [int(1025 * r / 48000) for r in want]
    asked.clear()
    list(resample.DegradeOnDevice(loader, _Cfg, "cpu", seed=7))
    assert [r for _, r in asked] == want
    asked.clear()
    list(resample.DegradeOnDevice(loader, _Cfg, "cpu", seed=8))
    assert [r for _, r in asked] != want


# ---- GPU: the kernel against scipy ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sr_from, sr_to, n_in", CASES)
def test_kernel_matches_scipy(golden, sr_from, sr_to, n_in):
    from vm_asr_amd import resample
    key = f"{sr_from}_{sr_to}_{n_in}"
    x = torch.from_numpy(golden["x_" + key]).cuda()
    assert x.shape == (2, n_in) and not torch.equal(x[0], x[1])
    y = resample.resample_poly(x, sr_to, sr_from)
    assert y.shape == (2, -(-n_in * sr_to // sr_from)) and y.dtype == torch.float32
    _check(f"resample {key}", y, golden["y32_" + key], golden["y64_" + key])


@pytest.mark.gpu
@pytest.mark.parametrize("sr_from, sr_to, n_in", STEEP)
def test_kernel_matches_scipy_on_strong_decimations(golden, sr_from, sr_to, n_in):
    from vm_asr_amd import resample
    key = f"{sr_from}_{sr_to}_{n_in}"
    xp = golden["xp_" + key]
    x = torch.from_numpy(np.tile(xp, (1, -(-n_in // xp.shape[1])))[:, :n_in]).cuda()
    y = resample.resample_poly(x, sr_to, sr_from)
    assert y.shape == (2, -(-n_in * sr_to // sr_from))
    _check(f"resample {key}", y, golden["y32_" + key], golden["y64_" + key])


@pytest.mark.gpu
def test_kernel_64_bit_indices_head_and_tail(golden):
    """47999/48000 at n_in = 50 000: half_len + m*down passes 2^31 for m > 44 739.  Input: the stored period tiled."""
    from vm_asr_amd import resample
    sr_from, sr_to, n_in = LONG
    key = f"{sr_from}_{sr_to}_{n_in}"
    xp = golden["xp_" + key]
    x = np.tile(xp, (1, -(-n_in // xp.shape[1])))[:, :n_in]
    y = resample.resample_poly(torch.from_numpy(x).cuda(), sr_to, sr_from)
    n_out = -(-n_in * sr_to // sr_from)
    assert y.shape == (2, n_out) and (n_out - 1) * 48000 > 2 ** 31
    assert torch.isfinite(y).all()
    _check(f"resample {key} head", y[:, :256], golden["y32h_" + key], golden["y64h_" + key])
    _check(f"resample {key} tail", y[:, -256:], golden["y32t_" + key], golden["y64t_" + key])


@pytest.mark.gpu
@pytest.mark.parametrize("sr, sr_input, n", DEGRADE)
def test_degrade_matches_the_scipy_chain(golden, sr, sr_input, n):
    from vm_asr_amd import resample
    key = f"{sr}_{sr_input}_{n}"
    x = torch.from_numpy(golden["deg_x_" + key]).cuda()
    y = resample.degrade(x, sr, sr_input)
    assert y.shape == x.shape and y.is_contiguous()
    _check(f"degrade {key}", y, golden["deg_y32_" + key], golden["deg_y64_" + key])
    assert resample.degrade(x, sr, sr) is x


@pytest.mark.gpu
def test_leading_dimensions_and_equal_rates(golden):
    from vm_asr_amd import resample
    key = "48000_16000_1000"
    x = torch.from_numpy(golden["x_" + key]).cuda()
    y = resample.resample_poly(x, 16000, 48000)
    y3 = resample.resample_poly(x.view(2, 1, 1000), 16000, 48000)
    assert y3.shape == (2, 1, 334) and torch.equal(y3.view(2, 334), y)
    y1 = resample.resample_poly(x[1], 16000, 48000)
    assert y1.shape == (334,) and torch.equal(y1, y[1])
    yt = resample.resample_poly(x.t().contiguous().t(), 16000, 48000)          # a non-contiguous view of the same values
    assert torch.equal(yt, y)
    same = resample.resample_poly(x, 44100, 44100)
    assert torch.equal(same, x) and same.data_ptr() != x.data_ptr()
    xg = x.clone().requires_grad_(True)
    assert not resample.resample_poly(xg, 1, 3).requires_grad                  # a data-preparation operator: no autograd


@pytest.mark.gpu
def test_call_runs_on_the_current_stream(golden, monkeypatch):
    from vm_asr_amd import _lib, resample
    lib = _lib.lib()
    real, seen = lib.vmasr_resample_poly, []

    def spy(*args):
        seen.append(args[-1].value or 0)      # (the null stream's handle reads back as None)
        return real(*args)
    spy.__name__ = "vmasr_resample_poly"
    monkeypatch.setattr(lib, "vmasr_resample_poly", spy)
    x = torch.from_numpy(golden["x_16000_48000_1000"]).cuda()
    want = resample.resample_poly(x, 3, 1)
    s = torch.cuda.Stream(device=x.device)
    s.wait_stream(torch.cuda.current_stream(x.device))
    with torch.cuda.stream(s):
        got = resample.resample_poly(x, 3, 1)
    s.synchronize()
    assert seen == [torch.cuda.current_stream(x.device).cuda_stream, s.cuda_stream] and seen[0] != seen[1]
    assert torch.equal(got, want)
