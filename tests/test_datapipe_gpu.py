"""The device half of the wav-folder pipeline (csrc/resample.hip, vm_asr_amd/resample.py, vm_asr_amd/data.py): the filter designed
on the device against the host design, the batched degradation against the single-ratio path (bitwise) and against scipy, and
PrepareOnDevice over a folder of wav files end to end.  The C ABI contract tests need no GPU.

Expected values are scipy's, stored by tests/golden/make_datapipe_golden.py in tests/golden/datapipe.npz.

Tolerances.  Taps: |h_dev - h64| <= 2^-23 |h64| + 1e-12 max|h64| element-wise — the first term is twice the half-ulp of the one
fp32 rounding, the second covers the sinc's zero crossings, where float64 sin(pi x), |x| <= 10, is accurate to a few 1e-15
absolute (a 100x margin).  Signals: the rule of tests/test_resample.py per row, max|y - y64| <= max(4 max|y32 - y64|,
2^-23 max|y64|), y32 / y64 = scipy in fp32 / float64.
"""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from test_data import FILES, SEG, make_config, make_folder

SR = 48000
DESIGN = [(1, 3), (3, 1), (160, 147), (823, 3200), (3200, 823), (47999, 48000)]
CASES = ["b3_t2000", "b1_t2000", "b3_t7"]


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "datapipe.npz")) as z:
        return {k: z[k] for k in z.files}


def _long_input(golden):
    xp = golden["xp_long"]
    return np.tile(xp, (1, -(-50000 // xp.shape[1])))[:, :50000]


def _case(golden, name):
    """-> (x (B, T) on the GPU, rates)"""
    x = _long_input(golden) if name == "long" else golden["x_" + name]
    return torch.from_numpy(np.ascontiguousarray(x)).cuda(), [int(r) for r in golden["rates_" + name]]


def _check_row(what, got, y32, y64):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == y64.shape, (what, got.shape, y64.shape)
    tol = max(4.0 * float(np.abs(y32.astype(np.float64) - y64).max()), 2.0 ** -23 * float(np.abs(y64).max()))
    err = float(np.abs(got - y64).max())
    print(f"{what}: max|hip - y64| = {err:.3e}, allowed {tol:.3e}, used {err / tol:.2f}")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


# ---- CPU: C ABI -----------------------------------------------------------------------------------------------------------------
_P = 64   # any non-null address: a refused call dereferences nothing


def test_entry_points_are_declared_and_named():
    from vm_asr_amd import _lib
    import re
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vmasr_hip.h")).read(),
                 flags=re.S)
    for name in ("vmasr_resample_design", "vmasr_resample_design_workspace", "vmasr_degrade_batch", "vmasr_degrade_batch_workspace"):
        assert re.search(r"\b" + name + r"\s*\(", src) and hasattr(_lib.lib(), name) and name in _lib.SYMBOLS
    names = [_lib.lib().vmasr_prof_name(k) for k in range(_lib.K_COUNT)]
    assert b"resample_design" in names and b"degrade_batch" in names and len(set(names)) == _lib.K_COUNT
    from vm_asr_amd import resample
    assert resample._ITEM.itemsize == 48          # sizeof(vmasr_degrade_item)


@pytest.mark.parametrize("change, message", [
    (dict(h=None), b"null"), (dict(ws=None), b"null"), (dict(up=0), b"non-positive"), (dict(down=-1), b"non-positive"),
    (dict(up=6, down=4), b"lowest terms"), (dict(half_len=0), b"half_len"), (dict(half_len=-5), b"half_len"),
    (dict(ws_bytes=100), b"workspace"),
])
def test_design_contract_violations_return_einval_before_any_launch(change, message):
    from vm_asr_amd import _lib
    lib = _lib.lib()
    assert lib.vmasr_resample_design_workspace(30) == (61 + 1024) * 8 and lib.vmasr_resample_design_workspace(0) == 0
    a = dict(dict(h=_P, up=3, down=1, half_len=30, ws=_P, ws_bytes=(61 + 1024) * 8), **change)
    assert lib.vmasr_resample_design(a["h"], a["up"], a["down"], a["half_len"], a["ws"], a["ws_bytes"], None) == -1
    assert message in lib.vmasr_last_error(), lib.vmasr_last_error()


def _items(T, clips):
    """clips: [(up, down)] -> the host table as degrade_batch lays it out (taps at a dummy address)."""
    from vm_asr_amd import resample
    items, off = np.zeros(len(clips), dtype=resample._ITEM), 0
    for b, (up, down) in enumerate(clips):
        n_mid = -(-T * up // down)
        items[b] = (0 if up == down else _P, 0 if up == down else _P, n_mid, off, up, down, 10 * max(up, down), 10 * max(up, down))
        off += 0 if up == down else -(-n_mid // 4) * 4
    return items


@pytest.mark.parametrize("what, message", [
    ("x", b"null"), ("y", b"null"), ("items", b"null"), ("items_dev", b"null"), ("ws", b"workspace"), ("B0", b"non-positive"),
    ("Bbig", b"65535"), ("T0", b"non-positive"), ("gcd", b"lowest terms"), ("up0", b"non-positive"), ("n_mid", b"n_mid"),
    ("ws_small", b"workspace"), ("overlap", b"overlaps"), ("taps", b"null taps"),
])
def test_degrade_batch_contract_violations_return_einval_before_any_launch(what, message):
    from vm_asr_amd import _lib
    lib = _lib.lib()
    T = 100
    items = _items(T, [(1, 3), (823, 3200), (1, 1)])
    need = lib.vmasr_degrade_batch_workspace(items.ctypes.data, 3)
    assert need == 4 * (36 + 28)                  # ceil(100/3) = 34 -> 36 floats, ceil(100*823/3200) = 26 -> 28; none for the copy
    a = dict(x=_P, y=_P, items=items.ctypes.data, items_dev=_P, B=3, T=T, ws=_P, ws_bytes=need)
    if what in a:
        a[what] = None
    elif what == "B0":
        a["B"] = 0
    elif what == "Bbig":
        a["B"] = 65536
    elif what == "T0":
        a["T"] = 0
    elif what == "gcd":
        items[1]["up"], items[1]["down"] = 2, 4
    elif what == "up0":
        items[0]["up"] = 0
    elif what == "n_mid":
        items[0]["n_mid"] = 33
    elif what == "ws_small":
        a["ws_bytes"] = need - 16           # 60 floats; the last intermediate ends at 36 + 26
    elif what == "overlap":
        items[1]["mid_off"] = 32
    elif what == "taps":
        items[1]["h_up"] = 0
    assert lib.vmasr_degrade_batch(a["x"], a["y"], a["items"], a["items_dev"], a["B"], a["T"], a["ws"], a["ws_bytes"], None) == -1
    assert message in lib.vmasr_last_error(), lib.vmasr_last_error()
    assert lib.vmasr_degrade_batch_workspace(None, 3) == 0 and lib.vmasr_degrade_batch_workspace(items.ctypes.data, 0) == 0


def test_misuse_of_the_python_layer_raises_before_any_launch(monkeypatch):
    from vm_asr_amd import _lib, resample
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("a launch was attempted"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        resample.degrade_batch(torch.zeros(2, 100), SR, [16000, 16000])
    with pytest.raises(RuntimeError, match="no CPU path"):
        resample.design_on_device(3, 1, "cpu")
    with pytest.raises(RuntimeError, match="positive"):
        resample.design_on_device(0, 1, "cuda")


# ---- GPU: filter design ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("up, down", DESIGN)
def test_device_design_matches_the_host_design(up, down):
    from vm_asr_amd import resample
    h64, half_len = resample.design(up, down)
    dev = torch.device("cuda", torch.cuda.current_device())
    resample._designed.clear()
    h = resample.design_on_device(up, down, dev)
    assert h.dtype == torch.float32 and h.shape == (2 * half_len + 1,) and h.device == dev
    assert resample.design_on_device(2 * up, 2 * down, dev) is h                        # reduced by the gcd, kept
    resample._designed.clear()
    again = resample.design_on_device(up, down, dev)
    assert again is not h and torch.equal(again, h)                                     # bit-identical from call to call
    got = h.cpu().numpy().astype(np.float64)
    err, allowed = np.abs(got - h64), 2.0 ** -23 * np.abs(h64) + 1e-12 * np.abs(h64).max()
    differ = int((h.cpu().numpy() != h64.astype(np.float32)).sum())
    print(f"design {up}/{down}: {h64.size} taps, {differ} differ from float32(h64), worst |h_dev - h64| / allowed = {float((err / allowed).max()):.3f}")
    assert (err <= allowed).all(), f"design {up}/{down}: {int((err > allowed).sum())} taps outside, worst {float((err / allowed).max()):.3f} of the allowance"


@pytest.mark.gpu
def test_design_cache_is_bounded():
    from vm_asr_amd import resample
    resample._designed.clear()
    first = resample.design_on_device(3, 1, "cuda")
    for d in range(2, 2 + resample.CACHE_RATIOS):
        resample.design_on_device(1, d, "cuda")
    assert len(resample._designed) == resample.CACHE_RATIOS and all(k[:2] != (3, 1) for k in resample._designed)
    assert torch.equal(resample.design_on_device(3, 1, "cuda"), first)


# ---- GPU: the batch against the single-ratio path and against scipy --------------------------------------------------------------
def _host_taps(rates, device):
    from vm_asr_amd import resample
    taps = {}
    for r in rates:
        up, down = resample._reduced(r, SR)
        if up != down:
            for key in ((up, down), (down, up)):
                taps[key] = torch.from_numpy(resample.design(*key)[0].astype(np.float32)).to(device)
    return taps


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES + ["long"])
def test_batch_is_bit_identical_to_degrade_given_the_same_taps(golden, name):
    from vm_asr_amd import resample
    x, rates = _case(golden, name)
    keep = x.clone()
    y = resample.degrade_batch(x, SR, rates, taps=_host_taps(rates, x.device))
    assert y.shape == x.shape and y.dtype == torch.float32 and torch.equal(x, keep)
    for b, r in enumerate(rates):
        assert torch.equal(y[b], resample.degrade(x[b], SR, r)), (name, b, r)
        if r == SR:
            assert torch.equal(y[b], x[b])
    y3 = resample.degrade_batch(x.unsqueeze(1), SR, rates, taps=_host_taps(rates, x.device))
    assert y3.shape == (x.shape[0], 1, x.shape[1]) and torch.equal(y3[:, 0], y)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_batch_with_device_designed_taps_matches_scipy(golden, name):
    from vm_asr_amd import resample
    x, rates = _case(golden, name)
    resample._designed.clear()
    y = resample.degrade_batch(x, SR, rates)
    for b, r in enumerate(rates):
        _check_row(f"degrade_batch {name} row {b} ({r} Hz)", y[b], golden["y32_" + name][b], golden["y64_" + name][b])
    assert len(resample._designed) == 2 * len({r for r in rates if r != SR})            # each direction designed once


@pytest.mark.gpu
def test_long_batch_with_device_designed_taps_matches_scipy(golden):
    from vm_asr_amd import resample
    x, rates = _case(golden, "long")
    y = resample.degrade_batch(x, SR, rates)
    for b, r in enumerate(rates):
        _check_row(f"degrade_batch long row {b} ({r} Hz) head", y[b, :256], golden["y32h_long"][b], golden["y64h_long"][b])
        _check_row(f"degrade_batch long row {b} ({r} Hz) tail", y[b, -256:], golden["y32t_long"][b], golden["y64t_long"][b])


@pytest.mark.gpu
def test_result_is_trimmed_to_the_clip(golden):
    from vm_asr_amd import resample
    x, rates = _case(golden, "b3_t2000")
    full = golden["full64_trim"]
    assert rates[1] == 12345 and full.size == 2003 and -(-(-(-2000 * 823 // 3200)) * 3200 // 823) == 2003   # the two passes give 2003
    y = resample.degrade_batch(x[1:2], SR, [12345])
    assert y.shape == (1, 2000)
    _check_row("trim 48000 -> 12345 -> 48000", y[0], golden["y32_b3_t2000"][1], full[:2000])


@pytest.mark.gpu
def test_misuse_on_the_gpu_raises_before_any_launch(monkeypatch):
    from vm_asr_amd import _lib, resample
    x = torch.zeros(2, 100, device="cuda")
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("a launch was attempted"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        resample.degrade_batch(x.cpu(), SR, [16000, 16000])
    with pytest.raises(RuntimeError, match="float32"):
        resample.degrade_batch(x.half(), SR, [16000, 16000])
    with pytest.raises(RuntimeError, match="rates"):
        resample.degrade_batch(x, SR, [16000])
    with pytest.raises(RuntimeError, match="positive"):
        resample.degrade_batch(x, SR, [16000, 0])
    with pytest.raises(RuntimeError, match="positive"):
        resample.degrade_batch(x, SR, [-8000, 16000])
    with pytest.raises(RuntimeError, match="taps="):
        resample.degrade_batch(x, SR, [16000, 16000], taps={})


# ---- GPU: a folder of wav files end to end ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_prepare_on_device_over_a_wav_folder(tmp_path, monkeypatch):
    """wave_in is compared bitwise with resample.degrade of the yielded target at the drawn rate.  degrade's own filters are
    designed on the host and differ from the device-designed ones at the sinc's 20 zero crossings (an exact zero against float64
    sin's 1e-17: profiles/datapipe.md), so for this comparison degrade is given the filters the pipeline uses (resample._taps ->
    design_on_device): same taps, same bits."""
    from vm_asr_amd import data, resample
    make_folder(tmp_path)
    noise = 1e-3
    cfg = make_config(tmp_path, NUM_WORKERS=0, PAD_WHITENOISE=noise)
    device = torch.device("cuda", torch.cuda.current_device())
    ds = data.WavFolder(cfg, training=True)

    def batches(seed):
        loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, num_workers=0, collate_fn=data.collate_clips)
        return list(data.PrepareOnDevice(loader, cfg, device, training=True, seed=seed))

    got = batches(11)
    assert len(got) == 2
    for a, b in zip(got, batches(11)):                                                       # the same seed: the same batches
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] and torch.equal(a[4], b[4])
    assert not torch.equal(got[0][0], batches(12)[0][0])                                     # another seed: other rates
    monkeypatch.setattr(resample, "_taps", resample.design_on_device)                        # (from here on: see the docstring)
    rng = random.Random(11)
    for wave_in, wave_tgt, highcut, names, pad in got:
        assert wave_in.shape == wave_tgt.shape == (2, 1, SEG) and wave_in.device == device and wave_tgt.dtype == torch.float32
        assert highcut.dtype == torch.int64 and highcut.shape == (2,) and len(names) == 2
        for b, name in enumerate(names):
            sr, n, _ = FILES[name]
            n_target = min(-(-min(n, SEG) * SR // sr), SEG)              # the first SEG frames, at the target rate, cut to the segment
            assert int(pad[b]) == SEG - n_target, (name, pad)
            rate = rng.randint(8000, 48000)
            assert int(highcut[b]) == resample.highcut_bin(cfg, rate)
            assert torch.equal(wave_in[b], resample.degrade(wave_tgt[b], SR, rate)), (name, rate)
            if pad[b] > 100:
                std = float(wave_tgt[b, 0, n_target:].std())
                assert noise / 2 <= std <= noise * 2, (name, std)
                assert float(wave_tgt[b, 0, :n_target].std()) > 10 * noise                   # the clip itself is in front of it
    assert sum(int(p) > 100 for _, _, _, _, pad in got for p in pad) == 1                    # p1_002.wav, 1000 frames


@pytest.mark.gpu
def test_evaluation_batches_keep_the_whole_file(tmp_path):
    from vm_asr_amd import data, resample
    make_folder(tmp_path)
    cfg = make_config(tmp_path, NUM_WORKERS=0)
    cfg.defrost()
    cfg.EVAL_MODE = True
    cfg.freeze()
    out = list(data.get_loader(cfg, "cuda"))
    assert [o[3] for o in out] == [["p3_001.wav"], ["p3_002.wav"]]
    assert out[0][0].shape == (1, 1, 3 * SEG) and int(out[0][4][0]) == 3 * SEG - 5000       # up to the next multiple of the segment
    assert out[1][0].shape == (1, 1, SEG) and int(out[1][4][0]) == SEG - 700
    assert int(out[0][2][0]) == resample.highcut_bin(cfg, 16000)                              # TAG's input rate
