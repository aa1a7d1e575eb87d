"""The fused metrics operator (csrc/metrics.hip: SNR, LSD, LSD-HF, LSD-LF of a batch in one library call), metric.per_clip /
metric.Accumulator on top of it, and the opt-in per-step metrics of the Trainer / fused metrics of the Tester.

CPU tests: the C ABI's declarations, workspace size and argument checks (nothing is launched), the accumulator's and the
trainer's host logic on the oracle STFT.  GPU tests: the kernel against the reference-made goldens, the oracle's C restatement
and a float64 numpy restatement of model/metric.py (`_ref64`, itself proven against the goldens)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "vmasr_hip.h")
EINVAL, ENOSPACE = -1, -3          # include/vmasr_hip.h: contract violated / workspace too small
ORDER = ("snr", "lsd", "lsd_hf", "lsd_lf")


def _ref64(out, tgt, hf, n_fft=2048, hop=512):
    """(B,4) float64, columns snr, lsd, lsd_hf, lsd_lf: model/metric.py in numpy float64 — torch.stft(center=True) = reflect
    padding by n_fft/2, periodic hann, rfft per frame, not normalised; an empty band is NaN (mean of nothing)."""
    out, tgt = np.asarray(out, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    B, T = out.shape
    M, F = 1 + T // hop, n_fft // 2 + 1
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    idx = np.arange(M)[:, None] * hop + np.arange(n_fft)[None, :]

    def logspec(x):
        p = np.pad(x, n_fft // 2, mode="reflect")
        return np.log10(np.maximum(np.abs(np.fft.rfft(p[idx] * win, axis=1)) ** 2, 1e-8))      # (M, F)

    res = np.zeros((B, 4))
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            d2 = (logspec(out[b]) - logspec(tgt[b])) ** 2
            h = int(hf[b])
            res[b, 0] = 20.0 * np.log10(np.linalg.norm(tgt[b]) / max(np.linalg.norm(out[b] - tgt[b]), 1e-8))
            res[b, 1] = np.sqrt(d2.mean(axis=1)).mean()
            res[b, 2] = np.sqrt(d2[:, h:].sum(axis=1) / max(F - h, 0)).mean() if h < F else np.nan
            res[b, 3] = np.sqrt(d2[:, :h].sum(axis=1) / h).mean() if h > 0 else np.nan
    return res


def _gate(got, want, tol=1e-4):
    """the golden gate of tests/test_metric.py"""
    return abs(float(got) - float(want)) <= tol * max(1.0, abs(float(want)))


def _pair(B, T, seed, noise=0.03):
    g = torch.Generator().manual_seed(seed)
    a = 0.1 * torch.randn(B, T, generator=g)
    return a, a + noise * torch.randn(B, T, generator=g)


# ---- trainer helpers (as in tests/test_trainer.py) -------------------------------------------------------------------------
def _tiny_config(gan=True, batch=2, print_freq=None):
    from vm_asr_amd.config import get_default_config, update_config
    c = get_default_config()
    c.MODEL.NAME = "DualStreamInteractiveMambaUNet"
    c.MODEL.VSSM.DIMS = 8
    c.MODEL.VSSM.DROP_PATH_RATE = 0.0
    c.DATA.STFT.N_FFT = 128
    c.DATA.STFT.WIN_LENGTH = 128
    c.DATA.TARGET_SR = 16000           # -> hop 80
    c.DATA.SEGMENT = 80 * 63 / 16000   # 64 frames, 5040 samples (> 1024: the metrics' reflect padding)
    c.DATA.BATCH_SIZE = batch
    c.TRAIN.LOW_FREQ_REPLACEMENT = True
    c.TRAIN.ADVERSARIAL.ENABLE = gan
    c.TRAIN.ADVERSARIAL.DISCRIMINATORS = ["mpd"]
    c.TRAIN.ADVERSARIAL.MPD_HIDDEN = 2
    if print_freq is not None:
        c.PRINT_FREQ = print_freq
    return update_config(c)


def _batch(cfg, n, seed=0):
    T = int(cfg.DATA.SEGMENT * cfg.DATA.TARGET_SR)
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(n, 1, T, generator=g), 0.1 * torch.randn(n, 1, T, generator=g),
            torch.full((n,), 300, dtype=torch.int64))


def _four():
    from vm_asr_amd import metric
    return [metric.snr, metric.lsd, metric.lsd_hf, metric.lsd_lf]


def _make_trainer(cfg, device, metric_ftns, loader, **kw):
    import vm_asr_amd
    from vm_asr_amd.trainer import Trainer, build_optimizer
    torch.manual_seed(cfg.SEED)
    models = vm_asr_amd.get_model(cfg)
    if device == "cpu":
        from oracle.torch_backend import use_oracle
        use_oracle(models["generator"])
    opts = {"generator": build_optimizer(cfg, models["generator"]), "discriminator": build_optimizer(cfg, [models["mpd"]])}
    return Trainer(models, metric_ftns, opts, cfg, torch.device(device), loader, None, {}, amp=False, gan=True,
                   len_epoch=len(loader) if loader is not None else 0, **kw)


def _epoch_with_collected_outputs(tr):
    """Run one training epoch; -> [(wave_out, wave_target, highcut)] of every step, collected around train_step."""
    seen, inner = [], tr.train_step

    def wrapped(wave_input, wave_target, highcut):
        wave_out, logs = inner(wave_input, wave_target, highcut)
        seen.append((wave_out.detach().clone(), wave_target.clone(), highcut.clone()))
        return wave_out, logs
    tr.train_step = wrapped
    tr._train_epoch(1)
    tr.train_step = inner
    return seen


def _composed(seen, which):
    """{name: fp64 mean over the steps in `which` of the composed metric functions}"""
    out = {}
    for f in _four():
        vals = [float(f(seen[i][0].float().squeeze(1), seen[i][1].squeeze(1), hf=seen[i][2])) for i in which]
        out[f.__name__] = sum(vals) / len(vals)
    return out


# ---- CPU: C ABI ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported():
    from vm_asr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(vmasr_[a-z0-9_]+)\s*\(", src))
    lib = _lib.lib()
    for n in ("vmasr_metrics", "vmasr_metrics_workspace"):
        assert n in declared, f"{n} is not declared in include/vmasr_hip.h"
        assert hasattr(lib, n) and n in _lib.SYMBOLS


def test_workspace_size():
    from vm_asr_amd import _lib
    ws = _lib.lib().vmasr_metrics_workspace
    for bad in ((0, 8192, 2048, 512), (4, 0, 2048, 512), (4, 8192, 0, 512), (4, 8192, 2048, 0), (-1, 8192, 2048, 512),
                (4, -5, 2048, 512), (4, 8192, 2048, -512)):
        assert ws(*bad) == 0, bad
    base = ws(4, 8192, 2048, 512)
    assert base > 0
    assert ws(8, 8192, 2048, 512) > base and ws(4, 122640, 2048, 512) > base


def test_contract_violations_are_refused_before_any_launch():
    """No GPU needed: every check runs before the first launch, so the (host) dummy operands are never touched."""
    from vm_asr_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30

    def call(out=p, tgt=p, hf=p, res=p, acc=None, B=4, T=8192, n_fft=2048, hop=512, ws=p, ws_bytes=big):
        return lib.vmasr_metrics(out, tgt, hf, res, acc, B, T, n_fft, hop, ws, ws_bytes, None)
    for n_fft in (0, 32, 100, 1000, 4096, -2048):
        assert call(n_fft=n_fft) == EINVAL, n_fft
        assert lib.vmasr_last_error()
    assert call(hop=0) == EINVAL and call(hop=-1) == EINVAL
    assert call(B=0) == EINVAL and call(B=-1) == EINVAL and call(B=65536) == EINVAL
    assert call(T=1024) == EINVAL and call(T=0) == EINVAL                    # T > n_fft/2 (reflect padding)
    assert call(n_fft=64, T=32) == EINVAL
    for k in ("out", "tgt", "hf", "res"):
        assert call(**{k: None}) == EINVAL, k
    need = lib.vmasr_metrics_workspace(4, 8192, 2048, 512)
    assert call(ws=None) == ENOSPACE
    assert call(ws_bytes=need - 1) == ENOSPACE and call(ws_bytes=0) == ENOSPACE
    # an invalid shape is reported as such even when the workspace is missing too
    assert call(B=0, ws=None, ws_bytes=0) == EINVAL


def test_per_clip_needs_device_tensors():
    from vm_asr_amd import metric
    a, b = _pair(2, 4096, 0)
    with pytest.raises(RuntimeError):
        metric.per_clip(a, b, [100, 200])
    assert metric.METRIC_ORDER == ORDER


# ---- CPU: host logic --------------------------------------------------------------------------------------------------------
def test_accumulator_cpu_is_the_mean_of_the_composed_batch_values():
    from oracle.torch_backend import oracle_stft_patch
    from vm_asr_amd import metric
    batches = [(*_pair(2, T, seed), torch.tensor(hf)) for T, seed, hf in ((4096, 1, [100, 300]), (5000, 2, [171, 512]),
                                                                           (3000, 3, [20, 900]))]
    with oracle_stft_patch():
        want = {f.__name__: [float(f(a, b, hf=hf)) for a, b, hf in batches] for f in _four()}
        acc = metric.Accumulator("cpu")
        assert acc.read() == {} and acc.count == 0
        for a, b, hf in batches:
            assert acc.update(a.unsqueeze(1), b.unsqueeze(1), hf) is None       # (B,1,T) as the trainer passes it
        assert acc.count == 3
        peek = acc.read(reset=False)
        assert acc.count == 3
        got = acc.read()
        assert acc.count == 0 and acc.read() == {}
        acc.update(*batches[0])
        again = acc.read()
    assert tuple(got) == ORDER and peek == got
    for k in ORDER:
        mean = sum(want[k]) / 3.0
        assert abs(got[k] - mean) <= 1e-12 * abs(mean), (k, got[k], mean)
        assert abs(again[k] - want[k][0]) <= 1e-12 * abs(want[k][0])           # after the reset: the new batch alone


def test_trainer_step_metrics_cpu_averages_every_step():
    from oracle.torch_backend import oracle_stft_patch
    cfg = _tiny_config(print_freq=10)           # lines at steps 0 and 2 (the last one) of 3
    loader = [(*_batch(cfg, 2, seed=s), ["x"] * 2, 0) for s in (11, 12, 13)]
    with oracle_stft_patch():
        tr = _make_trainer(cfg, "cpu", _four(), loader, step_metrics=True)
        seen = _epoch_with_collected_outputs(tr)
        assert len(seen) == 3
        want = _composed(seen, (0, 1, 2))
        for k in ORDER:
            assert k in tr.epoch_log, k
            assert abs(tr.epoch_log[k] - want[k]) <= 1e-12 * abs(want[k]), (k, tr.epoch_log[k], want[k])
        assert "total_loss" in tr.epoch_log and "epoch_seconds" in tr.epoch_log
        # off: today's behaviour — the metrics of the printed steps only
        tr0 = _make_trainer(cfg, "cpu", _four(), loader)
        seen0 = _epoch_with_collected_outputs(tr0)
        want0 = _composed(seen0, (0, 2))
        for k in ORDER:
            assert abs(tr0.epoch_log[k] - want0[k]) <= 1e-12 * abs(want0[k]), (k, tr0.epoch_log[k], want0[k])
        assert set(tr0.epoch_log) == set(tr.epoch_log)


def test_trainer_step_metrics_refuses_foreign_metric_functions():
    def my_metric(output, target, hf=None):
        return (output - target).abs().mean()
    cfg = _tiny_config()
    with pytest.raises(ValueError, match="my_metric"):
        _make_trainer(cfg, "cpu", _four() + [my_metric], None, step_metrics=True)
    _make_trainer(cfg, "cpu", _four() + [my_metric], None)          # fine without the option


def test_float64_helper_reproduces_the_goldens():
    """Proves `_ref64`, the yardstick of the GPU tests below, not the feature.  1e-6 is taken relative to max(1, |want|), like the
    other gates: the goldens are fp32 numbers made with fp32 sums, and the SNR (14.011425) has an fp32 ulp of 9.5e-7 — the helper
    differs from it by 1.06e-6 absolute = 7.6e-8 relative; the three LSD values (~0.3) agree to 6e-8 absolute."""
    z = np.load(os.path.join(GOLDEN, "metric.npz"))
    got = _ref64(z["a"], z["b"], z["hf"]).mean(axis=0)
    for i, k in enumerate(ORDER):
        print(k, got[i], float(z[k]))
        assert abs(got[i] - float(z[k])) <= 1e-6 * max(1.0, abs(float(z[k]))), (k, got[i], float(z[k]))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_per_clip_goldens():
    from vm_asr_amd import metric
    z = np.load(os.path.join(GOLDEN, "metric.npz"))
    a, b = torch.from_numpy(z["a"]).cuda(), torch.from_numpy(z["b"]).cuda()
    res = metric.per_clip(a, b, torch.from_numpy(z["hf"]))          # host hf: copied non-blocking
    assert res.shape == (3, 4) and res.dtype == torch.float32 and res.is_cuda
    got = res.double().mean(0).tolist()
    for i, k in enumerate(ORDER):
        print(k, got[i], float(z[k]))
        assert _gate(got[i], z[k]), (k, got[i], float(z[k]))
    # (B,1,T), a list for hf, 16-bit output: same call
    res3 = metric.per_clip(a.unsqueeze(1), b.unsqueeze(1), [int(v) for v in z["hf"]])
    assert torch.equal(res3, res)
    assert metric.per_clip(a.bfloat16(), b, z["hf"].tolist()).shape == (3, 4)


@pytest.mark.gpu
def test_per_clip_full_clip_vs_oracle_and_float64():
    """B=4, T=122 640 with the inputs of test_lsd_full_clip_hip_vs_oracle."""
    import oracle
    from vm_asr_amd import metric
    g = torch.Generator().manual_seed(9)
    a = 0.1 * torch.randn(4, 122640, generator=g)
    b = a + 0.03 * torch.randn(4, 122640, generator=g)
    hf = [171, 342, 513, 1024]
    res = metric.per_clip(a.cuda(), b.cuda(), hf).double().cpu().numpy()
    lsd, snr = res[:, 1].mean(), res[:, 0].mean()
    want_lsd, want_snr = oracle.lsd(a.numpy(), b.numpy()), oracle.snr(a.numpy(), b.numpy())
    print("lsd", lsd, want_lsd, "snr", snr, want_snr)
    assert abs(lsd - want_lsd) < 1e-4
    assert abs(snr - want_snr) < 1e-3
    ref = _ref64(a.numpy(), b.numpy(), hf)
    for c in (2, 3):
        for i in range(4):
            print(ORDER[c], i, res[i, c], ref[i, c])
            assert _gate(res[i, c], ref[i, c]), (ORDER[c], i, res[i, c], ref[i, c])


@pytest.mark.gpu
def test_per_clip_empty_bands_are_nan():
    from vm_asr_amd import metric
    a, b = _pair(2, 8192, 4)
    a, b = a.cuda(), b.cuda()
    lo = metric.per_clip(a, b, [0, 0]).cpu()
    hi = metric.per_clip(a, b, [1025, 1025]).cpu()
    assert torch.isnan(lo[:, 3]).all() and torch.isfinite(lo[:, :3]).all()           # LF empty
    assert torch.isnan(hi[:, 2]).all() and torch.isfinite(hi[:, [0, 1, 3]]).all()    # HF empty
    # the composed functions give the same pattern
    assert torch.isnan(metric.lsd_lf(a, b, [0, 0])) and torch.isfinite(metric.lsd_hf(a, b, [0, 0]))
    assert torch.isnan(metric.lsd_hf(a, b, [1025, 1025])) and torch.isfinite(metric.lsd_lf(a, b, [1025, 1025]))
    # with nothing in the other band, the full band IS that band
    assert torch.equal(lo[:, 1], lo[:, 2]) and torch.equal(hi[:, 1], hi[:, 3])


@pytest.mark.gpu
def test_per_clip_identical_signals():
    """LSD / HF / LF exactly 0.  SNR: 20 log10(|x| / 1e-8) ~ 190 dB; the composed value sums |x|^2 in fp32 where the kernel sums
    frame partials in fp64 — relative error of an fp32 norm over 1e5 samples ~ 1e-6, i.e. 1e-5 dB, and one fp32 ulp at 190 dB is
    1.5e-5: the existing SNR gate of 1e-3 dB holds both."""
    from vm_asr_amd import metric
    x = _pair(3, 20000, 5)[0].cuda()
    res = metric.per_clip(x, x, [171, 300, 512])
    assert (res[:, 1:] == 0.0).all(), res
    want = float(metric.snr(x, x))
    got = float(res[:, 0].double().mean())
    print("snr(x, x)", got, want)
    assert abs(got - want) < 1e-3


@pytest.mark.gpu
def test_per_clip_awkward_sizes():
    """T not a multiple of hop, few frames; and n_fft 512 / hop 128 through the raw ABI."""
    from vm_asr_amd import _lib, metric
    for B, T, hf, seed in ((1, 1500, [300], 6), (2, 8192 + 77, [171, 700], 7)):
        a, b = _pair(B, T, seed)
        res = metric.per_clip(a.cuda(), b.cuda(), hf).double().cpu().numpy()
        ref = _ref64(a.numpy(), b.numpy(), hf)
        for i in range(B):
            for c in range(4):
                print(B, T, ORDER[c], res[i, c], ref[i, c])
                assert _gate(res[i, c], ref[i, c]), (T, i, ORDER[c], res[i, c], ref[i, c])
    B, T, n_fft, hop = 3, 3000, 512, 128
    a, b = _pair(B, T, 8)
    hf = [40, 129, 257]
    lib = _lib.lib()
    da, db, dh = a.cuda(), b.cuda(), torch.tensor(hf, dtype=torch.int64).cuda()
    need = lib.vmasr_metrics_workspace(B, T, n_fft, hop)
    ws = torch.empty(need // 4 + 1, dtype=torch.float32, device="cuda")
    res = torch.empty(B, 4, dtype=torch.float32, device="cuda")
    _lib.check(lib.vmasr_metrics(_lib.ptr(da), _lib.ptr(db), _lib.ptr(dh), _lib.ptr(res), None, B, T, n_fft, hop, _lib.ptr(ws),
                                 need, _lib.current_stream(da.device)), "metrics")
    res = res.double().cpu().numpy()
    ref = _ref64(a.numpy(), b.numpy(), hf, n_fft, hop)
    assert np.isnan(ref[2, 2]) and np.isnan(res[2, 2])              # hf == F: the HF band is empty
    for i in range(B):
        for c in range(4):
            if not np.isnan(ref[i, c]):
                print(n_fft, ORDER[c], res[i, c], ref[i, c])
                assert _gate(res[i, c], ref[i, c]), (i, ORDER[c], res[i, c], ref[i, c])


@pytest.mark.gpu
def test_per_clip_is_repeatable_bit_for_bit():
    from vm_asr_amd import metric
    a, b = _pair(4, 122640, 10)
    a, b = a.cuda(), b.cuda()
    first = metric.per_clip(a, b, [171, 342, 513, 1024])
    for _ in range(3):
        assert torch.equal(metric.per_clip(a, b, [171, 342, 513, 1024]), first)


@pytest.mark.gpu
def test_accumulator_gpu():
    from vm_asr_amd import metric
    dev = torch.device("cuda:0")
    batches = [(*[t.cuda() for t in _pair(B, T, seed)], hf) for B, T, seed, hf in
               ((2, 8192, 21, [171, 300]), (4, 20000, 22, [100, 200, 512, 900]), (1, 3000, 23, [342]))]   # B and T grow, then shrink
    acc = metric.Accumulator(dev)
    assert acc.read() == {}
    want = np.zeros(4)
    for a, b, hf in batches:
        assert acc.update(a, b, hf) is None
        pc = metric.per_clip(a, b, hf).double().cpu().numpy()
        mean = np.zeros(4)
        for row in pc:                  # clip order, fp64
            mean += row
        want += mean / len(pc)
    assert acc.count == 3
    peek = acc.read(reset=False)
    got = acc.read()
    assert peek == got and acc.count == 0 and acc.read() == {}
    for i, k in enumerate(ORDER):
        print(k, got[k], want[i] / 3)
        assert abs(got[k] - want[i] / 3) <= 1e-12 * abs(want[i] / 3), (k, got[k], want[i] / 3)
    # a NaN batch mean sticks until the reset
    a, b, _ = batches[0]
    acc.update(a, b, [0, 300])
    acc.update(a, b, [171, 300])
    r = acc.read()
    assert np.isnan(r["lsd_lf"]) and all(np.isfinite(r[k]) for k in ("snr", "lsd", "lsd_hf"))
    acc.update(a, b, [171, 300])
    assert all(np.isfinite(v) for v in acc.read().values())


@pytest.mark.gpu
def test_update_has_no_host_read():
    """One update captured into a graph (a host read inside the capture would raise) and replayed twice."""
    from vm_asr_amd import graph_step, metric
    dev = torch.device("cuda:0")
    if not graph_step.replay_selftest(dev):
        pytest.skip("this runtime does not replay captured graphs faithfully")
    a, b = (t.cuda() for t in _pair(4, 20000, 31))
    hf = torch.tensor([171, 342, 513, 1024], device=dev)
    acc = metric.Accumulator(dev)
    acc.update(a, b, hf)                               # eager warm-up: the workspace exists before the capture
    torch.cuda.synchronize()
    before = acc._acc.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        acc.update(a, b, hf)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    delta = (acc._acc - before).cpu().numpy()
    assert delta[4] == 2.0
    pc = metric.per_clip(a, b, hf).double().cpu().numpy()
    mean = np.zeros(4)
    for row in pc:
        mean += row
    mean /= len(pc)
    assert np.array_equal(before.cpu().numpy()[:4], mean)           # the warm-up call added exactly the batch means
    for i in range(4):
        assert abs(delta[i] - 2 * mean[i]) <= 1e-12 * abs(2 * mean[i]), (ORDER[i], delta[i], 2 * mean[i])


@pytest.mark.gpu
def test_trainer_step_metrics_gpu():
    cfg = _tiny_config(print_freq=10)
    loader = [(*_batch(cfg, 2, seed=s), ["x"] * 2, 0) for s in (11, 12, 13)]
    tr = _make_trainer(cfg, "cuda:0", _four(), loader, step_metrics=True)
    seen = _epoch_with_collected_outputs(tr)
    assert len(seen) == 3
    want = _composed(seen, (0, 1, 2))
    for k in ORDER:
        print(k, tr.epoch_log[k], want[k])
        assert _gate(tr.epoch_log[k], want[k]), (k, tr.epoch_log[k], want[k])


@pytest.mark.gpu
def test_tester_fused_metrics(tmp_path):
    import vm_asr_amd
    from vm_asr_amd.tester import Tester
    from vm_asr_amd.trainer import SyntheticVCTK
    cfg = _tiny_config()
    cfg.defrost()
    cfg.OUTPUT = str(tmp_path / "ckpt")
    cfg.freeze()
    tr = _make_trainer(cfg, "cuda:0", [], None)
    tr._save_checkpoint(1, save_best=True)
    ev = cfg.clone()
    ev.defrost()
    ev.MODEL.RESUME_PATH, ev.OUTPUT, ev.TAG, ev.EVAL_MODE = str(tmp_path / "ckpt"), str(tmp_path / "out"), "8000_16000", True
    ev.TEST.SAVE_RESULT = False
    ev.freeze()
    loader = torch.utils.data.DataLoader(SyntheticVCTK(ev, length=2, sr_in=8000), batch_size=1)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        res = {}
        for fused in (False, True):
            gen = vm_asr_amd.get_model(ev)["generator"]
            t = Tester({"generator": gen}, _four(), ev, torch.device("cuda:0"), loader, fused_metrics=fused)
            assert (t._fused_names is not None) == fused
            res[fused] = t.evaluate()
    finally:
        os.chdir(cwd)
    for k in ORDER:
        print(k, res[True][k], res[False][k])
        assert _gate(res[True][k], res[False][k]), (k, res[True][k], res[False][k])
