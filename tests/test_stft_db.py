"""The "dB" spectrogram scale without a GPU: what the Python surface and the C ABI refuse, and the float64 restatement
(tests/stft_db_ref.py) that adjudicates the kernels in tests/test_stft_db_gpu.py, checked against a closed form."""
import ctypes
import math

import pytest
import torch

import stft_db_ref as ref


def test_unknown_scale_still_raises_not_implemented():
    from vm_asr_amd import stft
    wave, spec = torch.zeros(1, 1, 2048), torch.zeros(1, 1, 65, 65)
    for scale in ("ln", "db", "DB", "log10", "", None):
        with pytest.raises(NotImplementedError):
            stft.wav2spectro(wave, 128, 32, 128, scale)
        with pytest.raises(NotImplementedError):
            stft.spectro2wav(spec, spec, 128, 32, 128, scale)
    # a known scale gets past that check and stops at the next one: there is no CPU path
    for scale in ("log2", "dB"):
        with pytest.raises(RuntimeError, match="CUDA"):
            stft.wav2spectro(wave, 128, 32, 128, scale)
        with pytest.raises(RuntimeError, match="CUDA"):
            stft.spectro2wav(spec, spec, 128, 32, 128, scale)


def test_db_entry_points_reject_bad_arguments():
    """Contract violations return the invalid-argument code (-1) before anything is launched (no GPU needed): null tensors, n_fft not a power of two,
    win > n_fft, a short workspace, an unknown scale."""
    from vm_asr_amd import _lib
    lib = _lib.lib()
    EINVAL = -1
    buf = (ctypes.c_float * 64)()     # stands in for device memory: nothing may touch it
    p = ctypes.cast(buf, ctypes.c_void_p)
    B, T, n, hop, win = 2, 150, 64, 16, 64
    F, M = n // 2 + 1, 1 + T // hop
    wsb = lib.vmasr_stft_db_workspace(B, T, n, hop)
    assert wsb == B * ((M + 1) // 2) * 4
    assert lib.vmasr_stft_db_workspace(0, T, n, hop) == 0

    def fwd(wav=p, mag=p, phase=p, n=n, win=win, ws=p, ws_bytes=wsb):
        return lib.vmasr_stft_db(wav, mag, phase, B, T, n, hop, win, 1, 80.0, ws, ws_bytes, None)

    for kw, msg in ((dict(wav=None), b"null"), (dict(mag=None), b"null"), (dict(phase=None), b"null"),
                    (dict(n=96), b"power of two"), (dict(n=32), b"power of two"), (dict(win=65), b"win <= n_fft"),
                    (dict(ws=None), b"workspace"), (dict(ws_bytes=wsb - 1), b"workspace"), (dict(ws_bytes=0), b"workspace")):
        assert fwd(**kw) == EINVAL, kw
        assert msg in lib.vmasr_last_error(), (kw, lib.vmasr_last_error())
    assert lib.vmasr_stft_db(p, p, p, B, n // 2, n, hop, win, 1, 80.0, p, wsb, None) == EINVAL      # T <= n_fft/2: no reflect padding

    iwsb = lib.vmasr_istft_workspace(B, F, M, hop)

    def inv(mag=p, phase=p, wav=p, F=F, win=win, scale=1, ws=p, ws_bytes=iwsb):
        return lib.vmasr_istft_scaled(mag, phase, wav, B, F, M, hop, win, scale, ws, ws_bytes, None)

    for kw, msg in ((dict(mag=None), b"null"), (dict(phase=None), b"null"), (dict(wav=None), b"null"), (dict(F=49), b"power of two"),
                    (dict(win=65), b"win <= n_fft"), (dict(scale=2), b"scale"), (dict(scale=-1), b"scale"),
                    (dict(ws=None), b"workspace"), (dict(ws_bytes=iwsb - 1), b"workspace")):
        assert inv(**kw) == EINVAL, kw
        assert msg in lib.vmasr_last_error(), (kw, lib.vmasr_last_error())

    def bwd(mag=p, phase=p, g=p, dmag=p, dphase=p, F=F, win=win, scale=1):
        return lib.vmasr_istft_scaled_bwd(mag, phase, g, dmag, dphase, B, F, M, hop, win, scale, None)

    for kw, msg in ((dict(mag=None), b"null"), (dict(phase=None), b"null"), (dict(g=None), b"null"), (dict(dmag=None), b"null"),
                    (dict(dphase=None), b"null"), (dict(F=49), b"power of two"), (dict(win=65), b"win <= n_fft"),
                    (dict(scale=2), b"scale")):
        assert bwd(**kw) == EINVAL, kw
        assert msg in lib.vmasr_last_error(), (kw, lib.vmasr_last_error())
    assert all(v == 0.0 for v in buf)


@pytest.mark.parametrize("n_fft,hop,win,k", [(64, 16, 64, 8), (64, 16, 48, 6), (1024, 240, 1024, 100)])
def test_restatement_matches_the_closed_form_of_a_bin_centred_sine(n_fft, hop, win, k):
    """A full-scale sine at a bin centre: the peak bin of every frame that does not reach the clip's edges is
    20 log10(sum(window) / 2 / sqrt(n_fft)); the neighbours of a hann-windowed bin-centred sine are 6.02 dB down."""
    T = 8 * n_fft
    t = torch.arange(T, dtype=torch.float64)
    wave = torch.sin(2 * math.pi * k * t / win + 0.3)[None]
    mag, _, raw = ref.wav2spectro_db(wave, n_fft, hop, win)
    M = mag.shape[-1]
    inner = [m for m in range(M) if m * hop - n_fft // 2 >= 0 and m * hop + n_fft // 2 <= T]
    assert len(inner) >= 3
    kb = k * n_fft // win                      # the bin of the padded transform that k cycles per window fall on
    want = ref.peak_db_of_bin_centred_sine(1.0, n_fft, win)
    assert want == pytest.approx(20 * math.log10(torch.hann_window(win, dtype=torch.float64).sum().item() / 2 / math.sqrt(n_fft)), abs=1e-12)
    peak = mag[0, kb, inner]
    assert (peak - want).abs().max().item() < 1e-9
    assert (mag[0, :, inner].argmax(0) == kb).all()
    if win == n_fft:
        assert (mag[0, kb - 1, inner] - (want - 20 * math.log10(2))).abs().max().item() < 1e-9
    assert torch.equal(mag, torch.maximum(raw, raw.amax() - 80.0))
    assert mag.min().item() == mag.max().item() - 80.0 and (raw < raw.amax() - 80.0).any()


def test_restatement_floor_is_taken_over_the_whole_batch():
    """Two clips, the second 40 dB quieter: the quiet clip's minimum is max(loud) - 80, not max(quiet) - 80."""
    n_fft, hop, win, T = 64, 16, 64, 150
    x = ref.clips(2, T, win)
    mag, _, raw = ref.wav2spectro_db(x, n_fft, hop, win)
    loud_max, quiet_max = mag[0].max().item(), mag[1].max().item()
    assert 35.0 < loud_max - quiet_max < 45.0
    assert mag[1].min().item() == loud_max - 80.0
    assert mag[1].min().item() > quiet_max - 80.0 + 35.0
    alone, _, _ = ref.wav2spectro_db(x[1:], n_fft, hop, win)
    # alone, the quiet clip's own floor (max(quiet) - 80, below 10 log10(amin) = -100 here) leaves bins that the joint call floors
    assert alone.min().item() == max(quiet_max - 80.0, -100.0) < loud_max - 80.0
    assert ((alone[0] < loud_max - 80.0) & (alone[0] > quiet_max - 80.0)).any()
    assert torch.equal(mag[1], torch.maximum(alone[0], mag[0].max() - 80.0))


def test_restatement_zero_clip_sits_on_amin_then_on_the_floor():
    n_fft, hop, win, T = 64, 16, 64, 150
    x = ref.clips(3, T, win)
    assert not x[1].any()
    mag, _, raw = ref.wav2spectro_db(x, n_fft, hop, win)
    assert (raw[1] == -100.0).all()                       # 10 log10(amin)
    assert (mag[1] == mag.max() - 80.0).all()
    for dtype in (torch.float64, torch.float32):          # the inverse undoes the forward where nothing was clamped
        g = torch.Generator().manual_seed(3)
        w = 0.1 * torch.randn(2, 640, generator=g, dtype=torch.float64)
        m, p, r = ref.wav2spectro_db(w, n_fft, hop, win, dtype)
        assert torch.equal(m, r)
        back = ref.spectro2wav_db(m, p, hop, win, dtype)
        assert (back.double() - w).abs().max().item() < (1e-12 if dtype == torch.float64 else 1e-5)
