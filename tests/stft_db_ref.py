"""The reference's "dB" spectrogram scale (utils/stft.py:59-62, :95-97) restated with torch.stft / torch.istft on the CPU, in
float64 (the adjudicator) or float32 (the yardstick a fp32 kernel is held to), and the clips the dB tests share.

torchaudio's AmplitudeToDB(stype="power", top_db=80) on P = |S|^2 is 10 log10 clamp(P, min=1e-10) (reference value 1: the
db_multiplier term is 0), then max(x, amax(x) - 80) with ONE amax over the whole (B', F, M) tensor: a 3-D input is read as packed
channels of a single item.  DB_to_amplitude(mag, ref=1, power=1) is 10^(0.1 mag), and its square root the amplitude 10^(mag/20)."""
import math

import torch

TOP_DB = 80.0
AMIN = 1e-10


def wav2spectro_db(wave, n_fft, hop, win, dtype=torch.float64, top_db=TOP_DB):
    """-> (mag, phase, unfloored mag), each (..., F, M) in `dtype`."""
    *other, T = wave.shape
    w = wave.detach().cpu().to(dtype).reshape(-1, T)
    S = torch.stft(w, n_fft, hop, win, torch.hann_window(win, dtype=dtype), center=True, normalized=True, return_complex=True)
    x = 10.0 * torch.log10(torch.clamp(S.abs().pow(2), min=AMIN))
    mag = torch.maximum(x, x.amax() - top_db)
    F, M = x.shape[-2:]
    return mag.view(*other, F, M), torch.angle(S).view(*other, F, M), x.view(*other, F, M)


def spectro2wav_db(mag, phase, hop, win, dtype=torch.float64):
    """(..., F, M) -> (..., hop * (M - 1)); differentiable wrt (mag, phase)."""
    *other, F, M = mag.shape
    m, p = mag.to(dtype).reshape(-1, F, M), phase.to(dtype).reshape(-1, F, M)
    amp = torch.pow(torch.pow(10.0, 0.1 * m), 0.5)
    S = torch.polar(amp, p)
    w = torch.istft(S, 2 * F - 2, hop, win, torch.hann_window(win, dtype=dtype), center=True, normalized=True)
    return w.view(*other, w.shape[-1])


def peak_db_of_bin_centred_sine(amplitude, n_fft, win):
    """Closed form: a sine of `amplitude` at a bin centre of the window (k cycles per win samples, 0 < k < win/2) in a frame away
    from the clip's edges has |S| = amplitude * sum(window) / 2 / sqrt(n_fft) at that bin (the other half of the sine's energy sits
    at the negative frequency), and the periodic hann window sums to win / 2."""
    return 20.0 * math.log10(amplitude * (win / 2.0) / 2.0 / math.sqrt(n_fft))


def _tones(T, win, amps_bins, gen=None):
    """Cosines at bin centres of the window; random phases from `gen`, or phase 0: even about t = 0, so the reflect padding
    continues them (and at T = win/2 + 1 on both sides: even the shortest clip keeps its energy in a few bins)."""
    t = torch.arange(T, dtype=torch.float64)
    x = torch.zeros(T, dtype=torch.float64)
    for a, k in amps_bins:
        ph = 0.0 if gen is None else 2 * math.pi * torch.rand((), generator=gen, dtype=torch.float64)
        x += a * torch.cos(2 * math.pi * k * t / win + ph)
    return x


def clips(B, T, win, seed=0):
    """(B, T) float32.  Clip 0: loud tones at bin centres plus white noise 100 dB below them (most bins end on the top_db floor).
    B = 2: + a clip 40 dB quieter than the loudest.  B = 3: loud, all zeros (amin, then the floor), quiet."""
    g = torch.Generator().manual_seed(1000 * seed + T)
    k1, k2 = max(2, win // 8), max(3, win // 3)
    loud = _tones(T, win, [(0.5, k1), (0.25, k2)]) + 0.5e-5 * torch.randn(T, generator=g, dtype=torch.float64)
    quiet = 0.01 * (_tones(T, win, [(0.5, k1 + 1), (0.3, k2 - 1)], g) + 1e-3 * torch.randn(T, generator=g, dtype=torch.float64))
    rows = {1: [loud], 2: [loud, quiet], 3: [loud, torch.zeros(T, dtype=torch.float64), quiet]}[B]
    return torch.stack(rows).float()
