"""STFT / iSTFT front-end (HIP).  Same names, arguments and return values as the
reference's utils/stft.py:

    wav2spectro(waveform, n_fft, hop_length, win_length, spectro_scale) -> (mag, phase)   # :22-68
    spectro2wav(mag, phase, n_fft, hop_length, win_length, spectro_scale) -> waveform      # :71-115

spectro_scale is one of the reference's two (config.py:58):

    "log2"  mag = log2(|S| + 1e-8),                      |S| = 2^mag              (every shipped config)
    "dB"    mag = 10 log10 max(|S|^2, 1e-10), floored    |S| = 10^(mag / 20)
            at max(mag) - 80 (torchaudio's AmplitudeToDB(stype="power", top_db=80), restated: torchaudio is not imported)

The dB floor follows the reference: ONE maximum over every clip of the call (torchaudio reads the leading
dimension of the (B', F, M) map as packed channels of a single item), not one per clip.  A clip's dB map
therefore depends on what else is in the batch: under "dB", Inferencer(segment_batch > 1) floors every segment
against the loudest segment of its generator call, where segment_batch = 1 floors each segment against itself.
The maximum is found and applied on the device (two launches, no host read): the call can be captured in a HIP
graph and gives the same bits every time.  Any other scale raises NotImplementedError.

spectro2wav is differentiable wrt (mag, phase) (training back-propagates through it);
wav2spectro is not differentiable (its input is the network input).

Compute: vm_asr_amd/csrc/stft.hip.  No CPU fallback.
"""
from typing import Tuple

import torch

from . import _lib

__all__ = ["wav2spectro", "spectro2wav", "stft_complex", "stft_reim", "ISTFTFunction", "STFTReImFunction"]


def _stft(waveform, n_fft, hop, win, normalized, logmag):
    _lib.require_cuda("wav2spectro", waveform)
    *other, length = waveform.shape
    w = waveform.reshape(-1, length).float().contiguous()
    Bn = w.shape[0]
    F, M = n_fft // 2 + 1, 1 + length // hop
    o0 = torch.empty((Bn, F, M), dtype=torch.float32, device=w.device)
    o1 = torch.empty_like(o0)
    _lib.call(_lib.lib().vmasr_stft, w, o0, o1, Bn, length, n_fft, hop, win, int(normalized), int(logmag))
    return o0.view(*other, F, M), o1.view(*other, F, M)


# spectro_scale -> the scale codes of include/vmasr_hip.h
_SCALES = {"log2": 0, "dB": 1}
TOP_DB = 80.0   # the reference hard-codes it (utils/stft.py:61)


def _scale_code(spectro_scale):
    try:
        return _SCALES[spectro_scale]
    except (KeyError, TypeError):
        raise NotImplementedError(f"spectro_scale must be 'log2' or 'dB' (got {spectro_scale!r})") from None


def _stft_db(waveform, n_fft, hop, win):
    _lib.require_cuda("wav2spectro", waveform)
    *other, length = waveform.shape
    w = waveform.reshape(-1, length).float().contiguous()
    Bn = w.shape[0]
    F, M = n_fft // 2 + 1, 1 + length // hop
    mag = torch.empty((Bn, F, M), dtype=torch.float32, device=w.device)
    phase = torch.empty_like(mag)
    lib = _lib.lib()
    wsb = lib.vmasr_stft_db_workspace(Bn, length, n_fft, hop)
    ws = torch.empty(max(1, wsb // 4), dtype=torch.float32, device=w.device)
    _lib.call(lib.vmasr_stft_db, w, mag, phase, Bn, length, n_fft, hop, win, 1, TOP_DB, ws, wsb)
    return mag.view(*other, F, M), phase.view(*other, F, M)


@torch.no_grad()
def wav2spectro(waveform: torch.Tensor, n_fft: int, hop_length: int, win_length: int,
                spectro_scale: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mag, phase) of the normalized, centred STFT.  Under "dB" the -80 dB floor is taken below the maximum over ALL clips of
    this call, as in the reference (see the module docstring)."""
    if _scale_code(spectro_scale) == 1:
        return _stft_db(waveform, n_fft, hop_length, win_length)
    return _stft(waveform, n_fft, hop_length, win_length, True, True)


@torch.no_grad()
def stft_complex(waveform, n_fft, hop_length, win_length, normalized=False):
    """(re, im) of torch.stft(center=True, window=hann(win_length)) — used by loss/metrics."""
    return _stft(waveform, n_fft, hop_length, win_length, normalized, False)


class STFTReImFunction(torch.autograd.Function):
    """Differentiable (re, im) of torch.stft(center=True, window=hann(win_length)) for the losses:
    forward = vmasr_stft(logmag=0), backward = vmasr_stft_bwd.  Unlike torch.stft (rocFFT) both
    directions are plain kernel launches and therefore HIP-graph capturable."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, wave, n_fft, hop, win, normalized):
        _lib.require_cuda("stft_reim", wave)
        ctx.cfg = (wave.shape, n_fft, hop, win, bool(normalized))
        return _stft(wave, n_fft, hop, win, normalized, False)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gre, gim):
        shape, n_fft, hop, win, normalized = ctx.cfg
        T = shape[-1]
        F, M = n_fft // 2 + 1, 1 + T // hop
        gre, gim = gre.reshape(-1, F, M).float().contiguous(), gim.reshape(-1, F, M).float().contiguous()
        Bn = gre.shape[0]
        lib = _lib.lib()
        gw = torch.empty((Bn, T), dtype=torch.float32, device=gre.device)
        wsb = lib.vmasr_stft_bwd_workspace(Bn, T, n_fft, hop)
        ws = torch.empty(wsb // 4, dtype=torch.float32, device=gre.device)
        _lib.call(lib.vmasr_stft_bwd, gre, gim, gw, Bn, T, n_fft, hop, win, int(normalized), ws, wsb)
        return gw.view(shape), None, None, None, None


def stft_reim(waveform, n_fft, hop_length, win_length, normalized=False):
    """(re, im), each (..., n_fft/2+1, 1+T//hop); differentiable wrt `waveform`."""
    return STFTReImFunction.apply(waveform, n_fft, hop_length, win_length, normalized)


class ISTFTFunction(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, mag, phase, hop, win, scale="log2"):
        code = _scale_code(scale)
        Bn, F, M = mag.shape
        mag, phase = mag.contiguous(), phase.contiguous()
        lib = _lib.lib()
        wav = torch.empty((Bn, hop * (M - 1)), dtype=torch.float32, device=mag.device)
        wsb = lib.vmasr_istft_workspace(Bn, F, M, hop)
        ws = torch.empty(wsb // 4, dtype=torch.float32, device=mag.device)
        _lib.call(lib.vmasr_istft_scaled, mag, phase, wav, Bn, F, M, hop, win, code, ws, wsb)
        ctx.save_for_backward(mag, phase)
        ctx.cfg = (hop, win, code)
        return wav

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        mag, phase = ctx.saved_tensors
        hop, win, code = ctx.cfg
        Bn, F, M = mag.shape
        g = g.float().contiguous()
        dmag, dphase = torch.empty_like(mag), torch.empty_like(phase)
        _lib.call(_lib.lib().vmasr_istft_scaled_bwd, mag, phase, g, dmag, dphase, Bn, F, M, hop, win, code)
        return dmag, dphase, None, None, None


def spectro2wav(mag: torch.Tensor, phase: torch.Tensor, n_fft: int, hop_length: int, win_length: int,
                spectro_scale: str) -> torch.Tensor:
    """The wave of X = |X| e^{i phase}, |X| = 2^mag ("log2") or 10^(mag/20) ("dB"); differentiable wrt (mag, phase)."""
    _scale_code(spectro_scale)
    _lib.require_cuda("spectro2wav", mag)
    *other, freqs, frames = mag.shape
    # the reference derives n_fft from the bin count (utils/stft.py:89)
    wav = ISTFTFunction.apply(mag.reshape(-1, freqs, frames), phase.reshape(-1, freqs, frames), hop_length,
                              win_length, spectro_scale)
    return wav.view(*other, wav.shape[-1])
