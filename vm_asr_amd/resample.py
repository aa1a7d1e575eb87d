"""Polyphase resampling on the device and the input degradation built on it.

    design(up, down)              -> (h float64 numpy, half_len)     scipy.signal.resample_poly's default filter
    resample_poly(x, up, down)    -> (..., ceil(T*up/down))          scipy.signal.resample_poly(x, up, down, axis=-1)
    degrade(wave, sr, sr_input)   -> wave's shape                    down to sr_input, up again, align_waveform
    DegradeOnDevice(loader, ...)                                     any loader's wave_in replaced by degrade(target)

The reference makes every low-resolution input on the CPU with scipy, one clip at a time: resample the target down to the
input rate and up again (data_loader/data_loaders.py:424-488 `_get_io_pair`; the low-pass result computed there is overwritten
by the first resample, so the degradation IS the two polyphase passes plus `align_waveform`, :523-535), and the inferencer
resamples a file to the target rate the same way (trainer/inferencer.py:239-277).  Here the operator is one library call
(csrc/resample.hip) on the current stream: no CPU path, no autograd (a data-preparation operator), RuntimeError on misuse.

The filter is scipy's: firwin(2*half_len + 1, 1/max(up, down), window=("kaiser", 5.0)) with half_len = 10*max(up, down), times
`up` — restated below with numpy alone (sinc times np.kaiser, unit DC gain), designed in float64 once per reduced ratio, and
kept as fp32 on each device it is used on.  Both caches are least-recently-used with CACHE_RATIOS entries: the fixed rates of
evaluation and inference stay resident, while the random rates of DegradeOnDevice's training branch (40 001 possible rates at
48 kHz, a quarter of them coprime to 48 000 with 960 001-tap filters of 7.7 MB float64 + 3.8 MB fp32 each) are designed per
clip like the reference's scipy call and pushed out again, so the memory held is bounded (profiles/resample.md has the cost).
"""
import collections
import functools
import math
import random

import numpy as np
import torch

from . import _lib

__all__ = ["design", "resample_poly", "degrade", "highcut_bin", "DegradeOnDevice"]


def _reduced(up, down):
    up, down = int(up), int(down)
    if up <= 0 or down <= 0:
        raise RuntimeError(f"resample_poly: up and down must be positive (got {up}, {down})")
    g = math.gcd(up, down)
    return up // g, down // g


CACHE_RATIOS = 16     # filters kept, on the host and per device cache alike (worst case 16 x 7.7 MB float64, 16 x 3.8 MB fp32)


@functools.lru_cache(maxsize=CACHE_RATIOS)
def _design(up, down):
    half_len = 10 * max(up, down)
    fc = 1.0 / max(up, down)                                  # cutoff relative to Nyquist
    m = np.arange(2 * half_len + 1, dtype=np.float64) - half_len
    h = fc * np.sinc(fc * m) * np.kaiser(2 * half_len + 1, 5.0)
    h /= h.sum()                                              # unit gain at DC
    h *= up
    h.setflags(write=False)
    return h, half_len


def design(up, down):
    """(h, half_len): the 2*half_len + 1 float64 taps scipy.signal.resample_poly(x, up, down) filters with (already times
    `up`).  Cached per reduced ratio (the CACHE_RATIOS most recently used); the array is read-only."""
    return _design(*_reduced(up, down))


_device_taps = collections.OrderedDict()     # (up, down, device) -> fp32 taps on that device, least recently used first


def _taps(up, down, device):
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (up, down, device)
    t = _device_taps.get(key)
    if t is None:
        h, _ = _design(up, down)
        t = _device_taps[key] = torch.from_numpy(h.astype(np.float32)).to(device)
        while len(_device_taps) > CACHE_RATIOS:
            old = _device_taps.popitem(last=False)[1]
            if old.is_cuda:      # a launch on another stream may still read it; evictions are rare (a new ratio: a design of
                torch.cuda.synchronize(old.device)      # milliseconds and a copy come with each), so wait rather than track streams
    else:
        _device_taps.move_to_end(key)
    return t


@torch.no_grad()
def resample_poly(x, up, down):
    """x (..., T) fp32 on the GPU -> (..., ceil(T*up/down)): every row resampled by up/down (reduced by their gcd) with
    scipy's default Kaiser filter and zero padding.  up == down returns a clone."""
    _lib.require_cuda("resample_poly", x)
    if x.dtype != torch.float32:
        raise RuntimeError(f"resample_poly: expected float32, got {x.dtype}")
    if x.dim() < 1 or x.shape[-1] < 1 or x.numel() == 0:
        raise RuntimeError(f"resample_poly: expected (..., T) with T >= 1 and no empty dimension, got {tuple(x.shape)}")
    up, down = _reduced(up, down)
    if up == down:
        return x.clone()
    T = x.shape[-1]
    rows = _lib.rows2d(x, T)
    n_out = -(-T * up // down)
    h = _taps(up, down, x.device)
    y = torch.empty((rows.shape[0], n_out), dtype=torch.float32, device=x.device)
    _lib.call(_lib.lib().vmasr_resample_poly, rows, h, y, rows.shape[0], T, n_out, up, down, (h.numel() - 1) // 2)
    return y.view(*x.shape[:-1], n_out)


def degrade(wave, sr, sr_input):
    """The reference's low-resolution input of `wave` (..., T) at rate `sr`: resampled down to `sr_input`, up to `sr` again,
    zero-padded or trimmed to T (align_waveform).  Equal rates return `wave` itself, as the reference does."""
    sr, sr_input = int(sr), int(sr_input)
    if sr_input == sr:
        _lib.require_cuda("degrade", wave)
        return wave
    back = resample_poly(resample_poly(wave, sr_input, sr), sr, sr_input)
    T = wave.shape[-1]
    if back.shape[-1] < T:
        return torch.nn.functional.pad(back, (0, T - back.shape[-1]))
    return back[..., :T].contiguous()


def highcut_bin(config, sr_input):
    """First STFT bin above the input's band: int((N_FFT//2 + 1) * sr_input / TARGET_SR) (data_loaders.py:482-486)."""
    return int((config.DATA.STFT.N_FFT // 2 + 1) * int(sr_input) / config.DATA.TARGET_SR)


class DegradeOnDevice:
    """Wraps a loader of the batch contract `(wave_in, wave_tgt, highcut, name, pad)`: the target goes to `device`, `wave_in`
    becomes degrade(target) clip by clip, `highcut` the bin of the rate used.  `sr_input` fixed is the evaluation branch of
    `_get_io_pair` (the rate of TAG); None is its training branch: an integer drawn uniformly from DATA.RANDOM_RESAMPLE
    [first, last] per clip, from random.Random(seed) (one stream of draws over the wrapper's lifetime)."""

    def __init__(self, loader, config, device, sr_input=None, seed=0):
        self.loader, self.config, self.device = loader, config, torch.device(device)
        self.sr_input = None if sr_input is None else int(sr_input)
        self.target_sr = int(config.DATA.TARGET_SR)
        self._rng = random.Random(seed)

    def __len__(self):
        return len(self.loader)

    def draw_rate(self):
        if self.sr_input is not None:
            return self.sr_input
        rr = self.config.DATA.RANDOM_RESAMPLE
        return self._rng.randint(int(rr[0]), int(rr[-1]))

    def __iter__(self):
        for _, wave_tgt, _, name, pad in self.loader:
            rates = [self.draw_rate() for _ in range(wave_tgt.shape[0])]
            tgt = wave_tgt.to(self.device, non_blocking=True)
            wave_in = torch.stack([degrade(tgt[i], self.target_sr, r) for i, r in enumerate(rates)])
            highcut = torch.tensor([highcut_bin(self.config, r) for r in rates], dtype=torch.int64)
            yield wave_in, tgt, highcut, name, pad
