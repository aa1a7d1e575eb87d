"""Polyphase resampling on the device and the input degradation built on it.

    design(up, down)              -> (h float64 numpy, half_len)     scipy.signal.resample_poly's default filter
    resample_poly(x, up, down)    -> (..., ceil(T*up/down))          scipy.signal.resample_poly(x, up, down, axis=-1)
    degrade(wave, sr, sr_input)   -> wave's shape                    down to sr_input, up again, align_waveform
    DegradeOnDevice(loader, ...)                                     any loader's wave_in replaced by degrade(target)
    design_on_device(up, down, device) -> fp32 taps on `device`      the same filter designed by the library, no host work
    degrade_batch(waves, sr, rates)    -> waves' shape               degrade() of every clip at its own rate, two launches

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

__all__ = ["design", "resample_poly", "degrade", "highcut_bin", "DegradeOnDevice", "design_on_device", "degrade_batch"]


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


# ---- a batch at per-clip rates: filters designed on the device, two launches (csrc/resample.hip) ----------------------------------------
# The random rates of training rarely repeat (40 001 possible at 48 kHz), so the host design of `_taps` (75 ms for a rate coprime
# to 48 000: profiles/resample.md) is replaced by one library call per direction, and the clips of a batch share two launches
# instead of two launches, a pad or slice and a stack each (profiles/datapipe.md has the measured difference).

_designed = collections.OrderedDict()        # (up, down, device) -> fp32 taps designed on that device, least recently used first

_ITEM = np.dtype([("h_down", "u8"), ("h_up", "u8"), ("n_mid", "i8"), ("mid_off", "i8"), ("up", "i4"), ("down", "i4"),
                  ("half_len", "i4"), ("half_len_up", "i4")])            # vmasr_degrade_item (include/vmasr_hip.h)


@torch.no_grad()
def design_on_device(up, down, device):
    """The 2*half_len + 1 fp32 taps of `design(up, down)` (half_len = 10*max(up, down) of the reduced ratio) on the GPU `device`,
    computed there in float64 by one library call: no host design, no copy.  The CACHE_RATIOS most recently used ratios per
    process are kept; an evicted filter is freed once the launches that read it have run (a user on another stream than the
    one it was designed on records that stream, as degrade_batch does)."""
    up, down = _reduced(up, down)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("design_on_device: expected a CUDA (HIP) device; vm_asr_amd has no CPU path")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (up, down, device)
    h = _designed.get(key)
    if h is not None:
        _designed.move_to_end(key)
        return h
    half_len = 10 * max(up, down)
    lib = _lib.lib()
    ws_bytes = lib.vmasr_resample_design_workspace(half_len)
    with torch.cuda.device(device):
        h = torch.empty(2 * half_len + 1, dtype=torch.float32, device=device)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    _lib.call(lib.vmasr_resample_design, h, up, down, half_len, ws, ws_bytes)
    _designed[key] = h
    while len(_designed) > CACHE_RATIOS:
        _designed.popitem(last=False)
    return h


@torch.no_grad()
def degrade_batch(waves, sr, rates, taps=None):
    """waves (B, T) or (B, 1, T) fp32 on the GPU -> the same shape: row b is degrade(waves[b], sr, rates[b]) — down to rates[b],
    up to `sr` again, trimmed or zero-filled to T; a clip whose rate equals `sr` is copied — for the whole batch in one library
    call of two launches.  `taps`: {(up, down) reduced: fp32 taps on waves' device} for both directions of every ratio used
    (given the taps degrade() uses, a row is bit-identical to it); absent, every distinct direction is designed on the device
    (design_on_device) once.  No autograd, no CPU path; RuntimeError on misuse."""
    _lib.require_cuda("degrade_batch", waves)
    if waves.dtype != torch.float32:
        raise RuntimeError(f"degrade_batch: expected float32, got {waves.dtype}")
    if not (waves.dim() == 2 or (waves.dim() == 3 and waves.shape[1] == 1)) or waves.numel() == 0:
        raise RuntimeError(f"degrade_batch: expected (B, T) or (B, 1, T) with B, T >= 1, got {tuple(waves.shape)}")
    B, T = waves.shape[0], waves.shape[-1]
    rates = [int(r) for r in rates]
    if len(rates) != B:
        raise RuntimeError(f"degrade_batch: {len(rates)} rates for {B} clips")
    ratios = [_reduced(r, sr) for r in rates]                  # (up, down) of the down pass; RuntimeError for a rate <= 0
    stream = torch.cuda.current_stream(waves.device)
    filt = {}

    def taps_of(up, down):
        h = filt.get((up, down))
        if h is None:
            if taps is None:
                h = design_on_device(up, down, waves.device)
                h.record_stream(stream)                        # (a no-op on the stream it was designed on)
            else:
                h = taps.get((up, down))
                if h is None:
                    raise RuntimeError(f"degrade_batch: taps= has no filter for the ratio {up}/{down}")
                if not (h.is_cuda and h.device == waves.device and h.dtype == torch.float32 and h.dim() == 1 and h.is_contiguous()
                        and h.numel() % 2 == 1):
                    raise RuntimeError(f"degrade_batch: taps[{(up, down)}] must be an odd number of contiguous fp32 taps on {waves.device}")
            filt[(up, down)] = h
        return h

    items, off = np.zeros(B, dtype=_ITEM), 0
    for b, (up, down) in enumerate(ratios):
        n_mid = -(-T * up // down)
        items[b]["up"], items[b]["down"], items[b]["n_mid"] = up, down, n_mid
        if up != down:
            hd, hu = taps_of(up, down), taps_of(down, up)
            items[b]["h_down"], items[b]["h_up"] = hd.data_ptr(), hu.data_ptr()
            items[b]["half_len"], items[b]["half_len_up"] = (hd.numel() - 1) // 2, (hu.numel() - 1) // 2
            items[b]["mid_off"] = off
            off += -(-n_mid // 4) * 4
    x = _lib.rows2d(waves, T)
    lib = _lib.lib()
    host = items.ctypes.data
    ws_bytes = lib.vmasr_degrade_batch_workspace(host, B)
    y = torch.empty_like(x)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    table = torch.from_numpy(items.view(np.uint8)).to(x.device)
    _lib.call(lib.vmasr_degrade_batch, x, y, host, table, B, T, ws, ws_bytes)
    return y.view(waves.shape)
