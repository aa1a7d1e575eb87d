"""Evaluation metrics on the HIP STFT: SNR, LSD, LSD-HF, LSD-LF (model/metric.py:5-67).

LSD (the parity metric of BASELINE.json) = mean_t sqrt(mean_f (log10|S_out|^2 - log10|S_tgt|^2)^2)
with a non-normalised hann STFT, n_fft 2048 / hop 512.  Unlike the reference these return
tensors (no per-metric .item() host sync, trainer/trainer.py:179-182); call float() to read.

The four functions compose `stft_complex` with ATen ops (three STFT pairs, one host read of `hf` per clip).  `per_clip` and
`Accumulator` are the per-step path: all four values of a batch from ONE library call (csrc/metrics.hip: out / tgt frames as one
packed complex FFT in LDS, band sums reduced on chip) with no host read, and a running average on the device that is read once.
"""
import torch

from . import _lib
from .stft import stft_complex

__all__ = ["stft", "snr", "lsd", "lsd_hf", "lsd_lf", "METRIC_ORDER", "per_clip", "Accumulator"]

METRIC_ORDER = ("snr", "lsd", "lsd_hf", "lsd_lf")
N_FFT, HOP = 2048, 512      # model/metric.py:5-12


def stft(audio, n_fft=2048, hop_length=512):
    """|STFT| of (B,T) audio -> (B, n_fft/2+1, frames)."""
    re, im = stft_complex(audio, n_fft, hop_length, n_fft, normalized=False)
    return torch.sqrt(re.pow(2) + im.pow(2))


def snr(output, target, **kwargs):
    return (20 * torch.log10(torch.norm(target, dim=-1) / torch.norm(output - target, dim=-1).clamp(min=1e-8))).mean()


def _logspec(x):
    return torch.log10(stft(x).square().clamp(1e-8))


def lsd(output, target, **kwargs):
    return (_logspec(output) - _logspec(target)).square().mean(dim=1).sqrt().mean()


def _lsd_band(output, target, hf, high):
    sp, st = _logspec(output), _logspec(target)
    vals = []
    for i in range(output.size(0)):
        h = int(hf[i])
        d = (sp[i, h:] - st[i, h:]) if high else (sp[i, :h] - st[i, :h])
        vals.append(d.square().mean(dim=0).sqrt().mean())
    return torch.stack(vals).mean()


def lsd_hf(output, target, hf):
    return _lsd_band(output, target, hf, True)


def lsd_lf(output, target, hf):
    return _lsd_band(output, target, hf, False)


def _fused_args(output, target, hf):
    """(B,T) fp32 contiguous output / target and (B) int64 device hf — nothing here waits for the device."""
    _lib.require_cuda("metric.per_clip", output, target)
    if output.dim() == 3:
        output = output.squeeze(1)
    if target.dim() == 3:
        target = target.squeeze(1)
    if output.dim() != 2 or output.shape != target.shape:
        raise RuntimeError(f"metric.per_clip: expected (B,T) or (B,1,T) output and target of one shape, got "
                           f"{tuple(output.shape)} and {tuple(target.shape)}")
    output, target = output.float().contiguous(), target.float().contiguous()
    if not torch.is_tensor(hf):
        hf = torch.as_tensor(hf, dtype=torch.int64)
    hf = hf.reshape(-1).to(device=output.device, dtype=torch.int64, non_blocking=True).contiguous()
    if hf.numel() != output.shape[0]:
        raise RuntimeError(f"metric.per_clip: hf has {hf.numel()} entries for a batch of {output.shape[0]}")
    return output, target, hf


def _workspace(ws, B, T, device):
    need = _lib.lib().vmasr_metrics_workspace(B, T, N_FFT, HOP)
    if ws is None or ws.numel() * 4 < need or ws.device != device:
        ws = torch.empty(max(1, need // 4), dtype=torch.float32, device=device)
    return ws, need


def _launch(output, target, hf, acc, ws):
    B, T = output.shape
    ws, _ = _workspace(ws, B, T, output.device)
    res = torch.empty((B, 4), dtype=torch.float32, device=output.device)
    _lib.call(_lib.lib().vmasr_metrics, output, target, hf, res, acc, B, T, N_FFT, HOP, ws, ws.numel() * 4)
    return res, ws


@torch.no_grad()
def per_clip(output, target, hf):
    """(B,4) fp32 tensor, columns METRIC_ORDER: the four metrics of every clip from one library call on the current stream
    (no host read).  output / target: (B,T) or (B,1,T); hf: (B) band edges — device or host tensor, or a list."""
    output, target, hf = _fused_args(output, target, hf)
    return _launch(output, target, hf, None, None)[0]


class Accumulator:
    """Running average of the four metrics over `update` calls, as the reference's per-step average computes it
    (trainer/trainer.py:158-182): read() = mean over the calls of each call's batch mean.  On a CUDA device an update is one
    library call that adds the batch means to five doubles on the device; nothing is read on the host before read().  On a CPU
    device (host-logic tests) an update composes the four functions above and sums in fp64 on the host."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.count = 0
        self._ws = None
        self._acc = torch.zeros(5, dtype=torch.float64, device=self.device) if self.device.type == "cuda" else [0.0] * 4

    @torch.no_grad()
    def update(self, output, target, hf):
        if self.device.type == "cuda":
            output, target, hf = _fused_args(output, target, hf)
            _, self._ws = _launch(output, target, hf, self._acc, self._ws)
        else:
            if output.dim() == 3:
                output = output.squeeze(1)
            if target.dim() == 3:
                target = target.squeeze(1)
            output = output.float()
            for i, f in enumerate((snr, lsd, lsd_hf, lsd_lf)):
                self._acc[i] += float(f(output, target, hf=hf).double())
        self.count += 1

    def sums(self):
        """The four sums of batch means as a float64 tensor on the accumulator's device (no sync on CUDA; the cross-rank
        all-reduce of a validation epoch adds these)."""
        if self.device.type == "cuda":
            return self._acc[:4].clone()
        return torch.tensor(self._acc, dtype=torch.float64)

    def reset(self):
        self.count = 0
        if self.device.type == "cuda":
            self._acc.zero_()
        else:
            self._acc = [0.0] * 4

    def read(self, reset=True):
        """{name: float} means over the updates so far ({} before the first one).  The only host sync."""
        if self.count == 0:
            return {}
        sums = self._acc[:4].tolist() if self.device.type == "cuda" else list(self._acc)
        out = {k: v / self.count for k, v in zip(METRIC_ORDER, sums)}
        if reset:
            self.reset()
        return out
