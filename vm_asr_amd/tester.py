"""Evaluation harness: the reference's Tester on the HIP path (trainer/tester.py:15-240, base/base_tester.py:10-90,
utils/post_processing.py:4-34).

    Tester(models, metric_ftns, config, device, data_loader, logger).evaluate() -> dict

Same flow: generator in eval mode, batch-1 clips `(wave_in, wave_tgt, highcut, name, pad)`; clips longer than one
training segment are cut into overlapping segments (TEST.OVERLAP samples), enhanced one by one and cross-averaged
back (`unfold_audio` / `fold_audio`); metrics = config.TRAIN.METRICS (SNR, LSD, LSD-HF, LSD-LF on the HIP STFT) plus
RTF = processing time / clip duration; the summary row is appended to `results_{16,48}kHz.csv` with the reference's
columns (SAMPLE_RATE, SNR, LSD, LSD_HF, LSD_LF, RTF, RTF_RECIPROCAL).  Differences: the processing time is taken
with a device synchronise on both sides (the reference reads the host clock without one, so its RTF under-reports);
wav files are written with the standard library (`wave`, 16-bit PCM) because torchaudio is not a dependency here.
The checkpoint is the generator's `checkpoint-best-G.pth` (utils/utils.py:153-176), read through the yacs-compatible
loader of trainer.BaseTrainer.
"""
import csv
import os
import time
import wave

import torch

from .optim import unwrap

__all__ = ["unfold_audio", "fold_audio", "frames_per_segment", "write_pcm16", "device_sync", "enhance", "BaseTester", "Tester"]


def unfold_audio(audio, segment_length, overlap):
    """(B, C, T) -> (B, C, n_seg, segment_length) overlapping segments (utils/post_processing.py:4-9)."""
    return audio.unfold(dimension=-1, size=segment_length, step=segment_length - overlap)


def fold_audio(segments, total_length, segment_length, overlap):
    """Inverse of unfold_audio with the overlaps averaged; samples no segment covers stay 0
    (utils/post_processing.py:12-34)."""
    step = segment_length - overlap
    B, C, n, _ = segments.shape
    out = torch.zeros(B, C, total_length, dtype=segments.dtype, device=segments.device)
    cnt = torch.zeros(B, C, total_length, dtype=segments.dtype, device=segments.device)
    for i in range(n):
        out[:, :, i * step:i * step + segment_length] += segments[:, :, i]
        cnt[:, :, i * step:i * step + segment_length] += 1
    return out / cnt.clamp(min=1)


def frames_per_segment(config, target_sr):
    """Samples of one training segment at `target_sr` (trainer/tester.py:38-42, trainer/inferencer.py:35-39)."""
    return int(int(config.DATA.SEGMENT * config.DATA.FLAC2WAV.SRC_SR) * target_sr / config.DATA.FLAC2WAV.SRC_SR)


def write_pcm16(path, wave_1d, sample_rate):
    """Mono 16-bit PCM wav of a 1-D float tensor in [-1, 1] (clamped; scaled by 32767, rounded)."""
    pcm = (wave_1d.float().clamp(-1, 1) * 32767.0).round().to(torch.int16).cpu().numpy()
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(sample_rate))
        f.writeframes(pcm.tobytes())


def device_sync(device):
    """Wait for the device's queued work (the timed region of an evaluation or inference run starts and ends here)."""
    if device.type == "cuda":
        torch.cuda.synchronize(device)


def enhance(gen, wave_input, highcut, segment_length, overlap, segment_batch=1):
    """gen over (B, C, T): one call when T fits a segment, else over overlapping segments cross-averaged back
    (trainer/tester.py:92-130, trainer/inferencer.py:75-103).  Up to `segment_batch` segments of a clip go through one
    generator call, stacked in the batch dimension with the clip's highcut repeated; 1 is the reference's loop."""
    if wave_input.size(2) <= segment_length:
        return gen(wave_input, highcut)
    segs = unfold_audio(wave_input, segment_length, overlap)              # (B, C, n, seg)
    B, C, n, _ = segs.shape
    done = torch.zeros_like(segs)
    for i in range(0, n, segment_batch):
        k = min(segment_batch, n - i)
        if k == 1:
            done[:, :, i] = gen(segs[:, :, i].contiguous(), highcut)
        else:
            out = gen(segs[:, :, i:i + k].transpose(1, 2).reshape(B * k, C, segment_length), highcut.repeat_interleave(k))
            done[:, :, i:i + k] = out.view(B, k, C, segment_length).transpose(1, 2)
    return fold_audio(done, wave_input.size(2), segment_length, overlap)


class BaseTester:
    def __init__(self, models, metric_ftns, config, logger=None):
        from .trainer import _Logger      # (not at the top: trainer imports data, which imports this module)
        self.config, self.logger = config, logger or _Logger()
        self.models, self.metric_ftns = models, metric_ftns
        tag = str(config.TAG).split("_")
        if len(tag) != 2:
            raise ValueError("config.TAG must be '{input_sr}_{target_sr}' in evaluation mode (main.py:244-248)")
        self.input_sr, self.target_sr = int(tag[0]), int(tag[1])
        self.output_dir = config.OUTPUT
        if config.MODEL.RESUME_PATH is not None:
            self._resume_checkpoint()

    def _resume_checkpoint(self):
        from .config import yacs_pickle_compat
        path = self.config.MODEL.RESUME_PATH
        for kind in ("best", "latest"):
            f = os.path.join(path, f"checkpoint-{kind}-G.pth")
            if os.path.exists(f):
                with yacs_pickle_compat():
                    ck = torch.load(f, map_location="cpu", weights_only=False)
                unwrap(self.models["generator"]).load_state_dict(ck["state_dict"], strict=True)
                self.logger.info(f"Loaded generator from {f}")
                break
        else:
            raise FileNotFoundError(f"No generator checkpoint found in {path}")
        if self.target_sr != self.config.DATA.TARGET_SR:
            raise ValueError(f"Target sampling rate mismatch: {self.target_sr} vs {self.config.DATA.TARGET_SR}")


class Tester(BaseTester):
    def __init__(self, models, metric_ftns, config, device, data_loader, logger=None, fused_metrics=False):
        """fused_metrics: on a GPU, when every entry of `metric_ftns` is one of vm_asr_amd.metric's four, a clip's metrics
        come from one metric.per_clip call instead of the composed functions (three STFT pairs and ~30 launches per clip)."""
        super().__init__(models, metric_ftns, config, logger)
        self.device = device[0] if isinstance(device, (tuple, list)) else device
        from . import metric
        known = {getattr(metric, n): n for n in metric.METRIC_ORDER}
        self._fused_names = ([known[m] for m in metric_ftns]
                             if fused_metrics and self.device.type == "cuda" and all(m in known for m in metric_ftns) else None)
        self.test_loader = data_loader
        self.test_log = {}
        self.num_frames_per_seg = frames_per_segment(config, self.target_sr)
        for k, m in self.models.items():
            self.models[k] = m.to(self.device)

    def _sync(self):
        device_sync(self.device)

    def _enhance(self, wave_input, highcut):
        return enhance(self.models["generator"], wave_input, highcut, self.num_frames_per_seg, self.config.TEST.OVERLAP)

    @torch.no_grad()
    def evaluate(self):
        for m in self.models.values():
            m.eval()
        sums, n = {}, 0
        for wave_input, wave_target, highcut, filename, pad_length in self.test_loader:
            wave_input, wave_target = wave_input.to(self.device), wave_target.to(self.device)
            self._sync()
            t0 = time.time()
            wave_out = self._enhance(wave_input, highcut)
            self._sync()
            run_time = time.time() - t0
            pad = int(pad_length[0]) if hasattr(pad_length, "__getitem__") else int(pad_length)
            rtf = run_time / ((wave_input.size(2) - pad) / self.config.DATA.TARGET_SR)
            vals = self._evaluate_batch(wave_out, wave_target, highcut)
            vals["rtf"], vals["rtf_reciprocal"] = rtf, 1.0 / rtf
            for k, v in vals.items():
                sums[k] = sums.get(k, 0.0) + float(v)
            n += 1
            if self.config.TEST.SAVE_RESULT:
                self._save_wavs(wave_input, wave_out, wave_target, filename, pad)
        self.test_log = {k: v / max(1, n) for k, v in sums.items()}
        self.test_log["sample_rate"] = self.input_sr
        self.logger.info("Summary of Evaluation: " + " | ".join(f"{k}={v:.4f}" for k, v in self.test_log.items()))
        self.save_results_to_csv(self.test_log, "results_16kHz.csv" if self.target_sr == 16000 else "results_48kHz.csv")
        return self.test_log

    def _evaluate_batch(self, wave_out, wave_target, highcut):
        if self._fused_names is not None:
            from . import metric
            means = dict(zip(metric.METRIC_ORDER, metric.per_clip(wave_out, wave_target, highcut).mean(0).tolist()))
            return {k: means[k] for k in self._fused_names}
        return {m.__name__: m(wave_out.float().squeeze(1), wave_target.squeeze(1), hf=highcut) for m in self.metric_ftns}

    def _save_wavs(self, wave_input, wave_out, wave_target, filename, pad):
        os.makedirs(self.output_dir, exist_ok=True)
        stem = str(filename[0] if isinstance(filename, (list, tuple)) else filename).replace(".wav", "")
        keep = wave_input.size(2) - pad
        for tag, w in (("up", wave_out), ("orig", wave_target), ("down", wave_input)):
            write_pcm16(os.path.join(self.output_dir, f"{stem}_{tag}.wav"), w[0, 0, :keep], self.config.DATA.TARGET_SR)

    def save_results_to_csv(self, results, filename="results.csv"):
        """One row per evaluation, the reference's column order (trainer/tester.py:221-240)."""
        order = ["sample_rate", "snr", "lsd", "lsd_hf", "lsd_lf", "rtf", "rtf_reciprocal"]
        row = {k: results.get(k, "") for k in order}
        exists = os.path.isfile(filename)
        with open(filename, mode="a", newline="") as f:
            w = csv.writer(f)
            if not exists:
                w.writerow([k.upper() for k in row])
            w.writerow(row.values())
