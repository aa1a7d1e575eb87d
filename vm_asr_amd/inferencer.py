"""Wav-file inference: the reference's Inferencer on the HIP path (trainer/inferencer.py:16-277, base/base_inference.py:8-71).

    inf = Inferencer(models, config, device, logger=None, segment_batch=1)
    inf.infer_file("speech.wav", output_dir=None)          -> enhanced wave (1, 1, T), writes {stem}_enhanced.wav
    inf.infer_directory("clips/", output_dir=None)         -> [written paths]

Same flow: TAG = '{input_sr}_{target_sr}' names the checkpoint's rates (input_sr must lie within DATA.RANDOM_RESAMPLE), the
generator comes from `checkpoint-*-G.pth` (tester.BaseTester); a file is decoded, brought to the target rate, padded with
white noise (torch.randn * DATA.PAD_WHITENOISE) up to one segment or to a multiple of it, and enhanced: one segment directly,
a longer file cut into overlapping segments (TEST.OVERLAP), enhanced and cross-averaged back (tester.enhance, the segment
loop the Tester runs).  The segment is always the training segment at the target rate (tester.frames_per_segment).

Built differently: wav decoding is the standard library's `wave` (integer PCM; 16-bit is the required case, 8 / 24 / 32-bit
are decoded where `wave` opens them) because torchaudio is not a dependency; resampling to the target rate runs on the device
(vm_asr_amd.resample.resample_poly, scipy's resample_poly filter); up to `segment_batch` segments go through the generator per
call, stacked in the batch dimension (1 = the reference's loop); the run is timed with a device synchronise on both sides and
the real-time factor is logged.

Deliberate deviations from the reference:
  * highcut.  The reference computes it after `sr` has been overwritten with the target rate (inferencer.py:196-201,228-230),
    so it is always N_FFT//2 + 1, which with LOW_FREQ_REPLACEMENT copies every input bin over the output: output == input.
    Here highcut = int((N_FFT//2 + 1) * eff / TARGET_SR) with eff = the file's own rate when that is below the target rate,
    otherwise TAG's input_sr (a file already at the target rate says nothing about its bandwidth).
  * output_dir.  The reference ignores the argument and writes into config.OUTPUT (inferencer.py:111-112); it is honoured here.
  * The written file is trimmed to the input's length at the target rate; the reference writes the white-noise tail too.
"""
import glob
import os
import time
import wave

import numpy as np
import torch

from .resample import resample_poly
from .tester import BaseTester, device_sync, enhance, frames_per_segment, write_pcm16

__all__ = ["read_wav", "Inferencer"]


def read_wav(path):
    """(audio (channels, T) float32 in [-1, 1), sample rate) of an integer-PCM wav file; ValueError for anything else."""
    try:
        with wave.open(path, "rb") as f:
            ch, width, sr, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
            raw = f.readframes(n)
    except (wave.Error, EOFError) as e:
        raise ValueError(f"{path}: not an integer-PCM wav file the standard library can decode ({e}); "
                         "convert it to 16-bit PCM") from e
    if width == 1:                                   # unsigned, offset binary
        a = np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0
    elif width == 2:
        a = np.frombuffer(raw, dtype="<i2").astype(np.float32)
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        a = (((b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) ^ 0x800000) - 0x800000).astype(np.float32)
    elif width == 4:
        a = np.frombuffer(raw, dtype="<i4").astype(np.float64)
    else:
        raise ValueError(f"{path}: {8 * width}-bit samples are not supported; convert the file to 16-bit PCM")
    if ch < 1 or a.size == 0:
        raise ValueError(f"{path}: no audio frames")
    a = (a / float(1 << (8 * width - 1))).astype(np.float32)
    return torch.from_numpy(a.reshape(-1, ch).T.copy()), int(sr)


class Inferencer(BaseTester):
    def __init__(self, models, config, device, logger=None, segment_batch=1):
        super().__init__(models, None, config, logger)
        rr = config.DATA.RANDOM_RESAMPLE
        if not int(rr[0]) <= self.input_sr <= int(rr[-1]):
            raise ValueError(f"Input sampling rate mismatch: {self.input_sr} not in {list(rr)}, please choose the correct checkpoint.")
        self.device = device[0] if isinstance(device, (tuple, list)) else torch.device(device)
        self.segment_batch = max(1, int(segment_batch))
        self.num_frames_per_seg = frames_per_segment(config, self.target_sr)
        for k, m in self.models.items():
            if m is not None:
                self.models[k] = m.to(self.device)

    def highcut_for(self, file_sr):
        """The first STFT bin above the file's band (module docstring: the file's own rate below the target rate, else TAG's)."""
        eff = file_sr if file_sr < self.target_sr else self.input_sr
        return int((self.config.DATA.STFT.N_FFT // 2 + 1) * eff / self.config.DATA.TARGET_SR)

    def pad_length(self, n):
        """White-noise samples appended to n samples: up to one segment, or to the next multiple of the segment."""
        seg = self.num_frames_per_seg
        return seg - n if n < seg else (seg - n % seg) % seg

    def load_input(self, path):
        """-> (wave (1, 1, T + pad) on the device at the target rate, highcut (1) int64, pad)."""
        audio, sr = read_wav(path)
        audio = audio.mean(dim=0, keepdim=True).to(self.device)          # (1, T) mono
        if sr != self.target_sr:
            audio = resample_poly(audio, self.target_sr, sr)
        pad = self.pad_length(audio.shape[-1])
        if pad:
            noise = (torch.randn(pad) * self.config.DATA.PAD_WHITENOISE).unsqueeze(0)
            audio = torch.cat((audio, noise.to(self.device)), dim=-1)
        return audio.unsqueeze(0), torch.tensor([self.highcut_for(sr)], dtype=torch.int64), pad

    @torch.no_grad()
    def infer_file(self, path, output_dir=None):
        """Enhance one wav file; writes `{stem}_enhanced.wav` (16-bit PCM, target rate, pad trimmed) into `output_dir`
        (default config.OUTPUT) and returns the enhanced wave (1, 1, T) it holds."""
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        output_dir = output_dir or self.output_dir
        os.makedirs(output_dir, exist_ok=True)
        self.models["generator"].eval()
        wave_input, highcut, pad = self.load_input(path)
        keep = wave_input.size(2) - pad
        device_sync(self.device)
        t0 = time.time()
        wave_out = enhance(self.models["generator"], wave_input, highcut, self.num_frames_per_seg, self.config.TEST.OVERLAP,
                           self.segment_batch)
        device_sync(self.device)
        run_time = time.time() - t0
        rtf = run_time / (keep / self.target_sr)
        out_path = os.path.join(output_dir, os.path.splitext(os.path.basename(path))[0] + "_enhanced.wav")
        write_pcm16(out_path, wave_out[0, 0, :keep], self.target_sr)
        self.logger.info(f"{os.path.basename(path)}: {keep / self.target_sr:.2f} s enhanced in {run_time:.3f} s "
                         f"(RTF {rtf:.4f}, {1.0 / max(rtf, 1e-12):.1f}x real time) -> {out_path}")
        return wave_out[:, :, :keep]

    def infer_directory(self, dir_path, output_dir=None, file_types=(".wav",)):
        """Enhance every file of `dir_path` with one of the extensions; -> the written paths (sorted by input name)."""
        if not os.path.isdir(dir_path):
            raise FileNotFoundError(dir_path)
        output_dir = output_dir or os.path.join(self.output_dir, os.path.basename(os.path.normpath(dir_path)))
        files = sorted(f for ext in file_types for f in glob.glob(os.path.join(dir_path, f"*{ext}")))
        if not files:
            self.logger.warning(f"No audio files found in {dir_path}")
            return []
        self.logger.info(f"Found {len(files)} audio files to process ({self.input_sr} to {self.target_sr})")
        written = []
        for f in files:
            self.infer_file(f, output_dir)
            written.append(os.path.join(output_dir, os.path.splitext(os.path.basename(f))[0] + "_enhanced.wav"))
        self.logger.info(f"Processed {len(written)} files")
        return written
